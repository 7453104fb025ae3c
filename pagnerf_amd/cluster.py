"""Mean-shift clustering of the instance embedding on the GPU - utils/clustering/{clustering_base,mean_shift}.py, utils/embedding.py and
pc_nerf/clustering_nef.py of the reference, on pag_meanshift_fit / pag_meanshift_predict (csrc/cluster.hip).

The contrastive configs (`nef_type: MeanShift*NeF`, `inst_loss: sup_contrastive`) train an instance embedding that carries no ids of its own;
ids come from clustering it.  pc_nerf/trainer.py:948-970 fits the clustering on the class means of `num_clustering_samples` training rays per
validation (`nef.train_clustering(F.normalize(emb), ids)`), and :737-738 labels every validation image with `nef.predict_clusters(inst_embedding)`.
The reference runs both through sklearn on the host; here every pass stays on the device and a fit reads back 24 bytes once, at its end.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import ops
from .dd import PanopticDDensityNeF
from .nef import PanopticDeltaNeF, PanopticNeF

MAX_K = 32768            # class centres per fit (20 000 training rays bound K in the trainer)
MAX_D = 512
MAX_ROWS = 1 << 24       # rows of one fit
_FLAG_K_OVERFLOW = 1


def _features(X, what):
    if X.dtype not in (torch.float32, torch.bfloat16):
        X = X.float()
    if X.dim() >= 2 and X.shape[-1] > MAX_D:
        raise ValueError("%s: embedding dimension %d > %d" % (what, X.shape[-1], MAX_D))
    return X


def _fit(X, labels, stages, quantile=0.08, max_iter=300):
    """pag_meanshift_fit on X [B, P, D] (labels [B, P], or None: every row is its own class) -> (means [K, D], bandwidth, centres [C, D], n_iter);
    one host synchronisation, at the end.  K == 0 -> (empty means, None, None, 0)."""
    B, P, D = X.shape
    dev = X.device
    if B * P == 0 or D == 0:
        return X.new_zeros((0, D), dtype=torch.float32), None, None, 0
    if B * P > MAX_ROWS:
        raise ValueError("mean-shift fit: %d rows > %d" % (B * P, MAX_ROWS))
    if labels is None and B * P > MAX_K:
        raise ValueError("mean-shift fit: %d centres > K limit %d" % (B * P, MAX_K))
    if (D > 1 and X.stride(2) != 1) or (P > 1 and X.stride(1) < D) or X.stride(0) < 0:       # expanded or transposed rows: one copy
        X = X.contiguous()
    image_stride, row_stride = (X.stride(0) if B > 1 else 0), (X.stride(1) if P > 1 else D)
    kcap = min(B * P, MAX_K)
    nbytes = int(L.load().pag_meanshift_workspace_bytes(B, P, D))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    means = torch.empty(kcap, D, device=dev)
    centres = torch.empty(kcap, D, device=dev) if stages >= 3 else None
    out = torch.zeros(24, device=dev, dtype=torch.uint8)            # info i32 [4] | bandwidth f64: one read-back for both
    ops._call("pag_meanshift_fit", X.data_ptr(), L.dtype_code(X), B, P, D, image_stride, row_stride,
              labels.data_ptr() if labels is not None else None, float(quantile), int(max_iter), stages, ws.data_ptr(), nbytes,
              means.data_ptr(), out.data_ptr() + 16 if stages >= 2 else None, centres.data_ptr() if centres is not None else None, out.data_ptr(),
              L.stream())
    host = out.cpu()
    K, C, n_iter, flags = host[:16].view(torch.int32).tolist()
    if flags & _FLAG_K_OVERFLOW:
        raise ValueError("mean-shift fit: more than %d class centres" % MAX_K)
    bw = float(host[16:].view(torch.float64)[0]) if stages >= 2 else None
    if stages >= 3 and C == 0:
        raise ValueError("No point was within bandwidth=%f of any seed." % bw)          # sklearn MeanShift.fit's error
    return means[:K], bw, (centres[:C] if centres is not None else None), n_iter


def _labels(labels, shape):
    ops._check_gpu(labels)
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError("labels must be an integer tensor, got %s" % labels.dtype)
    if tuple(labels.shape) != tuple(shape):
        raise ValueError("labels %s do not match the embedding's leading shape %s" % (tuple(labels.shape), tuple(shape)))
    return labels.detach().long().contiguous()


def mean_class_embedding(embeddings, labels):
    """utils/embedding.py::mean_class_embedding: embeddings [B, P, D], labels [B, P] -> f32 [K, D], one centre per (image, distinct label) - images
    in order, labels ascending within an image, negative labels included - each the fp32 sum of its rows over the count."""
    ops._check_gpu(embeddings, labels)
    if embeddings.dim() != 3:
        raise ValueError("embeddings must be [B, P, D], got %s" % (tuple(embeddings.shape),))
    X = _features(embeddings.detach(), "mean_class_embedding")
    lab = _labels(labels, X.shape[:2])
    return _fit(X, lab, 1)[0]


def estimate_bandwidth(centres, quantile=0.08):
    """sklearn.cluster.estimate_bandwidth(centres, quantile) as utils/clustering/mean_shift.py:22 calls it: the mean over the centres of the exact
    Euclidean distance to the k-th nearest centre (itself included), k = max(1, int(K quantile)), fp64 arithmetic on the fp32 values.

    Divergence for k = 1 (K < 1 / quantile, i.e. K < 25) and for sets whose k-th distances are all 0 (K = 1, identical centres): the result here is
    exactly 0, and MeanShift then makes every distinct centre its own cluster.  sklearn's rounding leaves a bandwidth of ~1e-9 there, at the size of
    its own error for a centre's distance to itself, so the reference's MeanShift drops some seeds at random; where its bandwidth is exactly 0 (K = 1,
    identical centres) it raises InvalidParameterError instead of fitting."""
    ops._check_gpu(centres)
    if centres.dim() != 2 or centres.shape[0] == 0:
        raise ValueError("centres must be a non-empty [K, D] tensor, got %s" % (tuple(centres.shape),))
    if not 0.0 <= float(quantile) <= 1.0:
        raise ValueError("quantile %r not in [0, 1]" % (quantile,))
    X = _features(centres.detach(), "estimate_bandwidth")
    return _fit(X.reshape(1, *X.shape), None, 2, quantile=quantile)[1]


class ClusteringBase(nn.Module):
    """utils/clustering/clustering_base.py::ClusteringBase: the constructor's three arguments are kept as attributes and otherwise unused (as in the
    reference); unknown keyword arguments are accepted because ClusteringNeF hands the clustering object every NeF argument."""

    def __init__(self, num_clusters: int = -1, distance_func: str = 'cosine', num_clustering_workers: int = 1, **kwargs):
        super().__init__()
        self.distance_func = distance_func
        self.num_clusters = num_clusters
        self.num_workers = num_clustering_workers

    def train_clustering(self, X=None, labels=None):
        raise NotImplementedError("'train_clustering' is not implemented for this NeF.")

    def predict_clusters(self, X=None):
        raise NotImplementedError("'predict_clusters' is not implemented for this NeF.")


class MeanShift(ClusteringBase):
    """utils/clustering/mean_shift.py::MeanShift on the device.

    train_clustering(X [B, P, D], labels [B, P]): centres = mean_class_embedding(X, labels); nothing happens (the previous fit stays) when there are
    none; bandwidth = estimate_bandwidth(centres, 0.08); then sklearn's MeanShift(bandwidth, bin_seeding=False, cluster_all=True, max_iter=300)
    on the centres.  Sets `cluster_centers_` (f32 [C, D] on the device), `bandwidth` (float), `n_iter_` and `n_centres_` (K).  One host
    synchronisation, at the end (K and C size the result).  With K < 25 or identical centres the bandwidth is 0 and every distinct centre is its
    own cluster; the reference drops some seeds there or raises (see estimate_bandwidth).

    predict_clusters(X [..., D]) -> int64 [...]: index of the nearest cluster centre (Euclidean; exact ties to the lowest index), on X as given - the
    trainer fits on normalised embeddings and predicts on the raw ones (pc_nerf/trainer.py:970 vs :738), and so does this.  Before any fit:
    argmax(F.normalize(X, dim=-1), -1), as the reference.  No host synchronisation."""

    QUANTILE = 0.08
    MAX_ITER = 300

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.cluster_centers_ = None
        self.bandwidth = None
        self.n_iter_ = None
        self.n_centres_ = None

    @property
    def fitted(self):
        return self.cluster_centers_ is not None

    def train_clustering(self, X, labels):
        ops._check_gpu(X, labels)
        if X.dim() != 3:
            raise ValueError("X must be [B, P, D], got %s" % (tuple(X.shape),))
        Xf = _features(X.detach(), "MeanShift.train_clustering")
        lab = _labels(labels, Xf.shape[:2])
        means, bw, centres, n_iter = _fit(Xf, lab, 3, quantile=self.QUANTILE, max_iter=self.MAX_ITER)
        if means.shape[0] == 0:
            return
        self.cluster_centers_ = centres.clone()
        self.bandwidth = bw
        self.n_iter_ = n_iter
        self.n_centres_ = int(means.shape[0])

    def predict_clusters(self, X=None):
        ops._check_gpu(X)
        if not self.fitted:
            return torch.argmax(F.normalize(X, dim=-1), dim=-1)
        C, D = self.cluster_centers_.shape
        if X.shape[-1] != D:
            raise ValueError("predict_clusters: embedding dimension %d, the clustering was fitted on %d" % (X.shape[-1], D))
        lead = X.shape[:-1]
        x = _features(X.detach(), "MeanShift.predict_clusters")
        x = x.reshape(-1, D)                                            # a view wherever the rows keep one stride
        N = x.shape[0]
        if (D > 1 and x.stride(1) != 1) or (N > 1 and x.stride(0) < D):   # elements not adjacent (even in a single row), or rows overlapping
            x = x.contiguous()
        out = torch.empty(N, device=x.device, dtype=torch.int64)
        if N:
            ops._call("pag_meanshift_predict", x.data_ptr(), L.dtype_code(x), N, D, x.stride(0) if N > 1 else D,
                      self.cluster_centers_.data_ptr(), C, out.data_ptr(), L.stream())
        return out.reshape(lead)


class ClusteringNeF:
    """pc_nerf/clustering_nef.py::ClusteringNeF as a mixin over this package's NeFs: a `clusters` channel that returns the embedding channel (the
    tracer renders it through its extra-channel path, pc_nerf's tracers :184-192), and train_clustering / predict_clusters delegated to the
    clustering object.  The base NeF's first channel function is wrapped, as register_forward_functions does there."""

    def _init_clustering(self, cluster_class, embedding_channel, **kwargs):
        self.clustering_obj = cluster_class(**kwargs)
        assert embedding_channel in self.get_supported_channels(), \
            f'"{embedding_channel}" Channel not supported for custering, supported channels by NeF are: {self.get_supported_channels()}'
        self.embedding_channel = embedding_channel
        fn, chans = self._fns[0]
        self.nef_forward = fn
        self._fns = [(self.cluster_nef, set(chans) | {"clusters"})] + list(self._fns[1:])

    def get_nef_type(self):
        return f'clustering_{super().get_nef_type()}'

    def train_clustering(self, X=None, labels=None):
        self.clustering_obj.train_clustering(X, labels)

    def predict_clusters(self, X=None):
        return self.clustering_obj.predict_clusters(X)

    def cluster_nef(self, coords, ray_d=None, compute_channels=None, pidx=None, lod_idx=None, ridx=None, ray_dirs=None, ray_packs=None):
        if isinstance(compute_channels, str):
            compute_channels = [compute_channels]
        want = compute_channels is not None and 'clusters' in compute_channels
        chans = set(compute_channels or ()) - {'clusters'}
        if want:
            chans.add(self.embedding_channel)
        outputs = self.nef_forward(coords=coords, ray_d=ray_d, compute_channels=chans, pidx=pidx, lod_idx=lod_idx, ridx=ridx, ray_dirs=ray_dirs,
                                   ray_packs=ray_packs)
        if want:
            outputs['clusters'] = outputs[self.embedding_channel]
        return outputs


_CLUSTER_KW = ("num_clusters", "distance_func", "num_clustering_workers")


def _split_kwargs(kwargs):
    return {k: kwargs.pop(k) for k in _CLUSTER_KW if k in kwargs}


class MeanShiftPanopticNeF(ClusteringNeF, PanopticNeF):
    def __init__(self, *args, **kwargs):
        ckw = _split_kwargs(kwargs)
        PanopticNeF.__init__(self, *args, **kwargs)
        self._init_clustering(MeanShift, 'inst_embedding', **ckw)

    def get_nef_type(self):
        return 'mean_shift_panoptic_nef'


class MeanShiftPanopticDDensityNeF(ClusteringNeF, PanopticDDensityNeF):
    def __init__(self, *args, **kwargs):
        ckw = _split_kwargs(kwargs)
        PanopticDDensityNeF.__init__(self, *args, **kwargs)
        self._init_clustering(MeanShift, 'inst_embedding', **ckw)


class MeanShiftPanopticDeltaNeF(ClusteringNeF, PanopticDeltaNeF):
    def __init__(self, *args, **kwargs):
        ckw = _split_kwargs(kwargs)
        PanopticDeltaNeF.__init__(self, *args, **kwargs)
        self._init_clustering(MeanShift, 'inst_embedding', **ckw)

    def get_nef_type(self):
        return 'mean_shift_panoptic_delta_nef'
