"""Panoptic evaluation of validation images on the GPU - utils/metrics/panoptic_quality{,_func}.py (PanopticQuality, panoptic_quality), the instance
cleanup of pc_nerf/trainer.py:750-772 and the semantic IoU of :670-671 / :720, on pag_panoptic_pq_update / pag_panoptic_clean / pag_confusion_matrix
(csrc/panoptic.hip).

The reference's PQ loops in Python over every (pred, target) segment pair with a host round trip per pair, and its cleanup builds one int64 [K, H, W]
mask per instance id (about 1.5 GB at 720 x 1280 with 200 ids).  Here `update`, `clean_instances` and `MulticlassIoU.update` are a few device passes
over O(B H W) workspace with no host synchronisation (PanopticQuality.update with allow_unknown_preds_category=False reads one flag back, as the
reference's check needs), so they can be captured in a graph; `compute()` reads the small per-category state back once.

Inputs must be device tensors (the project has no CPU fallback) and are never modified.  Divergence: for B > 1 the reference adds the batch offsets of
_make_instance_ids_batch_unique into the caller's preds and target in place; here the caller's tensors stay as they are.
"""
import ctypes
from collections.abc import Set

import torch

from . import _lib as L
from . import ops

MAX_CATEGORIES = 1024
_FLAG_UNKNOWN_PRED = 1
_FLAG_INST_RANGE = 2
_IDX = {torch.int32: L.I32, torch.int64: L.I64}


def _is_set_int(value):
    return isinstance(value, Set) and set(map(type, value)).issubset({int})


def _validate_categories(things, stuff):
    if not _is_set_int(things):
        raise ValueError("Expected argument `things` to be of type `Set[int]`")
    if len(things) == 0:
        raise ValueError("Expected argument `things` to be a non-empty `Set[int]`")
    if not _is_set_int(stuff):
        raise ValueError("Expected argument `stuff` to be of type `Set[int]`")
    if len(stuff) == 0:
        raise ValueError("Expected argument `stuff` to be a non-empty `Set[int]`")
    if stuff & things:
        raise ValueError("Expected arguments `things` and `stuffs` to have distinct keys.")
    if len(things) + len(stuff) > MAX_CATEGORIES:
        raise ValueError("PanopticQuality: %d categories > %d" % (len(things) + len(stuff), MAX_CATEGORIES))


def _validate_inputs(preds, target):
    if not isinstance(preds, torch.Tensor):
        raise ValueError("Expected argument `preds` to be of type `torch.Tensor`")
    if not isinstance(target, torch.Tensor):
        raise ValueError("Expected argument `target` to be of type `torch.Tensor`")
    if preds.shape != target.shape:
        raise ValueError("Expected argument `preds` and `target` to have the same shape")
    if preds.dim() != 4 or preds.shape[1] != 2:
        raise ValueError("Expected argument `preds` to have shape [batch, 2, height, width]. Dim 1 corresponds to (category_id, instance_id)")


def void_color(things, stuff):
    """The colour of pixels whose category is neither a thing nor a stuff: (1 + max(things | stuff | {0}), 0)."""
    return (1 + max([0] + list(things) + list(stuff)), 0)


def category_to_continuous_id(things, stuff):
    """{category id: continuous id}: things numbered 0 .. len(things)-1 in the SET'S ITERATION ORDER (not sorted: list({8, 1, 3}) == [8, 1, 3]),
    then stuff from len(things) on, likewise - the order in which the reference enumerates them, and so the order of the state tensors."""
    ids = {c: i for i, c in enumerate(things)}
    ids.update({c: i + len(things) for i, c in enumerate(stuff)})
    return ids


def _index(t, what):
    if t.dtype not in _IDX:
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise TypeError("%s must be an integer tensor, got %s" % (what, t.dtype))
        t = t.long()
    return t


def _strides(t, ndim=4):
    """Host int64 [4] array of element strides; missing leading dimensions get stride 0."""
    st = [0] * (ndim - t.dim()) + list(t.stride())
    return (ctypes.c_int64 * 4)(*st)


def _pq_compute(n_things, n_stuff, iou_sum, tp, fp, fn):
    """The reference's per-category formulas and means over the categories with tp + fp + fn != 0 (an empty group gives nan), on the host tensors."""
    dets = tp + fp + fn
    denom = (tp + 0.5 * fp + 0.5 * fn).double()
    pq = torch.where(denom > 0.0, iou_sum / denom, 0.0)
    sq = torch.where(tp > 0.0, iou_sum / tp, 0.0)
    rq = torch.where(denom > 0.0, tp / denom, 0.0)

    def group(lo, hi, n):
        keep = dets[lo:hi] != 0
        return dict(pq=torch.mean(pq[lo:hi][keep]), rq=torch.mean(rq[lo:hi][keep]), sq=torch.mean(sq[lo:hi][keep]), n=n)

    n = n_things + n_stuff
    return dict(all=group(0, n, n), things=group(0, n_things, n_things), stuff=group(n_things, n, n_stuff))


class PanopticQuality:
    """utils/metrics/panoptic_quality.py::PanopticQuality on the device.

    PanopticQuality(things, stuff, allow_unknown_preds_category=False); update(preds, target) with both [B, 2, H, W] integer device tensors (dim 1 =
    (category_id, instance_id)); compute() -> {'all' | 'things' | 'stuff': {'pq', 'rq', 'sq': f64 0-d tensors, 'n': int}}; reset(); to(device) returns
    self.  States (names, dtypes and shapes of the reference): iou_sum f64 [n_cat], true_positives / false_positives / false_negatives i32 [n_cat],
    indexed by category_to_continuous_id (set iteration order).

    Semantics of the reference, reproduced exactly:
    - preprocessing: image b's instance ids get the cumulative offset sum_{b' < b} max(instance channel of b'), taken over the whole channel before
      the stuff reset (so ids of different images can still collide, e.g. image 0 ids {0, 3} and image 1 ids {0, 2}); stuff pixels get instance 0;
      categories in neither set become void_color(things, stuff).  Unknown pred categories raise ValueError unless allow_unknown_preds_category
      (what the trainer passes; then update issues no host synchronisation).
    - a (pred, target) segment pair with a non-void target of the same category is a true positive when intersection / union > 0.5 (strict), with
      the int64 union pred_area - pred_void_area + target_area - void_target_area - intersection and the quotient in float32, as torch's int64
      tensor division gives; every qualifying pair counts and adds its IoU to iou_sum.  Each update's IoUs are f32 multiples of 2^-24 in (0.5, 1],
      summed exactly (as integers), so the f64 per-update sum equals the reference's in its torch.unique order; it is then added to the state.
    - an unmatched non-void target (pred) segment is a false negative (positive) unless void_target_area / target_area (pred_void_area /
      pred_area), in float32, is > 0.5.
    - compute(): the reference's per-category pq / sq / rq and their means over the categories with tp + fp + fn != 0; an empty group gives nan.
      It runs on the host copy of the states (a few elements), so it equals the reference's CPU arithmetic bit for bit; the results are returned
      on the states' device.
    Instance ids outside int32 after the batch offsets set a device flag, and compute() raises ValueError on it.  B*H*W <= 2^28, at most 1024
    categories.  Divergence: the caller's tensors are never modified (the reference adds the batch offsets into them in place for B > 1)."""

    def __init__(self, things, stuff, allow_unknown_preds_category=False, **kwargs):
        _validate_categories(things, stuff)
        self.things = things
        self.stuff = stuff
        self.void_color = void_color(things, stuff)
        self.cat_id_to_continuous_id = category_to_continuous_id(things, stuff)
        self.allow_unknown_preds_category = allow_unknown_preds_category
        n = len(things) + len(stuff)
        self.iou_sum = torch.zeros(n, dtype=torch.double)
        self.true_positives = torch.zeros(n, dtype=torch.int)
        self.false_positives = torch.zeros(n, dtype=torch.int)
        self.false_negatives = torch.zeros(n, dtype=torch.int)
        self._flags = torch.zeros(1, dtype=torch.int32)
        order = sorted(self.cat_id_to_continuous_id)
        self._cat_ids = torch.tensor(order, dtype=torch.int64)
        self._cat_cont = torch.tensor([self.cat_id_to_continuous_id[c] for c in order], dtype=torch.int32)

    _STATE = ("iou_sum", "true_positives", "false_positives", "false_negatives", "_flags", "_cat_ids", "_cat_cont")

    @property
    def device(self):
        return self.iou_sum.device

    def to(self, device):
        for name in self._STATE:
            setattr(self, name, getattr(self, name).to(device))
        return self

    def reset(self):
        for name in self._STATE[:5]:
            getattr(self, name).zero_()

    def update(self, preds, target):
        _validate_inputs(preds, target)
        ops._check_gpu(preds, target)
        if preds.device != target.device:
            raise ValueError("preds on %s, target on %s" % (preds.device, target.device))
        preds, target = _index(preds, "preds"), _index(target, "target")
        if self.device != preds.device:
            self.to(preds.device)
        B, _, H, W = preds.shape
        if B * H * W == 0:
            return
        n_cat = len(self.cat_id_to_continuous_id)
        nbytes = int(L.load().pag_panoptic_pq_workspace_bytes(B, H, W, n_cat))
        if nbytes == 0:
            raise ValueError("PanopticQuality.update: %d pixels > 2^28" % (B * H * W))
        ws = torch.empty(nbytes, device=preds.device, dtype=torch.uint8)
        ops._call("pag_panoptic_pq_update", preds.data_ptr(), _IDX[preds.dtype], _strides(preds), target.data_ptr(), _IDX[target.dtype],
                  _strides(target), B, H, W, self._cat_ids.data_ptr(), self._cat_cont.data_ptr(), n_cat, len(self.things),
                  int(bool(self.allow_unknown_preds_category)), ws.data_ptr(), nbytes, self.iou_sum.data_ptr(), self.true_positives.data_ptr(),
                  self.false_positives.data_ptr(), self.false_negatives.data_ptr(), self._flags.data_ptr(), L.stream())
        if not self.allow_unknown_preds_category and int(ws[:4].view(torch.int32)[0]) & _FLAG_UNKNOWN_PRED:
            raise ValueError("Unknown categories found in preds")            # the state was left unchanged on the device

    def compute(self):
        if int(self._flags[0]) & _FLAG_INST_RANGE:
            raise ValueError("PanopticQuality: an instance id lies outside int32 after the batch offsets")
        res = _pq_compute(len(self.things), len(self.stuff), self.iou_sum.cpu(), self.true_positives.cpu(), self.false_positives.cpu(),
                          self.false_negatives.cpu())
        dev = self.device
        return {g: {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()} for g, d in res.items()}


def panoptic_quality(preds, target, things, stuff, allow_unknown_preds_category=False):
    """utils/metrics/panoptic_quality_func.py::panoptic_quality: the 'all' PQ of one update (f64 0-d tensor); see PanopticQuality."""
    _validate_categories(things, stuff)
    _validate_inputs(preds, target)
    m = PanopticQuality(things, stuff, allow_unknown_preds_category)
    m.update(preds, target)
    return m.compute()["all"]["pq"]


def clean_instances(instances, num_openings=1, outlier_rejection=False, min_area=100, std_threshold=2.0):
    """The label path of pc_nerf/trainer.py:750-772 (inst_num_dilations = num_openings, inst_outlier_rejection = outlier_rejection) on an [H, W]
    int32 / int64 id image -> the cleaned id image (same dtype, contiguous); the bounding-box drawing is not part of it.

    - the background is mask_ids[0], the SMALLEST id of the image (not necessarily 0); every other id is a mask; an image with one distinct id comes
      back unchanged.
    - num_openings >= 1: kornia's flat 3x3 opening of each mask, restated as erosion (pixels outside the image count as inside the mask) followed by
      dilation (outside pixels count as outside).  The masks are disjoint, so this is one 5x5 stencil on the label image: a pixel keeps its id iff
      some in-image 3x3 neighbour has its whole in-image 3x3 neighbourhood of that id.  Opening is idempotent, so any num_openings >= 1 gives the
      result of 1; 0 skips it.  kornia is third party and not installed where this was written: parity at the image border is unpinned.
    - outlier_rejection (utils/outlier_rejection.py::mask_center_of_mass_outlier_rejection): per remaining id, the centre of mass, each pixel's
      distance to it, their mean and population std over the mask; pixels with d > mean + std_threshold * std are dropped (an empty mask stays
      empty).  The reference sums in float32 in an order of its own; here the moments are exact integers, the distances fp64 and their sum 2^-20
      fixed point, so the two agree except for pixels within rounding of the threshold.
    - masks with fewer than min_area pixels are dropped (this runs with num_openings == 0 too); dropped pixels get the background id.
    No host synchronisation; H, W <= 32768, H*W <= 2^28.  The input is not modified."""
    ops._check_gpu(instances)
    if instances.dim() != 2:
        raise ValueError("instances must be an [H, W] id image, got %s" % (tuple(instances.shape),))
    if instances.dtype not in _IDX:
        raise TypeError("instances must be int32 or int64, got %s" % instances.dtype)
    if int(num_openings) < 0:
        raise ValueError("num_openings %d < 0" % num_openings)
    H, W = instances.shape
    out = torch.empty((H, W), device=instances.device, dtype=instances.dtype)
    if H * W == 0:
        return out
    nbytes = int(L.load().pag_panoptic_clean_workspace_bytes(H, W))
    if nbytes == 0:
        raise ValueError("clean_instances: image %d x %d past the limits (H, W <= 32768, H*W <= 2^28)" % (H, W))
    ws = torch.empty(nbytes, device=instances.device, dtype=torch.uint8)
    ops._call("pag_panoptic_clean", instances.data_ptr(), _IDX[instances.dtype], H, W, instances.stride(0), instances.stride(1), int(num_openings),
              int(bool(outlier_rejection)), int(min_area), float(std_threshold), ws.data_ptr(), nbytes, out.data_ptr(), L.stream())
    return out


class MulticlassIoU:
    """The semantic IoU of pc_nerf/trainer.py:670-671 / :720 (torchmetrics JaccardIndex(task='multiclass', average='macro')): update(preds, target)
    adds to an int64 [C, C] confusion matrix (rows target, columns pred) on the device; compute() -> f32 0-d tensor, the mean over the classes of
    tp / (tp + fp + fn).

    torchmetrics is third party and not installed where this was written, so its semantics are stated as recalled and parity is unpinned:
    - classes with tp + fp + fn == 0 are left out of the mean (none present: nan);
    - target or pred values outside [0, C) are ignored (e.g. the unlabelled -1).  This differs on purpose from torchmetrics, which raises.
    preds and target are integer label tensors of one shape (class indices, not scores); no host synchronisation in update."""

    def __init__(self, num_classes, **kwargs):
        if int(num_classes) < 1 or int(num_classes) > 65536:
            raise ValueError("num_classes %r not in [1, 65536]" % (num_classes,))
        self.num_classes = int(num_classes)
        self.confmat = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64)

    @property
    def device(self):
        return self.confmat.device

    def to(self, device):
        self.confmat = self.confmat.to(device)
        return self

    def reset(self):
        self.confmat.zero_()

    def update(self, preds, target):
        ops._check_gpu(preds, target)
        if preds.shape != target.shape:
            raise ValueError("preds %s and target %s must have the same shape" % (tuple(preds.shape), tuple(target.shape)))
        if preds.device != target.device:
            raise ValueError("preds on %s, target on %s" % (preds.device, target.device))
        preds, target = _index(preds, "preds"), _index(target, "target")
        if preds.dim() > 4:
            preds, target = preds.reshape(-1), target.reshape(-1)
        if self.device != preds.device:
            self.to(preds.device)
        shape = (ctypes.c_int64 * 4)(*([1] * (4 - preds.dim()) + list(preds.shape)))
        ops._call("pag_confusion_matrix", preds.data_ptr(), _IDX[preds.dtype], _strides(preds), target.data_ptr(), _IDX[target.dtype], _strides(target),
                  shape, self.num_classes, self.confmat.data_ptr(), L.stream())

    def compute(self):
        return iou_from_confmat(self.confmat)


def iou_from_confmat(confmat):
    """Macro IoU of an int64 [C, C] confusion matrix (rows target, columns pred): f32 mean of tp / (tp + fp + fn) over the classes where that
    denominator is not 0."""
    tp = torch.diagonal(confmat)
    denom = confmat.sum(0) + confmat.sum(1) - tp
    iou = tp.float() / denom.clamp(min=1).float()
    present = (denom > 0).float()
    return (iou * present).sum() / present.sum()
