"""Panoptic evaluation of validation images on the GPU - utils/metrics/panoptic_quality{,_func}.py (PanopticQuality, panoptic_quality), the instance
cleanup of pc_nerf/trainer.py:750-772 and the semantic IoU of :670-671 / :720, on pag_panoptic_pq_update / pag_panoptic_clean / pag_confusion_matrix
(csrc/panoptic.hip).

The reference's PQ loops in Python over every (pred, target) segment pair with a host round trip per pair, and its cleanup builds one int64 [K, H, W]
mask per instance id (about 1.5 GB at 720 x 1280 with 200 ids).  Here `update`, `clean_instances` and `MulticlassIoU.update` are a few device passes
over O(B H W) workspace with no host synchronisation (PanopticQuality.update with allow_unknown_preds_category=False reads one flag back, as the
reference's check needs), so they can be captured in a graph; `compute()` reads the small per-category state back once.

Inputs must be device tensors (the project has no CPU fallback) and are never modified.  Divergence: for B > 1 the reference adds the batch offsets of
_make_instance_ids_batch_unique into the caller's preds and target in place; here the caller's tensors stay as they are.

The other two figures of the reference's validation row (trainer.py:651-941 evaluate_metrics) and the row itself: MaskMeanAveragePrecision, the mask
mAP of :674-675 / :794-798 from label images on pag_mask_ap_update (no [K, H, W] mask stack, no host run-length encoding); PeakSignalNoiseRatio
(:677, :708) in tensor ops; ValidationMetrics, which feeds the five metrics one image at a time as :684-843 does and names the columns as :898-934.
"""
import ctypes
import math
from collections.abc import Set

import numpy as np
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


# ------------------------------------------------------------------------------------------------- mask mAP
AP_THRESHOLDS = np.linspace(0.5, 0.95, 10)
AP_RECALLS = np.linspace(0.0, 1.0, 101)
MAX_MASK_IDS = 4096
_AP_FLAG_IDS = 1
_AP_FLAG_PRED_ID = 2


def _ap_from_slots(words, npig):
    """(map, map_50, map_75) in fp64 from the slot words of every update in order and the ground-truth count: COCOeval's accumulate for one class,
    every score equal (so the stable sort keeps the state order) and no ignored ground truth."""
    if npig == 0:
        return -1.0, -1.0, -1.0
    words = np.asarray(words, dtype=np.int64)
    words = words[(words & 1) != 0]
    aps = []
    for k in range(len(AP_THRESHOLDS)):
        matched = ((words >> (1 + k)) & 1) != 0
        tp = np.cumsum(matched).astype(np.float64)
        fp = np.cumsum(~matched).astype(np.float64)
        rc = tp / npig
        pr = tp / (tp + fp + np.spacing(1))
        pr = np.maximum.accumulate(pr[::-1])[::-1]              # non-increasing from the right
        inds = np.searchsorted(rc, AP_RECALLS, side="left")
        q = np.zeros(len(AP_RECALLS), np.float64)
        ok = inds < len(pr)
        q[ok] = pr[inds[ok]]
        aps.append(np.mean(q))
    return float(np.mean(aps)), float(aps[0]), float(aps[5])


class MaskMeanAveragePrecision:
    """The mask mAP of pc_nerf/trainer.py:674-675, :794-798, :839-843 (torchmetrics MeanAveragePrecision(iou_type="segm")) for the one way the trainer
    uses it - a single class, every score 1.0 - with the masks given as label images, on pag_mask_ap_update (csrc/panoptic.hip).

    MaskMeanAveragePrecision(max_detections=100); update(pred, target, pred_raw=None, empty_detection_if_single_id=False) with [H, W] int32 / int64
    device tensors of any strides (never modified); compute() -> {'map', 'map_50', 'map_75'} f32 0-d tensors on the state's device; reset();
    to(device) returns self.

    The reference stacks one [K, H, W] mask per id (1.47 GB as int64 at 720 x 1280 with 200 ids) and hands the stack to pycocotools, which
    run-length-encodes every mask on the host.  The masks of one label image are disjoint, so the areas and pairwise intersection counts of the two
    label images carry the same information: two pixel passes and a matching kernel over a workspace that does not grow with the image, no host
    synchronisation in update.

    torchmetrics and pycocotools are third party and not installed where this was written: the definition below is recalled from COCOeval and is
    this project's definition of record; parity is unpinned.
    - Detections of one update: the distinct ids of pred_raw (default pred) in ascending order without the smallest (mask_ids[1:], :753-755), the
      first max_detections of them (all scores tie and COCOeval's sort is stable).  The mask of a detection is the pixels of pred with its id: pred
      is the cleaned image, clean_instances only moves pixels to the smallest id, and a detection that lost every pixel stays a detection of area
      0 (:766-767 keeps zeroed masks).  empty_detection_if_single_id: a pred_raw of one distinct id gives one empty detection (:780-781).
    - Ground truths: the distinct ids of target without the smallest, whatever it is - in a partly labelled frame that holds -1, the -1 is dropped
      and 0 becomes a mask (gt_ids[1:], :791-792).  None is ignored, none is crowd.
    - IoU = double(i) / double(a_d + a_g - i) of exact integer counts when i > 0, else 0.
    - Matching, independently for each threshold of np.linspace(0.5, 0.95, 10), detections in order: the not yet matched ground truth of the
      largest IoU >= min(t, 1 - 1e-10), the later one on a tie.
    - State: max_detections int32 slot words per update in update order (bit 0 present, bit 1 + k matched at threshold k; 0 for a missing
      detection), the int64 ground-truth count npig and an int32 flag word.  The slot buffer grows on the host by doubling.
    - compute() reads the state back once and runs COCOeval's accumulate in numpy fp64: per threshold tp / fp cumulative sums over the present
      detections, precision tp / (tp + fp + eps) made non-increasing from the right, sampled at the 101 recalls np.linspace(0, 1, 101) (0 past the
      last recall), averaged; map is the mean over the thresholds, map_50 / map_75 thresholds 0 / 5; all -1 without a ground truth; rounded to
      f32 last.  compute_fp64() gives the same three as Python floats before that rounding.
    More than 4096 distinct ids in pred_raw or target, or an id of pred that pred_raw lacks, sets a device flag and drops that update; compute()
    then raises ValueError.  H*W <= 2^28, max_detections <= 4096."""

    def __init__(self, max_detections=100, **kwargs):
        if int(max_detections) < 1 or int(max_detections) > MAX_MASK_IDS:
            raise ValueError("max_detections %r not in [1, %d]" % (max_detections, MAX_MASK_IDS))
        self.max_detections = int(max_detections)
        self.slots = torch.zeros(4 * self.max_detections, dtype=torch.int32)
        self.npig = torch.zeros(1, dtype=torch.int64)
        self._flags = torch.zeros(1, dtype=torch.int32)
        self.num_updates = 0
        self._thresholds = (ctypes.c_double * len(AP_THRESHOLDS))(*AP_THRESHOLDS.tolist())

    _STATE = ("slots", "npig", "_flags")

    @property
    def device(self):
        return self.slots.device

    def to(self, device):
        for name in self._STATE:
            setattr(self, name, getattr(self, name).to(device))
        return self

    def reset(self):
        for name in self._STATE:
            getattr(self, name).zero_()
        self.num_updates = 0

    def update(self, pred, target, pred_raw=None, empty_detection_if_single_id=False):
        raw = pred if pred_raw is None else pred_raw
        ops._check_gpu(pred, target, raw)
        for t, what in ((pred, "pred"), (target, "target"), (raw, "pred_raw")):
            if t.dim() != 2:
                raise ValueError("%s must be an [H, W] id image, got %s" % (what, tuple(t.shape)))
            if t.dtype not in _IDX:
                raise TypeError("%s must be int32 or int64, got %s" % (what, t.dtype))
            if t.shape != pred.shape or t.device != pred.device:
                raise ValueError("%s %s on %s, pred %s on %s" % (what, tuple(t.shape), t.device, tuple(pred.shape), pred.device))
        if self.device != pred.device:
            self.to(pred.device)
        H, W = pred.shape
        if H * W == 0:
            return
        nbytes = int(L.load().pag_mask_ap_workspace_bytes(H, W, self.max_detections))
        if nbytes == 0:
            raise ValueError("MaskMeanAveragePrecision.update: %d pixels > 2^28" % (H * W))
        md = self.max_detections
        if (self.num_updates + 1) * md > self.slots.numel():
            grown = torch.zeros(2 * self.slots.numel(), device=self.device, dtype=torch.int32)
            grown[:self.slots.numel()] = self.slots
            self.slots = grown
        ws = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
        ops._call("pag_mask_ap_update", pred.data_ptr(), _IDX[pred.dtype], pred.stride(0), pred.stride(1), raw.data_ptr(), _IDX[raw.dtype], raw.stride(0),
                  raw.stride(1), target.data_ptr(), _IDX[target.dtype], target.stride(0), target.stride(1), H, W, md,
                  int(bool(empty_detection_if_single_id)), self._thresholds, ws.data_ptr(), nbytes,
                  self.slots.data_ptr() + 4 * self.num_updates * md, self.npig.data_ptr(), self._flags.data_ptr(), L.stream())
        self.num_updates += 1

    def compute_fp64(self):
        flags = int(self._flags[0])
        if flags & _AP_FLAG_IDS:
            raise ValueError("MaskMeanAveragePrecision: an update had more than %d distinct ids (or the id -2^63)" % MAX_MASK_IDS)
        if flags & _AP_FLAG_PRED_ID:
            raise ValueError("MaskMeanAveragePrecision: pred held an id that pred_raw lacks")
        words = self.slots[:self.num_updates * self.max_detections].cpu().numpy()
        return dict(zip(("map", "map_50", "map_75"), _ap_from_slots(words, int(self.npig[0]))))

    def compute(self):
        return {k: torch.tensor(v, dtype=torch.float32, device=self.device) for k, v in self.compute_fp64().items()}


# ------------------------------------------------------------------------------------------------- PSNR
class PeakSignalNoiseRatio:
    """torchmetrics.PeakSignalNoiseRatio() as pc_nerf/trainer.py:677, :708, :900 uses it (data_range=None), in tensor ops; recalled, parity unpinned.

    States: sum_squared_error f64, total i64, min_target / max_target f32, both starting at 0.0 - so the range of all-positive images is max - 0.
    update(preds, target): one shape, any strides (e.g. gts[..., :3]); a uint8 target is converted with dataset._u8_table; d = preds.float() -
    target, squared in f32 and summed in f64; total += numel; min and max of target folded in; no host synchronisation.  compute(): with r =
    max_target - min_target, (2 log r - log(sse / total)) * 10 / log 10, logarithms in f32, as an f32 0-d tensor.
    Divergence: the reference accumulates the squared error in f32."""

    def __init__(self, **kwargs):
        self.sum_squared_error = torch.zeros((), dtype=torch.float64)
        self.total = torch.zeros((), dtype=torch.int64)
        self.min_target = torch.zeros((), dtype=torch.float32)
        self.max_target = torch.zeros((), dtype=torch.float32)

    _STATE = ("sum_squared_error", "total", "min_target", "max_target")

    @property
    def device(self):
        return self.sum_squared_error.device

    def to(self, device):
        for name in self._STATE:
            setattr(self, name, getattr(self, name).to(device))
        return self

    def reset(self):
        for name in self._STATE:
            getattr(self, name).zero_()

    def update(self, preds, target):
        if preds.shape != target.shape:
            raise ValueError("preds %s and target %s must have the same shape" % (tuple(preds.shape), tuple(target.shape)))
        if preds.device != target.device:
            raise ValueError("preds on %s, target on %s" % (preds.device, target.device))
        if target.numel() == 0:
            return
        if self.device != preds.device:
            self.to(preds.device)
        if target.dtype == torch.uint8:
            from .dataset import _u8_table
            target = _u8_table(target.device)[target.long()]
        target = target.float()
        d = preds.float() - target
        self.sum_squared_error += (d * d).sum(dtype=torch.float64)
        self.total += target.numel()
        self.min_target = torch.minimum(self.min_target, target.min())
        self.max_target = torch.maximum(self.max_target, target.max())

    def compute(self):
        r = self.max_target - self.min_target
        mse = (self.sum_squared_error / self.total).float()
        return (2.0 * torch.log(r) - torch.log(mse)) * (10.0 / math.log(10.0))


# ------------------------------------------------------------------------------------------------- the validation row
class ValidationMetrics:
    """The metric half of PanopticTrainer.evaluate_metrics (pc_nerf/trainer.py:684-843, :898-934), one image per update: PSNR, semantic IoU,
    panoptic quality and mask mAP of the render, and the same for the network predictions the dataset may carry (`_pred`).  Pictures, videos, the
    pickles, the CSV row and TensorBoard are the caller's.

    ValidationMetrics(num_classes, things_ids, stuff_ids, inst_num_dilations=-1, inst_outlier_rejection=False, predict_clusters=None) - the
    defaults of config_parser.py:331, :401; predict_clusters is the contrastive NeFs' clustering (:738), else argmax.
    update(rb, gts, sem_gts=None, inst_gts=None, sem_pred=None, inst_pred=None, labelled=None), rb a RenderBuffer reshaped to [H, W, .]:
    - PSNR of rb.rgb[..., :3] against gts[..., :3], always (:708);
    - with rb.semantics and sem_gts: semantics = argmax; the IoU is updated when the frame is labelled, and a second IoU from sem_pred (:715-729);
    - with rb.inst_embedding and inst_gts: instances = predict_clusters(rb.inst_embedding) or argmax, inst_conf = max, then
      clean_instances(instances, max(0, inst_num_dilations), inst_outlier_rejection, min_area=100) (:738-772); when both label images are
      labelled, PanopticQuality(allow_unknown_preds_category=True) of (semantics, cleaned) against (sem_gts, inst_gts) and
      MaskMeanAveragePrecision.update(cleaned, inst_gts, pred_raw=instances, empty_detection_if_single_id=True) (:784-798); with sem_pred and
      inst_pred the `_pred` pair from them, without cleaning and without the empty detection (:808-843).
    "Labelled" is the reference's `not torch.all(x == -1)`: labelled=(semantics, instances) from the caller (the dataset knows which frames carry
    labels) makes update free of host synchronisation; labelled=None reads one two-element flag tensor back.
    update returns {'semantics', 'instances', 'inst_conf'}: the label images and the confidence that save_preds pickles (:844-853), device tensors
    (None where the channel or its labels were not given).
    compute() -> Python floats under the reference's column names, quirks included: val/psnr, val/iou, val/map_, val/map_50_, val/map_75_,
    val/{pq,rq,sq}_{all,things,stuff}; once a `_pred` input was seen also val/map__pred, val/map_50__pred, val/map_75__pred, val/iou_pred,
    val/{pq,rq,sq}_{all,things,stuff}_pred, val/iou_gain and val/pq_things_gain (:908-934).
    Divergence: the reference always emits the `_pred` columns and gains, from metrics that never saw an update."""

    def __init__(self, num_classes, things_ids, stuff_ids, inst_num_dilations=-1, inst_outlier_rejection=False, predict_clusters=None):
        things, stuff = set(int(c) for c in things_ids), set(int(c) for c in stuff_ids)
        self.inst_num_dilations = int(inst_num_dilations)
        self.inst_outlier_rejection = bool(inst_outlier_rejection)
        self.predict_clusters = predict_clusters
        self.psnr = PeakSignalNoiseRatio()
        self.iou, self.iou_pred = MulticlassIoU(num_classes), MulticlassIoU(num_classes)
        self.pq = PanopticQuality(things, stuff, allow_unknown_preds_category=True)
        self.pq_pred = PanopticQuality(things, stuff, allow_unknown_preds_category=True)
        self.map, self.map_pred = MaskMeanAveragePrecision(), MaskMeanAveragePrecision()
        self.seen_pred = False

    def _metrics(self):
        return (self.psnr, self.iou, self.iou_pred, self.pq, self.pq_pred, self.map, self.map_pred)

    def to(self, device):
        for m in self._metrics():
            m.to(device)
        return self

    def reset(self):
        for m in self._metrics():
            m.reset()
        self.seen_pred = False

    def update(self, rb, gts, sem_gts=None, inst_gts=None, sem_pred=None, inst_pred=None, labelled=None):
        rgb, sem, emb = rb.rgb, getattr(rb, "semantics", None), getattr(rb, "inst_embedding", None)
        ops._check_gpu(rgb, gts, sem, emb, sem_gts, inst_gts, sem_pred, inst_pred)
        self.psnr.update(rgb[..., :3], gts[..., :3])
        if labelled is not None:
            sem_l, inst_l = bool(labelled[0]), bool(labelled[1])
        else:
            no = torch.zeros((), dtype=torch.bool, device=rgb.device)
            sem_l, inst_l = torch.stack([no if x is None else (x != -1).any() for x in (sem_gts, inst_gts)]).tolist()
        out = dict(semantics=None, instances=None, inst_conf=None)
        semantics = None
        if sem is not None and sem_gts is not None:
            semantics = torch.argmax(sem, dim=-1)
            out["semantics"] = semantics
            if sem_l:
                self.iou.update(semantics, sem_gts)
            if sem_pred is not None:
                self.seen_pred = True
                if sem_l:
                    self.iou_pred.update(sem_pred, sem_gts)
        if emb is not None and inst_gts is not None:
            instances = self.predict_clusters(emb) if self.predict_clusters is not None else torch.argmax(emb, dim=-1)
            if instances.dtype not in _IDX:
                instances = instances.long()
            out["inst_conf"] = torch.max(emb, dim=-1)[0]
            cleaned = clean_instances(instances, num_openings=max(0, self.inst_num_dilations), outlier_rejection=self.inst_outlier_rejection,
                                      min_area=100)
            out["instances"] = cleaned
            both = sem_l and inst_l
            if both and semantics is None:
                raise ValueError("ValidationMetrics.update: the panoptic quality needs rb.semantics and sem_gts beside the instances")
            gt_ids = inst_gts if inst_gts.dtype in _IDX else inst_gts.long()
            if both:
                labels = torch.stack((sem_gts.long(), gt_ids.long()))[None]
                self.pq.update(torch.stack((semantics, cleaned.long()))[None], labels)
                self.map.update(cleaned, gt_ids, pred_raw=instances, empty_detection_if_single_id=True)
            if sem_pred is not None and inst_pred is not None:
                self.seen_pred = True
                if both:
                    self.pq_pred.update(torch.stack((sem_pred.long(), inst_pred.long()))[None], labels)
                    self.map_pred.update(inst_pred if inst_pred.dtype in _IDX else inst_pred.long(), gt_ids)
        return out

    def compute(self):
        out = {"val/psnr": self.psnr.compute().item()}
        suffixes = ("", "_pred") if self.seen_pred else ("",)
        ious = [m.compute() for m in (self.iou, self.iou_pred)]
        pqs = [m.compute() for m in (self.pq, self.pq_pred)]
        if self.seen_pred:
            out["val/iou_gain"] = (ious[0] - ious[1]).item()
            out["val/pq_things_gain"] = (pqs[0]["things"]["pq"] - pqs[1]["things"]["pq"]).item()
        for m, suffix in zip((self.map, self.map_pred), suffixes):
            for metric, v in m.compute().items():
                out["val/%s_%s" % (metric, suffix)] = v.item()
        for v, suffix in zip(ious, suffixes):
            out["val/iou%s" % suffix] = v.item()
        for res, suffix in zip(pqs, suffixes):
            for group in res:
                for metric in ("pq", "rq", "sq"):
                    out["val/%s_%s%s" % (metric, group, suffix)] = res[group][metric].item()
        return out
