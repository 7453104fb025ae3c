"""CPU side of the validation row (pagnerf_amd/metrics.py: MaskMeanAveragePrecision, PeakSignalNoiseRatio, ValidationMetrics): an independent numpy
restatement of the mask mAP - per-id boolean masks and Python loops, no code shared with metrics.py - checked against cases small enough to work out
by hand; the PSNR against fp64 numpy; the column names; refusal of CPU tensors and of bad arguments; the workspace size.  The GPU tests compare the
device against the same restatement.

Case F of the hand cases (a tie between two ground truths that a second detection makes visible) cannot be built as an image: the masks of one
label image are disjoint, every threshold is >= 0.5, and IoU(d, g1) >= 0.5 and IoU(d, g2) >= 0.5 with g1, g2 disjoint force i1 = i2 = |d| / 2 and
|g1| = i1, |g2| = i2, i.e. d = g1 u g2 - so no second detection can overlap g2 at all, and which of the two was taken never shows in the result.  The
tie rule is therefore checked where it can be: on the restated matcher with a hand-made IoU matrix (later-wins differs from earlier-wins), and on
the one tie images allow (d = g1 u g2, IoU exactly 0.5 with both: matched at threshold 0 only)."""
import ctypes

import numpy as np
import pytest
import torch

THRESHOLDS = np.linspace(0.5, 0.95, 10)
RECALLS = np.linspace(0.0, 1.0, 101)


# ----------------------------------------------------------------------------------------------- numpy restatement: mask mAP
def np_iou_matrix(det_masks, gt_masks):
    iou = np.zeros((len(det_masks), len(gt_masks)), np.float64)
    for d, dm in enumerate(det_masks):
        for g, gm in enumerate(gt_masks):
            i = int(np.count_nonzero(dm & gm))
            if i > 0:
                iou[d, g] = np.float64(i) / np.float64(int(dm.sum()) + int(gm.sum()) - i)
    return iou


def np_match(iou, later_wins=True):
    """[D][10] matched flags of COCOeval's greedy matching; later_wins=False is the other tie rule (for the check that the two differ)."""
    D, G = iou.shape
    out = [[False] * len(THRESHOLDS) for _ in range(D)]
    for k, t in enumerate(THRESHOLDS):
        taken = [False] * G
        for d in range(D):
            best = min(t, 1 - 1e-10)
            m = -1
            for g in range(G):
                if taken[g]:
                    continue
                if iou[d, g] < best:
                    continue
                if not later_wins and m >= 0 and iou[d, g] == best:
                    continue
                best = iou[d, g]
                m = g
            if m >= 0:
                taken[m] = True
                out[d][k] = True
    return out


def np_map_update(pred, target, pred_raw=None, empty_detection_if_single_id=False, max_detections=100, later_wins=True):
    """One image -> (slot words [max_detections], number of ground truths)."""
    pred, target = np.asarray(pred), np.asarray(target)
    raw = pred if pred_raw is None else np.asarray(pred_raw)
    ids = sorted(int(v) for v in set(raw.reshape(-1).tolist()))
    det_masks = [pred == i for i in ids[1:][:max_detections]]
    if empty_detection_if_single_id and len(ids) == 1:
        det_masks = [np.zeros(pred.shape, bool)]
    gt_ids = sorted(int(v) for v in set(target.reshape(-1).tolist()))[1:]
    gt_masks = [target == i for i in gt_ids]
    matched = np_match(np_iou_matrix(det_masks, gt_masks), later_wins)
    words = [0] * max_detections
    for d in range(len(det_masks)):
        words[d] = 1
        for k in range(len(THRESHOLDS)):
            if matched[d][k]:
                words[d] |= 2 << k
    return words, len(gt_masks)


def np_map_compute(words, npig):
    """(map, map_50, map_75) in fp64 from the words of every update in order."""
    if npig == 0:
        return -1.0, -1.0, -1.0
    present = [w for w in words if w & 1]
    aps = []
    for k in range(len(THRESHOLDS)):
        tp = fp = 0
        rc, pr = [], []
        for w in present:
            if (w >> (1 + k)) & 1:
                tp += 1
            else:
                fp += 1
            rc.append(tp / npig)
            pr.append(tp / (tp + fp + np.spacing(1)))
        for i in range(len(pr) - 1, 0, -1):
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        q = []
        for r in RECALLS:
            idx = len(rc)
            for j, v in enumerate(rc):
                if v >= r:
                    idx = j
                    break
            q.append(pr[idx] if idx < len(pr) else 0.0)
        aps.append(float(np.mean(np.array(q, np.float64))))
    return float(np.mean(np.array(aps, np.float64))), aps[0], aps[5]


def np_map(updates, max_detections=100):
    """updates: [(pred, target, kwargs)] -> (all words, npig, (map, map_50, map_75))."""
    words, npig = [], 0
    for pred, target, kw in updates:
        w, g = np_map_update(pred, target, max_detections=max_detections, **kw)
        words += w
        npig += g
    return words, npig, np_map_compute(words, npig)


# ----------------------------------------------------------------------------------------------- the hand cases
def _img(fill=0):
    return np.full((16, 16), fill, np.int64)


def hand_cases():
    """name -> ([(pred, target, kwargs)], expected (map, map_50, map_75))."""
    cases = {}
    t = _img(); t[1:5, 1:5] = 1; t[8:12, 8:12] = 2
    p = _img(); p[1:5, 1:5] = 7
    cases["A"] = ([(p, t, {})], (51 / 101,) * 3)
    t = _img(); t[4:8, 4:8] = 1
    p = _img(); p[0:2, 0:2] = 1; p[4:8, 4:8] = 2
    cases["B"] = ([(p, t, {})], (0.5,) * 3)
    p = _img(); p[4:8, 4:6] = 5
    cases["C"] = ([(p, t, {})], (0.1, 1.0, 0.0))
    raw = _img(); raw[0, 0] = 1; raw[4:8, 4:8] = 2
    p = raw.copy(); p[0, 0] = 0
    cases["D_raw"] = ([(p, t, dict(pred_raw=raw))], (0.5,) * 3)
    cases["D_plain"] = ([(p, t, {})], (1.0,) * 3)
    p = _img(); p[4:8, 4:8] = 3
    te = t.copy(); te[15, 15] = -1
    cases["E"] = ([(p, te, {})], (51 / 101,) * 3)
    cases["G_none"] = ([(p, _img(), {})], (-1.0,) * 3)
    cases["G_fp_only"] = ([(p, _img(), {}), (p, t, {})], (0.5,) * 3)       # the first image's detection is a false positive ahead of the hit
    return cases


def tie_image():
    """The one tie label images allow: the detection is the union of two equal ground truths, IoU exactly 0.5 with both."""
    t = _img(); t[2:4, 2:6] = 1; t[4:6, 2:6] = 2
    p = _img(); p[2:6, 2:6] = 9
    return p, t


def blocky_case(seed, n_images=3, H=48, W=80):
    """The random case: targets of 8 x 8 blocks of 12 ids; the prediction is the target with a quarter of the blocks set to one random id each and
    15 % of the pixels set to random ids, all below 150 - more than 100 raw ids per image, so the detection cap is exercised."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n_images):
        cells = rs.randint(0, 12, size=(H // 8, W // 8))
        target = np.kron(cells, np.ones((8, 8), np.int64)).astype(np.int64)
        moved = np.where(rs.rand(H // 8, W // 8) < 0.25, rs.randint(0, 150, size=cells.shape), cells)
        pred = np.kron(moved, np.ones((8, 8), np.int64)).astype(np.int64)
        noise = rs.rand(H, W) < 0.15
        pred[noise] = rs.randint(0, 150, size=int(noise.sum()))
        out.append((pred, target, {}))
    return out


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(name):
    updates, want = hand_cases()[name]
    _, _, got = np_map(updates)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg=name)


def test_hand_case_details():
    cases = hand_cases()
    words, npig, _ = np_map(cases["C"][0])
    assert npig == 1 and words[0] == 1 | 2 and words[1:] == [0] * 99          # IoU exactly 0.5: matched at threshold 0 alone
    words, npig, _ = np_map(cases["D_raw"][0])
    assert words[:3] == [1, 0x7ff, 0] and npig == 1                           # the emptied detection stays, as a false positive
    words, npig, _ = np_map(cases["E"][0])
    assert npig == 2 and words[0] == 0x7ff                                    # -1 dropped, the background a ground truth
    words, npig, _ = np_map(cases["G_fp_only"][0])
    assert npig == 1 and words[0] == 1 and words[100] == 0x7ff


def test_tie_rule():
    # on the matcher: d0 ties between g0 and g1, d1 overlaps g1 alone.  Later-wins: d0 takes g1 and d1 goes empty-handed.
    iou = np.array([[0.6, 0.6], [0.0, 0.7]])
    later, earlier = np_match(iou, True), np_match(iou, False)
    assert later[0][0] and not later[1][0]
    assert earlier[0][0] and earlier[1][0]
    assert later != earlier
    # on an image: both rules give the same words (see the module docstring), matched at threshold 0 only
    p, t = tie_image()
    w_later, g = np_map_update(p, t)
    w_earlier, _ = np_map_update(p, t, later_wins=False)
    assert g == 2 and w_later[0] == 1 | 2 and w_later == w_earlier
    np.testing.assert_allclose(np_map_compute(w_later, g), (0.1 * 51 / 101, 51 / 101, 0.0), rtol=0, atol=1e-12)


def test_max_detections_and_empty_detection():
    p = _img(); p[0, :5] = [1, 2, 3, 4, 5]; p[4:8, 4:8] = 6
    t = _img(); t[4:8, 4:8] = 1
    words, g = np_map_update(p, t, max_detections=5)
    assert words == [1] * 5 and g == 1                                        # the hit is detection 6: past the cap
    words, g = np_map_update(p, t, max_detections=6)
    assert words == [1] * 5 + [0x7ff]
    one = _img(3)
    assert np_map_update(one, t)[0][0] == 0 and np_map_update(one, t, empty_detection_if_single_id=True)[0][:2] == [1, 0]


def test_blocky_case_is_meaningful():
    words, npig, (m, m50, m75) = np_map(blocky_case(5))
    for pred, _, _ in blocky_case(5):
        assert len(np.unique(pred)) > 101
    assert 0 < m < m50 < 1
    present = [w for w in words if w & 1]
    assert sum((w >> 1) & 1 for w in present) != sum((w >> 10) & 1 for w in present)


def test_compute_matches_restatement():
    from pagnerf_amd.metrics import _ap_from_slots
    rs = np.random.RandomState(0)
    for n, npig in ((0, 3), (1, 1), (250, 40), (1000, 700)):
        words = [int(v) for v in (rs.randint(0, 1 << 10, size=n) << 1 | (rs.rand(n) < 0.8))]
        np.testing.assert_allclose(_ap_from_slots(np.array(words, np.int32), npig), np_map_compute(words, npig), rtol=0, atol=1e-12)
    assert _ap_from_slots(np.array([2047], np.int32), 0) == (-1.0, -1.0, -1.0)
    words, npig, want = np_map(blocky_case(5))
    np.testing.assert_allclose(_ap_from_slots(np.array(words, np.int32), npig), want, rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------------------------- PSNR
def np_psnr(pairs):
    """fp64 PSNR over (preds, target) float arrays with torchmetrics' data_range=None rule: the target range starts at [0, 0]."""
    sse, n, lo, hi = 0.0, 0, 0.0, 0.0
    for p, t in pairs:
        p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
        sse += float(((p - t) ** 2).sum())
        n += t.size
        lo, hi = min(lo, float(t.min())), max(hi, float(t.max()))
    return 10.0 * np.log10((hi - lo) ** 2 / (sse / n))


@pytest.mark.parametrize("shape", [(7, 5, 3), (37, 129, 3)])
def test_psnr_against_fp64(shape):
    from pagnerf_amd.metrics import PeakSignalNoiseRatio
    rs = np.random.RandomState(1)
    m = PeakSignalNoiseRatio()
    pairs = []
    for _ in range(2):
        t = rs.rand(*shape).astype(np.float32)
        p = np.clip(t + 0.05 * rs.randn(*shape), 0, 1).astype(np.float32)
        m.update(torch.from_numpy(p), torch.from_numpy(t))
        pairs.append((p, t))
    out = m.compute()
    assert out.dtype == torch.float32 and out.dim() == 0
    assert m.sum_squared_error.dtype == torch.float64 and m.total.dtype == torch.int64 and int(m.total) == 2 * int(np.prod(shape))
    assert abs(float(out) - np_psnr(pairs)) <= 1e-4
    m.reset()
    assert int(m.total) == 0 and float(m.sum_squared_error) == 0.0 and float(m.max_target) == 0.0


def test_psnr_views_uint8_and_range():
    from pagnerf_amd.metrics import PeakSignalNoiseRatio
    rs = np.random.RandomState(2)
    t4 = rs.rand(37, 129, 4).astype(np.float32)
    p = rs.rand(37, 129, 3).astype(np.float32)
    m = PeakSignalNoiseRatio()
    m.update(torch.from_numpy(p), torch.from_numpy(t4)[..., :3])                   # strided view of a four-channel target
    assert abs(float(m.compute()) - np_psnr([(p, t4[..., :3])])) <= 1e-4
    u8 = rs.randint(0, 256, size=(37, 129, 4)).astype(np.uint8)
    m = PeakSignalNoiseRatio()
    m.update(torch.from_numpy(p), torch.from_numpy(u8)[..., :3])
    assert abs(float(m.compute()) - np_psnr([(p, u8[..., :3].astype(np.float64) / 255.0)])) <= 1e-4
    t = (0.2 + 0.4 * rs.rand(7, 5, 3)).astype(np.float32)
    t[0, 0, 0], t[1, 1, 1] = 0.2, 0.6
    m = PeakSignalNoiseRatio()
    m.update(torch.from_numpy(p[:7, :5]), torch.from_numpy(t))
    assert float(m.min_target) == 0.0 and float(m.max_target) == np.float32(0.6)   # the range is 0.6, not 0.4
    assert abs(float(m.compute()) - np_psnr([(p[:7, :5], t)])) <= 1e-4
    with pytest.raises(ValueError, match="same shape"):
        m.update(torch.zeros(3, 3), torch.zeros(3, 4))


# ----------------------------------------------------------------------------------------------- evaluator, refusals, entry points
BASE_KEYS = {"val/psnr", "val/iou", "val/map_", "val/map_50_", "val/map_75_"} | {"val/%s_%s" % (m, g) for m in ("pq", "rq", "sq")
                                                                                 for g in ("all", "things", "stuff")}
PRED_KEYS = {"val/iou_pred", "val/map__pred", "val/map_50__pred", "val/map_75__pred", "val/iou_gain", "val/pq_things_gain"} | {
    "val/%s_%s_pred" % (m, g) for m in ("pq", "rq", "sq") for g in ("all", "things", "stuff")}


def test_validation_metrics_keys():
    from pagnerf_amd.metrics import ValidationMetrics
    ev = ValidationMetrics(6, [1, 2, 3, 4], [0, 5])
    assert ev.inst_num_dilations == -1 and ev.inst_outlier_rejection is False and ev.predict_clusters is None
    out = ev.compute()
    assert set(out) == BASE_KEYS
    assert all(isinstance(v, float) for v in out.values())
    assert out["val/map_"] == -1.0
    ev.seen_pred = True
    assert set(ev.compute()) == BASE_KEYS | PRED_KEYS
    ev.reset()
    assert set(ev.compute()) == BASE_KEYS


def test_cpu_tensors_refused():
    from pagnerf_amd import MaskMeanAveragePrecision, PeakSignalNoiseRatio, RenderBuffer, ValidationMetrics    # noqa: F401  (the exports)
    x = torch.zeros(4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        MaskMeanAveragePrecision().update(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        MaskMeanAveragePrecision().update(x, x, pred_raw=x)
    rb = RenderBuffer(rgb=torch.zeros(4, 4, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        ValidationMetrics(3, [1], [0]).update(rb, torch.zeros(4, 4, 3))
    with pytest.raises(ValueError, match="max_detections"):
        MaskMeanAveragePrecision(max_detections=0)
    m = MaskMeanAveragePrecision(max_detections=7)
    assert m.slots.dtype == torch.int32 and m.npig.dtype == torch.int64 and m.to("cpu") is m
    assert m.compute_fp64() == {"map": -1.0, "map_50": -1.0, "map_75": -1.0}
    out = m.compute()
    assert out["map"].dtype == torch.float32 and out["map"].dim() == 0 and float(out["map_75"]) == -1.0


def test_workspace_bytes():
    from pagnerf_amd import _lib
    lib = _lib.load()
    n = lib.pag_mask_ap_workspace_bytes(720, 1280, 100)
    assert 0 < n <= 16 << 20
    assert n == lib.pag_mask_ap_workspace_bytes(64, 64, 100)
    assert lib.pag_mask_ap_workspace_bytes(720, 1280, 200) > n
    for bad in ((0, 5, 100), (5, 0, 100), (1 << 14, (1 << 14) + 1, 100), (4, 4, 0), (4, 4, 4097)):
        assert lib.pag_mask_ap_workspace_bytes(*bad) == 0, bad


def test_entry_point_rejects_bad_arguments():
    """Every refusal comes before any launch, so it needs no GPU; the pointers are never dereferenced."""
    from pagnerf_amd import _lib
    lib = _lib.load()
    thr = (ctypes.c_double * 10)(*THRESHOLDS.tolist())
    ws_bytes = lib.pag_mask_ap_workspace_bytes(4, 4, 100)
    P = 4096            # a non-NULL address

    def call(pred=P, pred_dtype=_lib.I64, raw=P, raw_dtype=_lib.I64, target=P, target_dtype=_lib.I32, H=4, W=4, md=100, thresholds=thr, ws=P,
             nbytes=ws_bytes, slots=P, npig=P, flags=P):
        return lib.pag_mask_ap_update(pred, pred_dtype, W, 1, raw, raw_dtype, W, 1, target, target_dtype, W, 1, H, W, md, 0, thresholds, ws, nbytes,
                                      slots, npig, flags, None)

    for kw in (dict(pred=None), dict(raw=None), dict(target=None), dict(thresholds=None), dict(ws=None), dict(slots=None), dict(npig=None),
               dict(flags=None), dict(pred_dtype=_lib.F32), dict(raw_dtype=7), dict(target_dtype=_lib.BF16), dict(H=0), dict(W=0),
               dict(H=1 << 14, W=(1 << 14) + 1), dict(md=0), dict(md=4097), dict(nbytes=ws_bytes - 1)):
        assert call(**kw) != 0, kw
        assert b"pag_mask_ap_update" in lib.pag_last_error_string()
