"""CPU side of the panoptic evaluation (pagnerf_amd/metrics.py): a numpy restatement of the reference's PQ update / compute, of the trainer's instance
cleanup and of the macro IoU, pinned to g13_panoptic.npz (made from the reference by tests/golden/make_golden_panoptic.py); refusal of CPU tensors, the
reference's validation errors and the set-order category mapping.  The GPU tests compare the device against the same restatement."""
import numpy as np
import pytest
import torch

from conftest import golden


# ----------------------------------------------------------------------------------------------- synthetic label images
def blocky(rs, H, W, cell, values):
    """[H, W] image of random `values` on a grid of cell x cell blocks, cut to H x W."""
    h, w = -(-H // cell), -(-W // cell)
    return np.kron(rs.choice(values, size=(h, w)), np.ones((cell, cell), dtype=np.int64))[:H, :W].astype(np.int64)


def synth_panoptic(rs, B, H, W, things, stuff, n_inst, cell=8, flip=0.05, extra_cats=()):
    """(pred, target) [B, 2, H, W] int64: block-structured semantics and instance ids; the prediction flips a fraction of the blocks' labels and
    ids and sprinkles single-pixel noise."""
    cats = sorted(things) + sorted(stuff) + list(extra_cats)
    target = np.zeros((B, 2, H, W), np.int64)
    for b in range(B):
        target[b, 0] = blocky(rs, H, W, cell, cats)
        target[b, 1] = blocky(rs, H, W, cell, np.arange(n_inst))
    pred = target.copy()
    for b in range(B):
        m = blocky(rs, H, W, cell, [0, 1]) & (rs.rand(H, W) < 2 * flip)
        pred[b, 0][m.astype(bool)] = rs.choice(cats, size=int(m.sum()))
        m2 = rs.rand(H, W) < flip
        pred[b, 1][m2] = rs.randint(0, 2 * n_inst, size=int(m2.sum()))
        m3 = rs.rand(H, W) < flip / 4
        pred[b, 0][m3] = rs.choice(cats, size=int(m3.sum()))
    return pred, target


def synth_ids(rs, H, W, ids, cell=8, noise=0.02):
    img = blocky(rs, H, W, cell, ids)
    m = rs.rand(H, W) < noise
    img[m] = rs.choice(ids, size=int(m.sum()))
    return img


# ----------------------------------------------------------------------------------------------- numpy restatement: PQ
def cont_ids(things, stuff):
    d = {c: i for i, c in enumerate(things)}
    d.update({c: i + len(things) for i, c in enumerate(stuff)})
    return d


def np_preprocess(img, things, stuff, void):
    img = np.array(img, dtype=np.int64, copy=True)
    for b in range(img.shape[0] - 1):
        img[b + 1, 1] += img[b, 1].max()
    flat = np.moveaxis(img, 1, -1).reshape(-1, 2).copy()
    st = np.isin(flat[:, 0], list(stuff))
    th = np.isin(flat[:, 0], list(things))
    flat[st, 1] = 0
    unknown = ~(st | th)
    flat[unknown] = void
    return flat, bool(unknown.any())


def _areas(rows):
    keys, counts = np.unique(rows, axis=0, return_counts=True)
    return {tuple(int(v) for v in k): int(c) for k, c in zip(keys, counts)}


def np_pq_update(preds, target, things, stuff):
    """(iou_sum f64, tp, fp, fn i32) of one update; pairs visited in ascending (pred_cat, pred_inst, tgt_cat, tgt_inst) order, IoUs float32,
    summed sequentially in float64 - the reference's arithmetic."""
    void = (1 + max([0] + list(things) + list(stuff)), 0)
    cid = cont_ids(things, stuff)
    fp_, _ = np_preprocess(preds, things, stuff, void)
    ft_, _ = np_preprocess(target, things, stuff, void)
    n = len(cid)
    iou_sum = np.zeros(n, np.float64)
    tp, fp, fn = (np.zeros(n, np.int32) for _ in range(3))
    pa, ta = _areas(fp_), _areas(ft_)
    inter = _areas(np.concatenate([fp_, ft_], axis=1))
    mp, mt = set(), set()
    for k, c in inter.items():
        p, t = k[:2], k[2:]
        if t == void or p[0] != t[0]:
            continue
        u = pa[p] - inter.get(p + void, 0) + ta[t] - inter.get(void + t, 0) - c
        iou = np.float32(c) / np.float32(u)
        if iou > 0.5:
            mp.add(p)
            mt.add(t)
            iou_sum[cid[p[0]]] += np.float64(iou)
            tp[cid[p[0]]] += 1
    for t in set(ta) - mt - {void}:
        if not np.float32(inter.get(void + t, 0)) / np.float32(ta[t]) > 0.5:
            fn[cid[t[0]]] += 1
    for p in set(pa) - mp - {void}:
        if not np.float32(inter.get(p + void, 0)) / np.float32(pa[p]) > 0.5:
            fp[cid[p[0]]] += 1
    return iou_sum, tp, fp, fn


def np_pq_compute(n_things, n_stuff, iou_sum, tp, fp, fn):
    from pagnerf_amd.metrics import _pq_compute
    return _pq_compute(n_things, n_stuff, torch.from_numpy(iou_sum), torch.from_numpy(tp), torch.from_numpy(fp), torch.from_numpy(fn))


# ----------------------------------------------------------------------------------------------- numpy restatement: cleanup
def np_opening(lab, bg):
    """One flat 3x3 opening of every non-background id (geodesic borders) -> keep mask."""
    H, W = lab.shape
    pad = np.pad(lab, 1, mode="edge")                  # edge copies are in-image neighbours already: only in-image pixels are compared
    er = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            er &= pad[dy:dy + H, dx:dx + W] == lab
    pe, pl = np.pad(er, 1), np.pad(lab, 1, mode="edge")
    keep = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            keep |= pe[dy:dy + H, dx:dx + W] & (pl[dy:dy + H, dx:dx + W] == lab)
    return keep & (lab != bg)


def np_outliers(lab, keep, std_threshold):
    out = keep.copy()
    for v in np.unique(lab[keep]):
        ys, xs = np.nonzero(keep & (lab == v))
        cy, cx = ys.mean(), xs.mean()
        d = np.sqrt((ys - cy) ** 2 + (xs - cx) ** 2)
        thr = d.mean() + std_threshold * d.std()
        out[ys[d > thr], xs[d > thr]] = False
    return out


def np_clean(ids, num_openings=1, outlier_rejection=False, min_area=100, std_threshold=2.0):
    ids = np.asarray(ids)
    u = np.unique(ids)
    if u.size <= 1:
        return ids.copy()
    bg = u[0]
    lab = ids.copy()
    keep = lab != bg
    for _ in range(num_openings):
        keep = np_opening(lab, bg)
        lab = np.where(keep, ids, bg)
    if outlier_rejection:
        keep = np_outliers(lab, keep, std_threshold)
    vals, counts = np.unique(ids[keep], return_counts=True)
    small = vals[counts < min_area]
    keep &= ~np.isin(ids, small)
    return np.where(keep, ids, bg).astype(ids.dtype)


def np_iou(preds, target, C):
    p, t = np.asarray(preds).reshape(-1), np.asarray(target).reshape(-1)
    ok = (p >= 0) & (p < C) & (t >= 0) & (t < C)
    cm = np.bincount(t[ok] * C + p[ok], minlength=C * C).reshape(C, C)
    tp = np.diag(cm)
    den = cm.sum(0) + cm.sum(1) - tp
    return cm, float(np.mean(tp[den > 0] / den[den > 0])) if (den > 0).any() else float("nan")


# ----------------------------------------------------------------------------------------------- fixture access
def pq_case(g, n):
    things = set(int(v) for v in g[n + "/things"])
    stuff = set(int(v) for v in g[n + "/stuff"])
    updates = [(g["%s/preds%d" % (n, i)], g["%s/target%d" % (n, i)]) for i in range(int(g[n + "/n_updates"]))]
    return things, stuff, updates


def pq_names(g):
    return [str(v) for v in g["pq_names"]]


def clean_names(g):
    return [str(v) for v in g["clean_names"]]


def clean_args(g, n):
    a = g[n + "/args"]
    return dict(num_openings=int(a[0]), outlier_rejection=bool(a[1]), min_area=int(a[2]), std_threshold=float(a[3]))


def restated_states(things, stuff, updates):
    n = len(things) + len(stuff)
    st = [np.zeros(n, np.float64)] + [np.zeros(n, np.int32) for _ in range(3)]
    for p, t in updates:
        for i, v in enumerate(np_pq_update(p, t, things, stuff)):
            st[i] = st[i] + v
    return st


# ----------------------------------------------------------------------------------------------- tests
def test_g13_pq_restatement():
    g = golden("g13_panoptic.npz")
    assert len(pq_names(g)) >= 8
    for n in pq_names(g):
        things, stuff, updates = pq_case(g, n)
        assert list(things) == [int(v) for v in g[n + "/things_order"]], n       # the set iteration order the fixture was made with
        iou, tp, fp, fn = restated_states(things, stuff, updates)
        np.testing.assert_array_equal(iou.view(np.int64), g[n + "/iou_sum"].view(np.int64), err_msg=n)
        for a, k in ((tp, "tp"), (fp, "fp"), (fn, "fn")):
            assert a.dtype == np.int32
            np.testing.assert_array_equal(a, g[n + "/" + k], err_msg=n)
        res = np_pq_compute(len(things), len(stuff), iou, tp, fp, fn)
        got = np.array([float(res[gr][k]) for gr in ("all", "things", "stuff") for k in ("pq", "rq", "sq")])
        np.testing.assert_array_equal(got.view(np.int64), g[n + "/compute"].view(np.int64), err_msg=n)
    r = g["docstring/compute"]
    assert round(float(r[0]), 4) == 0.5463
    assert np.isnan(g["no_detections/compute"]).any()


def test_g13_clean_restatement():
    g = golden("g13_panoptic.npz")
    assert len(clean_names(g)) >= 6
    for n in clean_names(g):
        out = np_clean(g[n + "/ids"], **clean_args(g, n))
        np.testing.assert_array_equal(out, g[n + "/cleaned"], err_msg=n)


def test_opening_idempotent():
    rs = np.random.RandomState(3)
    for _ in range(20):
        ids = synth_ids(rs, 40, 56, rs.randint(-3, 9, size=6), cell=4, noise=0.05)
        np.testing.assert_array_equal(np_clean(ids, 1, min_area=0), np_clean(ids, 3, min_area=0))


def test_iou_restatement_ignores_out_of_range():
    t = np.array([0, 1, 2, -1, 3, 1])
    p = np.array([0, 1, 1, 2, 0, 5])
    cm, iou = np_iou(p, t, 3)
    assert cm.sum() == 3 and cm[2, 1] == 1
    assert abs(iou - np.mean([1.0, 0.5, 0.0])) < 1e-12


def test_set_order_mapping():
    from pagnerf_amd.metrics import category_to_continuous_id, void_color
    things, stuff = {8, 1, 3}, {20, 5}
    assert list(things) == [8, 1, 3]
    m = category_to_continuous_id(things, stuff)
    assert m == cont_ids(things, stuff)
    assert [m[c] for c in (8, 1, 3)] == [0, 1, 2] and sorted(m[c] for c in stuff) == [3, 4]
    assert void_color(things, stuff) == (21, 0)
    assert void_color({-4}, {-2}) == (1, 0)


def test_cpu_tensors_refused():
    from pagnerf_amd.metrics import MulticlassIoU, PanopticQuality, clean_instances, panoptic_quality
    x = torch.zeros(1, 2, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        PanopticQuality({0}, {1}).update(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        panoptic_quality(x, x, {0}, {1})
    with pytest.raises(RuntimeError, match="GPU"):
        clean_instances(torch.zeros(4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        MulticlassIoU(3).update(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))


def test_validation_errors():
    from pagnerf_amd.metrics import PanopticQuality, panoptic_quality
    for things, stuff, msg in (([0], {1}, "`things` to be of type"), (set(), {1}, "`things` to be a non-empty"), ({0}, {1.0}, "`stuff` to be of type"),
                               ({0}, set(), "`stuff` to be a non-empty"), ({0, 1}, {1}, "distinct keys"), ({True}, {2}, "`things` to be of type")):
        with pytest.raises(ValueError, match=msg):
            PanopticQuality(things, stuff)
    m = PanopticQuality({0}, {1})
    a = torch.zeros(1, 2, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="`preds` to be of type"):
        m.update(a.numpy(), a)
    with pytest.raises(ValueError, match="`target` to be of type"):
        m.update(a, a.numpy())
    with pytest.raises(ValueError, match="same shape"):
        m.update(a, torch.zeros(1, 2, 4, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"shape \[batch, 2, height, width\]"):
        m.update(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match="same shape"):
        panoptic_quality(a, a[..., :2], {0}, {1})


def test_state_layout_and_to():
    from pagnerf_amd.metrics import PanopticQuality
    m = PanopticQuality({4, 2}, {7})
    assert m.iou_sum.dtype == torch.float64 and m.iou_sum.shape == (3,)
    for t in (m.true_positives, m.false_positives, m.false_negatives):
        assert t.dtype == torch.int32 and t.shape == (3,)
    assert m.to("cpu") is m
