"""GPU checks of the validation row (pagnerf_amd/metrics.py: MaskMeanAveragePrecision on pag_mask_ap_update, PeakSignalNoiseRatio,
ValidationMetrics): every comparison is against the numpy restatement of tests/test_validation_metrics_host.py - the hand cases, a random blocky
case past the detection cap, odd shapes and strides, id extremes, order and determinism, no host synchronisation, the id-count flag, and the
evaluator against the existing metrics called by hand in the reference's order."""
import numpy as np
import pytest
import torch

import test_validation_metrics_host as H

pytestmark = pytest.mark.gpu

THINGS, STUFF, NCLS = [1, 2, 3, 4], [0, 5], 6


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _run(updates, dtype=torch.int64, max_detections=100):
    from pagnerf_amd.metrics import MaskMeanAveragePrecision
    m = MaskMeanAveragePrecision(max_detections=max_detections).to("cuda")
    for pred, target, kw in updates:
        kw = dict(kw)
        if "pred_raw" in kw:
            kw["pred_raw"] = _dev(kw["pred_raw"], dtype)
        m.update(_dev(pred, dtype), _dev(target, dtype), **kw)
    return m


def _words(m):
    return m.slots[:m.num_updates * m.max_detections].cpu().numpy()


def _check(m, updates, msg=""):
    """Slot words and npig equal the restatement's; compute_fp64() within 1e-12 (both sides are fp64 means of at most 1010 values of [0, 1]: about
    1e-13); compute() is that value rounded to f32."""
    words, npig, want = H.np_map(updates, m.max_detections)
    np.testing.assert_array_equal(_words(m), np.array(words, np.int32), err_msg=msg)
    assert int(m.npig[0]) == npig, msg
    got = m.compute_fp64()
    np.testing.assert_allclose([got["map"], got["map_50"], got["map_75"]], want, rtol=0, atol=1e-12, err_msg=msg)
    out = m.compute()
    for k in ("map", "map_50", "map_75"):
        assert out[k].dtype == torch.float32 and out[k].dim() == 0 and out[k].is_cuda
        assert float(out[k]) == float(np.float32(got[k])), (msg, k)
    return got


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_hand_cases(gpu_device, dtype):
    for name, (updates, want) in sorted(H.hand_cases().items()):
        m = _run(updates, dtype)
        got = _check(m, updates, name)
        np.testing.assert_allclose([got["map"], got["map_50"], got["map_75"]], want, rtol=0, atol=1e-12, err_msg=name)
    p, t = H.tie_image()                         # the tie label images allow (case F, see the host file's docstring)
    m = _run([(p, t, {})], dtype)
    _check(m, [(p, t, {})], "tie")
    assert int(_words(m)[0]) == 1 | 2


def test_random_blocky_case(gpu_device):
    updates = H.blocky_case(5)
    m = _run(updates)
    got = _check(m, updates)
    assert 0 < got["map"] < got["map_50"] < 1
    w = _words(m)
    w = w[(w & 1) != 0]
    assert len(w) == 300                                                     # the cap of 100 detections per image was reached
    assert int(((w >> 1) & 1).sum()) != int(((w >> 10) & 1).sum())


def test_odd_shapes_strides_and_extremes(gpu_device):
    rs = np.random.RandomState(11)
    for shape in ((37, 129), (1, 1), (1, 200)):
        t = rs.randint(0, 5, size=(-(-shape[0] // 4), -(-shape[1] // 4)))
        t = np.kron(t, np.ones((4, 4), np.int64))[:shape[0], :shape[1]].astype(np.int64)
        p = t.copy()
        noise = rs.rand(*shape) < 0.1
        p[noise] = rs.randint(0, 9, size=int(noise.sum()))
        _check(_run([(p, t, {})]), [(p, t, {})], str(shape))
    # a transposed view equals its contiguous copy
    from pagnerf_amd.metrics import MaskMeanAveragePrecision
    (p, t, _), = H.blocky_case(7, n_images=1, H=40, W=56)
    a, b = MaskMeanAveragePrecision().to("cuda"), MaskMeanAveragePrecision().to("cuda")
    pt, tt = _dev(p.T.copy()), _dev(t.T.copy(), torch.int32)
    assert not pt.t().is_contiguous()
    a.update(pt.t(), tt.t(), pred_raw=pt.t())
    b.update(_dev(p), _dev(t, torch.int32))
    np.testing.assert_array_equal(_words(a), _words(b))
    _check(a, [(p, t, {})], "transposed")
    # int64 ids around +-2^40: the order is the signed order
    big = np.array([-(1 << 40) - 3, -(1 << 40), -5, 0, 7, (1 << 40), (1 << 40) + 9], np.int64)
    p2, t2 = big[(p % 7)], big[(t % 5)]
    _check(_run([(p2, t2, {})]), [(p2, t2, {})], "2^40")
    # one distinct id, with and without the empty detection
    one = np.full((9, 13), 4, np.int64)
    for flag in (False, True):
        kw = dict(empty_detection_if_single_id=flag)
        m = _run([(one, t[:9, :13], kw)])
        _check(m, [(one, t[:9, :13], kw)], "single id %s" % flag)
        assert int(_words(m)[0]) == int(flag)


def test_order_determinism_reset_and_no_sync(gpu_device):
    from pagnerf_amd.metrics import MaskMeanAveragePrecision
    updates = H.blocky_case(3, n_images=2, H=24, W=40)
    fwd, rev = _run(updates, max_detections=20), _run(updates[::-1], max_detections=20)
    wf, wr = _words(fwd), _words(rev)
    np.testing.assert_array_equal(wf[:20], wr[20:])
    np.testing.assert_array_equal(wf[20:], wr[:20])
    assert int(fwd.npig[0]) == int(rev.npig[0])
    again = _run(updates, max_detections=20)
    np.testing.assert_array_equal(_words(again), wf)
    assert int(again.npig[0]) == int(fwd.npig[0]) and int(again._flags[0]) == 0
    fwd.reset()
    assert fwd.num_updates == 0 and int(fwd.npig[0]) == 0 and not bool(fwd.slots.any())
    assert fwd.compute_fp64()["map"] == -1.0
    # more updates than the first buffer holds: it grows by doubling and keeps what it held; no synchronisation in update
    m = MaskMeanAveragePrecision(max_detections=20).to("cuda")
    tensors = [(_dev(p), _dev(t)) for p, t, _ in updates]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(6):
            m.update(*tensors[i % 2])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert m.slots.numel() == 160
    _check(m, [updates[i % 2] for i in range(6)], "six updates")


def test_too_many_ids_flag(gpu_device):
    from pagnerf_amd.metrics import MaskMeanAveragePrecision
    (p, t, _), = H.blocky_case(9, n_images=1, H=80, W=80)
    m = MaskMeanAveragePrecision().to("cuda")
    m.update(_dev(p), _dev(t))
    good = _words(m).copy()
    npig = int(m.npig[0])
    many = _dev(np.arange(6400, dtype=np.int64).reshape(80, 80))
    m.update(many, _dev(t))
    assert int(m._flags[0]) == 1
    assert int(m.npig[0]) == npig and not bool(m.slots[100:200].any())        # the flagged update left npig and its slots alone
    np.testing.assert_array_equal(_words(m)[:100], good)
    with pytest.raises(ValueError, match="distinct ids"):
        m.compute()
    m.reset()
    m.update(_dev(p), _dev(t))
    _check(m, [(p, t, {})], "after reset")
    # an id of pred that pred_raw lacks
    raw = p.copy()
    raw[p == p.max()] = 0
    m.update(_dev(p), _dev(t), pred_raw=_dev(raw))
    assert int(m._flags[0]) == 2
    with pytest.raises(ValueError, match="pred_raw lacks"):
        m.compute()


# ----------------------------------------------------------------------------------------------- the evaluator
def frame_np(seed, Hh=48, Ww=80, n_inst=40):
    """One synthetic validation frame as numpy arrays: softmax rows whose argmax follows a blocky label image on 90 % of the pixels and is noise on
    the rest (so the cleanup empties small masks and the raw ids outnumber the cleaned ones), and ground truths that are those label images with
    some 8 x 8 cells moved."""
    rs = np.random.RandomState(seed)
    up = lambda a, c: np.kron(a, np.ones((c, c), np.int64)).astype(np.int64)
    softmax = lambda x: np.exp(x) / np.exp(x).sum(-1, keepdims=True)
    inst = up(rs.randint(1, n_inst, size=(Hh // 16, Ww // 16)), 16)
    sem = up(rs.randint(0, NCLS, size=(Hh // 8, Ww // 8)), 8)
    keep = (rs.rand(Hh, Ww) < 0.9)[..., None]
    emb = softmax(3 * rs.randn(Hh, Ww, n_inst)) + 2.0 * keep * np.eye(n_inst)[inst]
    scores = softmax(3 * rs.randn(Hh, Ww, NCLS)) + 2.0 * keep * np.eye(NCLS)[sem]
    inst_gts = np.where(up(rs.rand(Hh // 8, Ww // 8) < 0.2, 8) > 0, 0, inst)
    sem_gts = np.where(up(rs.rand(Hh // 8, Ww // 8) < 0.1, 8) > 0, (sem + 1) % NCLS, sem)
    inst_pred = np.where(up(rs.rand(Hh // 8, Ww // 8) < 0.3, 8) > 0, 0, inst)
    sem_pred = np.where(rs.rand(Hh, Ww) < 0.1, (sem + 2) % NCLS, sem)
    return dict(rgb=rs.rand(Hh, Ww, 3).astype(np.float32), semantics=scores.astype(np.float32), inst_embedding=emb.astype(np.float32),
                gts=rs.rand(Hh, Ww, 4).astype(np.float32), sem_gts=sem_gts, inst_gts=inst_gts, sem_pred=sem_pred, inst_pred=inst_pred)


def _frame(seed):
    from pagnerf_amd import RenderBuffer
    f = {k: torch.from_numpy(v).cuda() for k, v in frame_np(seed).items()}
    rb = RenderBuffer(rgb=f["rgb"], semantics=f["semantics"], inst_embedding=f["inst_embedding"])
    return rb, f["gts"], f["sem_gts"], f["inst_gts"], f["sem_pred"], f["inst_pred"]


def _by_hand(frames, with_pred, predict_clusters=None):
    """trainer.py:708-798 with the existing metrics and the restated mAP, one frame after the other."""
    from pagnerf_amd.metrics import MulticlassIoU, PanopticQuality, PeakSignalNoiseRatio, clean_instances
    psnr, iou, iou_p = PeakSignalNoiseRatio(), MulticlassIoU(NCLS), MulticlassIoU(NCLS)
    pq, pq_p = (PanopticQuality(set(THINGS), set(STUFF), allow_unknown_preds_category=True) for _ in range(2))
    ups, ups_p = [], []
    for rb, gts, sem_gts, inst_gts, sem_pred, inst_pred in frames:
        psnr.update(rb.rgb[..., :3], gts[..., :3])
        semantics = torch.argmax(rb.semantics, dim=-1)
        iou.update(semantics, sem_gts)
        instances = predict_clusters(rb.inst_embedding) if predict_clusters else torch.argmax(rb.inst_embedding, dim=-1)
        cleaned = clean_instances(instances, num_openings=0, outlier_rejection=False, min_area=100)
        labels = torch.stack((sem_gts, inst_gts))[None]
        pq.update(torch.stack((semantics, cleaned))[None], labels)
        ups.append((cleaned.cpu().numpy(), inst_gts.cpu().numpy(), dict(pred_raw=instances.cpu().numpy(), empty_detection_if_single_id=True)))
        if with_pred:
            iou_p.update(sem_pred, sem_gts)
            pq_p.update(torch.stack((sem_pred, inst_pred))[None], labels)
            ups_p.append((inst_pred.cpu().numpy(), inst_gts.cpu().numpy(), {}))
    out = {"val/psnr": psnr.compute().item(), "val/iou": iou.compute().item()}
    a, b, c = H.np_map(ups)[2]
    out.update({"val/map_": float(np.float32(a)), "val/map_50_": float(np.float32(b)), "val/map_75_": float(np.float32(c))})
    res = pq.compute()
    out.update({"val/%s_%s" % (m, g): res[g][m].item() for g in res for m in ("pq", "rq", "sq")})
    if with_pred:
        a, b, c = H.np_map(ups_p)[2]
        out.update({"val/map__pred": float(np.float32(a)), "val/map_50__pred": float(np.float32(b)), "val/map_75__pred": float(np.float32(c))})
        out["val/iou_pred"] = iou_p.compute().item()
        res_p = pq_p.compute()
        out.update({"val/%s_%s_pred" % (m, g): res_p[g][m].item() for g in res_p for m in ("pq", "rq", "sq")})
        out["val/iou_gain"] = (iou.compute() - iou_p.compute()).item()
        out["val/pq_things_gain"] = (res["things"]["pq"] - res_p["things"]["pq"]).item()
    return out


def _same(got, want):
    """Equal column by column.  The mAP columns are f32 roundings of two fp64 values within 1e-12 of each other: at most one f32 ulp of [0.5, 1)
    apart, 2^-24."""
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        if "/map" in k:
            assert abs(got[k] - want[k]) <= 2.0 ** -24, (k, got[k], want[k])
        else:
            assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (k, got[k], want[k])


def test_validation_metrics_matches_by_hand(gpu_device):
    from pagnerf_amd.metrics import ValidationMetrics
    frames = [_frame(21), _frame(22)]
    want = _by_hand(frames, with_pred=False)
    assert want["val/map_"] > 0 and want["val/pq_all"] > 0                    # masks survived the cleanup and some matched
    assert abs(want["val/psnr"] - H.np_psnr([(f[0].rgb.cpu().numpy(), f[1][..., :3].cpu().numpy()) for f in frames])) <= 1e-4
    ev = ValidationMetrics(NCLS, THINGS, STUFF).to("cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for rb, gts, sem_gts, inst_gts, _, _ in frames:
            out = ev.update(rb, gts, sem_gts, inst_gts, labelled=(True, True))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert set(out) == {"semantics", "instances", "inst_conf"} and all(v.is_cuda for v in out.values())
    assert torch.equal(out["semantics"], torch.argmax(frames[-1][0].semantics, -1))
    assert torch.equal(out["inst_conf"], frames[-1][0].inst_embedding.max(-1)[0])
    got = ev.compute()
    assert set(got) == H.BASE_KEYS
    _same(got, want)
    # labelled=None reads the flags back and gives the same numbers
    ev.reset()
    for rb, gts, sem_gts, inst_gts, _, _ in frames:
        ev.update(rb, gts, sem_gts, inst_gts)
    _same(ev.compute(), want)


def test_validation_metrics_pred_columns_unlabelled_and_clusters(gpu_device):
    from pagnerf_amd.metrics import ValidationMetrics
    frames = [_frame(23)]
    want = _by_hand(frames, with_pred=True)
    ev = ValidationMetrics(NCLS, THINGS, STUFF)
    for f in frames:
        ev.update(*f)
    got = ev.compute()
    assert set(got) == H.BASE_KEYS | H.PRED_KEYS
    _same(got, want)
    # an all -1 frame updates the PSNR only
    rb, gts, sem_gts, inst_gts, sem_pred, inst_pred = _frame(24)
    before = {k: v for k, v in got.items() if k != "val/psnr"}
    ev.update(rb, gts, torch.full_like(sem_gts, -1), torch.full_like(inst_gts, -1), sem_pred, inst_pred)
    after = ev.compute()
    assert after["val/psnr"] != got["val/psnr"]
    _same({k: v for k, v in after.items() if k != "val/psnr"}, before)
    # predict_clusters is used when given
    calls = []

    def clusters(emb):
        calls.append(emb.shape)
        return (torch.argmax(emb, dim=-1) // 2) * 2

    ev = ValidationMetrics(NCLS, THINGS, STUFF, predict_clusters=clusters)
    ev.update(*frames[0][:4], labelled=(True, True))
    assert calls == [frames[0][0].inst_embedding.shape]
    _same(ev.compute(), _by_hand(frames, with_pred=False, predict_clusters=lambda e: (torch.argmax(e, dim=-1) // 2) * 2))
