"""GPU checks of the panoptic evaluation (pagnerf_amd/metrics.py on csrc/panoptic.hip): the reference's results in g13_panoptic.npz exactly, 720 x 1280
images against the numpy restatement of tests/test_panoptic_eval_host.py (int32 and int64), strided input, idempotent opening, determinism, graph
capture, memory, the device flags, and a NeF render through argmax, clean_instances, PQ and IoU."""
import numpy as np
import pytest
import torch

import test_panoptic_eval_host as H
from conftest import golden

pytestmark = pytest.mark.gpu

THINGS, STUFF, NCLS = {1, 2, 3, 4}, {0, 5}, 6


def _states(m):
    return [t.cpu().numpy() for t in (m.iou_sum, m.true_positives, m.false_positives, m.false_negatives)]


def _compute_vec(res):
    return np.array([float(res[g][k]) for g in ("all", "things", "stuff") for k in ("pq", "rq", "sq")])


def test_g13_reference_equality(gpu_device):
    from pagnerf_amd.metrics import PanopticQuality, clean_instances, panoptic_quality
    g = golden("g13_panoptic.npz")
    for n in H.pq_names(g):
        things, stuff, updates = H.pq_case(g, n)
        m = PanopticQuality(things, stuff, allow_unknown_preds_category=True).to("cuda")
        for p, t in updates:
            m.update(torch.from_numpy(p).to(gpu_device), torch.from_numpy(t).to(gpu_device))
        iou, tp, fp, fn = _states(m)
        np.testing.assert_array_equal(iou.view(np.int64), g[n + "/iou_sum"].view(np.int64), err_msg=n)
        for a, k in ((tp, "tp"), (fp, "fp"), (fn, "fn")):
            assert a.dtype == np.int32
            np.testing.assert_array_equal(a, g[n + "/" + k], err_msg=n)
        res = m.compute()
        assert res["all"]["n"] == len(things) + len(stuff) and res["things"]["n"] == len(things) and res["stuff"]["n"] == len(stuff)
        assert res["all"]["pq"].dtype == torch.float64 and res["all"]["pq"].dim() == 0
        np.testing.assert_array_equal(_compute_vec(res).view(np.int64), g[n + "/compute"].view(np.int64), err_msg=n)
        if len(updates) == 1:
            p, t = updates[0]
            v = panoptic_quality(torch.from_numpy(p).to(gpu_device), torch.from_numpy(t).to(gpu_device), things, stuff, True)
            assert float(v) == float(g[n + "/compute"][0]) or (np.isnan(float(v)) and np.isnan(g[n + "/compute"][0]))
    for n in H.clean_names(g):
        ids = torch.from_numpy(g[n + "/ids"]).to(gpu_device)
        out = clean_instances(ids, **H.clean_args(g, n))
        assert out.dtype == ids.dtype
        np.testing.assert_array_equal(out.cpu().numpy(), g[n + "/cleaned"], err_msg=n)
        np.testing.assert_array_equal(ids.cpu().numpy(), g[n + "/ids"], err_msg=n)        # input untouched


def _big_case(seed, H_=720, W_=1280):
    rs = np.random.RandomState(seed)
    sem_t = H.blocky(rs, H_, W_, 40, np.arange(NCLS))
    inst_t = H.blocky(rs, H_, W_, 40, np.arange(100))
    sem_p = sem_t.copy()
    flip = H.blocky(rs, H_, W_, 40, [0, 0, 0, 1]).astype(bool)
    sem_p[flip] = rs.randint(0, NCLS, size=int(flip.sum()))
    inst_p = H.synth_ids(rs, H_, W_, np.arange(200), cell=40, noise=0.01)
    sem_t[rs.rand(H_, W_) < 0.01] = -1
    return sem_p, inst_p, sem_t, inst_t


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_720p_matches_restatement(gpu_device, dtype):
    from pagnerf_amd.metrics import MulticlassIoU, PanopticQuality, clean_instances
    sem_p, inst_p, sem_t, inst_t = _big_case(31)
    d = lambda a: torch.from_numpy(a).to(gpu_device, dtype)
    cleaned = clean_instances(d(inst_p), num_openings=1, outlier_rejection=True)
    ref_clean = H.np_clean(inst_p, 1, True, 100, 2.0)
    np.testing.assert_array_equal(cleaned.cpu().numpy(), ref_clean)
    m = PanopticQuality(THINGS, STUFF, allow_unknown_preds_category=True).to("cuda")
    preds = torch.stack((d(sem_p), cleaned))[None]
    target = torch.stack((d(sem_t), d(inst_t)))[None]
    m.update(preds, target)
    iou, tp, fp, fn = H.np_pq_update(np.stack((sem_p, ref_clean))[None], np.stack((sem_t, inst_t))[None], THINGS, STUFF)
    got = _states(m)
    assert tp.sum() > 50 and fp.sum() > 0
    np.testing.assert_array_equal(got[0].view(np.int64), iou.view(np.int64))
    for a, b in zip(got[1:], (tp, fp, fn)):
        np.testing.assert_array_equal(a, b)
    miou = MulticlassIoU(NCLS).to("cuda")
    miou.update(d(sem_p), d(sem_t))
    cm, ref_iou = H.np_iou(sem_p, sem_t, NCLS)
    np.testing.assert_array_equal(miou.confmat.cpu().numpy(), cm)
    assert abs(float(miou.compute()) - ref_iou) < 1e-6


def test_strided_inputs(gpu_device):
    from pagnerf_amd.metrics import MulticlassIoU, PanopticQuality, clean_instances
    sem_p, inst_p, sem_t, inst_t = _big_case(32, 240, 320)
    d = lambda a: torch.from_numpy(a).to(gpu_device)
    ids_t = d(np.ascontiguousarray(inst_p.T)).t()                   # [H, W] view with strides (1, H)
    assert not ids_t.is_contiguous()
    a = clean_instances(ids_t, outlier_rejection=True)
    b = clean_instances(ids_t.contiguous(), outlier_rejection=True)
    assert torch.equal(a, b)
    pair_p = d(np.stack((sem_p, inst_p), -1)[None]).permute(0, 3, 1, 2)   # [B, 2, H, W] with the channel innermost
    pair_t = d(np.stack((sem_t, inst_t), -1)[None]).permute(0, 3, 1, 2)
    wide = torch.zeros(1, 2, 240, 640, dtype=torch.int64, device=gpu_device)[..., ::2]
    wide.copy_(pair_t)
    m1 = PanopticQuality(THINGS, STUFF, True).to("cuda")
    m1.update(pair_p, wide)
    m2 = PanopticQuality(THINGS, STUFF, True).to("cuda")
    m2.update(pair_p.contiguous(), pair_t.contiguous())
    for x, y in zip(_states(m1), _states(m2)):
        np.testing.assert_array_equal(x, y)
    i1, i2 = MulticlassIoU(NCLS).to("cuda"), MulticlassIoU(NCLS).to("cuda")
    i1.update(pair_p[0, 0], wide[0, 0])
    i2.update(pair_p[0, 0].contiguous(), pair_t[0, 0].contiguous())
    assert torch.equal(i1.confmat, i2.confmat)


def test_openings_idempotent_and_deterministic(gpu_device):
    from pagnerf_amd.metrics import PanopticQuality, clean_instances
    sem_p, inst_p, sem_t, inst_t = _big_case(33)
    ids = torch.from_numpy(inst_p).to(gpu_device)
    a = clean_instances(ids, num_openings=1, outlier_rejection=True)
    assert torch.equal(a, clean_instances(ids, num_openings=3, outlier_rejection=True))
    assert torch.equal(a, clean_instances(ids, num_openings=1, outlier_rejection=True))
    runs = []
    for _ in range(2):
        m = PanopticQuality(THINGS, STUFF, True).to("cuda")
        m.update(torch.from_numpy(np.stack((sem_p, inst_p))[None]).to(gpu_device), torch.from_numpy(np.stack((sem_t, inst_t))[None]).to(gpu_device))
        runs.append(_states(m))
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()


def test_graph_capture(gpu_device):
    from pagnerf_amd.metrics import MulticlassIoU, PanopticQuality, clean_instances
    sem_p, inst_p, sem_t, inst_t = _big_case(34, 360, 640)
    s_sem_p, s_inst = torch.from_numpy(sem_p).to(gpu_device), torch.from_numpy(inst_p).to(gpu_device)
    s_tgt = torch.from_numpy(np.stack((sem_t, inst_t))[None]).to(gpu_device)
    pq = PanopticQuality(THINGS, STUFF, True).to("cuda")
    iou = MulticlassIoU(NCLS).to("cuda")

    def step():
        c = clean_instances(s_inst, outlier_rejection=True)
        pq.update(torch.stack((s_sem_p, c))[None], s_tgt)
        iou.update(s_sem_p, s_tgt[0, 0])
        return c

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = step()
    for seed in (35, 36):
        sp, ip, st, it = _big_case(seed, 360, 640)
        s_sem_p.copy_(torch.from_numpy(sp))
        s_inst.copy_(torch.from_numpy(ip))
        s_tgt.copy_(torch.from_numpy(np.stack((st, it))[None]))
        pq.reset()
        iou.reset()
        graph.replay()
        torch.cuda.synchronize()
        got = _states(pq) + [iou.confmat.cpu().numpy()]
        pq.reset()
        iou.reset()
        eager = step()
        assert torch.equal(g_out, eager), seed
        for x, y in zip(got, _states(pq) + [iou.confmat.cpu().numpy()]):
            assert x.tobytes() == y.tobytes(), seed


def test_memory_720p(gpu_device):
    from pagnerf_amd.metrics import PanopticQuality, clean_instances
    sem_p, inst_p, sem_t, inst_t = _big_case(37)
    ids = torch.from_numpy(inst_p).to(gpu_device)
    sem = torch.from_numpy(sem_p).to(gpu_device)
    tgt = torch.from_numpy(np.stack((sem_t, inst_t))[None]).to(gpu_device)
    m = PanopticQuality(THINGS, STUFF, True).to("cuda")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    c = clean_instances(ids, outlier_rejection=True)
    m.update(torch.stack((sem, c))[None], tgt)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < 128 << 20, rise                  # the reference's int64 [K, H, W] masks alone take about 1.5 GB


def test_device_flags(gpu_device):
    from pagnerf_amd.metrics import PanopticQuality
    p = torch.zeros(1, 2, 8, 8, dtype=torch.int64, device=gpu_device)
    p[0, 0, :4] = 1
    t = p.clone()
    p[0, 0, 0, 0] = 9                              # unknown pred category
    m = PanopticQuality({1}, {0})
    with pytest.raises(ValueError, match="Unknown categories found in preds"):
        m.update(p, t)
    assert all(not a.any() for a in _states(m))    # the state is untouched, as the reference raises before updating it
    m2 = PanopticQuality({1}, {0}, allow_unknown_preds_category=True)
    m2.update(p, t)
    assert int(m2.true_positives.sum()) == 2
    big = torch.zeros(2, 2, 8, 8, dtype=torch.int64, device=gpu_device)
    big[:, 0] = 1
    big[0, 1, 0, 0] = 2 ** 31 - 10
    big[1, 1, 0, 0] = 20
    m3 = PanopticQuality({1}, {0}, True)
    m3.update(big, big)
    with pytest.raises(ValueError, match="outside int32"):
        m3.compute()


def test_nef_render_to_metrics(gpu_device):
    import test_gpu_parity as T
    from pagnerf_amd.metrics import MulticlassIoU, PanopticQuality, clean_instances
    side = 32
    nef, tracer, rays, occ, jitter = T._make_scene(gpu_device, "bf16", N=side * side, S=48, cap_log2=12)
    with torch.no_grad():
        rb = tracer(nef, channels={"rgb", "depth", "semantics", "inst_embedding"}, rays=rays, jitter=jitter.to(gpu_device), stage="train")
    sem = torch.argmax(rb.semantics.reshape(side, side, -1), dim=-1)
    inst = torch.argmax(rb.inst_embedding.reshape(side, side, -1), dim=-1)
    C = rb.semantics.shape[-1]
    things, stuff = set(range(1, C)), {0}
    cleaned = clean_instances(inst, num_openings=1, outlier_rejection=True, min_area=4)
    np.testing.assert_array_equal(cleaned.cpu().numpy(), H.np_clean(inst.cpu().numpy(), 1, True, 4, 2.0))
    rs = np.random.RandomState(38)
    sem_gt = H.blocky(rs, side, side, 8, np.arange(C))
    inst_gt = H.blocky(rs, side, side, 8, np.arange(6))
    m = PanopticQuality(things, stuff, True).to("cuda")
    m.update(torch.stack((sem, cleaned))[None], torch.from_numpy(np.stack((sem_gt, inst_gt))[None]).to(gpu_device))
    ref = H.np_pq_update(np.stack((sem.cpu().numpy(), cleaned.cpu().numpy()))[None], np.stack((sem_gt, inst_gt))[None], things, stuff)
    for a, b in zip(_states(m), ref):
        assert a.tobytes() == b.tobytes()
    got = _compute_vec(m.compute())
    want = _compute_vec(H.np_pq_compute(len(things), len(stuff), *ref))
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))
    iou = MulticlassIoU(C).to("cuda")
    iou.update(sem, torch.from_numpy(sem_gt).to(gpu_device))
    cm, ref_iou = H.np_iou(sem.cpu().numpy(), sem_gt, C)
    np.testing.assert_array_equal(iou.confmat.cpu().numpy(), cm)
    assert abs(float(iou.compute()) - ref_iou) < 1e-6
