"""GPU checks of the mean-shift clustering (pagnerf_amd/cluster.py on csrc/cluster.hip): the reference's results in g12_meanshift.npz, larger inputs
against the numpy fp64 restatement of tests/test_meanshift_host.py, bitwise determinism, graph capture of predict, memory without a K x K matrix,
bf16 and strided predict input, the empty and unfitted edge cases, and a MeanShiftPanopticDeltaNeF render through train_clustering / predict_clusters."""
import numpy as np
import pytest
import torch

import test_meanshift_host as H
from conftest import golden

pytestmark = pytest.mark.gpu


def _fit(dev, X, lab):
    from pagnerf_amd.cluster import MeanShift
    ms = MeanShift(num_clustering_workers=6)
    ms.train_clustering(torch.from_numpy(X).to(dev), torch.from_numpy(lab).to(dev))
    return ms


def test_g12_reference_equality(gpu_device):
    from pagnerf_amd.cluster import estimate_bandwidth, mean_class_embedding
    g = golden("g12_meanshift.npz")
    for n in [str(v) for v in g["names"]]:
        X, lab = H.case_inputs(int(g[n + "/seed"]), H._spec(g, n))
        Xd, Ld = torch.from_numpy(X).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
        C = mean_class_embedding(Xd, Ld)
        np.testing.assert_allclose(C.cpu().numpy(), g[n + "/centres"], rtol=0, atol=1e-6, err_msg=n)
        ref_bw = float(g[n + "/bandwidth"])
        bw = estimate_bandwidth(C)
        if C.shape[0] >= 25 and ref_bw > 0:
            assert abs(bw - ref_bw) <= 1e-5 * ref_bw, (n, bw, ref_bw)
        else:
            assert bw == 0.0, (n, bw)
        ms = _fit(gpu_device, X, lab)
        cen = ms.cluster_centers_.cpu().numpy()
        assert cen.shape == g[n + "/cluster_centers"].shape, (n, cen.shape)
        np.testing.assert_allclose(cen, g[n + "/cluster_centers"], rtol=0, atol=1e-5, err_msg=n)
        assert ms.bandwidth == bw and ms.n_iter_ == int(g[n + "/n_iter"]), (n, ms.n_iter_)
        q = torch.from_numpy(H.query_rows(g, n)).to(gpu_device)
        pred = ms.predict_clusters(q)
        assert pred.dtype == torch.int64 and pred.shape == q.shape[:1]
        np.testing.assert_array_equal(pred.cpu().numpy(), g[n + "/predict"], err_msg=n)


def _blobs(K, D, seed, n_blob=8):
    """K centres (one ray per label in one image: the class means are the rows themselves) in n_blob blobs of unequal sizes.  With fewer blobs than
    1 / quantile every blob holds more than k = int(0.08 K) centres, so the bandwidth lies within the blobs and each blob keeps its own cluster."""
    rs = np.random.RandomState(seed)
    protos = rs.standard_normal((n_blob, D))
    protos /= np.linalg.norm(protos, axis=1, keepdims=True)
    w = np.linspace(1.0, 2.0, n_blob)
    X = protos[rs.choice(n_blob, size=K, p=w / w.sum())] + rs.standard_normal((K, D)) * (0.25 / np.sqrt(D))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)[None], rs.permutation(K).astype(np.int64)[None]


@pytest.mark.parametrize("K,D,seed", [(8000, 200, 1), (20000, 16, 2)])
def test_large_fits_match_restatement(gpu_device, K, D, seed):
    """K = 8000 at D = 200 and K = 20000 at D = 16 against the fp64 restatement: 8 clusters, ordering, duplicates and suppression at full size.
    The device and the restatement sum the neighbours in the same order, so their means agree bitwise; their fp64 distances differ by ~1e-15
    relative, so every neighbour and suppression decision is first checked to lie more than 1e-11 relative away from the bandwidth."""
    X, lab = _blobs(K, D, seed)
    ms = _fit(gpu_device, X, lab)
    C = H.ref_class_means(X, lab)
    bw = H.ref_bandwidth(C)
    assert abs(ms.bandwidth - bw) <= 1e-9 * bw, (ms.bandwidth, bw)
    trace = []
    cen, n_iter = H.ref_mean_shift(C, bw, trace=trace)
    for kind, d, thr in trace:
        if len(d):
            assert float(np.min(np.abs(np.asarray(d) - thr))) > 1e-11 * thr, kind
    assert cen.shape[0] >= 4, cen.shape
    got = ms.cluster_centers_.cpu().numpy()
    assert got.shape == cen.shape and ms.n_iter_ == n_iter, (got.shape, cen.shape, ms.n_iter_, n_iter)
    np.testing.assert_allclose(got, cen, rtol=0, atol=1e-6)
    q = (X[0, :8192] * 2.5).astype(np.float32)
    pred = ms.predict_clusters(torch.from_numpy(q).to(gpu_device)).cpu().numpy()
    np.testing.assert_array_equal(pred, H.ref_predict(q, got))
    assert len(np.unique(pred)) == cen.shape[0]


@pytest.mark.parametrize("C,D", [(65, 240), (100, 256), (300, 512), (2000, 64)])
def test_predict_many_centres_and_wide_rows(gpu_device, C, D):
    """C > 64 (the kernel stages the centres block by block for every row tile) and D up to 512 (the widest instantiations and their LDS),
    f32 contiguous, f32 strided (scalar loads) and bf16, against the fp64 argmin."""
    from pagnerf_amd.cluster import MeanShift
    g = torch.Generator(gpu_device).manual_seed(C + D)
    ms = MeanShift()
    ms.cluster_centers_ = torch.randn(C, D, device=gpu_device, generator=g)
    cen = ms.cluster_centers_.cpu().numpy()
    pick = torch.randint(0, C, (5000,), device=gpu_device, generator=g)
    x = ms.cluster_centers_[pick] * 1.3 + torch.randn(5000, D, device=gpu_device, generator=g)
    np.testing.assert_array_equal(ms.predict_clusters(x).cpu().numpy(), H.ref_predict(x.cpu().numpy(), cen))
    buf = torch.zeros(5000, D + 3, device=gpu_device)
    buf[:, 1:1 + D] = x
    np.testing.assert_array_equal(ms.predict_clusters(buf[:, 1:1 + D]).cpu().numpy(), H.ref_predict(x.cpu().numpy(), cen))
    xb = x.to(torch.bfloat16)
    np.testing.assert_array_equal(ms.predict_clusters(xb).cpu().numpy(), H.ref_predict(xb.float().cpu().numpy(), cen))
    Z = torch.zeros(D, 3, device=gpu_device)
    Z[:, 1] = x[0]
    one = Z[:, 1]                                                    # a single row whose elements lie 3 apart
    assert one.stride(0) == 3
    assert int(ms.predict_clusters(one)) == int(H.ref_predict(x[:1].cpu().numpy(), cen)[0])
    assert int(ms.predict_clusters(Z.T[1:2])[0]) == int(H.ref_predict(x[:1].cpu().numpy(), cen)[0])


def test_bitwise_determinism(gpu_device):
    g = golden("g12_meanshift.npz")
    X, lab = H.case_inputs(int(g["trainer/seed"]), H._spec(g, "trainer"))
    q = torch.randn(50000, X.shape[-1], device=gpu_device)
    runs = []
    for _ in range(2):
        ms = _fit(gpu_device, X, lab)
        runs.append((ms.cluster_centers_.clone(), ms.bandwidth, ms.predict_clusters(q)))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and torch.equal(runs[0][2], runs[1][2])


def test_predict_graph_capture(gpu_device):
    g = golden("g12_meanshift.npz")
    X, lab = H.case_inputs(int(g["trainer/seed"]), H._spec(g, "trainer"))
    ms = _fit(gpu_device, X, lab)
    sx = torch.randn(3000, X.shape[-1], device=gpu_device)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ms.predict_clusters(sx)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = ms.predict_clusters(sx)
    for seed in (1, 2):
        x2 = torch.randn(3000, X.shape[-1], device=gpu_device, generator=torch.Generator(gpu_device).manual_seed(seed))
        sx.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_out, ms.predict_clusters(x2)), seed


def test_memory_has_no_k_by_k_matrix(gpu_device):
    K, D = 20000, 16
    rs = np.random.RandomState(7)
    X = rs.standard_normal((1, K, D)).astype(np.float32)
    lab = rs.permutation(K).astype(np.int64)[None]
    Xd, Ld = torch.from_numpy(X).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
    from pagnerf_amd.cluster import MeanShift
    ms = MeanShift()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms.train_clustering(Xd, Ld)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise <= 8 * K * D * 4 + 24 * K + (4 << 20), rise        # a K x K fp32 matrix alone would be 1.6 GB
    assert ms.cluster_centers_.shape[1] == D


def test_bf16_and_strided_predict(gpu_device):
    g = golden("g12_meanshift.npz")
    n = "raw_predict"
    X, lab = H.case_inputs(int(g[n + "/seed"]), H._spec(g, n))
    ms = _fit(gpu_device, X, lab)
    cen = ms.cluster_centers_.cpu().numpy()
    D = X.shape[-1]
    q = torch.from_numpy(H.query_rows(g, n)).to(gpu_device)
    buf = torch.zeros(q.shape[0], D + 7, device=gpu_device)
    buf[:, 3:3 + D] = q
    strided = buf[:, 3:3 + D]                                          # row stride D + 7, misaligned rows: the scalar-load path
    np.testing.assert_array_equal(ms.predict_clusters(strided).cpu().numpy(), g[n + "/predict"])
    qb = q.to(torch.bfloat16)
    bbuf = torch.zeros(q.shape[0], 2, D + 6, device=gpu_device, dtype=torch.bfloat16)
    bbuf[:, 1, :D] = qb
    view = bbuf[:, 1, :D]
    got = ms.predict_clusters(view).cpu().numpy()
    np.testing.assert_array_equal(got, H.ref_predict(qb.float().cpu().numpy(), cen))
    img = q[:600].reshape(20, 30, D)                                  # leading shape is kept
    assert ms.predict_clusters(img).shape == (20, 30)


def test_empty_fit_and_unfitted_fallback(gpu_device):
    import torch.nn.functional as F
    from pagnerf_amd.cluster import MeanShift
    ms = MeanShift()
    x = torch.randn(4, 5, 12, device=gpu_device)
    assert torch.equal(ms.predict_clusters(x), torch.argmax(F.normalize(x, dim=-1), dim=-1))
    g = golden("g12_meanshift.npz")
    X, lab = H.case_inputs(int(g["d16/seed"]), H._spec(g, "d16"))
    ms = _fit(gpu_device, X, lab)
    before = (ms.cluster_centers_.clone(), ms.bandwidth, ms.n_iter_)
    ms.train_clustering(torch.zeros(2, 0, 16, device=gpu_device), torch.zeros(2, 0, dtype=torch.int64, device=gpu_device))
    assert torch.equal(ms.cluster_centers_, before[0]) and (ms.bandwidth, ms.n_iter_) == before[1:]


def test_mean_shift_nef_render_and_clustering(gpu_device):
    import pagnerf_amd
    from pagnerf_amd.cluster import MeanShiftPanopticDeltaNeF
    dev = gpu_device
    torch.manual_seed(0)
    L_perm, cap = 24, 12
    nef = MeanShiftPanopticDeltaNeF(grid_type="PermutoGrid", feature_dim=2, num_lods=L_perm, num_classes=6, num_instances=32, sem_num_layers=1,
                                    sem_softmax=True, inst_num_layers=2, panoptic_features_type="delta", capacity_log_2=cap,
                                    delta_capacity_log_2=cap, coarsest_scale=1.0, finest_scale=1e-4, blas_level=5, precision="bf16",
                                    num_clusters=-1, distance_func="cosine", num_clustering_workers=6)
    assert nef.get_nef_type() == "mean_shift_panoptic_delta_nef" and "clusters" in nef.get_supported_channels()
    gen = torch.Generator().manual_seed(0)
    for grid in (nef.grid, nef.delta_grid):
        grid.init_from_scales(random_shift=torch.randn(L_perm, 3, generator=gen) * 10, tables=torch.randn(L_perm, 2 ** cap, 2, generator=gen) * 0.3)
    nef = nef.to(dev)
    for grid in (nef.grid, nef.delta_grid):
        grid.blas_init(torch.ones(2 ** 15, dtype=torch.bool))
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=32, bg_color="white")
    pipe = pagnerf_amd.Pipeline(nef, tracer)
    N = 4096
    o = (torch.rand(N, 3, generator=gen) - 0.5) * 0.6
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    rays = pagnerf_amd.Rays(o.to(dev), d.to(dev), dist_min=0.0, dist_max=2.0)
    with torch.no_grad():
        rb = tracer(nef, channels={"inst_embedding", "clusters"}, rays=rays)
        # the same field values, composited by the extra-channel path (live weights) and by the fused panoptic path (detached weights)
        assert rb.clusters.shape == rb.inst_embedding.shape
        err = float((rb.clusters.float() - rb.inst_embedding.float()).abs().max())
        assert err <= 1e-3 * max(1.0, float(rb.inst_embedding.abs().max())), err
        img = pagnerf_amd.batch_render(pipe, rays, channels=["inst_embedding"], render_batch=1024)
        emb = img.inst_embedding
        ids = (torch.arange(N, device=dev) % 7).reshape(16, N // 16)               # 16 pseudo-images sharing 7 ids: K = 112
        nef.train_clustering(torch.nn.functional.normalize(emb.reshape(16, N // 16, -1), dim=-1), ids)
        pred = nef.predict_clusters(emb.reshape(64, 64, -1))
    ms = nef.clustering_obj
    assert ms.fitted and ms.n_centres_ == 16 * 7 and pred.shape == (64, 64) and pred.dtype == torch.int64
    cen = ms.cluster_centers_.cpu().numpy()
    np.testing.assert_array_equal(pred.reshape(-1).cpu().numpy(), H.ref_predict(emb.float().cpu().numpy(), cen))
