"""CPU-side checks of the mean-shift clustering (pagnerf_amd/cluster.py, csrc/cluster.hip): a numpy fp64 restatement of its four steps pinned to
g12_meanshift.npz (made by tests/golden/make_golden_meanshift.py from the reference's MeanShift and sklearn), the constructor, refusal of CPU tensors,
argument and limit validation in the C ABI, and the nef_type strings.  tests/test_gpu_meanshift.py checks the device against the same restatement."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from conftest import golden

QUANTILE = 0.08
MAX_ITER = 300


# ------------------------------------------------------------------------------------------------ restatement (numpy, fp64)
def case_inputs(seed, spec):
    """Embeddings f32 [B, P, D] and labels i64 [B, P] of a case, regenerated from its seed (make_golden_meanshift.py uses this function).
    spec = (B, P, D, n_inst, noise, sizes): instance i has a random unit prototype and appears in sizes[i] of the B images (every image when sizes
    is empty); each ray of an image picks one of the image's instances, its embedding is the prototype plus Gaussian noise of norm ~noise,
    normalised (noise 0: one-hot prototypes, exact in every arithmetic).  Instance i gets the label 3 i - 1: -1 (the background), 2, 5, ...  The class centres of an instance form a blob of sizes[i]
    centres; blobs with at most k = int(0.08 K) centres put the bandwidth well between the blobs' spread and their distances."""
    B, P, D, n_inst, noise, sizes = spec
    rs = np.random.RandomState(seed)
    protos = rs.standard_normal((n_inst, D))
    protos /= np.linalg.norm(protos, axis=1, keepdims=True)
    if noise == 0.0:                                               # identical rows: one-hot prototypes, so that every distance is exactly 0
        protos = np.eye(D)[np.arange(n_inst) % D]
    present = np.ones((B, n_inst), dtype=bool)
    for i, s in enumerate(sizes):
        present[:, i] = False
        present[rs.permutation(B)[:int(s)], i] = True
    lab = np.empty((B, P), dtype=np.int64)
    for b in range(B):
        ids = np.nonzero(present[b])[0]
        lab[b] = ids[np.arange(P) % len(ids)] if len(ids) <= P else ids[:P]
        rs.shuffle(lab[b])
    X = protos[lab] + rs.standard_normal((B, P, D)) * (noise / np.sqrt(D))
    X /= np.linalg.norm(X, axis=-1, keepdims=True)
    return X.astype(np.float32), lab * 3 - 1


def ref_class_means(X, labels):
    out = []
    for x, l in zip(X, labels):
        for v in np.unique(l):
            rows = x[l == v].astype(np.float64)
            out.append(rows.sum(0) / len(rows))
    return np.asarray(out, dtype=np.float32).reshape(-1, X.shape[-1])


def _d2(a, c):
    """fp64 squared distances [len(a), len(c)] from fp32 rows; exact differences for small problems, the Gram form in blocks for large ones."""
    a = np.asarray(a, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    if a.shape[0] * c.shape[0] * c.shape[1] <= 4e7:
        return ((a[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    cc = (c * c).sum(1)
    return np.maximum((a * a).sum(1)[:, None] + cc[None, :] - 2.0 * (a @ c.T), 0.0)


def ref_bandwidth(C, quantile=QUANTILE):
    K = C.shape[0]
    k = max(1, int(K * quantile))
    kd = np.empty(K)
    for i0 in range(0, K, 512):
        d2 = _d2(C[i0:i0 + 512], C)
        kd[i0:i0 + 512] = np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
    return float(kd.mean())


def ref_mean_shift(C, bw, max_iter=MAX_ITER, trace=None):
    """All seeds at once: -> (cluster_centers_ f32 [n, D], n_iter).  trace(list) collects, per iteration, the distances that decided something (the
    neighbour tests and the stopping test) with their thresholds, for the margin check of the fixture's maker."""
    C = np.asarray(C, dtype=np.float32)
    K = C.shape[0]
    c64 = C.astype(np.float64)
    bw2, thr = bw * bw, 1e-3 * bw
    m = C.copy()
    active = np.ones(K, dtype=bool)
    inten = np.zeros(K, dtype=np.int64)
    iters = np.zeros(K, dtype=np.int64)
    completed = 0
    while active.any():
        idx = np.nonzero(active)[0]
        for i0 in range(0, len(idx), 256):                           # all active seeds advance by one iteration, 256 at a time
            sel = idx[i0:i0 + 256]
            d2 = _d2(m[sel], c64)
            nb = d2 <= bw2
            cnt = nb.sum(1)
            if trace is not None:
                trace.append(("nb", np.sqrt(d2).ravel(), bw))
            new = m[sel].copy()
            ok = cnt > 0
            for r in np.nonzero(ok)[0]:                              # the neighbours summed in ascending index order in fp64 (numpy reduces axis 0
                new[r] = (c64[nb[r]].sum(0) / cnt[r]).astype(np.float32)          # row after row), then rounded to fp32 - the device's order
            step = np.sqrt(((new.astype(np.float64) - m[sel].astype(np.float64)) ** 2).sum(1))
            if trace is not None:
                trace.append(("stop", step[ok], thr))
            m[sel] = new
            stop = ~ok | (step <= thr) | (completed == max_iter)
            inten[sel[stop]] = cnt[stop]
            iters[sel[stop]] = completed
            active[sel[stop]] = False
        completed += 1
    d = {}
    for i in range(K):
        if inten[i]:
            d[tuple(m[i].tolist())] = int(inten[i])
    ordered = sorted(d.items(), key=lambda t: (t[1], t[0]), reverse=True)
    cen = np.asarray([t[0] for t in ordered], dtype=np.float32).reshape(-1, C.shape[1])
    kept = []
    for i in range(len(cen)):
        if kept:
            dk = np.sqrt(_d2(cen[i:i + 1], cen[kept])[0])
            if trace is not None:
                trace.append(("nms", dk, bw))
            if (dk <= bw).any():
                continue
        kept.append(i)
    return cen[kept], int(iters.max())


def ref_predict(X, centres):
    X = np.asarray(X).reshape(-1, centres.shape[1])
    out = np.empty(X.shape[0], dtype=np.int64)
    for i0 in range(0, X.shape[0], 4096):
        out[i0:i0 + 4096] = np.argmin(_d2(X[i0:i0 + 4096], centres), axis=1)
    return out


def ref_fit(X, labels):
    C = ref_class_means(X, labels)
    bw = ref_bandwidth(C)
    cen, n_iter = ref_mean_shift(C, bw)
    return C, bw, cen, n_iter


# ------------------------------------------------------------------------------------------------ the restatement against g12
def _cases():
    g = golden("g12_meanshift.npz")
    names = [str(n) for n in g["names"]]
    return g, names


def test_restatement_matches_reference_fixture():
    g, names = _cases()
    assert len(names) >= 8
    for n in names:
        X, lab = case_inputs(int(g[n + "/seed"]), _spec(g, n))
        C, bw, cen, n_iter = ref_fit(X, lab)
        np.testing.assert_allclose(C, g[n + "/centres"], rtol=0, atol=1e-6, err_msg=n)
        if C.shape[0] >= 25:
            assert abs(bw - float(g[n + "/bandwidth"])) <= 1e-5 * float(g[n + "/bandwidth"]), (n, bw, float(g[n + "/bandwidth"]))
        else:
            assert bw == 0.0 and float(g[n + "/bandwidth"]) < 1e-6, (n, bw)
        assert cen.shape == g[n + "/cluster_centers"].shape, (n, cen.shape, g[n + "/cluster_centers"].shape)
        np.testing.assert_allclose(cen, g[n + "/cluster_centers"], rtol=0, atol=1e-5, err_msg=n)
        assert n_iter == int(g[n + "/n_iter"]), (n, n_iter, int(g[n + "/n_iter"]))
        q = query_rows(g, n)
        np.testing.assert_array_equal(ref_predict(q, cen), g[n + "/predict"], err_msg=n)


def _spec(g, n):
    B, P, D, n_inst = (int(v) for v in g[n + "/shape"])
    noise = float(g[n + "/noise"])
    sizes = [float(v) for v in g[n + "/sizes"]]
    return (B, P, D, n_inst, noise, sizes)


def query_rows(g, n):
    """The predict queries of a case: raw (unnormalised) rows - cluster centres plus noise of norm ~query_noise, times query_scale - regenerated
    from the case's query seed."""
    D = int(g[n + "/shape"][2])
    rs = np.random.RandomState(int(g[n + "/query_seed"]))
    cen = g[n + "/cluster_centers"].astype(np.float64)
    pick = rs.randint(0, cen.shape[0], size=int(g[n + "/n_query"]))
    q = cen[pick] + rs.standard_normal((len(pick), D)) * (float(g[n + "/query_noise"]) / np.sqrt(D))
    return (q * float(g[n + "/query_scale"])).astype(np.float32)


# ------------------------------------------------------------------------------------------------ host API
def test_constructor_signature_and_ignored_kwargs():
    from pagnerf_amd.cluster import ClusteringBase, MeanShift
    sig = inspect.signature(ClusteringBase.__init__)
    assert [p for p in sig.parameters][:4] == ["self", "num_clusters", "distance_func", "num_clustering_workers"]
    assert sig.parameters["num_clusters"].default == -1 and sig.parameters["distance_func"].default == "cosine"
    assert sig.parameters["num_clustering_workers"].default == 1
    ms = MeanShift(num_clusters=7, distance_func="euclidean", num_clustering_workers=6, grid_type="PermutoGrid", feature_dim=4)
    assert (ms.num_clusters, ms.distance_func, ms.num_workers) == (7, "euclidean", 6)
    assert ms.cluster_centers_ is None and ms.bandwidth is None and not ms.fitted


def test_cpu_tensors_are_refused():
    from pagnerf_amd import cluster
    X = torch.randn(2, 10, 8)
    lab = torch.zeros(2, 10, dtype=torch.int64)
    ms = cluster.MeanShift()
    with pytest.raises(RuntimeError, match="GPU"):
        ms.train_clustering(X, lab)
    with pytest.raises(RuntimeError, match="GPU"):
        ms.predict_clusters(X)
    with pytest.raises(RuntimeError, match="GPU"):
        cluster.mean_class_embedding(X, lab)
    with pytest.raises(RuntimeError, match="GPU"):
        cluster.estimate_bandwidth(X[0])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib
    return _lib.load()


def test_c_abi_validates_arguments(lib):
    buf = (ctypes.c_float * 64)()
    info = (ctypes.c_int * 4)()
    bw = (ctypes.c_double * 1)()
    need = lib.pag_meanshift_workspace_bytes(6, 3000, 200)
    assert need >= 18000 * 200 * 4 * 2 > 0                                               # K <= B P = 18000 centres, two [K, D] copies
    assert lib.pag_meanshift_workspace_bytes(1, 1 << 25, 16) == 0 and lib.pag_meanshift_workspace_bytes(1, 10, 513) == 0
    fit = lambda *a: lib.pag_meanshift_fit(*a)                                            # noqa: E731
    # features, dtype, B, P, D, image_stride, row_stride, labels, quantile, max_iter, stages, ws, ws_bytes, means, bw, centers, info, stream
    assert fit(buf, 0, 1, 10, 513, 5130, 513, buf, 0.08, 300, 3, buf, 1 << 40, buf, bw, buf, info, None) == -1    # D > 512
    assert b"D" in lib.pag_last_error_string()
    assert fit(buf, 0, 1, 10, 16, 160, 8, buf, 0.08, 300, 3, buf, 1 << 40, buf, bw, buf, info, None) == -1         # row_stride < D
    assert fit(buf, 0, 2, 1 << 24, 16, 0, 16, buf, 0.08, 300, 3, buf, 1 << 40, buf, bw, buf, info, None) == -1     # rows > 2^24
    assert fit(buf, 0, 1, 40000, 16, 0, 16, None, 0.08, 300, 2, buf, 1 << 40, buf, bw, None, info, None) == -1     # K > 32768 without labels
    assert b"K limit" in lib.pag_last_error_string()
    assert fit(buf, 1, 1, 10, 16, 160, 16, buf, 0.08, 300, 3, buf, 1 << 40, buf, bw, buf, info, None) == -1        # f16
    assert fit(buf, 0, 1, 10, 16, 160, 16, buf, 1.5, 300, 3, buf, 1 << 40, buf, bw, buf, info, None) == -1         # quantile
    assert fit(buf, 0, 1, 10, 16, 160, 16, buf, 0.08, 300, 4, buf, 1 << 40, buf, bw, buf, info, None) == -1        # stages
    assert fit(buf, 0, 1, 10, 16, 160, 16, buf, 0.08, 300, 3, buf, 1 << 40, buf, bw, None, info, None) == -1       # NULL centers
    assert b"NULL" in lib.pag_last_error_string()
    assert fit(buf, 0, 1, 10, 16, 160, 16, buf, 0.08, 300, 3, buf, 64, buf, bw, buf, info, None) == -1             # workspace
    assert b"workspace" in lib.pag_last_error_string()
    pred = lib.pag_meanshift_predict
    out = (ctypes.c_int64 * 4)()
    assert pred(None, 0, 0, 16, 16, None, 4, None, None) == 0                                 # no row: nothing to do
    assert pred(buf, 0, 4, 16, 16, buf, 0, out, None) == -1                                   # no centre
    assert pred(buf, 0, 4, 16, 16, buf, 32769, out, None) == -1                               # C > 32768
    assert pred(buf, 0, 4, 600, 600, buf, 4, out, None) == -1                                 # D > 512
    assert pred(buf, 0, 4, 16, 8, buf, 4, out, None) == -1                                    # row_stride < D
    assert pred(buf, 1, 4, 16, 16, buf, 4, out, None) == -1                                   # f16
    assert pred(buf, 0, 4, 16, 16, buf, 4, None, None) == -1 and b"NULL" in lib.pag_last_error_string()


def test_nef_type_strings():
    from pagnerf_amd.cluster import MeanShiftPanopticDDensityNeF, MeanShiftPanopticDeltaNeF, MeanShiftPanopticNeF
    # the reference's strings: two overrides, and clustering_ + the dd field's own 'delta_panoptic_nef' (clustering_nef.py:24-25, 79-99)
    assert MeanShiftPanopticNeF.get_nef_type(object.__new__(MeanShiftPanopticNeF)) == "mean_shift_panoptic_nef"
    assert MeanShiftPanopticDeltaNeF.get_nef_type(object.__new__(MeanShiftPanopticDeltaNeF)) == "mean_shift_panoptic_delta_nef"
    assert MeanShiftPanopticDDensityNeF.get_nef_type(object.__new__(MeanShiftPanopticDDensityNeF)) == "clustering_delta_panoptic_nef"


def test_package_exports():
    import pagnerf_amd
    for name in ("MeanShift", "mean_class_embedding", "estimate_bandwidth", "ClusteringNeF", "MeanShiftPanopticNeF", "MeanShiftPanopticDeltaNeF",
                 "MeanShiftPanopticDDensityNeF"):
        assert hasattr(pagnerf_amd, name), name
