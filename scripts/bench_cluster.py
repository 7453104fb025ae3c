#!/usr/bin/env python3
"""Device mean-shift clustering (pagnerf_amd.cluster.MeanShift, csrc/cluster.hip) at the sizes of the contrastive configs' validation, against the
reference's sklearn route on the same inputs when sklearn is importable.

    python scripts/bench_cluster.py [--iters 5] [--sklearn-max-k 2000] [--json out.json]

Fit: K class centres of D dimensions (K in {2000, 8000, 20000}, D in {16, 200}; 8 blobs on the unit sphere), the whole train_clustering call -
class means, bandwidth, mean shift, ordering and suppression, and its one read-back - timed on the host after a synchronisation (median of --iters
after one warm-up).  Predict: one 720 x 1280 image of 200-wide rows in f32 and bf16 against C in {8, 64} centres, HIP events (median of 20 after 5).
sklearn: estimate_bandwidth(quantile=0.08) + MeanShift(bandwidth, bin_seeding=False, n_jobs=6).fit and predict on host copies, as
utils/clustering/mean_shift.py does (num_clustering_workers: 6), for K <= --sklearn-max-k (the record's "sklearn" entries give the time it took
on the benchmark host; larger K takes minutes there); its predict (the host copy of the image and pairwise_distances_argmin) is timed with
--sklearn-predict.

Budgets (arithmetic, not measured): fit <= 100 ms at K = 8000, D = 200; predict <= 1 ms for 921 600 x 200 f32 at C <= 64.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def centres(K, D, seed=0, n_blob=8):
    """K unit-norm centres in n_blob blobs of unequal sizes.  With fewer blobs than 1 / quantile each blob holds more than k = int(0.08 K)
    centres, so the bandwidth lies within the blobs and the fit keeps one cluster per blob (with 40 blobs it would merge them all into one)."""
    rs = np.random.RandomState(seed + K + D)
    protos = rs.standard_normal((n_blob, D))
    protos /= np.linalg.norm(protos, axis=1, keepdims=True)
    w = np.linspace(1.0, 2.0, n_blob)
    X = protos[rs.choice(n_blob, size=K, p=w / w.sum())] + rs.standard_normal((K, D)) * (0.25 / np.sqrt(D))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def bench_fit(K, D, iters, dev, sk_max):
    from pagnerf_amd.cluster import MeanShift
    X = torch.from_numpy(centres(K, D)).to(dev)[None]
    lab = torch.randperm(K, generator=torch.Generator().manual_seed(K)).to(dev)[None]
    ms = MeanShift(num_clustering_workers=6)
    ms.train_clustering(X, lab)                        # warm-up
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms.train_clustering(X, lab)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    rec = {"K": K, "D": D, "device": {"fit_ms": statistics.median(times), "bandwidth": ms.bandwidth, "clusters": int(ms.cluster_centers_.shape[0]),
                                      "n_iter": ms.n_iter_},
           "budget_fit_ms": 100.0 if (K, D) == (8000, 200) else None}
    try:
        from sklearn.cluster import MeanShift as SkMeanShift, estimate_bandwidth
    except ImportError:
        rec["sklearn"] = "not importable"
        return rec
    if K > sk_max:
        rec["sklearn"] = "skipped (K > --sklearn-max-k)"
        return rec
    host = X[0].cpu().numpy()
    t0 = time.perf_counter()
    bw = estimate_bandwidth(host, quantile=0.08)
    sk = SkMeanShift(bandwidth=bw, bin_seeding=False, n_jobs=6).fit(host)
    rec["sklearn"] = {"fit_ms": (time.perf_counter() - t0) * 1e3, "bandwidth": float(bw), "clusters": int(sk.cluster_centers_.shape[0]),
                      "n_iter": int(sk.n_iter_)}
    return rec


def bench_predict(C, dtype, dev, sk):
    from pagnerf_amd.cluster import MeanShift
    D = 200
    ms = MeanShift()
    g = torch.Generator(dev).manual_seed(C)
    ms.cluster_centers_ = torch.nn.functional.normalize(torch.randn(C, D, device=dev, generator=g), dim=-1)
    x = torch.randn(720, 1280, D, device=dev, generator=g).to(dtype)
    for _ in range(5):
        ms.predict_clusters(x)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for a, b in ev:
        a.record()
        ms.predict_clusters(x)
        b.record()
    torch.cuda.synchronize()
    ms_t = statistics.median(a.elapsed_time(b) for a, b in ev)
    gb = x.numel() * x.element_size() / 1e9
    rec = {"image": [720, 1280, D], "dtype": str(dtype).replace("torch.", ""), "C": C,
           "device": {"predict_ms": ms_t, "read_GB_per_s": gb / (ms_t / 1e3), "GFLOP_per_s": 2.0 * x.shape[0] * x.shape[1] * C * D / (ms_t / 1e3) / 1e9},
           "budget_predict_ms": 1.0 if dtype == torch.float32 else None}
    if sk and dtype == torch.float32 and C == 8:
        from sklearn.metrics import pairwise_distances_argmin
        t0 = time.perf_counter()
        host = x.reshape(-1, D).cpu().numpy()                 # the reference copies the image to the host (predict_clusters)
        pairwise_distances_argmin(host, ms.cluster_centers_.cpu().numpy())
        rec["sklearn"] = {"predict_ms_incl_copy": (time.perf_counter() - t0) * 1e3}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sklearn-max-k", type=int, default=2000)
    ap.add_argument("--sklearn-predict", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    dev = torch.device("cuda:0")
    try:
        import sklearn  # noqa: F401
        sk = True
    except ImportError:
        sk = False
    out = {"fit": [], "predict": []}
    for D in (16, 200):
        for K in (2000, 8000, 20000):
            r = bench_fit(K, D, a.iters, dev, a.sklearn_max_k)
            print(json.dumps(r), flush=True)
            out["fit"].append(r)
    for dtype in (torch.float32, torch.bfloat16):
        for C in (8, 64):
            r = bench_predict(C, dtype, dev, sk and a.sklearn_predict)
            print(json.dumps(r), flush=True)
            out["predict"].append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
