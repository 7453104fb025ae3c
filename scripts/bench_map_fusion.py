#!/usr/bin/env python3
"""Voxel map fusion (pagnerf_amd/map_export.py, csrc/voxelmap.hip): the kernel path (VoxelMap: key kernel per chunk, two stable sorts, one
ordered-append call; instance_table: one sort, one call) and the tensor-op form (fuse_points_reference / label_table_reference moved to the
GPU) on the same device and the same points.

    python scripts/bench_map_fusion.py [--iters 5] [--json profiles/map_fusion.json]

Input: synthetic surface points seen by 42 cameras - spots on a bumpy sphere of radius 0.5, every observation the spot plus N(0, 0.002) noise
(about a quarter of a 2/256 voxel), 40 instances by spot with 10 % of the labels replaced by a random one, colours U(0, 1); generated on the device
from a seed.  Two sizes: the kept count of the mip-2 export, 11 % of 42 x 180 x 320 rays, and of the mip-0 export, 11 % of 42 x 720 x 1280; two
voxel sizes, 2/256 and 2/512.  The points arrive as 42 chunks (one add() per camera).  Device events around whole calls (fusion, then table), both
forms warmed up, alternated in one process, median of --iters.  Host synchronisations: those torch reports in its sync debug mode ("warn") during
one extra call of each form, with the source lines that caused them.  No ratio is promised or gated.
Byte model of the kernel path per point (K points, V voxels, colours present): key pass 12 B read + 8 B written; the two sorts are rocPRIM's (8 B
keys with 8 B indices, several passes each, not modelled); four gathers 8 + 8 + 12 + 12 B read and written (80 B); count pass 8 B, write pass 8 + 8 +
12 + 12 = 40 B read, and 52 B written per VOXEL.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CAMS = 42
SHARE = 0.11


def surface_cloud(K, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    spots = max(1, K // CAMS)
    d = torch.nn.functional.normalize(torch.randn(spots, 3, device=dev, generator=g), dim=-1)
    r = 0.5 + 0.05 * torch.sin(7.0 * d[:, :1]) * torch.cos(5.0 * d[:, 1:2])
    which = torch.randint(0, spots, (K,), device=dev, generator=g)
    points = (d * r)[which] + 0.002 * torch.randn(K, 3, device=dev, generator=g)
    ids = 1 + which % 40
    noisy = torch.rand(K, device=dev, generator=g) < 0.1
    ids = torch.where(noisy, torch.randint(0, 41, (K,), device=dev, generator=g), ids)
    return points.contiguous(), ids.contiguous(), torch.rand(K, 3, device=dev, generator=g)


def timed(fns, iters):
    """Alternate the callables; -> per callable (median ms, min ms)."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(statistics.median(t), min(t)) for t in ts]


def reported_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    sites = ["%s:%d" % (os.path.basename(w.filename), w.lineno) for w in seen if "synchroniz" in str(w.message).lower()]
    return {"count": len(sites), "sites": sorted(set(sites))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from pagnerf_amd import VoxelMap, fuse_points_reference, instance_table, label_table_reference
    dev = torch.device("cuda:0")
    sizes = {"mip2": int(SHARE * CAMS * 180 * 320), "mip0": int(SHARE * CAMS * 720 * 1280)}
    rows = []
    for name, K in sizes.items():
        points, ids, color = surface_cloud(K, dev)
        edges = [K * c // CAMS for c in range(CAMS + 1)]
        for cells in (256, 512):
            v = 2.0 / cells
            state = {}

            def kernel_fuse():
                vm = VoxelMap(v, device=dev)
                for s, e in zip(edges[:-1], edges[1:]):
                    vm.add(points[s:e], ids[s:e], color[s:e])
                state["kernel"] = vm.finish()

            def torch_fuse():
                state["torch"] = fuse_points_reference(points, ids, color, voxel_size=v)

            def kernel_table():
                state["kernel_table"] = instance_table(state["kernel"])

            def torch_table():
                state["torch_table"] = label_table_reference(state["kernel"])            # the same map for both tables

            (kf, kf_min), (tf, tf_min) = timed([kernel_fuse, torch_fuse], a.iters)
            (kt, kt_min), (tt, tt_min) = timed([kernel_table, torch_table], a.iters)
            k, t = state["kernel"], state["torch"]
            same = all(torch.equal(k[x], t[x]) for x in ("instances", "count", "voxels", "agreement"))
            close = max(float((k[x] - t[x]).abs().max()) for x in ("points", "color"))
            same_table = all(torch.equal(state["kernel_table"][x], state["torch_table"][x]) for x in ("ids", "voxels", "observations", "bbox_min", "bbox_max"))
            V = int(k["count"].numel())
            row = {"size": name, "points": K, "voxel_size": "2/%d" % cells, "voxels": V, "points_per_voxel": round(K / max(V, 1), 2),
                   "largest_run": int(k["count"].max()), "instances": int(state["kernel_table"]["ids"].numel()),
                   "kernel_fuse_ms": round(kf, 3), "kernel_fuse_min_ms": round(kf_min, 3), "torch_fuse_ms": round(tf, 3), "torch_fuse_min_ms": round(tf_min, 3),
                   "kernel_table_ms": round(kt, 3), "kernel_table_min_ms": round(kt_min, 3), "torch_table_ms": round(tt, 3), "torch_table_min_ms": round(tt_min, 3),
                   "torch_over_kernel_fuse": round(tf / kf, 2), "torch_over_kernel_table": round(tt / kt, 2),
                   "integers_equal": bool(same), "table_equal_except_means": bool(same_table), "largest_mean_difference": close,
                   "host_syncs_reported": {"kernel_fuse": reported_syncs(kernel_fuse), "torch_fuse": reported_syncs(torch_fuse),
                                           "kernel_table": reported_syncs(kernel_table), "torch_table": reported_syncs(torch_table)},
                   "model_bytes_kernel_fuse": K * (20 + 80 + 8 + 40) + V * 52}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del state
    res = {"device": torch.cuda.get_device_name(0), "cameras": CAMS, "kept_share": SHARE, "iters": a.iters, "chunks_per_fusion": CAMS, "runs": rows}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
