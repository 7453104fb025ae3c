#!/usr/bin/env python3
"""Connected components of the fused voxel map (pagnerf_amd/map_export.py, csrc/voxelmap.hip: pag_voxel_components): the device path
(connected_components, clean_map(mode="split")) and the CPU definitions (connected_components_reference, clean_map_reference) on the same maps.

    python scripts/bench_map_components.py [--iters 5] [--json profiles/map_components.json]

Input: two of the synthetic maps of scripts/bench_map_fusion.py, fused on the device: the mip-2 cloud at 2/256 (32 125 voxels) and the mip-0 cloud at
2/512 (572 921 voxels); 40 instances with 10 % label noise, so most ids have one large component and many specks.  The device forms get the map on
the device, the CPU forms a copy of it on the CPU made outside the timed region.  Device events around whole calls including the synchronisation,
both forms warmed up and alternated in one process, median of --iters.  Host synchronisations: those torch's sync debug mode ("warn") reports during
one extra call.  The numbers are recorded; no time or ratio is promised or gated.
Byte model of pag_voxel_components per voxel: prepare 2 x 12 B read + 12 B written; link 8 + 8 B and four searches of about log2 V 8-byte reads (the
upper levels from cache), 4 B atomics per link; flatten 4 B per step + 4 B written; count / number / label 3 x (4 + 8 + 8) B read + 8 B written.
"""
import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_map_fusion import CAMS, SHARE, surface_cloud, timed      # noqa: E402


def reported_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return len([w for w in seen if "called a synchronizing" in str(w.message)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from pagnerf_amd import _lib, VoxelMap, clean_map, clean_map_reference, connected_components, connected_components_reference
    dev = torch.device("cuda:0")
    rows = []
    for name, K, cells in (("mip2", int(SHARE * CAMS * 180 * 320), 256), ("mip0", int(SHARE * CAMS * 720 * 1280), 512)):
        points, ids, color = surface_cloud(K, dev)
        fused = VoxelMap(2.0 / cells, device=dev).add(points, ids, color).finish()
        del points, ids, color
        cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in fused.items()}
        state = {}

        def kernel_cc():
            state["kernel_cc"] = connected_components(fused)

        def cpu_cc():
            state["cpu_cc"] = connected_components_reference(cpu)

        def kernel_clean():
            state["kernel_clean"] = clean_map(fused, min_voxels=3, mode="split")

        def cpu_clean():
            state["cpu_clean"] = clean_map_reference(cpu, min_voxels=3, mode="split")

        (kc, kc_min), (cc, cc_min) = timed([kernel_cc, cpu_cc], a.iters)
        (kl, kl_min), (cl, cl_min) = timed([kernel_clean, cpu_clean], a.iters)
        k, c = state["kernel_cc"], state["cpu_cc"]
        sizes = torch.bincount(c["component"])[1:]
        same_clean = all(torch.equal(state["kernel_clean"][x].cpu(), state["cpu_clean"][x]) for x in ("points", "color", "instances", "count", "agreement",
                                                                                                    "voxels", "component"))
        V = int(cpu["instances"].numel())
        row = {"size": name, "voxel_size": "2/%d" % cells, "voxels": V, "components": c["components"], "largest_component": int(sizes.max()),
               "single_voxel_components": int((sizes == 1).sum()), "voxels_after_clean": int(state["cpu_clean"]["component"].numel()),
               "components_after_clean": int(state["cpu_clean"]["component"].max()),
               "kernel_components_ms": round(kc, 3), "kernel_components_min_ms": round(kc_min, 3), "cpu_components_ms": round(cc, 3),
               "cpu_components_min_ms": round(cc_min, 3), "kernel_clean_ms": round(kl, 3), "kernel_clean_min_ms": round(kl_min, 3),
               "cpu_clean_ms": round(cl, 3), "cpu_clean_min_ms": round(cl_min, 3),
               "cpu_over_kernel_components": round(cc / kc, 1), "cpu_over_kernel_clean": round(cl / kl, 1),
               "components_equal": bool(k["components"] == c["components"] and torch.equal(k["component"].cpu(), c["component"])),
               "clean_equal": bool(same_clean),
               "host_syncs_reported": {"connected_components": reported_syncs(kernel_cc), "clean_map": reported_syncs(kernel_clean)},
               "workspace_bytes_per_voxel": round(int(_lib.load().pag_voxel_components_workspace_bytes(V)) / V, 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del state, fused, cpu
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "connectivity": 26, "min_voxels": 3, "mode": "split", "runs": rows}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
