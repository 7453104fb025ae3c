#!/usr/bin/env python3
"""Matching and merging two windows' fused maps (pagnerf_amd/map_export.py, csrc/voxelmap.hip: pag_voxel_overlap / pag_overlap_cost /
pag_voxel_merge): associate_maps and merge_maps on the device against the CPU definitions on the same maps.

    python scripts/bench_map_merge.py [--iters 5] [--json profiles/map_merge.json]

Input: scripts/bench_map_fusion.py's synthetic surface cloud at its first and last rows (the mip-2 count at 2/256, the mip-0 count at 2/512), cut
into two windows along x - the points with x < 0.17 and those with x > -0.17, so that about half of each window's surface lies in the other - and
fused window by window; the second window's ids are permuted.  Device events around whole calls including their synchronisations, the device form and
the definition alternated in one process, median of --iters.  The join alone (ops.voxel_overlap) is also timed with and without the wave-level
combining of its adds, on the windows as they are and with every id set to 0 (one pair owns every shared voxel: all adds on one address).  Host synchronisations: those torch's sync debug mode ("warn") reports
during one extra call ("called a synchronizing ..."; the mode's own notice on being switched on is not one), with their source lines.
No time or ratio is promised or gated."""
import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def reported_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    sites = ["%s:%d" % (os.path.basename(w.filename), w.lineno) for w in seen if "called a synchronizing" in str(w.message)]
    return {"count": len(sites), "sites": sorted(set(sites))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from bench_map_fusion import CAMS, SHARE, surface_cloud, timed
    from pagnerf_amd import VoxelMap, associate_maps, associate_maps_reference, merge_maps, merge_maps_reference, ops
    dev = torch.device("cuda:0")
    rows = []
    for name, K, cells in (("mip2", int(SHARE * CAMS * 180 * 320), 256), ("mip0", int(SHARE * CAMS * 720 * 1280), 512)):
        points, ids, color = surface_cloud(K, dev)
        perm = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), 1 + torch.randperm(40, device=dev, generator=torch.Generator(device=dev).manual_seed(1))))
        maps = []
        for keep, relabel in ((points[:, 0] < 0.17, False), (points[:, 0] > -0.17, True)):
            i = perm[ids[keep]] if relabel else ids[keep]
            maps.append(VoxelMap(2.0 / cells, device=dev).add(points[keep], i, color[keep]).finish())
        wa, wb = maps
        ca, cb = ({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in m.items()} for m in maps)
        state = {}

        def dev_assoc():
            state["da"] = associate_maps(wa, wb)

        def cpu_assoc():
            state["ca"] = associate_maps_reference(ca, cb)

        def dev_merge():
            state["dm"] = merge_maps(wa, wb)

        def cpu_merge():
            state["cm"] = merge_maps_reference(ca, cb)

        (ka, ka_min), (ta, ta_min) = timed([dev_assoc, cpu_assoc], a.iters)
        (km, km_min), (tm, tm_min) = timed([dev_merge, cpu_merge], a.iters)
        same = all(torch.equal(state["da"][k].cpu(), state["ca"][k]) for k in ("table", "iou", "pairs", "mapping"))
        same_merge = all(torch.equal(state["dm"][k].cpu(), state["cm"][k]) for k in ("points", "color", "instances", "count", "agreement", "voxels"))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        join = {}
        for what, (ia, ib) in (("windows", (wa["instances"], wb["instances"])), ("one_pair", (torch.zeros_like(wa["instances"]), torch.zeros_like(wb["instances"])))):
            ua, ub = ia.unique(), ib.unique()
            fns = [lambda c=c: ops.voxel_overlap(wa["voxels"], ia, ua, wb["voxels"], ib, ub, status, combine=c) for c in (True, False)]
            (on, on_min), (off, off_min) = timed(fns, a.iters)
            join[what] = {"combined_ms": round(on, 4), "combined_min_ms": round(on_min, 4), "plain_ms": round(off, 4), "plain_min_ms": round(off_min, 4),
                          "largest_entry": int(fns[0]()["table"].max())}
        row = {"size": name, "voxel_size": "2/%d" % cells, "voxels_a": int(wa["count"].numel()), "voxels_b": int(wb["count"].numel()),
               "shared_voxels": int(state["ca"]["table"].sum()), "merged_voxels": int(state["cm"]["count"].numel()), "pairs": int(state["ca"]["pairs"].shape[0]),
               "device_associate_ms": round(ka, 3), "device_associate_min_ms": round(ka_min, 3), "cpu_associate_ms": round(ta, 3), "cpu_associate_min_ms": round(ta_min, 3),
               "device_merge_ms": round(km, 3), "device_merge_min_ms": round(km_min, 3), "cpu_merge_ms": round(tm, 3), "cpu_merge_min_ms": round(tm_min, 3),
               "association_equal": bool(same), "merge_equal": bool(same_merge), "join_three_launches": join,
               "host_syncs_reported": {"associate_maps": reported_syncs(dev_assoc), "merge_maps": reported_syncs(dev_merge)}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "runs": rows}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
