#!/usr/bin/env python3
"""Map export (pagnerf_amd/map_export.py, csrc/map.hip): the finalisation of already-rendered chunks by the kernel and by the reference's
tensor-op formulation (utils/render_map.py:107-120) on the same buffers, and the whole render_points_at_depth of a small scene.

    python scripts/bench_map_export.py [--cams 42] [--height 180] [--width 320] [--iters 5] [--json profiles/map_export.json]

Default size: the reference's own call (mip 2 on BUP20 shapes: 42 x 180 x 320 = 2 419 200 rays, I = 200, render_batch 20 000).  One chunk's
buffers are synthetic (gamma(2, 40) density, alpha U(0.7, 1), depth U(0.5, 0.9), 10 % misses: about 11 % kept) and reused for every chunk of the
pass, so a pass streams 121 chunks through either form.  Device events around whole passes, both forms warmed up, alternated in one process,
median of --iters.  The tensor-op form gathers with boolean masks (one host synchronisation each, three per chunk, and its per-chunk results are
concatenated at the end); the kernel form appends behind a device counter and synchronises once per pass - counted by construction and, for the
kernel form, checked by running its append loop under `torch.cuda.set_sync_debug_mode("error")`.
Byte model per ray: 13 B read by the count pass (depth, alpha, density, hit), 13 B again by the write pass, and per KEPT ray 4 I B of instance
row + 12 B colour + 24 B base ray read and 32 B written.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def chunk_buffers(n, I, dev, seed=0):
    import pagnerf_amd
    rs = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(a).to(dev)                                            # noqa: E731
    return pagnerf_amd.RenderBuffer(density=t(rs.gamma(2.0, 40.0, (n, 1)).astype(np.float32)), alpha=t(rs.uniform(0.7, 1.0, (n, 1)).astype(np.float32)),
                                    depth=t(rs.uniform(0.5, 0.9, (n, 1)).astype(np.float32)), hit=t(rs.rand(n) > 0.1),
                                    rgb=t(rs.rand(n, 3).astype(np.float32)), inst_embedding=t(rs.rand(n, I).astype(np.float32)))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=42)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--inst", type=int, default=200)
    ap.add_argument("--render-batch", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pagnerf_amd
    import test_map_export_host as H
    from pagnerf_amd import MapAccumulator, map_points_from_buffers, render_points_at_depth
    dev = torch.device("cuda:0")
    rpc, C, nb = a.height * a.width, a.cams, a.render_batch
    total = rpc * C
    view = H.view_matrices(np.random.RandomState(1), C)
    pipe = pagnerf_amd.BAPipeline(None, torch.from_numpy(view)).to(dev)
    bo, bd = H.base_rays_np(a.height, a.width)
    base = pagnerf_amd.Rays(torch.from_numpy(bo).to(dev), torch.from_numpy(bd).to(dev))
    cams = list(range(C))
    idx = pipe.camera_indices(cams)
    rb = chunk_buffers(nb, a.inst, dev)
    tail = total % nb
    rb_tail = chunk_buffers(tail, a.inst, dev, seed=1) if tail else None
    chunks = [(s, rb if s + nb <= total else rb_tail) for s in range(0, total, nb)]
    state = {}

    def kernel_pass():
        out = MapAccumulator(total, dev)
        for s, b in chunks:
            map_points_from_buffers(pipe, base, b, idx, ray0=s, out=out)
        state["kernel"] = out.finish()                                                   # the one synchronisation

    def torch_pass():
        parts = []
        for s, b in chunks:
            n = b.depth.shape[0]
            g = torch.arange(s, s + n, device=dev)
            points = pipe.rays_to_3d_points_indexed(base.origins[g % rpc], base.dirs[g % rpc], b.depth, idx[g // rpc])
            inst = torch.argmax(b.inst_embedding, dim=-1)
            m = b.density[:, 0] > 40
            m = torch.logical_and(m, b.alpha[:, 0] > 0.9)
            m = torch.logical_and(m, b.hit)
            m = torch.logical_and(m, b.depth[:, 0] < 0.8)
            m = torch.logical_and(m, b.depth[:, 0] > 0.6)
            parts.append((points[m], inst[m], b.rgb[m]))                                  # three boolean-index gathers: three synchronisations
        state["torch"] = tuple(torch.cat([p[i] for p in parts]) for i in range(3))

    (k_med, k_min), (t_med, t_min) = timed([kernel_pass, torch_pass], a.iters)
    kp, kc, ki = state["kernel"]
    tp, ti, tc = state["torch"]
    same = bool(torch.equal(ki, ti) and torch.equal(kc, tc) and torch.allclose(kp, tp, rtol=1e-5, atol=1e-6))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                              # a host synchronisation inside the append loop would raise
    try:
        out = MapAccumulator(total, dev)
        for s, b in chunks:
            map_points_from_buffers(pipe, base, b, idx, ray0=s, out=out)
        no_sync = True
    except RuntimeError as e:
        if "synchroniz" not in str(e).lower():
            raise
        no_sync = False
    finally:
        torch.cuda.set_sync_debug_mode("default")
    kept = int(kp.shape[0])
    bytes_moved = total * 26 + kept * (4 * a.inst + 12 + 24 + 32)
    res = {"cams": C, "image": [a.height, a.width], "rays": total, "inst": a.inst, "render_batch": nb, "chunks": len(chunks), "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "kept": kept, "kept_share": round(kept / total, 4),
           "kernel_pass_ms": round(k_med, 3), "kernel_pass_min_ms": round(k_min, 3), "torch_pass_ms": round(t_med, 3), "torch_pass_min_ms": round(t_min, 3),
           "torch_over_kernel": round(t_med / k_med, 2), "same_result": same,
           "host_syncs_kernel_pass": 1, "host_syncs_torch_pass": 3 * len(chunks), "append_loop_without_sync": bool(no_sync),
           "model_bytes_per_ray": round(bytes_moved / total, 1), "model_bytes_per_kept_ray": 4 * a.inst + 68,
           "kernel_model_gb_per_s": round(bytes_moved / (k_med * 1e-3) / 1e9, 1),
           "torch_form_bytes_per_ray_at_least": 4 * a.inst + 13}

    # the whole export on a small rendered scene (the nef of the parity tests, voxel march): 6 cameras of 90 x 160
    import test_gpu_parity as T
    nef, tracer, _, _, _ = T._make_scene(dev, "bf16", N=8, S=32)
    tracer.raymarch_type, tracer.num_steps, tracer.ray_max_travel = "voxel", 2, 0.8
    v6 = H.view_matrices(np.random.RandomState(77), 6)
    v6[:, :3, 3] = np.array([0.0, 0.0, -1.1], np.float32)
    pipe6 = pagnerf_amd.BAPipeline(nef, torch.from_numpy(v6), tracer=tracer, near=0.0, far=3.0).to(dev)
    b6 = H.base_rays_np(90, 160)
    base6 = pagnerf_amd.Rays(torch.from_numpy(b6[0]).to(dev), torch.from_numpy(b6[1]).to(dev))
    th = dict(min_density=0.0, min_alpha=0.5, depth_range=(0.0, 3.0))
    (w_med, w_min), = timed([lambda: state.__setitem__("whole", render_points_at_depth(pipe6, base6, render_batch=nb, **th))], max(2, a.iters // 2))
    res.update(whole_export_rays=6 * 90 * 160, whole_export_ms=round(w_med, 3), whole_export_min_ms=round(w_min, 3),
               whole_export_kept=int(state["whole"]["points"].shape[0]))
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
