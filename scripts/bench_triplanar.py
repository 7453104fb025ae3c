#!/usr/bin/env python3
"""TriplanarGridHIP (pagnerf_amd/triplanar.py, csrc/triplanar.hip): the grid kernels against the grid's own tensor-op form (per level three
grid_sample calls and their sum: 12 launches plus the sums per direction at 4 levels) on the same machine, in one process.

    python scripts/bench_triplanar.py [--rays 4096] [--iters 5] [--json profiles/triplanar.json]

The shape is configs/bup20/mean_shift_contrastive_app.yaml:137-144: base_lod 5, 4 levels, F = 4, feature_std 0.01.  Rows:
  grid_fwd            the grid alone under no_grad on samples marched along rays (--rays x 512 steps, ray order), fp32 and bf16 output
  grid_fwd_bwd        forward + table gradient, upstream gradients dense ("untrained") and with 85 % of the samples' gradients exactly zero in runs
                      along the rays ("trained_like")
  grid_fwd_bwd_xyz    the same with the position gradient (pose optimisation is on in the configuration that selects this grid)
  train_step          zero_grad + trace (rgb, semantics, inst_embedding; stage='train') + loss + backward + optim.Adam step of MeanShiftPanopticNeF
                      at --rays x 512 samples, eager launches
  render_chunk        one render_batch = 8000 validation chunk under no_grad
The grid rows also time the tensor-op form on contiguous planes in the REFERENCE's layout ([1,F,R,R]), so that the stored channel-last layout is not
what the comparison rests on.  Device events around whole calls, both forms warmed up and alternated, median and minimum of --iters.
Condition: the kernel path is faster than the tensor-op path in every row; a row where it is not says so, the last line says "ok": false and the exit
status is 1.  Derived figures: gather bytes/s of the forward = M x 48 taps x 16 B / time; atomic bytes/s of the table gradient as an UPPER bound =
(samples with a non-zero gradient) x 48 x 16 B / (fwd_bwd - fwd) - the kernel merges consecutive samples of a cell before it adds - against
1.3 TB/s of float atomics chip-wide.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 512
GRID = dict(feature_dim=4, base_lod=5, num_lods=4, feature_std=0.01)
TAP_BYTES = 4 * 12 * 4 * 4          # levels x (3 planes x 4 taps) x F floats


def timed(fns, iters):
    """Alternate the callables; -> per callable (median ms, min ms)."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
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


def make_rays(n, dev, seed=0):
    import pagnerf_amd
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(n, 3, generator=g) * 0.6 - 0.3
    o[:, 2] = -1.6
    d = F.normalize(torch.stack([torch.rand(n, generator=g) * 0.5 - 0.25, torch.rand(n, generator=g) * 0.5 - 0.25, torch.ones(n)], -1), dim=-1)
    return pagnerf_amd.Rays(o.to(dev), d.to(dev), 0.5, 2.9)        # 512 steps over 2.4: ~430 of them inside the cube, step 0.0047


def row(name, cond, k, t, extra=None):
    r = {"row": name, "condition": cond, "kernel_ms": k[0], "kernel_min_ms": k[1], "tensor_op_ms": t[0], "tensor_op_min_ms": t[1],
         "ratio_tensor_op_over_kernel": t[0] / k[0], "kernel_faster": bool(k[0] < t[0])}
    r.update(extra or {})
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pagnerf_amd
    from pagnerf_amd import optim
    from pagnerf_amd import triplanar as TP
    dev = torch.device("cuda:0")
    rows = []
    torch.manual_seed(0)
    grid = pagnerf_amd.TriplanarGridHIP(blas_level=7, **GRID).to(dev)
    rays = make_rays(a.rays, dev)
    _, _, samples, _, _, _ = grid.raymarch(rays, num_samples=STEPS, raymarch_type="ray")
    x = samples.reshape(-1, 3).contiguous()
    M = x.shape[0]
    ref_planes = [[t.detach().contiguous().requires_grad_(True) for t in level] for level in grid.planes()]      # the reference's layout as leaves

    def fwd(kernel, dtype=torch.float32):
        grid.use_kernel = kernel
        with torch.no_grad():
            return grid.interpolate_scaled(x[:, None], out_dtype=dtype)

    def fwd_ref():
        with torch.no_grad():
            return TP.triplanar_tensor_forward(ref_planes, x)
    k, t, r = timed([lambda: fwd(True), lambda: fwd(False), fwd_ref], a.iters)
    fwd_k = k[0]
    rows.append(row("grid_fwd", "fp32 out", k, t, {"M": M, "tensor_op_reference_layout_ms": r[0], "kernel_gather_TBps": M * TAP_BYTES / k[0] / 1e9}))
    k, t = timed([lambda: fwd(True, torch.bfloat16), lambda: fwd(False, torch.bfloat16)], a.iters)
    rows.append(row("grid_fwd", "bf16 out", k, t, {"M": M, "kernel_gather_TBps": M * TAP_BYTES / k[0] / 1e9}))
    gen = torch.Generator(device=dev).manual_seed(1)
    G = torch.randn(M, 16, device=dev, generator=gen)
    live = ((torch.arange(M, device=dev) // 64) % 20) < 3            # runs of 64 consecutive samples, 15 % of them live
    for need_x in (False, True):
        for cond, m in (("untrained", None), ("trained_like", live)):
            g1 = G if m is None else G * m[:, None]
            n_live = M if m is None else int(m.sum())

            def step(kernel):
                grid.use_kernel = kernel
                grid.tables.grad = None
                xx = x.detach().requires_grad_(need_x)
                (grid.interpolate_scaled(xx[:, None]) * g1).sum().backward()

            def step_ref():
                for p in [q for level in ref_planes for q in level]:
                    p.grad = None
                xx = x.detach().requires_grad_(need_x)
                (TP.triplanar_tensor_forward(ref_planes, xx) * g1).sum().backward()
            k, t, r = timed([lambda: step(True), lambda: step(False), step_ref], a.iters)
            bwd = max(k[0] - fwd_k, 1e-6)
            rows.append(row("grid_fwd_bwd_xyz" if need_x else "grid_fwd_bwd", cond, k, t,
                            {"M": M, "live_samples": n_live, "tensor_op_reference_layout_ms": r[0], "kernel_bwd_ms": bwd,
                             "kernel_bwd_atomic_TBps_upper_bound": None if need_x else n_live * TAP_BYTES / bwd / 1e9, "atomic_rate_TBps_chip": 1.3}))
    del G, x, samples, ref_planes, grid
    torch.cuda.empty_cache()
    # full training step and a validation chunk through the tracer
    torch.manual_seed(0)
    nef = pagnerf_amd.MeanShiftPanopticNeF(grid_type="TriplanarGrid", num_classes=7, num_instances=16, sem_softmax=True, inst_normalize=True,
                                           inst_detach=False, blas_level=7, **GRID).to(dev)
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=STEPS, bg_color="white", use_graphs=False)
    step_rays = make_rays(a.rays, dev, seed=2)
    target = torch.rand(a.rays, 3, device=dev)
    opt = optim.Adam(nef.parameters(), lr=1e-3, eps=1e-15)

    def train(kernel):
        nef.grid.use_kernel = kernel
        opt.zero_grad(set_to_none=True)
        rb = tracer(nef, channels={"rgb", "semantics", "inst_embedding"}, rays=step_rays, stage="train")
        loss = ((rb.rgb - target) ** 2).mean() - 0.1 * torch.log(rb.semantics.float()[:, 0] + 1e-27).mean() + 0.1 * rb.inst_embedding.float().pow(2).mean()
        loss.backward()
        opt.step()
    k, t = timed([lambda: train(None), lambda: train(False)], max(3, a.iters // 2 + 1))
    rows.append(row("train_step", "untrained", k, t, {"rays": a.rays, "steps": STEPS}))
    chunk = make_rays(8000, dev, seed=3)

    def render(kernel):
        nef.grid.use_kernel = kernel
        with torch.no_grad():
            return tracer(nef, channels={"rgb", "semantics", "inst_embedding"}, rays=chunk, stage="val")
    k, t = timed([lambda: render(None), lambda: render(False)], a.iters)
    rows.append(row("render_chunk", "untrained", k, t, {"rays": 8000, "steps": STEPS}))
    slower = [(r["row"], r["condition"]) for r in rows if not r["kernel_faster"]]
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "ok": not slower, "kernel_not_faster_in": slower}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps({"ok": out["ok"], "rows": len(rows), "kernel_not_faster_in": slower}))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
