#!/usr/bin/env python3
"""PanopticLiftingNeF (pagnerf_amd/panoptic_lifting.py, csrc/vm.hip): the grid kernels against the nef's own tensor-op path (the reference's
arithmetic: 12 grid_sample calls, a [144,M] product, a 144 -> 27 Linear) on the same machine, in one process.

    python scripts/bench_panoptic_lifting.py [--rays 4096] [--step-rays 12288] [--iters 5] [--json profiles/panoptic_lifting.json]

Rows, each at R = 128 and R = 192:
  grid_fwd          the grid alone under no_grad on samples marched along rays (512 steps, ray order)
  grid_fwd_bwd      forward + backward of the grid, upstream gradients dense ("untrained") and with 85 % of the samples' gradients exactly zero in
                    runs along the rays ("trained_like")
  train_step        zero_grad + trace (rgb, stage='train') + loss + backward + optim.Adam step at the configuration's shape (--step-rays x 512),
                    on the untrained scene (every sample carries gradient) and on a trained-like one (density positive in a slab holding 15 % of the
                    samples, so the rest have zero density, zero weight and exactly zero gradients)
  render_chunk      one render_batch = 8000 validation chunk (rgb, semantics, inst_embedding) under no_grad
The grid rows also time the tensor-op form on contiguous tables in the REFERENCE's layout ([1,C,R,R]), so that the stored channel-last layout is
not what the comparison rests on.  Device events around whole calls, both forms warmed up and alternated, median and minimum of --iters.
Condition: the kernel path is not slower than the tensor-op path in any row; a row where it is says so, the last line says "ok": false and the exit
status is 1.  Derived figures: gather bytes/s of the forward = M x 18 taps x 64 components x 4 B / time; atomic bytes/s of the backward as an UPPER
bound = (samples with a non-zero gradient) x 18 x 64 x 4 B / (fwd_bwd - fwd) - the kernel merges consecutive samples of a cell before it adds, so
the bytes that really leave the CU are fewer; against 1.3 TB/s of float atomics chip-wide.
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

TAP_BYTES = 18 * 64 * 4
STEPS = 512


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


def slab_density(nef):
    """Trained-like density: +30 inside |z| < 0.15, -1 outside (component 0 of plane 0 = 1, of line 0 = the profile, every other component 0)."""
    f = nef.grid.features
    with torch.no_grad():
        for t in list(f.density_plane) + list(f.density_line):
            t.zero_()
        f.density_plane[0][..., 0] = 1.0
        z = torch.linspace(-1, 1, f.res, device=f.density_line[0].device)
        f.density_line[0][:, 0] = torch.where(z.abs() < 0.15, torch.full_like(z, 30.0), torch.full_like(z, -1.0))


def row(name, res, cond, k, t, extra=None):
    r = {"row": name, "res": res, "condition": cond, "kernel_ms": k[0], "kernel_min_ms": k[1], "tensor_op_ms": t[0], "tensor_op_min_ms": t[1],
         "ratio_tensor_op_over_kernel": t[0] / k[0], "kernel_not_slower": bool(k[0] <= t[0])}
    r.update(extra or {})
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--step-rays", type=int, default=12288)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--resolutions", default="128,192")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pagnerf_amd
    from pagnerf_amd import optim
    from pagnerf_amd import panoptic_lifting as PL
    dev = torch.device("cuda:0")
    rows = []
    for res in [int(v) for v in a.resolutions.split(",")]:
        torch.manual_seed(0)
        nef = pagnerf_amd.PanopticLiftingNeF(num_classes=7, num_instances=16, sem_num_layers=5, sem_hidden_dim=256, inst_num_layers=3, inst_hidden_dim=256,
                                             sem_softmax=True, inst_softmax=True, base_resolution=res, max_resolution=res + 16, num_resolution=2).to(dev)
        f = nef.grid.features
        rays = make_rays(a.rays, dev)
        ridx, _, samples, _, _, _ = nef.grid.raymarch(rays, num_samples=STEPS, raymarch_type="ray")
        x = samples.reshape(-1, 3).contiguous()
        M = x.shape[0]
        # the reference's layout as contiguous leaves
        ref_tables = [[PL.plane_to_reference(t.detach()).contiguous().requires_grad_(True) for t in f.density_plane],
                      [PL.line_to_reference(t.detach()).contiguous().requires_grad_(True) for t in f.density_line],
                      [PL.plane_to_reference(t.detach()).contiguous().requires_grad_(True) for t in f.app_plane],
                      [PL.line_to_reference(t.detach()).contiguous().requires_grad_(True) for t in f.app_line]]
        ref_basis = f.basis_mat.weight.detach().clone().requires_grad_(True)

        def fwd(kernel):
            with torch.no_grad():
                return f(x, use_kernel=kernel)

        def fwd_ref():
            with torch.no_grad():
                return PL.vm_tensor_forward(*ref_tables, ref_basis, x)
        k, t, r = timed([lambda: fwd(True), lambda: fwd(False), fwd_ref], a.iters)
        fwd_k = k[0]
        rows.append(row("grid_fwd", res, "marched", k, t, {"M": M, "tensor_op_reference_layout_ms": r[0], "kernel_gather_TBps": M * TAP_BYTES / k[0] / 1e9}))
        gen = torch.Generator(device=dev).manual_seed(1)
        gs, ga = torch.randn(M, device=dev, generator=gen), torch.randn(M, 27, device=dev, generator=gen)
        live = ((torch.arange(M, device=dev) // 64) % 20) < 3            # runs of 64 consecutive samples, 15 % of them live
        for cond, m in (("untrained", None), ("trained_like", live)):
            g1, g2 = (gs, ga) if m is None else (gs * m, ga * m[:, None])
            n_live = M if m is None else int(m.sum())

            def step(kernel):
                for p in f.parameters():
                    p.grad = None
                s, ap_ = f(x, use_kernel=kernel)
                ((s * g1).sum() + (ap_ * g2).sum()).backward()

            def step_ref():
                for p in [q for grp in ref_tables for q in grp] + [ref_basis]:
                    p.grad = None
                s, ap_ = PL.vm_tensor_forward(*ref_tables, ref_basis, x)
                ((s * g1).sum() + (ap_ * g2).sum()).backward()
            k, t, r = timed([lambda: step(True), lambda: step(False), step_ref], a.iters)
            bwd = max(k[0] - fwd_k, 1e-6)
            rows.append(row("grid_fwd_bwd", res, cond, k, t, {"M": M, "live_samples": n_live, "tensor_op_reference_layout_ms": r[0],
                                                              "kernel_bwd_atomic_TBps_upper_bound": n_live * TAP_BYTES / bwd / 1e9,
                                                              "atomic_rate_TBps_chip": 1.3}))
        del gs, ga, x, samples, ref_tables
        torch.cuda.empty_cache()
        # full training step and a validation chunk through the tracer
        tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=STEPS, bg_color="white")
        step_rays = make_rays(a.step_rays, dev, seed=2)
        target = torch.rand(a.step_rays, 3, device=dev)
        for cond in ("untrained", "trained_like"):
            if cond == "trained_like":
                slab_density(nef)
            opt = optim.Adam([{"params": [p for n, p in nef.named_parameters() if n.startswith("grid.")], "lr": 0.02},
                              {"params": [p for n, p in nef.named_parameters() if not n.startswith("grid.")], "lr": 0.001}], eps=1e-15)
            state = {"kernel": None}
            real = nef.grid.interpolate
            nef.grid.interpolate = lambda *p, **kw: real(*p, **{**kw, "use_kernel": state["kernel"]})

            def train(kernel):
                state["kernel"] = kernel
                opt.zero_grad(set_to_none=True)
                rb = tracer(nef, channels={"rgb"}, rays=step_rays, stage="train")
                ((rb.rgb - target) ** 2).mean().backward()
                opt.step()
            k, t = timed([lambda: train(None), lambda: train(False)], max(3, a.iters // 2 + 1))
            rows.append(row("train_step", res, cond, k, t, {"rays": a.step_rays, "steps": STEPS}))
            if cond == "untrained":
                chunk = make_rays(8000, dev, seed=3)

                def render(kernel):
                    state["kernel"] = kernel
                    with torch.no_grad():
                        return tracer(nef, channels={"rgb", "semantics", "inst_embedding"}, rays=chunk, stage="val")
                k, t = timed([lambda: render(None), lambda: render(False)], a.iters)
                rows.append(row("render_chunk", res, cond, k, t, {"rays": 8000, "steps": STEPS}))
            del nef.grid.interpolate
            del opt
            torch.cuda.empty_cache()
        del nef
        torch.cuda.empty_cache()
    slower = [(r["row"], r["res"], r["condition"]) for r in rows if not r["kernel_not_slower"]]
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "ok": not slower, "kernel_slower_in": slower}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps({"ok": out["ok"], "rows": len(rows), "kernel_slower_in": slower}))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
