#!/usr/bin/env python3
"""The 128-wide decoders (pagnerf_amd/csrc/mlp_h128.hip through ops.fused_mlp128) against the tensor-op form and against the 64-wide family, on the same
machine, in one process.

    python scripts/bench_wide_decoder.py [--M 2097152] [--iters 7] [--rays 4096] [--samples 512] [--steps 10] [--json profiles/wide_decoder.json]

Per decoder shape of configs/bup20/config_hp_base.yaml at hidden width 128 (density 48 -> 16, colour 16 + 27 -> 3 with the per-ray view embedding,
semantics 48 -> 20 softmax, instances 48 -> 200 softmax; the grid features in the encoders' XCD8 layout) and M samples:
  * forward under no_grad, and forward + backward (loss = a seeded linear functional of the output),
  * ops.fused_mlp128, ops.wide_mlp_reference under bf16 autocast (the reference's formulation), and ops.fused_mlp on the same shape at width 64.
Then one headline-shaped training trace + backward (PanopticPackedRFTracer, HIP graphs, all four channels, `--rays` x `--samples`) of a nef with
inst_hidden_dim=128 against the same nef at inst_hidden_dim=64.
Device events around windows of 20 forward calls / 5 forward + backward calls / 1 training step, the forms warmed up and alternated; median and
minimum of --iters windows, per call.  Nothing is gated: the numbers are recorded
(DESIGN.md 4.25), and a shape where the fused launch is not faster than the tensor-op form is listed as such in the last line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, in_dim, hidden layers, out_dim, activation (0 none, 1 sigmoid, 2 softmax), bf16 out, k1 of a strided x1 followed by x2 (None: XCD8 features)
SHAPES = [("density", 48, 1, 16, 0, True, None), ("colour", 43, 2, 3, 1, False, 16), ("semantics", 48, 2, 20, 2, True, None),
          ("instances", 48, 1, 200, 2, True, None)]


def timed(fns, iters, reps=1):
    """Alternate the callables; a timed window is `reps` back-to-back calls between two device events (a single 0.1 ms launch would be timed by the
    host path that issues it, not by the kernel; with the queue kept full the window is device time); -> per callable (median, min) ms PER CALL."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) / reps)
    return [(statistics.median(t), min(t)) for t in ts]


FWD_REPS, STEP_REPS = 20, 5          # calls per timed window


def decoder_case(name, in_dim, n_hidden, out_dim, act, out_bf16, k1, M, iters, dev, gen):
    from pagnerf_amd import ops
    odt = torch.bfloat16 if out_bf16 else torch.float32

    def params(width):
        dims = [in_dim] + [width] * n_hidden + [out_dim]
        W = [(torch.randn(dims[i + 1], dims[i], device=dev, generator=gen) / dims[i] ** 0.5).requires_grad_(True) for i in range(len(dims) - 1)]
        b = [(torch.randn(dims[i + 1], device=dev, generator=gen) * 0.1).requires_grad_(True) for i in range(len(dims) - 1)]
        return W, b
    P128, P64 = params(128), params(64)
    if k1 is None:
        x = torch.randn(M, in_dim, device=dev, generator=gen)
        x8 = torch.zeros(8, M, 8, device=dev)
        for p, c in enumerate(ops.xcd8_columns(in_dim // 2, 2)):
            if c >= 0:
                x8[p >> 3, :, p & 7] = x[:, c]
        x1, grouped, x2, idx, dense = x8.bfloat16().requires_grad_(True), (in_dim // 2, 2), None, None, x.bfloat16().requires_grad_(True)
        del x, x8
    else:
        R = 4096
        x1 = torch.randn(M, k1, device=dev, generator=gen).bfloat16().requires_grad_(True)
        x2 = torch.zeros(R, 32, device=dev)
        x2[:, :in_dim - k1] = torch.randn(R, in_dim - k1, device=dev, generator=gen)
        idx = torch.arange(M, device=dev, dtype=torch.int32) // ((M + R - 1) // R)
        grouped, dense = None, None
    up = torch.randn(M, out_dim, device=dev, generator=gen).to(odt)

    def fused(op, P):
        return op(x1, P[0], P[1], x2=x2, x2_index=idx, in_dim=in_dim, out_act=act, out_dtype=odt, x1_grouped=grouped)

    def tensor_op():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            xin = dense if dense is not None else torch.cat([x1, x2[idx.long(), :in_dim - k1].to(x1.dtype)], -1)
            return ops.wide_mlp_reference(xin, P128[0], P128[1], act).to(odt)
    forms = {"fused_128": lambda: fused(ops.fused_mlp128, P128), "tensor_op_bf16_128": tensor_op, "fused_64": lambda: fused(ops.fused_mlp, P64)}

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def step(fn):
        def run():
            for t in [x1] + ([dense] if dense is not None else []) + P128[0] + P128[1] + P64[0] + P64[1]:
                t.grad = None
            (fn().float() * up).sum().backward()
        return run
    with torch.no_grad():
        agree = float((forms["fused_128"]().float() - forms["tensor_op_bf16_128"]().float()).abs().max())
    names = list(forms)
    fwd = timed([no_grad(forms[n]) for n in names], iters, FWD_REPS)
    both = timed([step(forms[n]) for n in names], iters, STEP_REPS)
    case = {"decoder": name, "M": M, "calls_per_window": {"fwd_no_grad": FWD_REPS, "fwd_bwd": STEP_REPS}, "in_dim": in_dim, "hidden_layers": n_hidden, "out_dim": out_dim, "max_abs_fused_minus_tensor_op": agree,
            "fwd_no_grad_ms": {n: {"median": fwd[i][0], "min": fwd[i][1]} for i, n in enumerate(names)},
            "fwd_bwd_ms": {n: {"median": both[i][0], "min": both[i][1]} for i, n in enumerate(names)}}
    mac = in_dim * 128 + (n_hidden - 1) * 128 * 128 + 128 * out_dim
    case["fused_128_fwd_tflops"] = 2.0 * mac * M / fwd[0][0] / 1e9
    return case


def train_case(rays, samples, steps, dev):
    """Trace + loss + backward of the headline shape (bench.py's permuto model, 'ray' march, every sample kept) per instance-head width."""
    import pagnerf_amd
    out = {}
    for width in (64, 128):
        torch.manual_seed(0)
        nef = pagnerf_amd.PanopticDeltaNeF(grid_type="PermutoGrid", num_lods=24, capacity_log_2=18, delta_capacity_log_2=18, coarsest_scale=1.0,
                                           finest_scale=1e-4, feature_dim=2, num_classes=6, num_instances=200, sem_num_layers=1, sem_softmax=True,
                                           inst_num_layers=2, inst_softmax=True, inst_hidden_dim=width, panoptic_features_type="delta", hidden_dim=64,
                                           num_layers=1, view_multires=4, precision="bf16", blas_level=7)
        for g in (nef.grid, nef.delta_grid):
            g.init_from_scales(tables=torch.randn(24, 2 ** 18, 2) * 1e-2)
        nef = nef.to(dev)
        tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=samples, bg_color="white", use_graphs=True)
        gen = torch.Generator().manual_seed(1)
        o = ((torch.rand(rays, 3, generator=gen) - 0.5) * 0.6).to(dev)
        d = torch.nn.functional.normalize(torch.randn(rays, 3, generator=gen), dim=-1).to(dev)
        r = pagnerf_amd.Rays(o, d, 0.0, 2.0)
        gt, sem_gt, inst_gt = torch.rand(rays, 3, generator=gen).to(dev), torch.randint(0, 6, (rays,), generator=gen).to(dev), torch.randint(0, 200, (rays,), generator=gen).to(dev)
        F = torch.nn.functional

        def step():
            for p in nef.parameters():
                p.grad = None
            rb = tracer(nef, channels={"rgb", "depth", "semantics", "inst_embedding"}, rays=r, stage="train")
            loss = 10.0 * torch.abs(rb.rgb - gt).mean() + 0.1 * F.nll_loss(torch.log(rb.semantics.float() + 1e-27), sem_gt) \
                + 1000.0 * F.nll_loss(torch.log(rb.inst_embedding.float() + 1e-27), inst_gt)
            loss.backward()
        for _ in range(4):
            step()
        (med, mn), = timed([step], steps)
        out["inst_hidden_dim_%d" % width] = {"median": med, "min": mn, "graph_replays": tracer._graphs.replays}
        del nef, tracer
        torch.cuda.empty_cache()
    return {"train_trace_backward_ms": out, "rays": rays, "samples": samples}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=2097152)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "cases": []}
    for shape in SHAPES:
        case = decoder_case(*shape, a.M, a.iters, dev, gen)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        torch.cuda.empty_cache()
    if a.rays:
        case = train_case(a.rays, a.samples, a.steps, dev)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    slower = [c["decoder"] + "/" + k for c in res["cases"] if "decoder" in c for k in ("fwd_no_grad_ms", "fwd_bwd_ms")
              if c[k]["fused_128"]["median"] > c[k]["tensor_op_bf16_128"]["median"]]
    res["fused_128_not_faster_than_tensor_op"] = slower
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"cases": len(res["cases"]), "fused_128_not_faster_than_tensor_op": slower}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
