#!/usr/bin/env python3
"""SemanticNeF (pagnerf_amd/semantic_nef.py, csrc/mlp_deep.hip): the fused launch against the tensor-op form in bf16 autocast - the reference's own
formulation of the network (pc_nerf/semantic_nerf.py under the trainer's autocast) - on the same machine, in one process.

    python scripts/bench_semantic_nef.py [--sizes 1048576,5242880] [--iters 5] [--image 720x1280] [--render-batch 8000] [--json profiles/semantic_nef.json]

Three cases: the forward under no_grad (density, rgb and semantics), forward + backward (loss = a seeded linear functional of the three channels), and
one validation image through PanopticPackedRFTracer at the reference's render_batch (dense occupancy, 'ray' march, 512 samples per ray).  Device
events around whole calls, both forms warmed up and alternated, median and minimum of --iters (training step: of --iters // 2, at least 2).
Condition: the fused no_grad forward is no slower than the tensor-op form measured in the same run, at every size; where it fails the last line says
"ok": false and the exit status is 1.  Everything else is recorded, not gated.  FLOP per sample: 631 552 MAC = 1.263 MFLOP forward
(63*256 + 4*256^2 + 319*256 + 2*256^2 + 256^2 + 256 + 319*128 + 128*3 + 256*128 + 128*6), three times that for forward + backward; the fraction is of the
2.5 PF dense BF16 peak.  The clock is torch.cuda.clock_rate() sampled right after the last fused forward (None where the runtime does not report it).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAC_PER_SAMPLE = 63 * 256 + 4 * 256 ** 2 + 319 * 256 + 2 * 256 ** 2 + 256 ** 2 + 256 + 319 * 128 + 128 * 3 + 256 * 128 + 128 * 6
PEAK_BF16 = 2.5e15
ALL = {"density", "rgb", "semantics"}


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


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,5242880")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--image", default="720x1280")
    ap.add_argument("--render-batch", type=int, default=8000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pagnerf_amd
    import test_semantic_nef_host as H
    assert MAC_PER_SAMPLE == 631552
    dev = torch.device("cuda:0")
    nef = H._nef().to(dev)

    class TensorOpNeF(pagnerf_amd.SemanticNeF):
        """The same module on the tensor-op path under bf16 autocast."""

        def _fused(self, x, ray_d, channels):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = self.tensor_forward(x, ray_d, channels)
            return {k: v.float() for k, v in out.items()}
    ref = TensorOpNeF(num_classes=H.CLASSES, hidden_dim=H.HIDDEN, blas_level=3).to(dev)
    ref.load_state_dict(nef.state_dict())
    res = {"flop_per_sample_fwd": 2 * MAC_PER_SAMPLE, "peak_bf16": PEAK_BF16, "cases": []}
    gen = torch.Generator(device=dev).manual_seed(0)
    for M in [int(s) for s in a.sizes.split(",") if s]:
        x = torch.rand(M, 1, 3, device=dev, generator=gen) * 2 - 1
        d = torch.nn.functional.normalize(torch.randn(M, 3, device=dev, generator=gen), dim=-1)
        up = {"density": torch.randn(M, 1, 1, device=dev, generator=gen), "rgb": torch.randn(M, 1, 3, device=dev, generator=gen),
              "semantics": torch.randn(M, H.CLASSES, device=dev, generator=gen)}

        def fwd(n):
            with torch.no_grad():
                return n(channels=ALL, coords=x, ray_d=d)

        def step(n):
            for p in n.parameters():
                p.grad = None
            out = n(channels=ALL, coords=x, ray_d=d)
            sum((out[c] * up[c]).sum() for c in ALL).backward()
        with torch.no_grad():
            o1, o2 = fwd(nef), fwd(ref)
            agree = {c: float((o1[c] - o2[c]).abs().max()) for c in ALL}
        (f_med, f_min), (t_med, t_min) = timed([lambda: fwd(nef), lambda: fwd(ref)], a.iters)
        mhz = clock_mhz()
        (fs_med, fs_min), (ts_med, ts_min) = timed([lambda: step(nef), lambda: step(ref)], max(2, a.iters // 2))
        flop = 2.0 * MAC_PER_SAMPLE * M
        case = {"M": M, "fwd_no_grad_ms": {"fused": f_med, "fused_min": f_min, "tensor_op_bf16": t_med, "tensor_op_bf16_min": t_min},
                "fwd_bwd_ms": {"fused": fs_med, "fused_min": fs_min, "tensor_op_bf16": ts_med, "tensor_op_bf16_min": ts_min},
                "fused_fwd_tflops": flop / f_med / 1e9, "fused_fwd_frac_of_peak": flop / (f_med * 1e-3) / PEAK_BF16,
                "fused_fwd_bwd_tflops": 3 * flop / fs_med / 1e9, "fused_fwd_bwd_frac_of_peak": 3 * flop / (fs_med * 1e-3) / PEAK_BF16,
                "tensor_op_fwd_tflops": flop / t_med / 1e9, "clock_mhz_after_fused_fwd": mhz, "max_abs_fused_minus_tensor_op": agree,
                "fwd_no_grad_fused_not_slower": bool(f_med <= t_med)}
        res["cases"].append(case)
        print(json.dumps(case))
        del x, d, up, o1, o2
        torch.cuda.empty_cache()
    if a.image:
        h, w = (int(v) for v in a.image.split("x"))
        n_rays = h * w
        o = torch.tensor([0.0, 0.0, -0.9], device=dev).repeat(n_rays, 1)
        ys, xs = torch.meshgrid(torch.linspace(-0.5, 0.5, h, device=dev), torch.linspace(-0.9, 0.9, w, device=dev), indexing="ij")
        dirs = torch.nn.functional.normalize(torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(n_rays, device=dev)], -1), dim=-1)
        rays = pagnerf_amd.Rays(o, dirs, 0.0, 6.0)
        tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=512, bg_color="white")

        def image(n):
            with torch.no_grad():
                rb = pagnerf_amd.batch_render(pagnerf_amd.Pipeline(n, tracer), rays, render_batch=a.render_batch, channels={"rgb", "depth", "semantics"})
            return rb
        (i_med, i_min), (j_med, j_min) = timed([lambda: image(nef), lambda: image(ref)], a.iters)
        case = {"image": a.image, "render_batch": a.render_batch, "samples_per_ray": 512,
                "validation_image_ms": {"fused": i_med, "fused_min": i_min, "tensor_op_bf16": j_med, "tensor_op_bf16_min": j_min}}
        res["cases"].append(case)
        print(json.dumps(case))
    res["device"] = torch.cuda.get_device_name(0)
    slower = [c["M"] for c in res["cases"] if not c.get("fwd_no_grad_fused_not_slower", True)]
    res["ok"] = not slower
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"ok": res["ok"], "cases": len(res["cases"]), "fwd_no_grad_fused_slower_at_M": slower}))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
