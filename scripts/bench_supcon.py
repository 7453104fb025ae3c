#!/usr/bin/env python3
"""Fused supervised-contrastive loss (pagnerf_amd.loss.SupConLoss, csrc/supcon.hip) against a tensor-op statement of the same formula, at the
trainer's shapes: 6 x 4096 x 200 with ~15 % of the rays masked out (the instance call of configs with inst_loss: sup_contrastive) and 6 x 4096 x 6
without a mask (the contrast_sem_weight call).

    python scripts/bench_supcon.py [--iters 20] [--warmup 5] [--json out.json]

Times forward and forward + backward with HIP events (median of --iters after --warmup), prints ms, the achieved TFLOP/s of the fused kernels against
the 155 TF f32-MFMA rate (forward 2 n^2 Dp per image, backward 4 n^2 Dp, Dp = D rounded up to 16, n = anchors), and the peak allocated memory.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 155.0


def tensor_op_supcon(x, labels, anchor_mask, T=0.07, Tb=0.07, pn_ratio=0.5):
    """The formula with tensor ops, one image at a time (what the reference's loop does): [n, n] logits, masks and exponentials per image."""
    pw, nw = min(1.0, 2 * pn_ratio), min(1.0, 2 * (1 - pn_ratio))
    f = torch.nn.functional.normalize(x, dim=-1)
    total = x.new_zeros(1)
    for b in range(x.shape[0]):
        fb, lb = (f[b][anchor_mask[b]], labels[b][anchor_mask[b]]) if anchor_mask is not None else (f[b], labels[b])
        if anchor_mask is not None and (fb.shape[0] == 0 or lb.unique().numel() < 2):
            continue
        A = fb @ fb.T / T
        lg = A - A.max(1, keepdim=True).values.detach()
        off = 1.0 - torch.eye(fb.shape[0], device=x.device)
        pos = (lb[:, None] == lb[None, :]).float() * off
        lse = torch.log((torch.exp(lg) * off).sum(1, keepdim=True))
        loss = -(T / Tb) * (pos * (pw * lg - nw * lse)).sum(1) / (pos.sum(1) + 1e-16)
        total = total + (loss.sum() / anchor_mask.sum() if anchor_mask is not None else loss.sum() / labels.numel())
    return total


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def run(name, D, masked, iters, warmup):
    from pagnerf_amd.loss import SupConLoss
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    B, P = 6, 4096
    x = torch.randn(B, P, D, generator=gen)
    if D == 6:
        x = torch.softmax(2 * x, -1) + 1e-27
    x = x.to(dev).requires_grad_(True)
    labels = torch.randint(0, 40 if D > 6 else 6, (B, P), generator=gen).to(dev)
    mask = (torch.rand(B, P, generator=gen) > 0.15).to(dev) if masked else None
    fused = SupConLoss()
    n = mask.sum(1).double() if masked else torch.full((B,), float(P), dtype=torch.float64)
    Dp = (D + 15) // 16 * 16
    sq = float((n * n).sum())
    flop_f, flop_b = 2 * sq * Dp, 4 * sq * Dp
    out = {"case": name, "B": B, "P": P, "D": D, "anchors": int(n.sum())}
    for impl, fn in (("fused", lambda: fused(x, labels, reduction="mean", anchor_mask=mask)), ("tensor_ops", lambda: tensor_op_supcon(x, labels, mask))):
        def fb():
            x.grad = None
            fn().sum().backward()

        def fwd():
            with torch.no_grad():
                fn()
        r = {"fwd_ms": timed(fwd, iters, warmup), "fwd_bwd_ms": timed(fb, iters, warmup)}
        torch.cuda.synchronize()
        x.grad = None
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fb()
        torch.cuda.synchronize()
        r["peak_extra_MB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        if impl == "fused":
            r["fwd_TFLOPs"] = flop_f / r["fwd_ms"] / 1e9
            r["fwd_bwd_TFLOPs"] = (flop_f + flop_b) / r["fwd_bwd_ms"] / 1e9
            r["fwd_bwd_share_of_155TF"] = r["fwd_bwd_TFLOPs"] / PEAK_TF
        out[impl] = r
    out["speedup_fwd_bwd"] = out["tensor_ops"]["fwd_bwd_ms"] / out["fused"]["fwd_bwd_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_supcon.py needs a GPU")
    res = [run("instance 6x4096x200, 15% masked", 200, True, a.iters, a.warmup), run("semantic 6x4096x6, no mask", 6, False, a.iters, a.warmup)]
    for r in res:
        f, t = r["fused"], r["tensor_ops"]
        print("%-34s fused fwd %.3f ms  fwd+bwd %.3f ms  (%.1f TF, %.0f %% of 155)  peak +%.1f MB | tensor ops fwd %.3f ms  fwd+bwd %.3f ms  peak +%.1f MB"
              % (r["case"], f["fwd_ms"], f["fwd_bwd_ms"], f["fwd_bwd_TFLOPs"], 100 * f["fwd_bwd_share_of_155TF"], f["peak_extra_MB"], t["fwd_ms"],
                 t["fwd_bwd_ms"], t["peak_extra_MB"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
