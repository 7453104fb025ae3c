"""The grid total-variation terms (pagnerf_amd/regularizers.py) on the GPU: the kernel path (pag_tv_fwd / pag_tv_bwd) against the tensor-op form on the same
tensors, the two alternating, device-event times after warm-up.

    python3 scripts/bench_tv.py [--reps 10] [--inner 10] [--n 100] [--out FILE]

Cases: tv_l1_loss / tv_l2_loss alone at [n+1, n+1, n+1, 48] fp32 (what grid.interpolate returns on the lattice) and [n+1, n+1, n+1, 200] bf16 (what the
instance head returns), forward and forward + backward; the whole grid_tvl2_reg term on the headline permuto grid and the whole delta_grid_tvl1_reg term on
the headline nef (bench.py's model), forward + backward, with the peak device memory of each path.
Algorithmic bytes come from the shapes: one read of the lattice forward, one read and one write backward; the kernel path's share of the 8 TB/s HBM roof is
those bytes over its time.  An event pair spans `inner` back-to-back calls, so the launch latency of the two or three launches is amortised.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM_PEAK = 8.0e12        # bytes / s (MI355X)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def ab(make, reps, inner, warmup=2):
    """make(kernels) -> callable; -> {True: median ms per call, False: ...} with the two paths alternating."""
    from pagnerf_amd import regularizers as R
    fns = {k: make(k) for k in (True, False)}
    times = {True: [], False: []}
    try:
        for it in range(warmup + reps):
            for k in (True, False):
                R.TV_KERNELS = k
                t = timed(fns[k], inner if it >= warmup else 1)
                if it >= warmup:
                    times[k].append(t)
    finally:
        R.TV_KERNELS = True
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


def peak(fn, kernels):
    from pagnerf_amd import regularizers as R
    R.TV_KERNELS = kernels
    try:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    finally:
        R.TV_KERNELS = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--n", type=int, default=100, help="tv_edge_num_samples: the lattice has n + 1 points per edge")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tv.py needs a GPU (no fallback)")
    import __graft_entry__ as ge
    ge.build()
    import bench
    import pagnerf_amd
    from pagnerf_amd import regularizers as R
    dev = torch.device("cuda:0")
    n = a.n
    out = dict(lattice=[n + 1] * 3, reps=a.reps, inner=a.inner, device=torch.cuda.get_device_name(0), cases=[])

    gen = torch.Generator(device=dev).manual_seed(0)
    for C, dtype in ((48, torch.float32), (200, torch.bfloat16)):
        x = torch.randn(n + 1, n + 1, n + 1, C, device=dev, generator=gen).to(dtype)
        nbytes = x.numel() * x.element_size()
        for power in (1, 2):
            for what in ("fwd", "fwd+bwd"):
                xx = x.clone().requires_grad_(what != "fwd")

                def make(kernels, xx=xx, power=power, what=what):
                    def fn():
                        loss = R.tv_loss(xx, power)
                        if what != "fwd":
                            xx.grad = None
                            loss.backward()
                    return fn
                t = ab(make, a.reps, a.inner)
                # same results first (measuring-on-mi355x 6): value and gradient of the two paths on this tensor
                R.TV_KERNELS = True
                vk = float(R.tv_loss(x, power))
                R.TV_KERNELS = False
                vf = float(R.tv_loss(x, power))
                R.TV_KERNELS = True
                alg = nbytes * (1 if what == "fwd" else 3)
                out["cases"].append(dict(case="tv_l%d_loss %s" % (power, what), shape=list(x.shape), dtype=str(dtype).replace("torch.", ""),
                                         algorithmic_bytes=alg, kernels=t[True], tensor_ops=t[False],
                                         speedup=t[False]["median_ms"] / t[True]["median_ms"],
                                         kernel_hbm_roof_share=alg / (t[True]["median_ms"] * 1e-3) / HBM_PEAK,
                                         value_kernels=vk, value_tensor_ops=vf, value_rel_diff=abs(vk - vf) / abs(vf)))
                print(json.dumps(out["cases"][-1]), flush=True)
        del x, xx

    args = bench.parse(["--grid", "permuto", "--precision", "bf16"])
    nef = bench.make_model(args, dev, seed=0)
    terms = (("grid_tvl2_reg term, headline permuto grid", dict(grid_tvl2_reg=1e-7), 48 * 4),
             ("delta_grid_tvl1_reg term, headline nef", dict(delta_grid_tvl1_reg=1e-7), 200 * 2))
    for name, kw, row_bytes in terms:
        def make(kernels, kw=kw):
            def fn():
                for p in nef.parameters():
                    p.grad = None
                torch.manual_seed(0)
                R.step_tv_terms(nef, tv_window_size=0.0001, tv_edge_num_samples=n, **kw).backward()
            return fn
        t = ab(make, a.reps, 1)
        mem = {k: peak(make(k), k) for k in (True, False)}
        alg = (n + 1) ** 3 * row_bytes * 3
        out["cases"].append(dict(case=name + " fwd+bwd", tv_algorithmic_bytes=alg, kernels=t[True], tensor_ops=t[False],
                                 speedup=t[False]["median_ms"] / t[True]["median_ms"], peak_bytes_kernels=mem[True], peak_bytes_tensor_ops=mem[False]))
        print(json.dumps(out["cases"][-1]), flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    print(json.dumps(dict(bench_tv="done", cases=len(out["cases"]))))


if __name__ == "__main__":
    main()
