"""The dataset's ray sampler (pagnerf_amd/dataset.py, pag_sample_batch) on the GPU at the shape of a configs/bup20/best.yaml step: B = 6 views of
n = 1280 x 720 = 921 600 pixels, k = 4096 pixels of each, the modes of that step (imgs f32 x 4, semantics and instance int64, two confidences f32, shared
base rays = two f32 x 3 arrays: seven arrays, 64 bytes per ray).

    python3 scripts/bench_sampler.py [--reps 10] [--inner 20] [--views 12] [--out profiles/sampler.json]

1. The kernel route - ds.sample(views, k, out=buffers) + ds.advance(): two launches - against the tensor-op route a caller would write on the same GPU,
   the reference's batch mode as it stands: torch.rand(B, n).argsort(1)[:, :k] and one index per array.  The two alternate; device-event times after
   warm-up, an event pair spanning `inner` calls.  Both routes are checked first: each ray_idx row without repeats and inside [0, n), and the kernel's rows
   equal to the tensor-op gather at the kernel's indices.
2. The headline step (bench.train_step on bench.py's model, 4096 rays x 512 samples) with and without a sample + advance in front of it, alternating.
Algorithmic bytes of a sample: B * k * 64 read and as many written; the launch is bound by the latency of the B * k * 7 random row reads, not by bytes.
Not a gate: it reports.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, reps, inner, warmup=2):
    """{name: callable} -> {name: median / min / max ms per call}, the callables taking turns."""
    times = {k: [] for k in fns}
    for it in range(warmup + reps):
        for k, fn in fns.items():
            t = timed(fn, inner if it >= warmup else 1)
            if it >= warmup:
                times[k].append(t)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--views", type=int, default=12, help="views in the dataset (B = 6 of them per step)")
    ap.add_argument("--pixels", type=int, default=921600)
    ap.add_argument("--step-reps", type=int, default=6)
    ap.add_argument("--step-inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sampler.py needs a GPU (no fallback)")
    import __graft_entry__ as ge
    ge.build()
    import bench
    import pagnerf_amd
    import train_synthetic as TS
    dev = torch.device("cuda:0")
    V, n, B, k = a.views, a.pixels, 6, 4096
    gen = torch.Generator(device=dev).manual_seed(0)
    data = {"imgs": torch.rand(V, n, 4, device=dev, generator=gen),
            "semantics": torch.randint(0, 6, (V, n, 1), device=dev, generator=gen),
            "instance": torch.randint(0, 200, (V, n, 1), device=dev, generator=gen),
            "sem_conf": torch.rand(V, n, 1, device=dev, generator=gen), "inst_conf": torch.rand(V, n, 1, device=dev, generator=gen),
            "base_rays": pagnerf_amd.Rays(torch.zeros(n, 3, device=dev), torch.rand(n, 3, device=dev, generator=gen))}
    ds = pagnerf_amd.DeviceMultiviewDataset(data, dev).seed(0)
    row_bytes = sum(l.row_bytes for l in ds._leaves)
    views = torch.arange(B, dtype=torch.int32, device=dev) * (V // B)
    views_l = views.long()
    buf = ds.empty_batch(B, k, ray_idx=True)

    def kernel_route():
        ds.sample(views, k, out=buf)
        ds.advance()

    tensors = [(key, v) for key, v in data.items() if key != "base_rays"]

    def tensor_route():
        idx = torch.rand(B, n, device=dev).argsort(dim=1)[:, :k]                # ray_sampler.py:27-30
        out = {key: v[views_l[:, None], idx].contiguous() for key, v in tensors}
        out["base_rays"] = (data["base_rays"].origins[idx].contiguous(), data["base_rays"].dirs[idx].contiguous())
        out["ray_idx"] = idx
        return out

    # same contract first: k distinct pixels of [0, n) per view, and the kernel's rows are the rows at its indices
    kernel_route()
    ref = tensor_route()
    for name, idx in (("kernel", buf["ray_idx"]), ("tensor_ops", ref["ray_idx"])):
        s = idx.sort(1).values
        assert bool((s[:, 1:] != s[:, :-1]).all()) and int(idx.min()) >= 0 and int(idx.max()) < n, name
    for key, v in tensors:
        assert torch.equal(buf[key], v[views_l[:, None], buf["ray_idx"]]), key
    assert torch.equal(buf["base_rays"].dirs, data["base_rays"].dirs[buf["ray_idx"]])

    out = dict(device=torch.cuda.get_device_name(0), views=V, pixels=n, batch=B, samples=k, arrays=len(ds._leaves), row_bytes=row_bytes,
               dataset_bytes=ds.nbytes, algorithmic_bytes_read=B * k * row_bytes, algorithmic_bytes_written=B * k * row_bytes, reps=a.reps, inner=a.inner)
    t = alternate({"kernel": kernel_route, "tensor_ops": tensor_route}, a.reps, a.inner)
    out["sample"] = dict(kernel=t["kernel"], tensor_ops=t["tensor_ops"], speedup=t["tensor_ops"]["median_ms"] / t["kernel"]["median_ms"])
    print(json.dumps(out["sample"]), flush=True)

    # the headline step with and without a sample in front (the step's own rays stay the same, so the step's work does)
    args = bench.parse(["--grid", "permuto", "--precision", "bf16"])
    nef, tracer, chans = bench.make_model(args, dev, seed=0), bench.make_tracer(args), ["rgb", "semantics", "inst_embedding"]
    opt = bench.make_optimizer(nef)
    rays, gt = TS.scene_rays(args.rays, torch.Generator().manual_seed(123), dev)

    def step():
        bench.train_step(nef, tracer, opt, rays, gt, chans, 1)

    def sample_and_step():
        kernel_route()
        step()

    def tensor_sample_and_step():
        tensor_route()
        step()

    for _ in range(5):
        step()
    t = alternate({"step": step, "kernel_sample+step": sample_and_step, "tensor_ops_sample+step": tensor_sample_and_step}, a.step_reps, a.step_inner)
    out["train_step"] = dict(rays=args.rays, samples=args.samples, **t)
    out["train_step"]["kernel_sample_adds_ms"] = t["kernel_sample+step"]["median_ms"] - t["step"]["median_ms"]
    out["train_step"]["tensor_ops_sample_adds_ms"] = t["tensor_ops_sample+step"]["median_ms"] - t["step"]["median_ms"]
    print(json.dumps(out["train_step"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1))
    print(json.dumps(dict(bench_sampler="done")))


if __name__ == "__main__":
    main()
