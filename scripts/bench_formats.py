"""View preparation of the NeRF-standard loader (pagnerf_amd/formats.py) on the GPU: the kernel path (pag_prepare_views, one launch per chunk) against the
tensor-op forms on the same device tensors, the two alternating, device-event times after warm-up.

    python3 scripts/bench_formats.py [--views 100] [--size 800] [--reps 10] [--out FILE]

Cases: `views` x size x size RGBA (nerf-synthetic: 100 x 800 x 800) at mip 0 and 1, prepared in the loader's chunks of 64 MiB of source.
Per case: the time of the WHOLE SET on either path (every chunk once, into its own place in the destinations; `inner` sets between two events on the
kernel path, so that a window is milliseconds and the source and outputs of a set - 0.85 to 2.6 GB - pass the 256 MB Infinity Cache between two uses of
an address); the kernel launches of one chunk (torch.profiler; "not measured" where it cannot trace); the peak
device memory of preparing the whole set chunk by chunk on either path, and of the stack route a user of the tensor ops alone would write (the float32 RGBA
stack of every view at full resolution, as datasets/formats/nerf_standard.py holds it on the host); the kernel's share of the 8 TB/s HBM roof by algorithmic
bytes, 4 f f read + 37 written per output pixel, over the event time (launch latency included; not a profiler's kernel time).  The three routes give the same images and masks (checked before timing).
Decoding is host work and is timed on its own: one size x size RGBA PNG through formats.decode_image.  The uploads are not timed.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

HBM_PEAK = 8.0e12        # bytes / s (MI355X)
CHUNK_BYTES = 64 << 20
INTRINSICS = (1111.1, 1111.1, 0.0, 0.0)


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    top = torch.cuda.max_memory_allocated() - base
    del out
    return top


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n if n else "not measured"
    except Exception as e:           # the tracer is not everywhere; the figure is then left out, not guessed
        return "not measured (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5, help="sets of the kernel path between two events")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_formats.py needs a GPU (no fallback)")
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import formats, ops
    dev = torch.device("cuda:0")
    V, H0 = a.views, a.size
    out = dict(views=V, size=H0, reps=a.reps, chunk_bytes=CHUNK_BYTES, device=torch.cuda.get_device_name(0), cases=[])

    gen = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, 256, (V, H0, H0, 4), dtype=torch.uint8, device=dev, generator=gen)
    q, _ = np.linalg.qr(np.random.RandomState(0).standard_normal((V, 3, 3)))
    c2w = torch.from_numpy(np.concatenate([q, np.ones((V, 3, 1))], axis=2)).float().to(dev)
    per_chunk = min(V, CHUNK_BYTES // (H0 * H0 * 4))
    chunks = [(off, min(per_chunk, V - off)) for off in range(0, V, per_chunk)]

    for mip in (0, 1):
        f = 1 << mip
        h = w = H0 // f

        def alloc():
            return dict(imgs=torch.empty(V, h, w, 3, device=dev), masks=torch.empty(V, h, w, 1, dtype=torch.bool, device=dev),
                        origins=torch.empty(V, h, w, 3, device=dev), dirs=torch.empty(V, h, w, 3, device=dev))

        def kernel_chunk(dst, off, n):
            ops.prepare_views(src[off:off + n], mip, "white", off, c2w=c2w, intrinsics=INTRINSICS, **dst)

        def tensor_chunk(dst, off, n):
            dst["imgs"][off:off + n], dst["masks"][off:off + n] = formats.prepare_views_reference(src[off:off + n], mip, "white")
            r = formats.rays_reference(c2w[off:off + n], w, h, *INTRINSICS)
            dst["origins"][off:off + n], dst["dirs"][off:off + n] = r.origins, r.dirs

        def whole(route):
            dst = alloc()
            for off, n in chunks:
                route(dst, off, n)
            return dst

        def stack_route():
            """Tensor ops over the whole set at once: the float32 RGBA stack at full resolution, then the area mean, the composite, the mask and the rays."""
            x = src.float() / 255
            x = x.reshape(V, h, f, w, f, 4).mean((2, 4))
            rgb, al = x[..., :3], x[..., 3:4]
            r = formats.rays_reference(c2w, w, h, *INTRINSICS)
            return dict(imgs=((rgb * al) + (1 - al)).clamp(0, 1), masks=al > 0.5, origins=r.origins, dirs=r.dirs)

        # the same results first (measuring-on-mi355x 6)
        dk, dt = whole(kernel_chunk), whole(tensor_chunk)
        same = dict(imgs=bool(torch.equal(dk["imgs"], dt["imgs"])), masks=bool(torch.equal(dk["masks"], dt["masks"])),
                    origins=bool(torch.equal(dk["origins"], dt["origins"])), dirs_max_abs_diff=float((dk["dirs"] - dt["dirs"]).abs().max()))
        def whole_into(route, dst):
            for off, n in chunks:
                route(dst, off, n)

        times = {"kernel": [], "tensor_ops": []}
        for it in range(2 + a.reps):
            for name, route, dst, inner in (("kernel", kernel_chunk, dk, a.inner), ("tensor_ops", tensor_chunk, dt, 1)):
                t = timed(lambda: whole_into(route, dst), inner if it >= 2 else 1)
                if it >= 2:
                    times[name].append(t)
        off, n = chunks[0]
        counts = dict(kernel=launches(lambda: kernel_chunk(dk, off, n)), tensor_ops=launches(lambda: tensor_chunk(dt, off, n)))
        del dk, dt
        mem = dict(kernel=peak(lambda: whole(kernel_chunk)), tensor_ops=peak(lambda: whole(tensor_chunk)), stack_route=peak(stack_route))
        t_stack = [timed(stack_route) for _ in range(3)][1:]
        alg = V * h * w * (4 * f * f + 37)
        stat = {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}
        out["cases"].append(dict(case="%d x %d x %d RGBA, mip %d" % (V, H0, H0, mip), views_per_chunk=per_chunk, chunks=len(chunks),
                                 output_bytes=V * h * w * 37,
                                 source_bytes=V * H0 * H0 * 4, set_algorithmic_bytes=alg, set_time=stat, kernel_sets_per_window=a.inner,
                                 set_speedup=stat["tensor_ops"]["median_ms"] / stat["kernel"]["median_ms"],
                                 kernel_hbm_roof_share=alg / (stat["kernel"]["median_ms"] * 1e-3) / HBM_PEAK,
                                 launches_per_chunk=counts, peak_bytes_beyond_source=mem, stack_route_ms=t_stack, same_results=same))
        print(json.dumps(out["cases"][-1]), flush=True)
    del src

    # decoding: host work, on its own
    yy, xx = np.mgrid[0:H0, 0:H0]
    pic = np.stack([(xx * 255 // H0), (yy * 255 // H0), ((xx ^ yy) & 255), np.where((xx - H0 / 2) ** 2 + (yy - H0 / 2) ** 2 < (H0 / 3) ** 2, 255, 0)], -1).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "frame.png")
        try:
            from PIL import Image
            Image.fromarray(pic, "RGBA").save(path)
            what = "RGBA, PIL"
        except ImportError:
            from pagnerf_amd.visualize import write_png
            write_png(path, pic[:, :, :3])
            what = "RGB, read_png"
        formats.decode_image(path)
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            formats.decode_image(path)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["decode"] = dict(what="one %d x %d %s, one thread" % (H0, H0, what), median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts),
                             file_bytes=os.path.getsize(path))
    print(json.dumps(out["decode"]), flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    print(json.dumps(dict(bench_formats="done", cases=len(out["cases"]))))


if __name__ == "__main__":
    main()
