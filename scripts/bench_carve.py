"""The depth carve (pagnerf_amd/carve.py, csrc/carve.hip) on the GPU, two measurements.  Not a gate: it reports.  Needs a GPU: there is no fallback.

    python3 scripts/bench_carve.py [--views 40] [--width 1280] [--height 720] [--reps 5] [--step-reps 4] [--step-inner 10] [--out profiles/carve.json]

1. The carve of a BUP20-shaped set at blas level 7: `--views` cameras (configs/bup20/best.yaml: a 40-frame window, mip 0 = 1280 x 720 pixels) looking
   down on an analytic scene - a sphere of radius 0.5 over the plane z = -0.7 - whose depth along each ray is known in closed form.  pag_carve_rays in
   chunks of 8 views + one pag_carve_finish (device events around the whole sequence, warm-up first, median of --reps) against carve_reference +
   carve_finish_reference, the tensor-op definition, on the same GPU (host clock around a synchronised run: one warm-up run, then the faster of two -
   it takes seconds).  The kernels' times start after the two bitfields' memsets.  The two results are compared bit for bit.  Rays are assigned to
   lanes in row order (pixel index = lane); a tiled assignment was not tried.
2. The dense 'ray'-march step of bench.py's best_yaml_step (6 images x 4096 rays x 512 samples, permutohedral grids, trainable extrinsics, channels
   rgb + depth) on the same scene seen by that step's six cameras: uncarved (every cell occupied) against carved from 6 depth images of 320 x 180 pixels
   with carve_occupancy's defaults (margin two cells, dilate 1, hull).  Two models built from the same seed, warmed up, then timed in alternation
   (--step-reps windows of --step-inner steps each, device synchronised); the samples per step and the share of cells the carve left are in the output.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

LEVEL = 7
NEAR, FAR = 0.0, 1.9
PLANE_Z = -0.7


def scene_hit(o, d):
    """Distance along unit world rays to the sphere of radius 0.5 at the origin, else to the plane z = PLANE_Z inside the cube, else 0 (no reading)."""
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - 0.25)
    ts = -b - torch.sqrt(disc.clamp_min(0))
    tp = (PLANE_Z - o[:, 2]) / d[:, 2]
    pp = o + d * tp[:, None]
    on_plane = (tp > 0) & (pp[:, :2].abs().max(-1)[0] < 1.0)
    return torch.where(disc > 0, ts, torch.where(on_plane, tp, torch.zeros_like(tp)))


def row_cameras(n, dev):
    """n camera centres along the x axis at height 0.95 (a robot's pass over a plant row), looking straight down."""
    x = torch.linspace(-0.6, 0.6, n, device=dev)
    return torch.stack([x, 0.05 * torch.sin(7 * x), torch.full_like(x, 0.95)], -1)


def view_rays(centres, w, h, dev, field=0.45):
    """World rays of len(centres) downward pinhole views of w x h pixels, row-major (x fast): origins, unit dirs [V * h * w, 3]."""
    ys, xs = torch.meshgrid(((torch.arange(h, device=dev) + 0.5) / h - 0.5) * 2 * field * h / w, ((torch.arange(w, device=dev) + 0.5) / w - 0.5) * 2 * field,
                            indexing="ij")
    d = torch.nn.functional.normalize(torch.stack([xs, -ys, -torch.ones_like(xs)], -1).reshape(-1, 3), dim=-1)
    V = centres.shape[0]
    return centres[:, None, :].expand(V, h * w, 3).reshape(-1, 3).contiguous(), d[None].expand(V, h * w, 3).reshape(-1, 3).contiguous()


def event_ms(fn, before=None):
    """Device time of fn() between two events; before() is queued ahead of the first event (the bitfields' memsets are not part of the carve)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if before is not None:
        before()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_carve(a, dev):
    from pagnerf_amd import carve, ops
    R = 2 ** LEVEL
    margin, words = 2 * 2.0 / R, carve.num_words(LEVEL)
    centres = row_cameras(a.views, dev)
    chunks = []
    for c in centres.split(8):
        o, d = view_rays(c, a.width, a.height, dev)
        chunks.append((o, d, scene_hit(o, d).contiguous()))
    rays = sum(c[2].numel() for c in chunks)
    valid = sum(int((c[2] > 0).sum()) for c in chunks)
    free, surface = torch.zeros(words, dtype=torch.int32, device=dev), torch.zeros(words, dtype=torch.int32, device=dev)
    out = torch.empty_like(free)

    def zero():
        free.zero_()
        surface.zero_()

    def kernels():
        for o, d, t in chunks:
            ops.carve_rays(o, d, t, NEAR, FAR, margin, LEVEL, free, surface)
        ops.carve_finish(free, surface, LEVEL, 1, "hull", out=out)

    def rays_only():
        for o, d, t in chunks:
            ops.carve_rays(o, d, t, NEAR, FAR, margin, LEVEL, free, surface)

    def finish_only():
        ops.carve_finish(free, surface, LEVEL, 1, "hull", out=out)

    def reference():
        f = s = None
        for o, d, t in chunks:
            f, s = carve.carve_reference(o, d, t, NEAR, FAR, margin, LEVEL, f, s)
        return f, s, carve.carve_finish_reference(f, s, LEVEL, 1, "hull")

    zero()
    kernels()
    reference()                                 # warm-up: the allocator's growth and the first calls of every tensor op are not the definition's time
    torch.cuda.synchronize()
    ref_times = []
    for _ in range(2):
        t0 = time.perf_counter()
        rf, rs, rout = reference()
        torch.cuda.synchronize()
        ref_times.append(time.perf_counter() - t0)
    ref_s = min(ref_times)
    same = bool(torch.equal(free, rf) and torch.equal(surface, rs) and torch.equal(out, rout))
    res = {}
    for name, fn, before in (("rays_and_finish", kernels, zero), ("rays", rays_only, zero), ("finish", finish_only, None)):
        event_ms(fn, before)
        times = [event_ms(fn, before) for _ in range(a.reps)]
        res[name] = dict(median_ms=round(statistics.median(times), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))
    zero()
    kernels()
    share = lambda b: round(float(carve.unpack_bits(b, R ** 3).sum()) / R ** 3, 4)
    return dict(workload="%d views x %d x %d pixels = %d rays (%d with a depth reading), blas level %d, margin %.5f, dilate 1, hull, chunks of 8 views, rays in row "
                         "order" % (a.views, a.width, a.height, rays, valid, LEVEL, margin),
                kernels=res, reference_tensor_ops_s=round(ref_s, 3), reference_runs_s=[round(t, 3) for t in ref_times], reference_over_kernels=round(ref_s * 1e3 / res["rays_and_finish"]["median_ms"], 1),
                bit_identical_to_reference=same, cells_free=share(free), cells_surface=share(surface), cells_occupied=share(out),
                reps=a.reps, tiled_ray_assignment="not tried")


class Step:
    """bench.py's best_yaml_step 'dense_rgb' job: 6 images x 4096 rays, 512 'ray' samples, permutohedral grids, pose optimisation, rgb + depth."""

    def __init__(self, bench, args, dev, images=6, per_image=4096):
        self.bench = bench
        total = images * per_image
        self.nef = bench.make_model(args, dev, seed=0, grid="permuto")
        self.tracer = bench.make_tracer(args, "ray", 512)
        self.pose = bench.PoseOpt(self.nef, self.tracer, total, images, dev, 0, total)
        _, self.gt = bench.make_rays(total, dev, seed=1000)
        self.opt = bench.make_optimizer(self.nef, self.pose.parameters())
        self.total, self.images = total, images

    def step(self):
        return self.bench.train_step(self.nef, self.tracer, self.opt, self.pose.rays, self.gt, {"rgb", "depth"}, 1)

    def samples(self):
        with torch.no_grad():
            out = self.nef.grid.raymarch(self.pose.rays(), level=None, num_samples=512, raymarch_type="ray")
        return int(out[2].shape[0])

    def carve(self, dev, w=320, h=180):
        """Carve from depth images of the step's own six cameras (their current extrinsics), w x h pixels over the step's field of view."""
        from pagnerf_amd import carve, ops
        ys, xs = torch.meshgrid(((torch.arange(h, device=dev) + 0.5) / h - 0.5) * 0.7, ((torch.arange(w, device=dev) + 0.5) / w - 0.5) * 0.7, indexing="ij")
        dc = torch.stack([xs, ys, -torch.ones_like(xs)], -1).reshape(-1, 3).repeat(self.images, 1)
        cam = torch.arange(self.images, device=dev, dtype=torch.int32)[:, None].expand(-1, h * w).reshape(-1).contiguous()
        with torch.no_grad():
            r = self.pose.pipe.transform_rays_indexed(torch.zeros_like(dc), dc, cam)
        o, d = r.origins.contiguous(), r.dirs.contiguous()
        t = scene_hit(o, d).contiguous()
        R, words = 2 ** LEVEL, carve.num_words(LEVEL)
        free, surface = torch.zeros(words, dtype=torch.int32, device=dev), torch.zeros(words, dtype=torch.int32, device=dev)
        ops.carve_rays(o, d, t, NEAR, FAR, 2 * 2.0 / R, LEVEL, free, surface)
        bits = ops.carve_finish(free, surface, LEVEL, 1, "hull")
        for g in (self.nef.grid, self.nef.delta_grid):
            g.set_carve(bits)
            g.blas_init_bits(bits)
        share = lambda b: round(float(carve.unpack_bits(b, R ** 3).sum()) / R ** 3, 4)
        return dict(depth_images="%d x %d x %d pixels" % (self.images, w, h), valid_pixels=int((t > 0).sum()), cells_free=share(free), cells_surface=share(surface),
                    cells_occupied=share(bits))


def bench_step(a, dev):
    import bench
    args = bench.parse([])
    jobs = {"uncarved": Step(bench, args, dev), "carved": Step(bench, args, dev)}
    report = jobs["carved"].carve(dev)
    for j in jobs.values():
        for _ in range(6):                      # step 0 learns the sample count, step 1 captures the graphs, the rest replay
            j.step()
    torch.cuda.synchronize()
    times = {k: [] for k in jobs}
    import gc
    gc.collect()
    gc.disable()
    for _ in range(a.step_reps):
        for k, j in jobs.items():
            for _ in range(3):                  # settle after the other job's window
                j.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.step_inner):
                j.step()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.step_inner * 1e3)
    gc.enable()
    out = dict(workload="bench.py best_yaml_step dense_rgb: 6 images x 4096 rays x 512 'ray' samples, permutohedral grids, trainable extrinsics, rgb + depth; "
                        "scene: sphere r = 0.5 over the plane z = %.1f" % PLANE_Z, carve=report, windows=a.step_reps, steps_per_window=a.step_inner)
    for k, j in jobs.items():
        g = getattr(j.tracer, "_graphs", None)
        out[k] = dict(ms_per_step_median=round(statistics.median(times[k]), 3), ms_per_step_min=round(min(times[k]), 3), ms_per_step_max=round(max(times[k]), 3),
                      samples_per_step=j.samples(), hip_graphs=None if g is None else dict(captures=g.captures, replays=g.replays, overflows=g.overflows))
    out["carved_over_uncarved_time"] = round(out["carved"]["ms_per_step_median"] / out["uncarved"]["ms_per_step_median"], 3)
    out["carved_over_uncarved_samples"] = round(out["carved"]["samples_per_step"] / max(1, out["uncarved"]["samples_per_step"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--step-inner", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true", help="measurement 1 only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_carve.py needs a GPU (no fallback)")
    import __graft_entry__ as ge
    ge.build()
    dev = torch.device("cuda", torch.cuda.current_device())
    result = dict(device=torch.cuda.get_device_name(dev), carve=bench_carve(a, dev))
    print(json.dumps(dict(carve=result["carve"])), flush=True)
    if not a.skip_step:
        torch.cuda.empty_cache()
        result["dense_step"] = bench_step(a, dev)
        print(json.dumps(dict(dense_step=result["dense_step"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
