"""What the native trainer's step costs over the benchmark's: PanopticTrainer.step against bench.train_step on the SAME model, in the same process, with
HIP graphs on, at the best.yaml shape (6 images x 4096 rays, pose optimisation) in the three regimes the schedule of best.yaml goes through:

    dense_rgb          epochs 0 - 201     dense occupancy, 'ray' march x 512, channels rgb + depth
    post_prune_rgb     epochs 202 - 600   voxel march (2 samples per voxel) on a pruned occupancy, channels rgb + depth
    post_prune_all     epochs 601 - 800   voxel march, all channels, LinAssignmentThingsLoss(outlier_rejection) + segment_consistency_regularizer, ONE backward()

Both sides step the same nef through the same tracer on the same fixed batch (one draw of the BatchSampler: the bench side gets it as the rays function and
target dict bench.train_step takes), each with its own optimiser: bench.make_optimizer's two groups against the trainer's six named groups.  Per regime:
warm-up (sample count, graph capture, first replays), then ROUNDS alternating blocks per side, each block between device synchronisations on the host
clock and long enough to last --block-seconds (at least --steps steps; the step count is fixed per regime from a trial block, the same for both sides);
the figure of a side is the median over its blocks.  One process on the GPU.  The sampler's cost per batch (its one launch, which a real
epoch adds to every step) is reported next to it.

    python scripts/bench_trainer.py [--block-seconds 1.0] [--rounds 5] [--out FILE.json]     -> one JSON line
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench

IMAGES, SIDE = 6, 64                     # 6 views of 64 x 64 = 4096 pixels: a batch takes every pixel of every view
CONFIG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "configs", "best.yaml")


def make_dataset(dev, seed=7):
    """BUP20-shaped synthetic views as bench.PoseOpt / bench.make_rays draw them: cameras above the scene looking down with a small yaw, random colours,
    ~24 'plants' per image on a 6 x 6 tiling (id > 0: thing classes 2 - 5, the rest stuff classes 0 - 1)."""
    import pagnerf_amd
    gen = torch.Generator().manual_seed(seed)
    n = SIDE * SIDE
    views = torch.eye(4).repeat(IMAGES, 1, 1)
    ang = (torch.rand(IMAGES, generator=gen) - 0.5) * 0.3
    views[:, 0, 0], views[:, 0, 1], views[:, 1, 0], views[:, 1, 1] = torch.cos(ang), -torch.sin(ang), torch.sin(ang), torch.cos(ang)
    views[:, :3, 3] = torch.cat([(torch.rand(IMAGES, 2, generator=gen) - 0.5) * 0.2, torch.full((IMAGES, 1), -0.95)], 1)
    ys, xs = torch.meshgrid((torch.arange(SIDE) + 0.5) / SIDE - 0.5, (torch.arange(SIDE) + 0.5) / SIDE - 0.5, indexing="ij")
    dirs = torch.stack([xs * 0.7, ys * 0.7, -torch.ones_like(xs)], -1).reshape(n, 3)
    cell = ((xs + 0.5) * 6).long().clamp(0, 5) * 6 + ((ys + 0.5) * 6).long().clamp(0, 5)
    inst = torch.where(cell % 3 != 0, cell + 1000, torch.zeros_like(cell)).reshape(1, n, 1).repeat(IMAGES, 1, 1)
    sem = torch.where(inst > 0, 2 + cell.reshape(1, n, 1) % 4, torch.randint(0, 2, (IMAGES, n, 1), generator=gen))
    data = dict(imgs=torch.rand(IMAGES, n, 3, generator=gen), semantics=sem, instance=inst,
                base_rays=pagnerf_amd.Rays(torch.zeros(n, 3), dirs, dist_min=0.0, dist_max=1.9))
    ds = pagnerf_amd.DeviceMultiviewDataset(data, dev)
    ds.view_matrices, ds.image_shape = views, (SIDE, SIDE)
    ds.semantic_info = dict(num_classes=6, num_instances=200, things_ids=[2, 3, 4, 5], stuff_ids=[0, 1])
    return ds


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def regime(name, epoch, prune, dev, a):
    import pagnerf_amd
    from pagnerf_amd import config
    from pagnerf_amd.loss import LinAssignmentThingsLoss
    cfg = config.load_config(CONFIG)
    cfg.update(batch_size=IMAGES, num_rays_sampled_per_img=SIDE * SIDE, anchor_frame_idxs=[0], optimize_val_extrinsics=False, log_dir=a.log_dir)
    args = bench.parse(["--pose-opt", "--images", str(IMAGES), "--rays", str(IMAGES * SIDE * SIDE), "--graphs", "on"])
    nef = bench.make_model(args, dev, seed=0)                                        # the benchmark's model (best.yaml's sizes)
    tracer = bench.make_tracer(args, raymarch="ray", samples=512)
    ds = make_dataset(dev)
    pipe = pagnerf_amd.BAPipeline(nef, ds.view_matrices, tracer=tracer, anchor_frame_idxs=[0], near=0.0, far=1.9).to(dev)
    occupied = bench.synthetic_prune(nef, 0.1) if prune else 1.0
    trainer = pagnerf_amd.PanopticTrainer(pipe, ds, None, **dict(cfg, use_graphs=True))
    trainer.epoch = epoch
    plan = trainer.begin_epoch()                                                     # sets the tracer's march and the channel set of that epoch
    batch = next(iter(trainer.sampler))
    base, cam = batch["base_rays"], batch["cam_idx"]
    sem = batch["semantics"].reshape(-1)
    gt = dict(rgb=batch["imgs"].reshape(-1, 3), sem=sem, inst_ids=batch["instance"].reshape(-1), stuff=torch.isin(sem, trainer.stuff_ids))
    rays_fn = lambda: pipe.transform_rays_indexed(base.origins.reshape(-1, 3), base.dirs.reshape(-1, 3), cam)
    points_fn = lambda depth: pipe.rays_to_3d_points_indexed(base.origins.reshape(-1, 3), base.dirs.reshape(-1, 3), depth, cam)
    bench_opt = bench.make_optimizer(nef, extra=[pipe.camera_extrinsics])
    panoptic = "semantics" in plan["channels"]
    kw = dict(lin_assign=LinAssignmentThingsLoss(outlier_rejection=True), images=IMAGES, points_fn=points_fn, seg_reg=True) if panoptic else {}
    channels = set(plan["channels"])
    sides = dict(bench=lambda: bench.train_step(nef, tracer, bench_opt, rays_fn, gt, channels, 1, **kw), trainer=lambda: trainer.step(batch))
    for fn in sides.values():                                                        # sample count, capture, first replays - per side
        for _ in range(a.warmup):
            fn()
    steps = max(a.steps, int(math.ceil(a.block_seconds * 1e3 / timed(sides["bench"], a.steps))))      # a block measures the step, not the clock
    blocks = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, fn in sides.items():
            blocks[k].append(timed(fn, steps))
    sampler_ms = timed(lambda: (ds.sample(batch["cam_id"], SIDE * SIDE), ds.advance()), 200)
    med = {k: statistics.median(v) for k, v in blocks.items()}
    graphs = tracer._graphs is not None
    spread = {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in blocks.items()}
    out = dict(epoch=epoch, steps_per_block=steps, block_spread=spread, channels=plan["channels"], raymarch=plan["raymarch_type"], num_steps=plan["num_steps"], occupied_fraction=round(occupied, 4),
               bench_ms=round(med["bench"], 4), trainer_ms=round(med["trainer"], 4), ratio=round(med["trainer"] / med["bench"], 4),
               bench_blocks_ms=[round(v, 4) for v in blocks["bench"]], trainer_blocks_ms=[round(v, 4) for v in blocks["trainer"]],
               sampler_ms_per_batch=round(sampler_ms, 4), graph_runner=graphs, loss_finite=bool(math.isfinite(float(trainer.log_epoch()["total_loss"]))))
    del trainer, pipe, nef, tracer, ds, batch
    torch.cuda.empty_cache()
    return name, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="fewest steps per timed block")
    ap.add_argument("--block-seconds", type=float, default=1.0, help="least duration of a timed block")
    ap.add_argument("--rounds", type=int, default=5, help="alternating blocks per side")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--log-dir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "pag_bench_trainer"))
    ap.add_argument("--out", help="also write the record to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_trainer.py measures on the GPU; none found")
    import __graft_entry__ as ge
    ge.build()
    dev = torch.device("cuda:0")
    record = dict(shape="%d images x %d rays" % (IMAGES, SIDE * SIDE), block_seconds=a.block_seconds, rounds=a.rounds, regimes={})
    for name, epoch, prune in (("dense_rgb", 0, False), ("post_prune_rgb", 300, True), ("post_prune_all", 601, True)):
        key, out = regime(name, epoch, prune, dev, a)
        record["regimes"][key] = out
        print("[bench_trainer] %s: %s" % (key, json.dumps(out)), file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps(record))
