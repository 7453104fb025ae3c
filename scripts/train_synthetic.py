"""End-to-end training check on an analytic scene (no dataset in this image): a textured sphere of radius 0.5 seen by downward
cameras, white background.  Ground truth per ray is computed in closed form (ray-sphere intersection): colour from the hit
point, semantic class = quadrant of the hit point, instance id = longitude sector; rays that miss carry the label -100
(F.nll_loss's ignore_index: the composited class probabilities of an empty ray are alpha * sum = 0 by construction, as in the
reference, tracers/panoptic_packed_rf_tracer.py:197-205, so they cannot be supervised).
Trains the bench's model / optimizer / loss (bench.py, BUP20 hyper-parameters) for --steps steps on fresh random rays and reports
PSNR, semantic and instance accuracy on held-out rays, once on the bf16 MFMA path and once on the fp32 parity path (the one the
oracle tests pin), same seeds.  usage: python3 scripts/train_synthetic.py [--steps 600] [--rays 4096] [--samples 128]

--inst-loss sup_contrastive trains the instance head as configs/bup20/best_contrast_delta.yaml does: a raw 200-wide embedding (no softmax),
inst_weight 0.1 x pagnerf_amd.loss.SupConLoss(temperature 0.07, pn_ratio 0.5) on the rays that hit (anchor_mask), next to the rgb and
semantic terms; instance accuracy is then nearest-centroid: held-out rays take the id whose mean normalised training-ray embedding is
closest in cosine (inst_acc), and - the configs' own route - mean-shift clusters of the training rays named by their majority id
(inst_acc_mean_shift, n_clusters; pagnerf_amd.cluster.MeanShift).  The default (nll) keeps the per-ray NLL instance term.

--grid-tvl1 / --grid-tvl2 / --delta-grid-tvl1 / --delta-grid-tvl2 W add the grid total-variation terms of pc_nerf/trainer.py:556-574 with those weights
(pagnerf_amd.step_tv_terms; the YAMLs' commented-out value is 1e-7) on a (--tv-edge-num-samples + 1)^3 lattice; all 0 (the default) leaves the step as it was.

--from-images V HxW trains from IMAGES instead of fresh random rays: the same closed form rendered into V images of H x W pixels from V fixed cameras,
held in a pagnerf_amd.DeviceMultiviewDataset and dealt by pagnerf_amd.BatchSampler (--batch-images views per step, --rays / that many pixels of each,
drawn without replacement by the sampling kernel) - the input side of pc_nerf/trainer.py:216-219 and :388-423.  --panoptic-epoch-start E keeps the
trainer's schedule: rgb alone before epoch E.  Without the flag nothing changes.
"""
import argparse
import json
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench


def scene_rays(n, gen, dev):
    import pagnerf_amd
    o = torch.cat([(torch.rand(n, 2, generator=gen) - 0.5) * 1.2, torch.full((n, 1), 0.95)], 1)
    tgt = torch.cat([(torch.rand(n, 2, generator=gen) - 0.5) * 1.4, torch.full((n, 1), -0.2)], 1)
    d = torch.nn.functional.normalize(tgt - o, dim=-1)
    rgb, sem, inst = scene_truth(o, d)
    rays = pagnerf_amd.Rays(o.to(dev), d.to(dev), dist_min=0.0, dist_max=1.9)
    return rays, dict(rgb=rgb.to(dev), sem=sem.to(dev), inst=inst.to(dev))


def scene_truth(o, d):
    """Closed-form ground truth of the rays (o, d) [n,3] on the CPU: colour [n,3], semantic class and instance id [n] (-100 where the ray misses)."""
    n = o.shape[0]
    # sphere |p| = 0.5
    b = (o * d).sum(-1)
    c = (o * o).sum(-1) - 0.25
    disc = b * b - c
    hit = disc > 0
    t = -b - torch.sqrt(disc.clamp_min(0))
    p = o + d * t[:, None]
    rgb = torch.where(hit[:, None], 0.5 + 0.5 * torch.sin(p * 9.0 + torch.tensor([0.0, 2.0, 4.0])), torch.ones(n, 3))
    sem = torch.where(hit, 1 + (p[:, 0] > 0).long() + 2 * (p[:, 1] > 0).long(), torch.full((n,), -100, dtype=torch.long))     # 1..4
    lon = torch.atan2(p[:, 1], p[:, 0])
    inst = torch.where(hit, 1 + ((lon + math.pi) / (2 * math.pi) * 12).long().clamp(0, 11), torch.full((n,), -100, dtype=torch.long))
    return rgb, sem, inst


def scene_images(V, H, W, dev):
    """The scene as a dataset: V cameras on a circle of radius 0.45 at height 0.95 looking down, each pixel's ray through a regular H x W lattice of the
    plane z = -0.2 (the plane scene_rays aims at); modes imgs [V,H,W,3], semantics / instance [V,H,W,1] int64, rays [V,H*W,3]."""
    import pagnerf_amd
    ang = torch.arange(V, dtype=torch.float32) * (2 * math.pi / V)
    cam = torch.stack([0.45 * torch.cos(ang), 0.45 * torch.sin(ang), torch.full((V,), 0.95)], -1)                       # [V,3]
    ys, xs = torch.meshgrid((torch.arange(H) + 0.5) / H - 0.5, (torch.arange(W) + 0.5) / W - 0.5, indexing="ij")
    tgt = torch.stack([xs * 1.4, ys * 1.4, torch.full_like(xs, -0.2)], -1).reshape(1, H * W, 3)
    o = cam[:, None, :].expand(V, H * W, 3).contiguous()
    d = torch.nn.functional.normalize(tgt - o, dim=-1)
    rgb, sem, inst = scene_truth(o.reshape(-1, 3), d.reshape(-1, 3))
    data = dict(imgs=rgb.reshape(V, H, W, 3), semantics=sem.reshape(V, H, W, 1), instance=inst.reshape(V, H, W, 1),
                rays=pagnerf_amd.Rays(o, d, dist_min=0.0, dist_max=1.9), filenames=["view_%03d" % v for v in range(V)])
    return pagnerf_amd.DeviceMultiviewDataset(data, dev)


def batch_to_step(batch):
    """A collated batch of the sampler -> (rays [B*k], targets) as bench.train_step takes them (pc_nerf/trainer.py:396-422 flattens the same way)."""
    import pagnerf_amd
    r = batch["rays"]
    rays = pagnerf_amd.Rays(r.origins.reshape(-1, 3), r.dirs.reshape(-1, 3), dist_min=r.dist_min, dist_max=r.dist_max)
    return rays, dict(rgb=batch["imgs"].reshape(-1, 3), sem=batch["semantics"].reshape(-1), inst=batch["instance"].reshape(-1))


def train_from_images(precision, a, dev, ds, steps, batch_images=None):
    """`steps` steps of bench.train_step on batches of a BatchSampler over `ds` (whole batches only, so that every step has --rays rays).
    a.panoptic_epoch_start (default 0): the epoch from which the semantic and instance terms are formed, as sem_epoch_start / inst_epoch_start of
    pc_nerf/trainer.py:400-432 (both 601 in configs/bup20/best.yaml); earlier epochs render and supervise rgb alone.
    -> (nef, tracer, the losses as one device tensor)."""
    import pagnerf_amd
    args = bench.parse(["--rays", str(a.rays), "--samples", str(a.samples), "--grid", a.grid, "--precision", precision, "--graphs", getattr(a, "graphs", "on")])
    nef, tracer = bench.make_model(args, dev, seed=0), bench.make_tracer(args)
    opt = bench.make_optimizer(nef)
    start = int(getattr(a, "panoptic_epoch_start", 0))
    B = min(batch_images or a.batch_images, ds.num_imgs)
    sampler = pagnerf_amd.BatchSampler(ds, batch_size=B, num_samples=max(1, a.rays // B), seed=123, drop_last=True)
    losses = []
    while len(losses) < steps:
        chans = ["rgb", "semantics", "inst_embedding"] if sampler.epoch >= start else ["rgb"]
        for batch in sampler:
            rays, gt = batch_to_step(batch)
            losses.append(bench.train_step(nef, tracer, opt, rays, gt, chans, 1).detach())
            if len(losses) == steps:
                break
    return nef, tracer, torch.stack(losses)


def run(precision, a, dev):
    if getattr(a, "from_images", None):
        return run_from_images(precision, a, dev)
    args = bench.parse(["--rays", str(a.rays), "--samples", str(a.samples), "--grid", a.grid, "--precision", precision])
    nef, tracer = bench.make_model(args, dev, seed=0), bench.make_tracer(args)
    opt = bench.make_optimizer(nef)
    chans = ["rgb", "semantics", "inst_embedding"]
    contrastive = a.inst_loss == "sup_contrastive"
    if contrastive:
        nef.inst_softmax = False                                     # best_contrast_delta.yaml: inst_softmax false
    tv = dict(grid_tvl1_reg=a.grid_tvl1, grid_tvl2_reg=a.grid_tvl2, delta_grid_tvl1_reg=a.delta_grid_tvl1, delta_grid_tvl2_reg=a.delta_grid_tvl2,
              tv_window_size=a.tv_window_size, tv_edge_num_samples=a.tv_edge_num_samples)
    if not any(tv[k] > 0.0 for k in ("grid_tvl1_reg", "grid_tvl2_reg", "delta_grid_tvl1_reg", "delta_grid_tvl2_reg")):
        tv = None
    gen = torch.Generator().manual_seed(123)
    for step in range(a.steps):
        rays, gt = scene_rays(a.rays, gen, dev)
        if contrastive:
            loss = contrastive_step(nef, tracer, opt, rays, gt, chans, tv)
        elif tv is not None:
            loss = nll_tv_step(nef, tracer, opt, rays, gt, chans, tv)
        else:
            loss = bench.train_step(nef, tracer, opt, rays, gt, chans, 1)
    gen = torch.Generator().manual_seed(999)
    rays, gt = scene_rays(4 * a.rays, gen, dev)
    with torch.no_grad():
        import pagnerf_amd
        rb = pagnerf_amd.batch_render(pagnerf_amd.Pipeline(nef, tracer), rays, channels=chans, render_batch=a.rays)
    mse = float(((rb.rgb - gt["rgb"]) ** 2).mean())
    vs_oracle = None
    if a.oracle_psnr:
        # "PSNR vs ref" anchored on the CPU oracle: the TRAINED parameters rendered by the HIP path and by the oracle chain (same samples,
        # same jitter) on a subset of the held-out rays; the helper lives under tests/ (nothing outside tests/ imports oracle/)
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        from test_gpu_trajectory import hip_vs_oracle_render
        import pagnerf_amd
        n = a.oracle_psnr
        sub = pagnerf_amd.Rays(rays.origins[:n], rays.dirs[:n], rays.dist_min, rays.dist_max)
        r = hip_vs_oracle_render(nef, tracer, sub, a.samples)
        g = gt["rgb"][:n].float().cpu()
        vs_oracle = dict(rays=n, samples=r["samples"], psnr_hip_vs_oracle_db=r["psnr_hip_vs_oracle_db"],
                         psnr_hip_vs_gt_db=round(-10 * math.log10(float(((r["rgb_hip"] - g) ** 2).mean())), 2),
                         psnr_oracle_vs_gt_db=round(-10 * math.log10(float(((r["rgb_oracle"] - g) ** 2).mean())), 2),
                         sem_max_abs_diff=round(r["sem_max_abs_diff"], 5), inst_max_abs_diff=round(r["inst_max_abs_diff"], 5))
    if contrastive:
        gen = torch.Generator().manual_seed(321)                     # training-distribution rays (not the held-out set) for the centroids
        train_rays, train_gt = scene_rays(4 * a.rays, gen, dev)
        with torch.no_grad():
            import pagnerf_amd
            tb = pagnerf_amd.batch_render(pagnerf_amd.Pipeline(nef, tracer), train_rays, channels=chans, render_batch=a.rays)
        inst_pred = nearest_centroid(tb.inst_embedding, train_gt["inst"], rb.inst_embedding)
        ms_pred, n_clusters = mean_shift_ids(tb.inst_embedding, train_gt["inst"], rb.inst_embedding)
    else:
        inst_pred = rb.inst_embedding.argmax(-1)
    hit = gt["inst"] >= 0
    out = dict(precision=precision, inst_loss=a.inst_loss, vs_oracle=vs_oracle, final_loss=float(loss.detach()), psnr_db=round(-10 * math.log10(mse), 2),
               sem_acc=round(float((rb.semantics.argmax(-1) == gt["sem"])[gt["sem"] >= 0].float().mean()), 4),
               inst_acc=round(float((inst_pred == gt["inst"])[hit].float().mean()), 4))
    if contrastive:
        out.update(inst_acc_mean_shift=round(float((ms_pred == gt["inst"])[hit].float().mean()), 4), n_clusters=n_clusters)
    return out


def run_from_images(precision, a, dev):
    """--from-images: train through the dataset and its sampler, then score on the held-out random rays of the default path."""
    import pagnerf_amd
    V, (H, W) = int(a.from_images[0]), (int(x) for x in a.from_images[1].lower().split("x"))
    ds = scene_images(V, H, W, dev)
    nef, tracer, losses = train_from_images(precision, a, dev, ds, a.steps)
    rays, gt = scene_rays(4 * a.rays, torch.Generator().manual_seed(999), dev)
    with torch.no_grad():
        rb = pagnerf_amd.batch_render(pagnerf_amd.Pipeline(nef, tracer), rays, channels=["rgb", "semantics", "inst_embedding"], render_batch=a.rays)
    mse = float(((rb.rgb - gt["rgb"]) ** 2).mean())
    hit = gt["inst"] >= 0
    return dict(precision=precision, images=[V, H, W], dataset_bytes=ds.nbytes, first_loss=float(losses[0]), final_loss=float(losses[-1]),
                psnr_db=round(-10 * math.log10(mse), 2), sem_acc=round(float((rb.semantics.argmax(-1) == gt["sem"])[gt["sem"] >= 0].float().mean()), 4),
                inst_acc=round(float((rb.inst_embedding.argmax(-1) == gt["inst"])[hit].float().mean()), 4))


def nll_tv_step(nef, tracer, opt, rays, gt, channels, tv):
    """bench.train_step's all-channel step (rgb L1 x 10, semantic NLL x 0.1, instance NLL x 1000) + the grid total-variation terms (trainer.py:556-574)."""
    from pagnerf_amd import step_tv_terms
    from pagnerf_amd.loss import render_loss, NllTerm
    opt.zero_grad(set_to_none=True)
    rb = tracer(nef, channels=channels, rays=rays, stage="train")
    loss, _ = render_loss(rb.rgb, gt["rgb"], 10.0, NllTerm(rb.semantics, gt["sem"], weight=0.1), NllTerm(rb.inst_embedding, gt["inst"], weight=1000.0))
    loss = loss + step_tv_terms(nef, **tv)
    loss.backward()
    opt.step()
    return loss


def contrastive_step(nef, tracer, opt, rays, gt, channels, tv=None):
    """rgb L1 (weight 10) + semantic NLL (0.1) as bench.train_step forms them, + inst_weight 0.1 x SupConLoss on the rays that hit
    (pc_nerf/trainer.py:499-503 with best_contrast_delta.yaml's weights); tv: the grid total-variation terms' options (trainer.py:556-574) or None."""
    from pagnerf_amd import step_tv_terms
    from pagnerf_amd.loss import render_loss, NllTerm, SupConLoss
    opt.zero_grad(set_to_none=True)
    rb = tracer(nef, channels=channels, rays=rays, stage="train")
    loss, _ = render_loss(rb.rgb, gt["rgb"], 10.0, NllTerm(rb.semantics, gt["sem"], weight=0.1))
    emb = rb.inst_embedding.reshape(1, -1, rb.inst_embedding.shape[-1])
    ids = gt["inst"].reshape(1, -1)
    loss = loss + 0.1 * SupConLoss(temperature=0.07, pn_ratio=0.5)(emb, ids, reduction="mean", anchor_mask=ids >= 0)
    if tv is not None:
        loss = loss + step_tv_terms(nef, **tv)
    loss.backward()
    opt.step()
    return loss


def mean_shift_ids(train_emb, train_ids, emb, images=16):
    """The contrastive configs' own route to ids (pc_nerf/trainer.py:948-970 and :737-738): MeanShift fitted on the normalised embeddings of the
    training rays that hit, split into `images` pseudo-images (class means per image and id, so K >= 25), then predict on the raw held-out
    embeddings.  Each cluster is named by the majority id of the training rays it predicts.  -> (ids of emb's rows, number of clusters)."""
    from pagnerf_amd.cluster import MeanShift
    keep = train_ids >= 0
    f, ids = train_emb[keep], train_ids[keep]
    m = f.shape[0] // images
    ms = MeanShift(num_clustering_workers=6)
    ms.train_clustering(torch.nn.functional.normalize(f[:images * m].float(), dim=-1).reshape(images, m, -1), ids[:images * m].reshape(images, m))
    C = ms.cluster_centers_.shape[0]
    n_ids = int(ids.max()) + 1
    votes = torch.bincount(ms.predict_clusters(f) * n_ids + ids, minlength=C * n_ids).reshape(C, n_ids)
    return votes.argmax(1)[ms.predict_clusters(emb)], C


def nearest_centroid(train_emb, train_ids, emb):
    """Per id the mean of the normalised training embeddings; each row of `emb` takes the id of the closest centroid in cosine."""
    f = torch.nn.functional.normalize(train_emb.float(), dim=-1)
    keep = train_ids >= 0
    ids = torch.unique(train_ids[keep])
    cent = torch.stack([f[train_ids == i].mean(0) for i in ids.tolist()])
    sim = torch.nn.functional.normalize(emb.float(), dim=-1) @ torch.nn.functional.normalize(cent, dim=-1).T
    return ids[sim.argmax(-1)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--grid", default="permuto")
    ap.add_argument("--oracle-psnr", type=int, default=0, metavar="RAYS",
                    help="also render RAYS held-out rays of the trained model with the CPU oracle (tests/test_gpu_trajectory.py) and report the "
                         "PSNR of the HIP render against it, next to both renders' PSNR against the ground truth")
    ap.add_argument("--inst-loss", choices=("nll", "sup_contrastive"), default="nll",
                    help="instance term: per-ray NLL on the softmaxed head (default), or the supervised-contrastive loss on a raw embedding")
    for flag in ("--grid-tvl1", "--grid-tvl2", "--delta-grid-tvl1", "--delta-grid-tvl2"):
        ap.add_argument(flag, type=float, default=0.0, metavar="W",
                        help="weight of the %s_reg term of pc_nerf/trainer.py:556-574 (0: the term is not formed)" % flag[2:].replace("-", "_"))
    ap.add_argument("--tv-window-size", type=float, default=0.0001, help="tv_window_size (the YAMLs' 0.0001): enters only the lattice's random first vertex")
    ap.add_argument("--tv-edge-num-samples", type=int, default=100, help="tv_edge_num_samples (the YAMLs' 100): the lattice has this + 1 points per edge")
    ap.add_argument("--from-images", nargs=2, metavar=("V", "HxW"), default=None,
                    help="train from V rendered images of H x W pixels through DeviceMultiviewDataset + BatchSampler instead of fresh random rays")
    ap.add_argument("--batch-images", type=int, default=None, help="--from-images: views per step (default 6, best.yaml's batch size)")
    ap.add_argument("--panoptic-epoch-start", type=int, default=0, metavar="E",
                    help="--from-images: epochs before E train rgb alone, as sem_epoch_start / inst_epoch_start do in the trainer (best.yaml: 601); 0 = all "
                         "terms from the first step, like the default path")
    a = ap.parse_args()
    if a.from_images is None and (a.batch_images is not None or a.panoptic_epoch_start):
        ap.error("--batch-images and --panoptic-epoch-start belong to --from-images")
    a.batch_images = 6 if a.batch_images is None else a.batch_images
    dev = torch.device("cuda:0")
    import __graft_entry__ as ge
    ge.build()
    out = [run(p, a, dev) for p in ("bf16", "fp32")]
    print(json.dumps(dict(scene="analytic sphere, %d steps x %d rays x %d samples, %s grid" % (a.steps, a.rays, a.samples, a.grid), runs=out)))
