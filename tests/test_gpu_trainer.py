"""PanopticTrainer on the GPU (pagnerf_amd/trainer.py, config.py, train.py): the epoch schedule end to end, the frozen-field validation-pose epoch, the
graph path through the schedule's switches, the contrastive route with its clustering, the validation row, resume, and the command line.

The scene is analytic: a textured sphere (radius 0.35, three 'thing' instances by longitude) over a plane (z = -0.4, 'stuff'), white background,
seen by downward cameras - 4 training and 2 validation views of 32 x 32 pixels with semantic and instance labels and world-to-camera matrices.
Model: PermutoGrid (8 levels x 2 features, 2^12 rows), 5 classes, 16 instances; batch 2 views x 128 rays, 32 march steps, render_batch 512."""
import csv
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

H = W = 32
THINGS, STUFF = [2, 3, 4], [0, 1]
NEAR, FAR = 0.0, 1.9


# ------------------------------------------------------------------------------------------------------------------------------------- the scene
def view_matrices(n, phase):
    """World -> camera matrices of n cameras at height 0.95 looking down, on a circle of radius 0.25, each turned a little about the vertical."""
    views = torch.eye(4).repeat(n, 1, 1)
    for i in range(n):
        a = phase + 2 * math.pi * i / n
        yaw = 0.1 * math.sin(3 * a)
        R = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        centre = torch.tensor([0.25 * math.cos(a), 0.25 * math.sin(a), 0.95])
        views[i, :3, :3] = R
        views[i, :3, 3] = -R @ centre                      # o_w = R^T (0 - t) = centre
    return views


def base_rays():
    """Camera-frame rays of one H x W image: origin 0, direction (x, y, -1) over a +-0.55 field."""
    ys, xs = torch.meshgrid((torch.arange(H) + 0.5) / H - 0.5, (torch.arange(W) + 0.5) / W - 0.5, indexing="ij")
    d = torch.stack([xs * 1.1, ys * 1.1, -torch.ones_like(xs)], -1).reshape(-1, 3)
    return torch.zeros_like(d), d


def scene_truth(o, d):
    """Closed form for world rays (o, unit d) [n,3]: colour, semantic class and instance id of the first hit (sphere, else plane, else background)."""
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - 0.35 ** 2)
    hit_s = disc > 0
    ts = -b - torch.sqrt(disc.clamp_min(0))
    ps = o + d * ts[:, None]
    tp = (-0.4 - o[:, 2]) / d[:, 2]
    pp = o + d * tp[:, None]
    hit_p = (tp > 0) & (pp[:, :2].abs().max(-1)[0] < 0.9)
    rgb_s = 0.5 + 0.5 * torch.sin(ps * 9.0 + torch.tensor([0.0, 2.0, 4.0]))
    rgb_p = torch.stack([0.25 + 0.2 * torch.sin(pp[:, 0] * 5), 0.45 + 0.2 * torch.cos(pp[:, 1] * 5), torch.full_like(tp, 0.2)], -1)
    rgb = torch.where(hit_s[:, None], rgb_s, torch.where(hit_p[:, None], rgb_p, torch.ones_like(rgb_p)))
    sector = ((torch.atan2(ps[:, 1], ps[:, 0]) + math.pi) / (2 * math.pi) * 3).long().clamp(0, 2)           # three things
    sem = torch.where(hit_s, 2 + sector % 2, torch.where(hit_p, torch.ones_like(sector), torch.zeros_like(sector)))
    inst = torch.where(hit_s, 1 + sector, torch.zeros_like(sector))
    return rgb.float(), sem, inst


def scene_arrays(views):
    oc, dc = base_rays()
    V = views.shape[0]
    R, t = views[:, :3, :3], views[:, :3, 3]
    o = torch.matmul(oc[None] - t[:, None, :], R)                                                            # R^T (o - t), row-vector form
    d = torch.nn.functional.normalize(torch.matmul(dc[None].expand(V, -1, -1), R), dim=-1)
    rgb, sem, inst = scene_truth(o.reshape(-1, 3), d.reshape(-1, 3))
    return dict(imgs=rgb.reshape(V, H, W, 3), semantics=sem.reshape(V, H, W, 1), instance=inst.reshape(V, H, W, 1)), oc, dc


def make_dataset(views, dev):
    import pagnerf_amd
    data, oc, dc = scene_arrays(views)
    data["base_rays"] = pagnerf_amd.Rays(oc, dc, dist_min=NEAR, dist_max=FAR)
    ds = pagnerf_amd.DeviceMultiviewDataset(data, dev)
    ds.view_matrices = views
    ds.image_shape = (H, W)
    ds.semantic_info = dict(num_classes=5, num_instances=16, things_ids=THINGS, stuff_ids=STUFF)
    ds.labelled = [(True, True)] * views.shape[0]
    ds.filenames = ["view_%02d.png" % i for i in range(views.shape[0])]
    return ds


TRAIN_VIEWS, VAL_VIEWS = view_matrices(4, 0.0), view_matrices(2, 0.6)

CFG = dict(nef_type="PanopticDeltaNeF", tracer_type="PanopticPackedRFTracer", grid_type="PermutoGrid", num_lods=8, feature_dim=2, capacity_log_2=12,
           delta_capacity_log_2=12, coarsest_scale=1.0, finest_scale=0.01, blas_level=5, hidden_dim=64, num_layers=1, sem_num_layers=1,
           inst_num_layers=2, sem_softmax=True, inst_softmax=True, panoptic_features_type="delta", view_multires=4, raymarch_type="ray", num_steps=32,
           samples_per_voxel=2, bg_color="white", ray_max_travel=2.0, batch_size=2, num_rays_sampled_per_img=128, render_batch=512, lr=0.001,
           grid_lr_weight=100.0, delta_grid_lr_weight=100.0, rgb_weight=10.0, sem_weight=0.1, inst_weight=1.0, inst_loss="linear_assignment_things",
           inst_outlier_rejection=True, inst_num_dilations=1, optimize_extrinsics=True, optimize_val_extrinsics=True, extrinsics_lr=1e-3,
           anchor_frame_idxs=[0], epochs=5, save_every=-1, valid_every=-1, sem_epoch_start=0, inst_epoch_start=0)


def make_trainer(dev, log_dir, seed=11, **over):
    """build_from_config on the scene.  The density bias puts the initial densities astride the prune threshold (0.01 * 512 / sqrt 3 = 2.956), and the
    tables start wide enough (sigma 1e-2) for the densities to differ from cell to cell."""
    from pagnerf_amd import config
    torch.manual_seed(seed)
    cfg = dict(CFG, log_dir=str(log_dir))
    cfg.update(over)
    pipe, tr = config.build_from_config(cfg, make_dataset(TRAIN_VIEWS, dev), make_dataset(VAL_VIEWS, dev), device=dev)
    with torch.no_grad():
        pipe.nef.decoder_density.lout.bias[0] = 2.96
        for g in (pipe.nef.grid, pipe.nef.delta_grid):
            g.tables.normal_(0.0, 1e-2)
    return pipe, tr


def snapshot(module):
    return {n: p.detach().clone() for n, p in module.named_parameters()}


def adam_state(opt, params):
    return [{k: v.clone() for k, v in opt.state[p].items()} for p in params if p in opt.state]


def step_counts(opt):
    return sorted({int(opt.state[p]["step"]) for g in opt.param_groups for p in g["params"] if p in opt.state})


# ----------------------------------------------------------------------------------------------------------------------- the schedule, end to end
SCHEDULE = dict(prune_at_epoch=1, voxel_raymarch_epoch_start=1, sem_epoch_start=3, inst_epoch_start=3, optimize_val_extrinsics=False)


def run_schedule(dev, log_dir, use_graphs):
    pipe, tr = make_trainer(dev, log_dir, use_graphs=use_graphs, **SCHEDULE)
    nef = pipe.nef
    frozen = lambda: {n: p.detach().clone() for n, p in nef.named_parameters() if n.startswith(("delta_grid.", "decoder_semantics.", "decoder_inst."))}
    rec = dict(initial=frozen(), logs=[], frozen_after=[], march=[], steps=[], optimizers=[], plans=[])
    for e in range(6):
        assert tr.epoch == e
        tr.run_epoch()
        rec["plans"].append(tr.plan)
        rec["logs"].append(dict(tr.log_dict))
        rec["frozen_after"].append(frozen())
        rec["march"].append((pipe.tracer.raymarch_type, pipe.tracer.num_steps, nef.raymarch_type))
        rec["steps"].append(step_counts(tr.optimizer))
        rec["optimizers"].append(tr.optimizer)
        if e == 1:
            rec["bits_after_prune"] = nef.grid.blas_bits.clone()
            rec["delta_bits_after_prune"] = nef.delta_grid.blas_bits.clone()
    rec["lrs"] = [(g["name"], g["lr"]) for g in tr.optimizer.param_groups]
    rec["final_bits"] = nef.grid.blas_bits.clone()
    rec["use_graphs"] = pipe.tracer.use_graphs
    rec["graph_runner"] = pipe.tracer._graphs
    return rec


@pytest.fixture(scope="module")
def eager_schedule(gpu_device, tmp_path_factory):
    return run_schedule(gpu_device, tmp_path_factory.mktemp("eager"), use_graphs=False)


def check_schedule(rec):
    assert [p["channels"] for p in rec["plans"]] == [["rgb", "depth"]] * 3 + [["rgb", "semantics", "inst_embedding", "depth"]] * 3
    assert rec["march"][0] == ("ray", 32, "ray")
    for e in range(1, 6):                                              # after epoch 1: the voxel march with samples_per_voxel
        assert rec["march"][e] == ("voxel", 2, "voxel"), e
    for e in range(3):                                                 # until epoch 3 the panoptic branch has not moved at all
        for n, v in rec["initial"].items():
            assert torch.equal(rec["frozen_after"][e][n], v), (e, n)
    assert not torch.equal(rec["frozen_after"][3]["delta_grid.tables"], rec["initial"]["delta_grid.tables"])
    assert not torch.equal(rec["frozen_after"][3]["decoder_inst.lout.weight"], rec["initial"]["decoder_inst.lout.weight"])
    # the prune of epoch 1 re-initialises the optimiser: a new object whose step counters start again
    assert rec["optimizers"][1] is not rec["optimizers"][0] and rec["optimizers"][2] is rec["optimizers"][1]
    assert rec["steps"][0] == [2] and rec["steps"][1] == [] and rec["steps"][2] == [2] and rec["steps"][5] == [6, 8]
    kept = int((rec["bits_after_prune"] != 0).sum())
    assert torch.equal(rec["bits_after_prune"], rec["delta_bits_after_prune"]) and kept > 0
    for e, log in enumerate(rec["logs"]):
        assert log["total_iter_count"] == 2
        for k in ("total_loss", "rgb_loss", "sem_loss", "contrast_sem_loss", "inst_loss"):
            assert math.isfinite(log[k]), (e, k, log[k])
        assert (log["sem_loss"] > 0) == (e >= 3) and (log["inst_loss"] > 0) == (e >= 3), (e, log)
    print("rgb loss per epoch", ["%.4f" % l["rgb_loss"] for l in rec["logs"]])
    assert rec["logs"][2]["rgb_loss"] < rec["logs"][0]["rgb_loss"]


def test_schedule_end_to_end(eager_schedule):
    """Six epochs, eager: rgb + depth with the ray march, prune and the switch to the voxel march after epoch 1, the panoptic heads from epoch 3."""
    assert eager_schedule["use_graphs"] is False
    check_schedule(eager_schedule)


def test_schedule_on_the_graph_path(gpu_device, tmp_path, eager_schedule):
    """The same schedule with use_graphs=True: it runs through every switch of the graph configuration (channel set, march, re-made parameters' optimiser)
    and ends in the same discrete state as the eager run from the same seed."""
    rec = run_schedule(gpu_device, tmp_path, use_graphs=True)
    assert rec["use_graphs"] is True and rec["graph_runner"] is not None
    check_schedule(rec)
    assert rec["march"] == eager_schedule["march"]
    assert rec["lrs"] == eager_schedule["lrs"]
    assert rec["steps"] == eager_schedule["steps"]
    diff = int((rec["bits_after_prune"] != eager_schedule["bits_after_prune"]).sum())
    print("occupancy words that differ between the graph and the eager run after the prune of epoch 1:", diff)
    assert torch.equal(rec["bits_after_prune"], eager_schedule["bits_after_prune"])
    assert torch.equal(rec["final_bits"], eager_schedule["final_bits"])


# ------------------------------------------------------------------------------------------------------------------- no added synchronisation
def count_syncs(fn, n):
    """Host waits for the device that torch reports (sync debug mode 'warn') over n calls of fn."""
    import warnings
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            for _ in range(n):
                fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def test_step_adds_no_host_synchronisation(gpu_device, tmp_path):
    """The full step (all channels, linear assignment with outlier rejection, pose optimisation, scheduler, log accumulation) on the graph path waits
    for the device no more often than the bare pieces called by hand on the same batch, and log_epoch() is the one read of the epoch."""
    from pagnerf_amd.loss import LinAssignmentThingsLoss, NllTerm, render_loss
    pipe, tr = make_trainer(gpu_device, tmp_path, use_graphs=True, optimize_val_extrinsics=False, use_lr_scheduler=True, lr_scheduler_type="step",
                            lr_step_size=50)
    tr.begin_epoch()
    batch = next(iter(tr.sampler))
    assert tr.plan["channels"] == ["rgb", "semantics", "inst_embedding", "depth"]
    inst_loss, stuff = LinAssignmentThingsLoss(outlier_rejection=True), torch.tensor(STUFF, device=gpu_device)

    def bare():
        tr.optimizer.zero_grad(set_to_none=True)
        o, d, cam = batch["base_rays"].origins.reshape(-1, 3), batch["base_rays"].dirs.reshape(-1, 3), batch["cam_idx"]
        rb = pipe.tracer(pipe.nef, channels=tr.plan["channels"], rays=pipe.transform_rays_indexed(o, d, cam), stage="train")
        sem = batch["semantics"].reshape(-1)
        loss, _ = render_loss(rb.rgb, batch["imgs"].reshape(-1, 3), 10.0, NllTerm(rb.semantics, sem, weight=0.1, mean_over="all"))
        pts = pipe.rays_to_3d_points_indexed(o, d, rb.depth.detach(), cam).reshape(2, -1, 3)
        il = inst_loss(rb.inst_embedding.reshape(2, -1, 16), batch["instance"].reshape(2, -1), stuff_mask=torch.isin(sem, stuff).reshape(2, -1), points_3d=pts)
        (loss + il.mean()).backward()
        tr.optimizer.step()
    for _ in range(4):                       # sample count, capture, first replays; both forms share the tracer's graph configuration
        tr.step(batch)
        bare()
    n_bare, n_trainer = count_syncs(bare, 3), count_syncs(lambda: tr.step(batch), 3)
    print("host synchronisations in 3 steps: bare pieces %d, PanopticTrainer.step %d" % (n_bare, n_trainer))
    assert n_trainer <= n_bare
    assert count_syncs(tr.log_epoch, 1) == 1 and math.isfinite(tr.log_dict["total_loss"]) and tr.log_dict["total_iter_count"] == 7


# --------------------------------------------------------------------------------------------------------------------- the validation-pose epoch
def test_validation_pose_epoch(gpu_device, tmp_path):
    pipe, tr = make_trainer(gpu_device, tmp_path, use_graphs=False, val_extrinsics_start=1, val_extrinsics_every=2)
    nef, ext = pipe.nef, pipe.camera_extrinsics
    assert ext.shape == (6, 9) and tr.val_cam_offset == 4
    start = ext.detach().clone()
    tr.run_epoch()
    tr.run_epoch()
    assert not tr.training_val_poses and "sem_loss" in tr.log_dict
    moved = (ext.detach() != start).any(1)
    assert moved[1:4].all() and not moved[0] and not moved[4:].any()           # training cameras move, the anchor and the unseen validation cameras do not
    nef_params = [p for p in nef.parameters()]
    before, state_before, ext_before = snapshot(nef), adam_state(tr.optimizer, nef_params), ext.detach().clone()
    assert len(state_before) > 0
    assert tr.epoch_plan(2)["val_pose_epoch"] and tr.epoch_plan(2)["channels"] == ["rgb", "depth"]
    tr.run_epoch()                                                             # epoch 2: validation poses only
    assert tr.training_val_poses
    for n, p in nef.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
        assert p.grad is None, n
    for a, b in zip(adam_state(tr.optimizer, nef_params), state_before):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    now = ext.detach()
    assert (now[4:] != ext_before[4:]).any(1).all(), "the validation cameras' rows did not move"
    assert torch.equal(now[:4], ext_before[:4]), "training / anchor rows moved in a validation-pose epoch"
    assert set(tr.log_dict) == {"rgb_val_pose_loss", "total_iter_count"} and math.isfinite(tr.log_dict["rgb_val_pose_loss"])
    assert tr.log_dict["rgb_val_pose_loss"] > 0 and tr.log_dict["total_iter_count"] == 1
    tr.run_epoch()                                                             # epoch 3: the field trains again
    assert not tr.training_val_poses and all(p.requires_grad for p in nef.parameters())
    changed = [n for n, p in nef.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert "grid.tables" in changed and "delta_grid.tables" in changed and "decoder_color.lout.weight" in changed
    assert "sem_loss" in tr.log_dict and "rgb_val_pose_loss" not in tr.log_dict


# ------------------------------------------------------------------------------------------------------- the contrastive route and the validation row
def read_csv(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_contrastive_route_fits_the_clustering(gpu_device, tmp_path):
    pipe, tr = make_trainer(gpu_device, tmp_path, use_graphs=False, nef_type="MeanShiftPanopticDeltaNeF", inst_loss="sup_contrastive", inst_softmax=False,
                            inst_outlier_rejection=False, inst_weight=0.1, num_clustering_samples=1024, num_clustering_workers=2)
    import pagnerf_amd
    assert isinstance(pipe.nef, pagnerf_amd.MeanShiftPanopticDeltaNeF) and not pipe.nef.clustering_obj.fitted
    tr.run_epoch()
    tr.run_epoch()
    assert math.isfinite(tr.log_dict["inst_loss"]) and tr.log_dict["inst_loss"] > 0
    metrics = tr.validate(1)
    assert pipe.nef.clustering_obj.fitted and pipe.nef.clustering_obj.cluster_centers_.shape[1] == 16
    rows = read_csv(os.path.join(str(tmp_path), "metrics.csv"))
    assert len(rows) == 2 and rows[0] == list(metrics) and float(rows[1][rows[0].index("epoch")]) == 1
    assert math.isfinite(metrics["val/psnr"])


def test_validation_row_and_saved_predictions(gpu_device, tmp_path):
    from pagnerf_amd.metrics import ValidationMetrics
    pipe, tr = make_trainer(gpu_device, tmp_path, use_graphs=False, save_preds=True)
    tr.run_epoch()
    first = tr.validate(0)
    second = tr.validate(1)
    rows = read_csv(os.path.join(str(tmp_path), "metrics.csv"))
    assert len(rows) == 3, "one header and one row per validate()"
    columns = list(ValidationMetrics(5, THINGS, STUFF).compute()) + ["epoch"]
    assert rows[0] == columns and list(first) == columns
    assert {"val/psnr", "val/iou", "val/map_", "val/pq_all", "val/sq_things", "val/rq_stuff", "epoch"} <= set(columns)
    assert [float(r[columns.index("epoch")]) for r in rows[1:]] == [0.0, 1.0]
    assert float(rows[1][columns.index("val/psnr")]) == pytest.approx(first["val/psnr"]) and math.isfinite(second["val/psnr"])
    assert 0 < first["val/psnr"] < 60
    for i in range(2):
        pan = np.load(os.path.join(str(tmp_path), "panoptic", "view_%02d.npy" % i))
        conf = np.load(os.path.join(str(tmp_path), "inst_conf", "view_%02d.npy" % i))
        assert pan.shape == (2, H, W) and pan.dtype == np.uint8 and pan[0].max() < 5 and pan[1].max() < 16
        assert conf.shape == (H, W) and conf.dtype == np.float32 and (conf >= 0).all() and (conf <= 1.001).all()
    assert pipe.training is False                                               # validate() leaves the pipeline in eval mode (fp32 coordinates)


# ---------------------------------------------------------------------------------------------------------------------------------------- resume
RESUME = dict(prune_at_epoch=0, voxel_raymarch_epoch_start=0, use_lr_scheduler=True, lr_scheduler_type="step", lr_step_size=1,
              lr_step_gamma=0.5, use_graphs=False, save_every=1, save_as_new=True, valid_every=1)


def discrete_state(pipe, tr):
    tr.train_sampler.set_epoch(tr.epoch)
    views = tr.train_sampler.views()
    nxt = tr.dataset.sample(views[0], tr.num_rays_sampled_per_img, ray_idx=True)
    return dict(epoch=tr.epoch, steps=step_counts(tr.optimizer), lrs=[g["lr"] for g in tr.optimizer.param_groups],
                march=(pipe.tracer.raymarch_type, pipe.tracer.num_steps), bits=pipe.nef.grid.blas_bits.clone(), views=[v.tolist() for v in views],
                pixels=nxt["ray_idx"].clone(), total_steps=tr.total_steps, sched=tr.lr_scheduler.last_epoch)


def test_resume_continues_the_run(gpu_device, tmp_path):
    """Three epochs in one go against two epochs + checkpoint + a FRESH trainer (other initial weights) + resume + one epoch.  The discrete state must be
    equal; the parameters may differ by what two uninterrupted runs from the same seed differ by (bit-identical if those are)."""
    def uninterrupted(name):
        pipe, tr = make_trainer(gpu_device, tmp_path / name, **RESUME)
        for _ in range(3):
            tr.run_epoch()
        return pipe, tr
    pipe_a, tr_a = uninterrupted("a")
    pipe_b, tr_b = uninterrupted("b")
    sa, sb = snapshot(pipe_a), snapshot(pipe_b)
    run_to_run = max(float((sa[n].double() - sb[n].double()).abs().max()) for n in sa)
    print("largest element-wise difference between two uninterrupted runs from the same seed: %.3e" % run_to_run)

    pipe_c, tr_c = make_trainer(gpu_device, tmp_path / "c", **RESUME)
    tr_c.run_epoch()
    tr_c.run_epoch()
    ckpt = tr_c.save_checkpoint(str(tmp_path / "c" / "two_epochs.pth"))
    pipe_d, tr_d = make_trainer(gpu_device, tmp_path / "d", seed=99, **RESUME)
    assert not torch.equal(pipe_d.nef.grid.tables, pipe_c.nef.grid.tables)
    tr_d.resume(ckpt)
    assert tr_d.epoch == 2 and pipe_d.tracer.raymarch_type == "voxel" and pipe_d.tracer.num_steps == 2
    for n, p in pipe_d.named_parameters():
        assert torch.equal(p.detach(), dict(pipe_c.named_parameters())[n].detach()), n
    assert torch.equal(pipe_d.nef.grid.blas_bits, pipe_c.nef.grid.blas_bits) and torch.equal(pipe_d.nef.grid.occupancy.cpu(), pipe_c.nef.grid.occupancy.cpu())
    tr_d.run_epoch()

    want, got = discrete_state(pipe_a, tr_a), discrete_state(pipe_d, tr_d)
    assert got["epoch"] == want["epoch"] == 3 and got["total_steps"] == want["total_steps"] == 6 and got["sched"] == want["sched"]
    assert got["steps"] == want["steps"] == [4] and got["lrs"] == want["lrs"] and got["march"] == want["march"] == ("voxel", 2)
    assert got["lrs"][0] == pytest.approx(0.001 * 0.5 ** 3)
    assert torch.equal(got["bits"], want["bits"]) and 0 < int((got["bits"] != 0).sum())
    assert got["views"] == want["views"] and torch.equal(got["pixels"], want["pixels"])
    sd = snapshot(pipe_d)
    resumed = max(float((sa[n].double() - sd[n].double()).abs().max()) for n in sa)
    print("largest element-wise difference between the resumed and an uninterrupted run: %.3e" % resumed)
    if run_to_run == 0.0:
        assert resumed == 0.0
    else:
        assert resumed <= 2 * run_to_run

    # the periodic checkpoint end_epoch() wrote on its own after epoch 1 of run a (after that epoch's validation and the optimiser's re-initialisation)
    periodic = str(tmp_path / "a" / "model-ep1.pth")
    assert os.path.exists(periodic) and os.path.exists(str(tmp_path / "a" / "model-ep2.pth")) and not os.path.exists(str(tmp_path / "a" / "model-ep0.pth"))
    pipe_e, tr_e = make_trainer(gpu_device, tmp_path / "e", seed=5, **RESUME)
    tr_e.resume(periodic)
    assert tr_e.epoch == 2 and pipe_e.tracer.raymarch_type == "voxel"
    tr_e.run_epoch()
    got = discrete_state(pipe_e, tr_e)
    assert got["epoch"] == 3 and got["steps"] == want["steps"] and got["lrs"] == want["lrs"] and got["march"] == want["march"] and got["sched"] == want["sched"]
    assert torch.equal(got["bits"], want["bits"]) and got["views"] == want["views"] and torch.equal(got["pixels"], want["pixels"])
    se = snapshot(pipe_e)
    periodic_diff = max(float((sa[n].double() - se[n].double()).abs().max()) for n in sa)
    print("largest element-wise difference between the run resumed from the periodic checkpoint and an uninterrupted run: %.3e" % periodic_diff)
    assert periodic_diff == 0.0 if run_to_run == 0.0 else periodic_diff <= 2 * run_to_run
    rows = read_csv(os.path.join(str(tmp_path / "a"), "metrics.csv"))
    assert [float(r[rows[0].index("epoch")]) for r in rows[1:]] == [1.0, 2.0]


# ------------------------------------------------------------------------------------------------------------------------------- the command line
def write_npz(path, views):
    data, oc, dc = scene_arrays(views)
    np.savez(path, imgs=data["imgs"].numpy(), semantics=data["semantics"].numpy(), instance=data["instance"].numpy(),
             base_rays_origins=oc.reshape(H, W, 3).numpy(), base_rays_dirs=dc.reshape(H, W, 3).numpy(), base_rays_range=np.array([NEAR, FAR], np.float32),
             view_matrices=views.numpy(), num_classes=5, num_instances=16, things_ids=np.array(THINGS), stuff_ids=np.array(STUFF),
             filenames=np.array(["view_%02d.png" % i for i in range(views.shape[0])]))


def test_command_line(gpu_device, tmp_path):
    """`python -m pagnerf_amd.train` in a fresh child process: two epochs (0 and 1) on the .npz of the scene leave a checkpoint and metrics.csv."""
    import yaml
    write_npz(tmp_path / "train.npz", TRAIN_VIEWS)
    write_npz(tmp_path / "val.npz", VAL_VIEWS)
    groups = dict(net={k: v for k, v in CFG.items() if k.startswith(("sem_", "inst_", "nef_", "hidden", "num_layers", "panoptic"))}, trainer={})
    groups["trainer"] = {k: v for k, v in CFG.items() if k not in groups["net"]}
    with open(tmp_path / "scene.yaml", "w") as f:
        yaml.safe_dump(groups, f)
    log_dir = tmp_path / "run"
    cmd = [sys.executable, "-m", "pagnerf_amd.train", "--config", str(tmp_path / "scene.yaml"), "--dataset", str(tmp_path / "train.npz"),
           "--val-dataset", str(tmp_path / "val.npz"), "--log-dir", str(log_dir), "--set", "epochs=1", "--set", "val_extrinsics_every=0"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    done = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    print(done.stdout[-3000:])
    assert done.returncode == 0
    assert os.path.getsize(log_dir / "model.pth") > 0
    rows = read_csv(log_dir / "metrics.csv")
    assert len(rows) == 2 and "val/psnr" in rows[0] and float(rows[1][rows[0].index("epoch")]) == 1
    state = torch.load(log_dir / "model.pth", map_location="cpu", weights_only=False)
    assert state["epoch"] == 2 and "nef.grid.tables" in state["pipeline"] and "camera_extrinsics" in state["pipeline"]
