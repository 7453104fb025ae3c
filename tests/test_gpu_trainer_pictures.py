"""PanopticTrainer(val_pictures=True) on the GPU: the files validate() writes under <log_dir>/val/epoch_<e>/, their content, and that the metrics do
not depend on the switch.

The scene is the analytic one of tests/test_gpu_trainer.py (a textured sphere of three 'thing' instances over a 'stuff' plane, downward cameras;
4 training and 3 validation views of 32 x 32 pixels), restated here; the model is that file's small PermutoGrid field."""
import csv
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 32
THINGS, STUFF = [2, 3, 4], [0, 1]
NEAR, FAR = 0.0, 1.9


def view_matrices(n, phase):
    views = torch.eye(4).repeat(n, 1, 1)
    for i in range(n):
        a = phase + 2 * math.pi * i / n
        yaw = 0.1 * math.sin(3 * a)
        R = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        centre = torch.tensor([0.25 * math.cos(a), 0.25 * math.sin(a), 0.95])
        views[i, :3, :3] = R
        views[i, :3, 3] = -R @ centre
    return views


def base_rays():
    ys, xs = torch.meshgrid((torch.arange(H) + 0.5) / H - 0.5, (torch.arange(W) + 0.5) / W - 0.5, indexing="ij")
    d = torch.stack([xs * 1.1, ys * 1.1, -torch.ones_like(xs)], -1).reshape(-1, 3)
    return torch.zeros_like(d), d


def scene_truth(o, d):
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
    sector = ((torch.atan2(ps[:, 1], ps[:, 0]) + math.pi) / (2 * math.pi) * 3).long().clamp(0, 2)
    sem = torch.where(hit_s, 2 + sector % 2, torch.where(hit_p, torch.ones_like(sector), torch.zeros_like(sector)))
    inst = torch.where(hit_s, 1 + sector, torch.zeros_like(sector))
    return rgb.float(), sem, inst


def make_dataset(views, dev, labelled=None, preds=False):
    """labelled: per view (semantics, instances) carry labels; an unlabelled view's label images are -1 throughout.  preds: add the `_pred` label
    images (the truth with one class / id moved) and an `inst_conf` image, as a dataset with network predictions carries them."""
    import pagnerf_amd
    oc, dc = base_rays()
    V = views.shape[0]
    R, t = views[:, :3, :3], views[:, :3, 3]
    o = torch.matmul(oc[None] - t[:, None, :], R)
    d = torch.nn.functional.normalize(torch.matmul(dc[None].expand(V, -1, -1), R), dim=-1)
    rgb, sem, inst = scene_truth(o.reshape(-1, 3), d.reshape(-1, 3))
    sem, inst = sem.reshape(V, H, W, 1).clone(), inst.reshape(V, H, W, 1).clone()
    labelled = labelled or [(True, True)] * V
    for v, (s, i) in enumerate(labelled):
        if not s:
            sem[v] = -1
        if not i:
            inst[v] = -1
    data = dict(imgs=rgb.reshape(V, H, W, 3), semantics=sem, instance=inst, base_rays=pagnerf_amd.Rays(oc, dc, dist_min=NEAR, dist_max=FAR))
    if preds:
        data["semantics_pred"] = torch.where(sem == 3, torch.full_like(sem, 2), sem).clamp_min(0)
        data["instance_pred"] = torch.where(inst == 2, torch.full_like(inst, 5), inst).clamp_min(0)
        data["inst_conf"] = (0.5 + 0.5 * torch.sin(torch.arange(V * H * W, dtype=torch.float32) * 0.01)).reshape(V, H, W, 1)
    ds = pagnerf_amd.DeviceMultiviewDataset(data, dev)
    ds.view_matrices = views
    ds.image_shape = (H, W)
    ds.semantic_info = dict(num_classes=5, num_instances=16, things_ids=THINGS, stuff_ids=STUFF)
    ds.labelled = labelled
    ds.filenames = ["view_%02d.png" % i for i in range(V)]
    return ds


TRAIN_VIEWS, VAL_VIEWS = view_matrices(4, 0.0), view_matrices(3, 0.6)
VAL_LABELLED = [(True, True), (True, True), (False, False)]

CFG = dict(nef_type="PanopticDeltaNeF", tracer_type="PanopticPackedRFTracer", grid_type="PermutoGrid", num_lods=8, feature_dim=2, capacity_log_2=12,
           delta_capacity_log_2=12, coarsest_scale=1.0, finest_scale=0.01, blas_level=5, hidden_dim=64, num_layers=1, sem_num_layers=1,
           inst_num_layers=2, sem_softmax=True, inst_softmax=True, panoptic_features_type="delta", view_multires=4, raymarch_type="ray", num_steps=32,
           samples_per_voxel=2, bg_color="white", ray_max_travel=2.0, batch_size=2, num_rays_sampled_per_img=128, render_batch=512, lr=0.001,
           grid_lr_weight=100.0, delta_grid_lr_weight=100.0, rgb_weight=10.0, sem_weight=0.1, inst_weight=1.0, inst_loss="linear_assignment_things",
           inst_outlier_rejection=True, inst_num_dilations=1, optimize_extrinsics=True, optimize_val_extrinsics=True, extrinsics_lr=1e-3,
           anchor_frame_idxs=[0], epochs=5, save_every=-1, valid_every=-1, sem_epoch_start=0, inst_epoch_start=1, use_graphs=False)


def make_trainer(dev, log_dir, seed=11, **over):
    from pagnerf_amd import config
    torch.manual_seed(seed)
    cfg = dict(CFG, log_dir=str(log_dir))
    cfg.update(over)
    pipe, tr = config.build_from_config(cfg, make_dataset(TRAIN_VIEWS, dev), make_dataset(VAL_VIEWS, dev, VAL_LABELLED, preds=True), device=dev)
    with torch.no_grad():
        pipe.nef.decoder_density.lout.bias[0] = 2.96
        for g in (pipe.nef.grid, pipe.nef.delta_grid):
            g.tables.normal_(0.0, 1e-2)
    return pipe, tr


def read_csv(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def run(dev, on_dir, off_dir):
    """Two epochs (0 and 1; the instance channel starts at epoch 1).  After each the SAME field is validated twice from the same generator state (the
    ray march of a validation image draws its jitter from torch's generator): with val_pictures into on_dir, without into off_dir - so the
    comparison of the two does not depend on what two training runs from one seed differ by."""
    pipe, tr = make_trainer(dev, on_dir, val_pictures=True, num_val_frames_to_save=2, render_val_labels=True)
    on, off = [], []
    for e in range(2):
        tr.run_epoch()
        torch.manual_seed(1000 + e)
        on.append(tr.validate(e))
        tr.val_pictures, tr.log_dir = False, str(off_dir)
        torch.manual_seed(1000 + e)
        off.append(tr.validate(e))
        tr.val_pictures, tr.log_dir = True, str(on_dir)
    return pipe, tr, on, off


@pytest.fixture(scope="module")
def runs(gpu_device, tmp_path_factory):
    on, off = tmp_path_factory.mktemp("pictures_on"), tmp_path_factory.mktemp("pictures_off")
    pipe, tr, m_on, m_off = run(gpu_device, on, off)
    return dict(on_dir=str(on), off_dir=str(off), pipe=pipe, tr=tr, on=m_on, off=m_off)


SEM = ["_sem", "_sem_rgb", "_sem_pred", "_sem_pred_rgb"]
INST = ["_inst", "_inst_conf", "_inst_rgb", "_inst_pred", "_inst_pred_rgb", "_inst_conf_pred"]


def expected_files(epoch):
    """Frames 0 and 2 by idx % 2 == 0, frame 1 because it carries labels and render_val_labels is on; frame 2 is unlabelled: no `_gt` label pictures."""
    names = []
    for idx in range(3):
        parts = ["", "_gt", "_depth"] + SEM + (["_sem_gt"] if VAL_LABELLED[idx][0] else [])
        if epoch >= 1:
            parts += INST + (["_inst_gt"] if all(VAL_LABELLED[idx]) else [])
        names += ["%d%s.png" % (idx, p) for p in parts]
    return sorted(names)


def test_expected_files_per_epoch(runs):
    log_dir = runs["on_dir"]
    assert sorted(os.listdir(os.path.join(log_dir, "val"))) == ["epoch_0", "epoch_1"]
    for e in range(2):
        got = sorted(os.listdir(os.path.join(log_dir, "val", "epoch_%d" % e)))
        assert got == expected_files(e), (e, sorted(set(got) ^ set(expected_files(e))))
    assert not any("_inst" in f for f in os.listdir(os.path.join(log_dir, "val", "epoch_0")))
    assert len(expected_files(0)) == 3 * 7 + 2 and len(expected_files(1)) == 3 * 13 + 4


def test_unlabelled_frame_is_left_out_without_render_val_labels_clause(gpu_device, tmp_path):
    """num_val_frames_to_save=0 leaves only the third clause: the labelled frames 0 and 1 are written, the unlabelled frame 2 is not."""
    pipe, tr = make_trainer(gpu_device, tmp_path, val_pictures=True, num_val_frames_to_save=0, render_val_labels=True)
    tr.validate(0)
    files = os.listdir(os.path.join(str(tmp_path), "val", "epoch_0"))
    assert {f.split("_")[0].split(".")[0] for f in files} == {"0", "1"}


def test_png_files_equal_the_rendered_pictures(gpu_device, runs):
    """Every file of the last validation read back equals ValidationPictures.render on that frame's inputs, rebuilt here from the trained pipeline."""
    import numpy as np
    from pagnerf_amd import batch_render
    from pagnerf_amd.metrics import ValidationMetrics
    from pagnerf_amd.visualize import ValidationPictures, read_png
    log_dir, pipe, tr = runs["on_dir"], runs["pipe"], runs["tr"]
    ds = tr.val_dataset
    ev = ValidationMetrics(5, THINGS, STUFF, inst_num_dilations=1, inst_outlier_rejection=True).to(gpu_device)
    vp = ValidationPictures()
    every = torch.arange(ds.num_pixels, device=gpu_device)[None]
    checked = 0
    torch.manual_seed(1001)                  # the generator state validate(1) started from: the same march jitter
    with torch.no_grad():
        for idx in range(3):
            data = ds.gather([idx], every)
            cam = torch.full((ds.num_pixels,), tr.val_cam_offset + idx, dtype=torch.int32, device=gpu_device)
            rays = pipe.transform_rays_indexed(data["base_rays"].origins.reshape(-1, 3), data["base_rays"].dirs.reshape(-1, 3), cam)
            rb = batch_render(pipe, rays, channels=["rgb", "semantics", "inst_embedding", "depth"], render_batch=512).reshape(H, W, -1)
            img = lambda k: data[k].reshape(H, W)
            out = ev.update(rb, data["imgs"].reshape(H, W, -1), img("semantics"), img("instance"), img("semantics_pred"), img("instance_pred"),
                            labelled=VAL_LABELLED[idx])
            pics = vp.render(rb, data["imgs"].reshape(H, W, -1), semantics=out["semantics"], instances=out["instances"], inst_conf=out["inst_conf"],
                             sem_gt=img("semantics") if VAL_LABELLED[idx][0] else None, inst_gt=img("instance") if all(VAL_LABELLED[idx]) else None,
                             sem_pred=img("semantics_pred"), inst_pred=img("instance_pred"), inst_conf_pred=img("inst_conf"))
            for name, pic in pics.items():
                path = os.path.join(log_dir, "val", "epoch_1", "%d.png" % idx if name == "rgb" else "%d_%s.png" % (idx, name))
                back = read_png(path)
                assert back.shape == (H, W, 3) and np.array_equal(back, pic.cpu().numpy()), (idx, name)
                checked += 1
    assert checked == len(expected_files(1))


def test_metrics_do_not_depend_on_the_switch(runs):
    assert len(runs["on"]) == len(runs["off"]) == 2 and math.isfinite(runs["on"][1]["val/psnr"])
    for on, off in zip(runs["on"], runs["off"]):
        assert list(on) == list(off)
        for k in on:            # the same number, or nan in both (a quality without a matched segment)
            assert on[k] == off[k] or (math.isnan(on[k]) and math.isnan(off[k])), (k, on[k], off[k])
    rows = read_csv(os.path.join(runs["on_dir"], "metrics.csv"))
    assert rows == read_csv(os.path.join(runs["off_dir"], "metrics.csv")) and len(rows) == 3
    assert not os.path.exists(os.path.join(runs["off_dir"], "val"))


def test_no_val_directory_by_default(gpu_device, tmp_path):
    """A trainer built without the option behaves as before: metrics.csv, no val/ directory - also with the frame options set."""
    pipe, tr = make_trainer(gpu_device, tmp_path, num_val_frames_to_save=1, render_val_labels=True)
    assert tr.val_pictures is False
    tr.validate(0)
    assert sorted(os.listdir(str(tmp_path))) == ["metrics.csv"]
