"""What tests/test_formats_host.py and tests/test_gpu_formats.py share: seeded poses and kernel inputs, and NeRF-standard folders written with
pagnerf_amd.visualize.write_png (8-bit RGB and grey: what both decoders read)."""
import json
import math
import os

import numpy as np
import torch

# (B, H0, W0, mip): odd output sizes, fewer output pixels than a wave, more than a workgroup with a ragged tail
SHAPES = ((3, 10, 14, 0), (3, 10, 14, 1), (2, 36, 52, 2), (1, 66, 130, 0))
# further shapes: widths that are multiples of 4 (every block row 16-byte aligned: the widest loads at mip 2 and 3, two of them per row at mip 3), less
# than a workgroup at each mip, and five workgroups with a ragged tail
WIDE_SHAPES = ((2, 12, 40, 0), (2, 12, 40, 1), (2, 24, 48, 2), (1, 34, 132, 0), (1, 16, 64, 3))
INTRINSICS = dict(fx=23.7, fy=19.3, x0=0.3, y0=-0.45)
RAY_TOL = 2e-6          # 32 ulp of 1.0: about ten fp32 roundings on components of magnitude <= 1


def rotations(n, seed):
    """n proper rotations, none axis-aligned: float64 [n,3,3]."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out)


def camera_to_world(n, seed):
    """float32 [n,3,4]: rotations(n, seed) with translations in [-1, 1]."""
    rs = np.random.RandomState(seed + 1000)
    return torch.from_numpy(np.concatenate([rotations(n, seed), rs.uniform(-1, 1, (n, 3, 1))], axis=2)).float()


def source(B, H0, W0, C0, seed):
    """Random uint8 [B,H0,W0,C0]; with an alpha channel its first pixels are 0, 127, 128 and 255 (at mip 0 the two sides of the mask threshold)."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (B, H0, W0, C0), dtype=torch.uint8, generator=g)
    if C0 == 4:
        src[:, 0, :4, 3] = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)
        src[:, 4:8, 4:8, 3] = 255        # whole blocks of alpha 255 and 0 at every mip of SHAPES (the shortest side is 10, at mip <= 1)
        src[:, 8:16, 8:16, 3] = 0
    return src


def write_folder(root, layout="three", n=5, H0=12, W0=20, labels=True, seed=0, missing=(), partial=False, extra=None):
    """A NeRF-standard folder under `root`: layout 'three' = transforms_{train,val,test}.json with frames `<split>/r_<i>` (no extension; one path with a
    backslash), 'one' = transforms.json with `images/<i>.png`.  labels: the package's label extension on every frame (partial: on the first only).
    missing: train frames that are listed but have no file.  -> {split: dict(images uint8 [V,H0,W0,3], semantics / instance uint8 [V,H0,W0], meta)}."""
    from pagnerf_amd.visualize import write_png
    rs = np.random.RandomState(seed)
    out = {}
    for s, split in enumerate(("train", "val", "test") if layout == "three" else ("train",)):
        sub = split if layout == "three" else "images"
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        count = n if split == "train" else 2
        R = rotations(count, seed + 10 * s)
        frames, kept = [], dict(images=[], semantics=[], instance=[])
        for i in range(count):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R[i], rs.uniform(-1, 1, 3)
            img = rs.randint(0, 256, (H0, W0, 3)).astype(np.uint8)
            sem, inst = rs.randint(0, 5, (H0, W0)).astype(np.uint8), rs.randint(0, 16, (H0, W0)).astype(np.uint8)
            name = "%s/r_%d" % (sub, i) if layout == "three" else "%s/%04d.png" % (sub, i)
            frame = dict(file_path=name.replace("/", "\\") if i == 1 else name, transform_matrix=T.tolist())
            if labels and (not partial or i == 0):
                frame.update(semantic_path="%s/sem_%d.png" % (sub, i), instance_path="%s/inst_%d" % (sub, i))
                write_png(os.path.join(root, sub, "sem_%d.png" % i), sem)
                write_png(os.path.join(root, sub, "inst_%d.png" % i), inst)
            frames.append(frame)
            if split == "train" and i in missing:
                continue
            write_png(os.path.join(root, name if name.endswith(".png") else name + ".png"), img)
            kept["images"].append(img)
            kept["semantics"].append(sem)
            kept["instance"].append(inst)
        meta = dict(camera_angle_x=0.9, cx=W0 / 2 + 0.6, cy=H0 / 2 - 0.3, aabb_scale=2.0, scale=0.5, offset=[0.1, -0.2, 0.05], frames=frames)
        if labels:
            meta.update(num_classes=5, num_instances=16, things_ids=[2, 3, 4], stuff_ids=[0, 1])
        meta.update(extra or {})
        with open(os.path.join(root, "transforms_%s.json" % split if layout == "three" else "transforms.json"), "w") as f:
            json.dump(meta, f)
        out[split] = dict({k: np.stack(v) for k, v in kept.items()}, meta=meta)
    return out


def leaves(ds):
    """{(mode, field): tensor} of a DeviceMultiviewDataset."""
    return {(l.key, l.field): l.src for l in ds._leaves}


# ------------------------------------------------------------------------------------------------------ the analytic scene of the trainer runs
# A textured sphere (radius 0.35, three 'thing' instances by longitude) over a plane (z = -0.4, 'stuff'), white background, seen by downward cameras:
# the scene of tests/test_gpu_trainer.py, restated here so that the two files do not depend on each other's constants.
SCENE_H = SCENE_W = 32
SCENE_TAN = 0.55                # half the field of view: the image spans +-0.55 at depth 1
SCENE_THINGS, SCENE_STUFF = [2, 3, 4], [0, 1]
TRAINER_CFG = dict(nef_type="PanopticDeltaNeF", tracer_type="PanopticPackedRFTracer", grid_type="PermutoGrid", num_lods=8, feature_dim=2, capacity_log_2=12,
                   delta_capacity_log_2=12, coarsest_scale=1.0, finest_scale=0.01, blas_level=5, hidden_dim=64, num_layers=1, sem_num_layers=1,
                   inst_num_layers=2, sem_softmax=True, inst_softmax=True, panoptic_features_type="delta", view_multires=4, raymarch_type="ray", num_steps=32,
                   samples_per_voxel=2, bg_color="white", ray_max_travel=2.0, batch_size=2, num_rays_sampled_per_img=128, render_batch=512, lr=0.001,
                   grid_lr_weight=100.0, delta_grid_lr_weight=100.0, rgb_weight=10.0, sem_weight=0.1, inst_weight=1.0, inst_loss="linear_assignment_things",
                   inst_outlier_rejection=True, inst_num_dilations=1, optimize_extrinsics=True, optimize_val_extrinsics=True, extrinsics_lr=1e-3,
                   anchor_frame_idxs=[0], epochs=5, save_every=-1, valid_every=-1, sem_epoch_start=0, inst_epoch_start=0)


def scene_cameras(n, phase):
    """Camera-to-world matrices float64 [n,4,4] (z up, the camera looks down its -z): n cameras at height 0.95 looking down, on a circle of radius 0.25,
    each turned a little about the vertical."""
    out = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    for i in range(n):
        a = phase + 2 * math.pi * i / n
        yaw = 0.1 * math.sin(3 * a)
        out[i, :3, :3] = torch.tensor([[math.cos(yaw), math.sin(yaw), 0.0], [-math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
        out[i, :3, 3] = torch.tensor([0.25 * math.cos(a), 0.25 * math.sin(a), 0.95], dtype=torch.float64)
    return out


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
    rgb_s = 0.5 + 0.5 * torch.sin(ps * 9.0 + torch.tensor([0.0, 2.0, 4.0], dtype=o.dtype))
    rgb_p = torch.stack([0.25 + 0.2 * torch.sin(pp[:, 0] * 5), 0.45 + 0.2 * torch.cos(pp[:, 1] * 5), torch.full_like(tp, 0.2)], -1)
    rgb = torch.where(hit_s[:, None], rgb_s, torch.where(hit_p[:, None], rgb_p, torch.ones_like(rgb_p)))
    sector = ((torch.atan2(ps[:, 1], ps[:, 0]) + math.pi) / (2 * math.pi) * 3).long().clamp(0, 2)
    sem = torch.where(hit_s, 2 + sector % 2, torch.where(hit_p, torch.ones_like(sector), torch.zeros_like(sector)))
    inst = torch.where(hit_s, 1 + sector, torch.zeros_like(sector))
    return rgb, sem, inst


def write_trainer_scene(root):
    """The scene as a NeRF-standard folder with labels: 4 train and 2 val / test views of 32 x 32.  The pictures are rendered here with plain pinhole
    algebra in the scene's own z-up frame - pixel centre (i + 0.5, j + 0.5), camera looking down -z with y up - and nothing of the package's ray code:
    the frames carry the Blender-style camera-to-world matrices, and whatever world basis the loader turns them into, a pixel keeps its colour."""
    from pagnerf_amd.visualize import write_png
    H, W = SCENE_H, SCENE_W
    focal = 0.5 * W / SCENE_TAN
    jj, ii = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    d_cam = torch.stack([(ii + 0.5 - W / 2) / focal, -(jj + 0.5 - H / 2) / focal, -torch.ones_like(ii)], -1).reshape(-1, 3)
    for split, cams in (("train", scene_cameras(4, 0.0)), ("val", scene_cameras(2, 0.6)), ("test", scene_cameras(2, 0.6))):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i, T in enumerate(cams):
            d = torch.nn.functional.normalize(d_cam @ T[:3, :3].T, dim=-1)
            rgb, sem, inst = scene_truth(T[:3, 3].expand_as(d), d)
            write_png(os.path.join(root, split, "r_%d.png" % i), (rgb.reshape(H, W, 3) * 255).round().to(torch.uint8))
            write_png(os.path.join(root, split, "sem_%d.png" % i), sem.reshape(H, W).to(torch.uint8))
            write_png(os.path.join(root, split, "inst_%d.png" % i), inst.reshape(H, W).to(torch.uint8))
            frames.append(dict(file_path="%s/r_%d" % (split, i), transform_matrix=T.tolist(), semantic_path="%s/sem_%d.png" % (split, i),
                               instance_path="%s/inst_%d.png" % (split, i)))
        meta = dict(camera_angle_x=2 * math.atan(SCENE_TAN), aabb_scale=1.0, num_classes=5, num_instances=16, things_ids=SCENE_THINGS, stuff_ids=SCENE_STUFF,
                    frames=frames)
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as f:
            json.dump(meta, f)
