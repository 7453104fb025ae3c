"""python -m pagnerf_amd.train --config YAML --dataset TRAIN.npz|DIR [--val-dataset VAL.npz|DIR] [--log-dir DIR] [--resume CKPT] [--valid-only]
                              [--val-pictures] [--save-map PATH [--map-voxel-size V [--map-min-votes N] [--map-min-component N] [--map-split MODE]]]
                              [--save-mesh PATH.ply [--mesh-resolution R] [--mesh-min-density D]] [--set key=value ...]
                              [--carve-from-depth [--carve-margin M] [--carve-dilate N] [--carve-mode hull|band] [--carve-stride S] [--carve-max-range METRES]]

The native counterpart of the reference's main_interactive.py: a shipped YAML, a dataset, and the trainer of trainer.py.

A dataset is a NeRF-standard folder (transforms*.json and image files; formats.load_nerf_standard with the YAML's `mip`, `bg_color` and
`dataset_num_workers`, split 'train' for --dataset and 'val' for --val-dataset; without --val-dataset the folder's own 'val' split when it has one), a
BUP20 folder (it holds BUP_20.json or CKA_sweet_pepper_2020_summer.json, or the YAML says `multiview_dataset_format: bup20` and the folder has no
transforms*.json; bup20.load_bup20 with the YAML's `load_modes`, `class_labels`, `dataset_center_idx`, `pose_src`, `max_depth`, `scale`, `offset` and
`model_rescaling`; the one folder serves both splits), or an .npz of arrays (python -m pagnerf_amd.formats or python -m pagnerf_amd.bup20 writes one
from a folder).  The .npz holds the arrays of the dict MultiviewDataset.init() leaves:

    imgs [V,H,W,3] float32 and every further per-view mode (semantics, instance, semantics_pred, instance_pred, sem_conf, inst_conf ...) [V,H,W,C]
    base_rays_origins, base_rays_dirs [H,W,3]   the camera-frame rays the views share (pose optimisation), base_rays_range [2] = (near, far)
    rays_origins, rays_dirs [V,H,W,3]           world-frame rays per view, rays_range [2]                      (either pair, or both)
    view_matrices [V,4,4]                        world -> camera, needed with optimize_extrinsics
    num_classes, num_instances (scalars), things_ids, stuff_ids (int arrays)    the `semantic_info` lists
    optional: scale (scalar), filenames [V]

The NeRF-standard loader, with this package's label extension, is formats.py; BUP20's own loader (bup20.py, agrobot_base.py) is bup20.py.
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

RESERVED = ("base_rays_origins", "base_rays_dirs", "base_rays_range", "rays_origins", "rays_dirs", "rays_range", "view_matrices", "num_classes",
            "num_instances", "things_ids", "stuff_ids", "scale", "filenames")


def load_npz_dataset(path, device):
    """The .npz of the module docstring -> DeviceMultiviewDataset with semantic_info / view_matrices / image_shape / filenames / scale attached."""
    from .core import Rays
    from .dataset import DeviceMultiviewDataset
    z = np.load(os.path.expanduser(path), allow_pickle=False)
    data = {k: torch.from_numpy(z[k]) for k in z.files if k not in RESERVED}
    if "imgs" not in data:
        raise ValueError("%s: no 'imgs' array" % path)
    H, W = data["imgs"].shape[1:3]
    for name in ("base_rays", "rays"):
        if name + "_origins" in z.files:
            lo, hi = (float(v) for v in z[name + "_range"]) if name + "_range" in z.files else (0.0, 6.0)
            data[name] = Rays(torch.from_numpy(z[name + "_origins"]).float(), torch.from_numpy(z[name + "_dirs"]).float(), dist_min=lo, dist_max=hi)
    ds = DeviceMultiviewDataset(data, device)
    ds.image_shape = (int(H), int(W))
    if "num_classes" in z.files:
        ds.semantic_info = dict(num_classes=int(z["num_classes"]), num_instances=int(z["num_instances"]),
                                things_ids=[int(v) for v in z["things_ids"]], stuff_ids=[int(v) for v in z["stuff_ids"]])
    if "view_matrices" in z.files:
        ds.view_matrices = torch.from_numpy(z["view_matrices"]).float()
    if "scale" in z.files:
        ds.scale = float(z["scale"])
    if "filenames" in z.files:
        ds.filenames = [str(v) for v in z["filenames"]]
    return ds


def is_bup20(path, cfg):
    """Whether the folder `path` goes to bup20.load_bup20: it holds BUP_20.json / CKA_sweet_pepper_2020_summer.json, or the YAML's
    multiview_dataset_format is one of the reference's four spellings of bup20 and the folder is not a NeRF-standard one (no transforms*.json)."""
    import glob
    from . import bup20
    if bup20.is_bup20_folder(path):
        return True
    return cfg.get("multiview_dataset_format") in bup20.FORMAT_NAMES and not glob.glob(os.path.join(path, "transforms*.json"))


def load_dataset(path, split, cfg, device):
    """--dataset / --val-dataset: a BUP20 folder (is_bup20) goes to bup20.load_bup20 with load_modes, class_labels, dataset_center_idx, pose_src,
    max_depth, scale, offset and model_rescaling from the YAML namespace (and `seq_num_frames`, this package's own key: the reference fixes the window at
    40; with `carve_from_depth` the training window keeps its `depths`, which the reference's mode filter drops), any other folder to formats.load_nerf_standard (split `split`; mip, bg_color
    and dataset_num_workers from the namespace for both), anything else to load_npz_dataset."""
    path = os.path.expanduser(path)
    if not os.path.isdir(path):
        return load_npz_dataset(path, device)
    from . import bup20, formats
    common = dict(mip=int(cfg.get("mip") or 0), bg_color=cfg.get("bg_color") or "white", device=device, num_workers=int(cfg.get("dataset_num_workers") or 0))
    if is_bup20(path, cfg):
        max_depth = cfg.get("max_depth")
        return bup20.load_bup20(path, split, load_modes=cfg.get("load_modes") or (), class_labels=cfg.get("class_labels") or (),
                                dataset_center_idx=int(cfg.get("dataset_center_idx") or 0), pose_src=cfg.get("pose_src") or "odom",
                                max_depth=-1 if max_depth is None else max_depth, scale=cfg.get("scale"), offset=cfg.get("offset"),
                                model_rescaling=cfg.get("model_rescaling") or "snap_to_bottom", seq_num_frames=int(cfg.get("seq_num_frames") or 40),
                                add_noise_to_train_poses=bool(cfg.get("add_noise_to_train_poses")), dataset_mode=cfg.get("dataset_mode") or "label_window",
                                keep_depths=bool(cfg.get("carve_from_depth")) and split == "train", **common)
    return formats.load_nerf_standard(path, split=split, **common)


def save_map(trainer, dataset, path, voxel_size=None, min_votes=1, min_component=None, split=None):
    """--save-map: the panoptic point cloud of the trained field from the training views (map_export.generate_pc_map_from_views).  With voxel_size
    (--map-voxel-size) the cloud is fused into the voxel map (map_export.fuse_map) before it is written, and the per-instance table goes beside it
    as PATH with its suffix replaced by .instances.csv.  With min_component / split (--map-min-component / --map-split) the fused map is cleaned
    first (map_export.clean_map: components of fewer than min_component voxels dropped, an id's further components kept, dropped or made new
    instances), carries a component label per voxel, and the table is the per-component one."""
    from . import map_export
    from .core import Rays
    leaf = {l.field: l.src for l in dataset._leaves if l.key == "base_rays"}
    if not leaf or not hasattr(trainer.pipeline, "camera_extrinsics"):
        raise ValueError("--save-map needs base_rays in the dataset and a BAPipeline (optimize_extrinsics)")
    near, far = dataset._rays_range["base_rays"]
    cloud = map_export.generate_pc_map_from_views(trainer.pipeline, Rays(leaf["origins"], leaf["dirs"], near, far),
                                                  cam_ids=list(range(dataset.num_imgs)), render_batch=trainer.render_batch or 20000)
    if voxel_size is not None:
        device = trainer.pipeline.camera_extrinsics.device
        fused = map_export.fuse_map(cloud, voxel_size, min_votes=min_votes, device=device, name=cloud[0]["name"])
        if min_component is not None or split is not None:
            fused = map_export.clean_map(fused, min_voxels=min_component or 1, mode=split or "keep", device=device)
            table = map_export.component_table(fused, device=device)
        else:
            table = map_export.instance_table(fused, device=device)
        map_export.save_instance_table(table, os.path.splitext(str(path))[0] + ".instances.csv")
        cloud = [fused]
    map_export.save_map(cloud, path)
    return path


def save_mesh(trainer, path, resolution=256, min_density=None):
    """--save-mesh: the panoptic triangle mesh of the trained field (mesh.extract_mesh: surface nets on the density lattice of `resolution` cells per
    axis at iso = min_density, the vertices labelled by instance and class and coloured) as a binary PLY, and its report line on stdout.  It needs the
    trained nef alone: no base rays, no BAPipeline."""
    from . import mesh
    nef = getattr(trainer.pipeline, "nef", trainer.pipeline)
    m = mesh.extract_mesh(nef, resolution=resolution, min_density=min_density)
    mesh.save_mesh(m, path)
    print(mesh.report_line(mesh.mesh_report(m)))
    return path


def make_parser():
    ap = argparse.ArgumentParser(prog="python -m pagnerf_amd.train", description=__doc__.split("\n\n")[1])
    ap.add_argument("--config", required=True, help="a YAML in the reference's layout (configs/bup20/*.yaml)")
    ap.add_argument("--dataset", required=True, help="training views: a NeRF-standard folder or an .npz")
    ap.add_argument("--val-dataset", help="validation views: a NeRF-standard folder or an .npz (needed with optimize_val_extrinsics and for validation; default: the "
                    "'val' split of a --dataset folder that has one)")
    ap.add_argument("--log-dir", help="overrides the YAML's log_dir")
    ap.add_argument("--resume", metavar="CKPT", help="continue the run of a PanopticTrainer checkpoint")
    ap.add_argument("--valid-only", action="store_true", help="validate the (resumed / pretrained) model and exit")
    ap.add_argument("--val-pictures", action="store_true", help="validation writes its frames as PNG files under <log_dir>/val/epoch_<e>/ (with "
                    "--valid-only --resume CKPT: render what was trained)")
    ap.add_argument("--save-map", metavar="PATH", help="after training export the panoptic point cloud of the training views")
    ap.add_argument("--map-voxel-size", type=float, metavar="V", help="--save-map writes the fused voxel map of edge V (one row per occupied voxel: mean "
                    "point and colour, voted instance id, count, agreement) and the instance table as PATH with the suffix .instances.csv")
    ap.add_argument("--map-min-votes", type=int, default=1, metavar="N", help="with --map-voxel-size: drop voxels that hold fewer than N points")
    ap.add_argument("--map-min-component", type=int, metavar="N", help="with --map-voxel-size: drop connected components of equal-id voxels that have fewer "
                    "than N voxels; the map gets a component label per voxel and the table one row per component")
    ap.add_argument("--map-split", choices=("keep", "largest", "split"), metavar="MODE", help="with --map-voxel-size: an id with several components keeps "
                    "them (keep), keeps only the largest (largest) or gives every further component a new id (split)")
    ap.add_argument("--save-mesh", metavar="PATH.ply", help="after training export the labelled, coloured triangle mesh of the field (surface nets on the "
                    "density lattice) as a binary PLY and print its report (counts, closed / oriented, Euler characteristic, area, volume)")
    ap.add_argument("--mesh-resolution", type=int, default=256, metavar="R", help="--save-mesh: lattice cells per axis (default 256)")
    ap.add_argument("--mesh-min-density", type=float, metavar="D", help="--save-mesh: the density of the surface (default: the dense map export's "
                    "0.01 * 512 / sqrt(3))")
    ap.add_argument("--carve-from-depth", action="store_true", help="before the first step carve both grids' occupancy from the training views' depth "
                    "images (the dataset needs its 'depths' mode and `scale`; the YAML key carve_from_depth does the same)")
    ap.add_argument("--carve-margin", type=float, metavar="M", help="--carve-from-depth: the band around a measured surface that stays occupied, in scene "
                    "units (default: two cells of the occupancy lattice); with pose optimisation it must cover the expected pose error")
    ap.add_argument("--carve-dilate", type=int, metavar="N", help="--carve-from-depth: rings of neighbour cells added to the surface cells, 0 .. 4 (default 1)")
    ap.add_argument("--carve-mode", choices=("hull", "band"), help="--carve-from-depth: hull keeps every cell no ray saw to be empty (default), band only "
                    "the neighbourhood of measured surfaces (depth holes lose geometry)")
    ap.add_argument("--carve-stride", type=int, metavar="S", help="--carve-from-depth: walk every S-th pixel per axis (default 1)")
    ap.add_argument("--carve-max-range", type=float, metavar="METRES", help="--carve-from-depth: depth readings beyond this many metres are not used")
    ap.add_argument("--set", action="append", default=[], metavar="key=value", help="override an option of the flattened namespace (repeatable)")
    ap.add_argument("--device", default="cuda")
    return ap


CARVE_KEYS = ("carve_margin", "carve_dilate", "carve_mode", "carve_stride", "carve_max_range")


def config_from_args(args):
    """The flattened namespace of a parsed command line: the YAML, then --set, then the flags that stand for a key (--log-dir, --valid-only,
    --val-pictures, --carve-from-depth and the --carve-* options that were given)."""
    from . import config
    cfg = config.load_config(args.config)
    config.apply_overrides(cfg, args.set)
    if args.log_dir:
        cfg["log_dir"] = args.log_dir
    if args.valid_only:
        cfg["valid_only"] = True
    if args.val_pictures:
        cfg["val_pictures"] = True
    if args.carve_from_depth:
        cfg["carve_from_depth"] = True
    for key in CARVE_KEYS:
        if getattr(args, key) is not None:
            cfg[key] = getattr(args, key)
    return cfg


def main(argv=None):
    args = make_parser().parse_args(argv)
    from . import config
    cfg = config_from_args(args)
    logging.basicConfig(level=int(cfg.get("log_level") or logging.INFO), format="%(asctime)s|%(levelname)8s| %(message)s")
    device = torch.device(args.device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())        # the dataset compares devices with their index
    dataset = load_dataset(args.dataset, "train", cfg, device)
    val_root = args.val_dataset
    if not val_root and os.path.isdir(os.path.expanduser(args.dataset)):
        if is_bup20(os.path.expanduser(args.dataset), cfg):
            val_root = args.dataset                                         # a BUP20 folder serves both splits
        else:
            from .formats import transforms_files
            val_root = args.dataset if "val" in transforms_files(args.dataset) else None
    val_dataset = load_dataset(val_root, "val", cfg, device) if val_root else None
    _, trainer = config.build_from_config(cfg, dataset, val_dataset, device=device)
    if args.resume:
        trainer.resume(args.resume)
    if args.valid_only:
        trainer.validate(trainer.epoch)
        return 0
    trainer.train()
    trainer.save_checkpoint(os.path.join(trainer.log_dir, "model.pth"))
    if val_dataset is not None and not (trainer.plan and trainer.plan["validate_after"]):      # the last epoch's own validation is not repeated
        trainer.validate(trainer.epoch - 1)
    if args.save_map:
        save_map(trainer, dataset, args.save_map, args.map_voxel_size, args.map_min_votes, args.map_min_component, args.map_split)
    if args.save_mesh:
        save_mesh(trainer, args.save_mesh, args.mesh_resolution, args.mesh_min_density)
    return 0


if __name__ == "__main__":
    sys.exit(main())
