"""python -m pagnerf_amd.bup20 ROOT [--split S] [--mip M] [--load-modes M ...] [--pose-src P] [--max-depth D] [--dataset-center-idx I] --out FILE.npz

The BUP20 sweet-pepper dataset from disk (datasets/formats/bup20.py:89-315 on top of datasets/formats/agrobot_base.py:22-556, `SequenceDataset` in mode
`label_window`): a folder with a COCO annotation file, an image-set YAML, sequence folders of timestamp-named frames with `depth/` 16-bit PNGs, odometry,
`params.yaml` and the detector's pickled predictions in, a DeviceMultiviewDataset out.  The reference needs pycocotools, torchvision, plyfile and cv2 and
prepares frame by frame on the host; here the COCO file is `json`, images are PIL, quaternions scipy, the PLY header is read by hand, and the per-frame
work runs on the device (csrc/bup20.hip): the polygon labels as two launches per chunk, the depth filter of the detector's instance masks, the label and
image shrink as two more, the rays by the existing pag_prepare_views.

THE DEFINITION is the tensor-op / NumPy form in this module (`polygon_keys_reference`, `polygon_mask_reference`, `coco_labels_reference`,
`pred_stats_reference`, `prepare_frames_reference`); it serves CPU tensors (and any device with use_kernel=False), and the kernels are held to it bit for
bit; ray directions to 2e-6 as in formats.py.

    coverage    pycocotools' rleFrPoly restated with integers (PARITY UNPINNED: pycocotools is not on the machine this was written on; the test against
                a float64 even-odd rule at the pixel centres is its guard).  A polygon part with vertices (px_j, py_j) in an h x w image:
                1. X_j = trunc(5 px_j + 0.5), Y_j likewise, in float64; the ring is closed.
                2. per edge dx = |dX|, dy = |dY|, x-major when dx >= dy.  An edge that runs backwards along its major axis has its ends swapped and is
                   walked in reverse (t = len - d), otherwise t = d, d = 0 .. len.  Point (xs + t, trunc(ys + s t + 0.5)), s = double(ye - ys) / dx (y-major
                   symmetric): one fp64 line per point, in this order, not contracted.  An edge of length 0 (a repeated vertex: 0 / 0 there) is its one point.
                3. per consecutive pair of the points of all edges with u_j != u_(j-1): xd = u_j if u_j < u_(j-1) else u_j - 1; kept when xd = 2 (mod 5)
                   and 0 <= X = (xd - 2) / 5 <= w - 1; Y = clamp(floor((min(v_j, v_(j-1)) + 2) / 5), 0, h); key = X h + Y.
                4. pixel (x, y) is covered iff the number of keys <= x h + y is odd (column-major; a key at Y = h carries into the next column).
                An annotation is the OR of its parts; an RLE segmentation's cumulative run lengths ARE its keys (uncompressed list or compressed string).
    labels      agrobot_base.py:524-547 over the image's annotations of the chosen categories in file order: semantics = min(max_label, sum label_a
                cover_a), the sum starting again from zero at an annotation that covers every pixel; instance = 1 + index of the last covering annotation,
                else 0.  An empty segmentation keeps its index and covers nothing.  Frames other than the window's centre are -1 everywhere.
    depth filter :442-461, only with max_depth > 0: per view and instance id, total = its pixels, valid = those with d = float(raw u16) * 0.001f, 0 < d <=
                max_depth; the id is kept when 2 valid > total (the reference's float32 valid / total > 0.5 for any image under 2^24 pixels; larger ones
                are refused).  inst' = inst where kept else 0; flipped = (inst != 0) != (inst' != 0); conf = 1 where flipped; sem' = 0 where inst' = 0.
                PARITY UNPINNED: torchvision's ToTensor treats 16-bit images differently between versions, so `raw * 0.001` is this module's reading.  A
                depth image of another size than the prediction is an error (the reference would resize it bilinearly).
    shrink      f = 2^mip divides both sides.  Labels: out[y, x] = src[y f, x f] (nearest).  imgs, depths, sem_conf, inst_conf: torch's
                interpolate(mode='bilinear') at an integer factor = the four source pixels at offsets f/2 - 1 and f/2 in each axis, a top-left, b
                top-right, c bottom-left, d bottom-right: ((0.25 a + 0.25 b) + 0.25 c) + 0.25 d in fp32, that order; f = 1 is the value itself.  An image
                value is float(u8) / 255f, one division; depths are metres, float(raw) * 0.001f (the reference stacks ToTensor's output: PARITY UNPINNED).
                RGB frames have no alpha: masks all true; a frame with alpha takes formats.py's composite rule on the shrunk channels.
    cameras     float64 throughout, rounded to float32 once (the reference works in float32 throughout): frame = E^-1 (odom_i^-1 odom_centre) E
                (:388-393), the OpenCV -> GL flip of datasets/utils.py:35-42, translation * scale + offset, then `bup20_cameras` (PARITY UNPINNED:
                kaolin's Camera.extrinsics.update, change_coordinate_system(diag(-1,-1,1)) and inv_transform_rays restated from memory).  near 0, far 2.

DEVIATIONS, all named where they occur: the reference copies CKA_sweet_pepper_2020_summer.* to BUP_20.* inside the dataset folder, this loader reads
whichever exists and writes nothing there; the reference resolves images against `<root>/../BUP_20`, this loader against `root` itself;
`add_noise_to_train_poses` and dataset_mode 'all_frames_window' raise NotImplementedError; Mask R-CNN masks are squeezed on their channel axis only.

A PREDICTION FILE IS A PICKLE: unpickling runs code chosen by whoever wrote the file.  Load predictions only from a dataset you trust.
"""
import argparse
import bz2
import concurrent.futures
import csv
import glob
import json
import logging
import os
import pathlib
import pickle
import sys
from collections import OrderedDict

import numpy as np
import torch

from .core import Rays
from .formats import _factor, _nothing, dataset_arrays

log = logging.getLogger(__name__)

DATASET_NAMES = ("BUP_20", "CKA_sweet_pepper_2020_summer")
FORMAT_NAMES = ("bup20", "bup_20", "BUP20", "BUP_20")           # datasets/multiview_dataset.py:95
DEFAULT_CLASS_LABELS = ("bg", "pepper")
DEFAULT_MODES = ("imgs", "depths", "semantic", "instance", "instance_preds", "semantic_preds")       # bup20.py:35-43
DEFAULT_FAR = 2.0               # bup20.py:249
NUM_INSTANCES = 200             # bup20.py:71
ODOMETRY_FILES = dict(rgbd="rgbd_odom.csv", odom="odometry.csv", metashape="metashape_cameras.npz")
METASHAPE_SCALE = 0.03          # agrobot_base.py:304
COCO_SCALE = 5                  # rleFrPoly's sub-pixel scale
COCO_MAX_PART_KEYS = 4096       # PAG_COCO_MAX_PART_KEYS: what pag_coco_keys sorts in LDS per polygon part (16 KB of keys)
COCO_MAX_COORD = 1 << 24        # |rounded vertex| below this: every product of the edge walk stays far inside int32 / exact in fp64
MAX_CHUNK_VIEWS = 65535


# ---------------------------------------------------------------------------------------------------------------------------------------- files
def dataset_files(root):
    """-> (json path, yaml path): BUP_20.* when present, else CKA_sweet_pepper_2020_summer.* read in place.  DEVIATION: bup20.py:163-172 copies the latter
    to the former inside the dataset folder; nothing is written here."""
    root = os.path.expanduser(str(root))
    out = []
    for ext in (".json", ".yaml"):
        for name in DATASET_NAMES:
            path = os.path.join(root, name + ext)
            if os.path.isfile(path):
                out.append(path)
                break
        else:
            raise FileNotFoundError("BUP20 dataset files not found in path: %s" % root)
    return tuple(out)


def is_bup20_folder(root):
    """A folder that holds one of the two COCO JSON names."""
    return any(os.path.isfile(os.path.join(os.path.expanduser(str(root)), name + ".json")) for name in DATASET_NAMES)


def dataset_rel_path(path):
    """agrobot_base.py:549-553: an image's `path` without its first three parts; fewer than four parts is an error."""
    parts = pathlib.PurePath(path).parts
    if len(parts) < 4:
        raise ValueError("Invalid dataset path, it only has 2 or less subpaths")
    return str(pathlib.PurePath(*parts[3:]))


def read_coco(path):
    """The COCO file with `json` -> dict(images {id: dict(id, path, height, width)}, anns {image id: [annotation, ...] in file order}, cats {id: category}
    in file order)."""
    with open(path) as f:
        doc = json.load(f)
    images = OrderedDict((im["id"], im) for im in doc.get("images", []))
    anns = {}
    for ann in doc.get("annotations", []):
        anns.setdefault(ann["image_id"], []).append(ann)
    cats = OrderedDict((c["id"], c) for c in doc.get("categories", []))
    return dict(images=images, anns=anns, cats=cats)


def class_map(cats, class_labels):
    """agrobot_base.py:67-76: category id -> index in class_labels, by supercategory first, then by name; the other categories are left out."""
    labels = list(class_labels)
    out = OrderedDict()
    for cid, c in cats.items():
        if c.get("supercategory") in labels:
            out[cid] = labels.index(c["supercategory"])
        elif c.get("name") in labels:
            out[cid] = labels.index(c["name"])
    return out


def semantic_info(class_labels=DEFAULT_CLASS_LABELS):
    """bup20.py:50-73."""
    labels = list(class_labels) or list(DEFAULT_CLASS_LABELS)
    present = list(range(len(labels)))
    return dict(class_id_to_name=dict(enumerate(labels)), num_classes=len(labels), classes_present=present, num_present_classes=len(present),
                stuff_ids=[present[0]], things_ids=present[1:], num_instances=NUM_INSTANCES)


def filter_load_modes(load_modes, split, keep_depths=False):
    """bup20.py:137-151 -> (preds_name, modes): the first mode with 'preds' in it names the prediction folder; split 'train' with predictions keeps only
    semantics / instance / instance_shuffled / sem_conf / inst_conf (so no depths, and the ground truth is whatever the window leaves), val and test drop
    the prediction modes.  The reference indexes [0] of an empty list without a prediction mode; here that is a ValueError.
    keep_depths (an addition of this package, off by default): split 'train' carries 'depths' as well, whether load_modes names it or not - what the
    depth carve (carve.carve_occupancy, the trainer's carve_from_depth) reads."""
    modes = list(load_modes) or list(DEFAULT_MODES)
    preds = [m for m in modes if "preds" in m]
    if not preds:
        raise ValueError("load_bup20: load_modes %r names no prediction folder (a mode with 'preds' in it, such as preds_mask2former)" % (modes,))
    if split == "train":
        modes = [m for m in modes if m in ("semantics", "instance", "instance_shuffled", "sem_conf", "inst_conf")]
        if keep_depths:
            modes.append("depths")
    elif split in ("val", "test"):
        modes = [m for m in modes if "preds" not in m]
    return preds[0], modes


# --------------------------------------------------------------------------------------------------------------------------------------- window
def window_deltas(n, split):
    """agrobot_base.py:110-115: wb = n if n is even else n - 1; train range(-wb-1, wb+2, 2), val range(-wb, wb+1, 2)."""
    wb = n if n % 2 == 0 else n - 1
    if split == "train":
        return list(range(-wb - 1, wb + 2, 2))
    if split in ("val", "valid"):
        return list(range(-wb, wb + 1, 2))
    raise ValueError("load_bup20: split %r is neither 'train' nor 'val'" % (split,))


def keep_eval_frames(eval_paths, sequence_of, n):
    """:86-103 with remove_edge_frames: the eval frames whose position in their sorted sequence folder is >= n + 1 from both ends, in the given order.
    sequence_of(path) -> the sorted paths of that folder with the frame's suffix."""
    kept = []
    for p in eval_paths:
        seq = sequence_of(p)
        pos = seq.index(p)
        if pos < n + 1 or len(seq) - pos < n + 1:
            continue
        kept.append(p)
    return kept


def window_paths(center, sequence, split, n, train_paths=(), eval_paths=()):
    """:326-337: the frames of the window about `center` in its sorted `sequence`: deltas walked in descending order, index seq_idx - d clamped into the
    sequence (repeats survive), frames of the detector's train set removed, and for split 'train' the kept eval frames as well."""
    idx = sequence.index(center)
    deltas = sorted(window_deltas(n, split), reverse=True)
    paths = [sequence[min(len(sequence) - 1, max(0, idx - d))] for d in deltas]
    train_paths = set(train_paths)
    paths = [p for p in paths if p not in train_paths]
    if split == "train":
        eval_paths = set(eval_paths)
        paths = [p for p in paths if p not in eval_paths]
    return paths


def list_sequence(path):
    """The sorted files of path's folder with path's suffix."""
    folder, suffix = os.path.dirname(path), os.path.splitext(path)[1]
    return sorted(os.path.join(folder, name) for name in os.listdir(folder) if os.path.splitext(name)[1] == suffix)


# ---------------------------------------------------------------------------------------------------------------------------------------- poses
def read_odometry_csv(path):
    """:258-278: rows of timestamp, tx ty tz qx qy qz qw under a header line -> {timestamp string: float64 [4,4]}."""
    from scipy.spatial.transform import Rotation
    out = {}
    with open(path, newline="") as f:
        reader = csv.reader(f)
        header = next(reader)
        header[0] = "ts"
        col = {name.strip(): i for i, name in enumerate(header)}
        for row in reader:
            if not row:
                continue
            T = np.eye(4)
            T[:3, 3] = [float(row[col[k]]) for k in ("tx", "ty", "tz")]
            T[:3, :3] = Rotation.from_quat([float(row[col[k]]) for k in ("qx", "qy", "qz", "qw")]).as_matrix()
            out[row[0]] = T
    return out


def read_odometry_npz(path):
    """:301-305: arr_0 the transforms (translation * 0.03), arr_1 the timestamps -> {timestamp string: float64 [4,4]}."""
    z = np.load(path, allow_pickle=False)
    tfs = np.array(z["arr_0"], dtype=np.float64)
    tfs[..., :3, 3] *= METASHAPE_SCALE
    return {str(ts): tf for ts, tf in zip(z["arr_1"], tfs)}


def read_odometry(folder, pose_src):
    if pose_src not in ODOMETRY_FILES:
        raise ValueError("BUP20 sequence dataset only supports [odom, rgbd, metashape] as poses source, but %s was given" % (pose_src,))
    path = os.path.join(folder, ODOMETRY_FILES[pose_src])
    return read_odometry_npz(path) if path.endswith(".npz") else read_odometry_csv(path)


def read_params(path):
    """params.yaml -> dict(intrinsics float64 [3,3], extrinsics float64 [4,4])."""
    import yaml
    with open(path) as f:
        doc = yaml.safe_load(f)
    return {k: np.asarray(v, dtype=np.float64) for k, v in doc.items()}


def frame_poses(odom, names, center, extrinsics):
    """:388-393 in float64: frame_i = E^-1 (odom_i^-1 odom_centre) E for the timestamps `names` -> [V,4,4]."""
    E = np.asarray(extrinsics, dtype=np.float64)
    Ei = np.linalg.inv(E)
    c = np.asarray(odom[center], dtype=np.float64)
    return np.stack([Ei @ (np.linalg.inv(np.asarray(odom[n], dtype=np.float64)) @ c) @ E for n in names])


def cv_to_gl(poses):
    """datasets/utils.py:35-42: poses @ diag(1, -1, -1, 1)."""
    return np.asarray(poses, dtype=np.float64) @ np.diag([1.0, -1.0, -1.0, 1.0])


def scale_and_shift(poses, scale, offset):
    """bup20.py:245-246: translation * scale + offset."""
    out = np.array(poses, dtype=np.float64)
    out[..., :3, 3] = out[..., :3, 3] * float(scale) + np.asarray(offset, dtype=np.float64)
    return out


def bup20_cameras(poses):
    """The step from the reference's pose to the camera -> world matrix its rays use.  PARITY UNPINNED: kaolin is third party and not on the machine
    this was written on; restated from memory: `Camera.extrinsics.update(pose)` makes the pose the VIEW matrix (world -> camera),
    `change_coordinate_system(B)` with B = diag(-1, -1, 1) right-multiplies the view matrix by B (B is its own inverse and transpose, so only the
    side is a choice), and `inv_transform_rays` applies the inverse view matrix.  -> c2w float32 [V,3,4], view_matrices float32 [V,4,4]; float64 inside."""
    view = np.asarray(poses, dtype=np.float64) @ np.diag([-1.0, -1.0, 1.0, 1.0])
    c2w = np.linalg.inv(view)[:, :3, :]
    return torch.from_numpy(np.ascontiguousarray(c2w)).float(), torch.from_numpy(np.ascontiguousarray(view)).float()


def bup20_intrinsics(K, mip, h, w):
    """bup20.py:237-242: K / 2^mip; fx, fy, x0 = cx - w // 2, y0 = cy - h // 2."""
    K = np.asarray(K, dtype=np.float64) / float(2 ** int(mip))
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]) - (w // 2), float(K[1, 2]) - (h // 2)


# ------------------------------------------------------------------------------------------------------------------------------ scale and offset
_PLY_TYPES = dict(char="i1", int8="i1", uchar="u1", uint8="u1", short="i2", int16="i2", ushort="u2", uint16="u2", int="i4", int32="i4", uint="u4",
                  uint32="u4", float="f4", float32="f4", double="f8", float64="f8")


def ply_vertex_bounds(path):
    """[[min, max] of x, y, z] float64 [3,2] of a PLY file's vertex element, which must be its first (plyfile's elements[0], as the reference takes it):
    ascii and binary_little_endian."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, count, props, in_vertex, seen = None, None, [], False, 0
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            words = line.decode("ascii", "replace").split()
            if not words or words[0] == "comment":
                continue
            if words[0] == "format":
                fmt = words[1]
            elif words[0] == "element":
                seen += 1
                in_vertex = seen == 1
                if in_vertex:
                    if words[1] != "vertex":
                        raise ValueError("%s: the first element is %r, not vertex" % (path, words[1]))
                    count = int(words[2])
            elif words[0] == "property" and in_vertex:
                if words[1] == "list":
                    raise ValueError("%s: a list property in the vertex element" % path)
                props.append((words[2], _PLY_TYPES[words[1]]))
            elif words[0] == "end_header":
                break
        if count is None or not all(k in dict(props) for k in "xyz"):
            raise ValueError("%s: no vertex element with x, y, z" % path)
        if fmt == "ascii":
            rows = np.loadtxt(f, dtype=np.float64, max_rows=count, ndmin=2) if count else np.zeros((0, len(props)))
            cols = {name: rows[:, i] for i, (name, _) in enumerate(props)}
        elif fmt == "binary_little_endian":
            rows = np.fromfile(f, dtype=np.dtype([(name, "<" + t) for name, t in props]), count=count)
            cols = {name: rows[name] for name, _ in props}
        else:
            raise ValueError("%s: format %r is neither ascii nor binary_little_endian" % (path, fmt))
    if count == 0:
        raise ValueError("%s: no vertices" % path)
    return np.array([[cols[k].min(), cols[k].max()] for k in "xyz"], dtype=np.float64)


def scale_from_bounds(bounds, scaling_option="snap_to_bottom"):
    """datasets/utils.py:7-33 on the vertex bounds [3,2] -> (scale, offset [3]), float64 (the reference computes in the vertices' dtype)."""
    bounds = np.asarray(bounds, dtype=np.float64)
    lengths = np.abs(bounds[:, 1] - bounds[:, 0])
    centers = (bounds[:, 1] + bounds[:, 0]) / 2.0
    if scaling_option == "largest":
        scale = 0.98 * 2.0 / lengths[np.argmax(lengths)]
        offset = -centers * scale
    elif scaling_option == "snap_to_bottom":
        scale = 2.0 / lengths[np.argmax(lengths[:2])]
        offset = -centers * scale
        offset[2] = -bounds[2, 0] * scale - 1
    else:
        raise NotImplementedError("Unimplememnted model scaling option: %s" % scaling_option)
    return float(scale), [float(v) for v in offset]


def load_scale_and_offset(root, model_rescaling="snap_to_bottom"):
    """bup20.py:76-86: from the first `<root>/../*.ply`, else (1.0, [0, 0, -1.4])."""
    meshes = sorted(glob.glob(os.path.join(os.path.expanduser(str(root)), "..", "*.ply")))
    if meshes:
        return scale_from_bounds(ply_vertex_bounds(meshes[0]), model_rescaling)
    return 1.0, [0.0, 0.0, -1.4]


# ---------------------------------------------------------------------------------------------------------------------------------- predictions
def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def decode_unet(preds):
    """agrobot_base.py:463-471 -> (semantics int32 [H,W], instance int32 [H,W], confidence float32 [H,W])."""
    conf = _np(preds["sem_seg"]["confidence"]).squeeze()
    return _np(preds["sem_seg"]["preds"]).astype(np.int32), _np(preds["instances"]["imap"]).astype(np.int32), conf.astype(np.float32)


def decode_maskrcnn(preds):
    """:473-486: masks float [N,1,H,W]; instance = 1 + the first mask above 0.5, else 0; semantics = instance > 0; confidence = the largest mask value, 0.9
    where that is 0.  DEVIATION: the channel axis alone is squeezed (the reference's bare squeeze() also drops N = 1)."""
    masks = torch.as_tensor(preds["masks"]).detach().cpu().float().squeeze(1)
    hit = (masks > 0.5).to(masks.dtype)
    imap = ((hit.sum(0) > 0).long() + hit.argmax(0)).numpy().astype(np.int32)
    conf = masks.max(dim=0).values.numpy().astype(np.float32)
    conf[conf == 0.0] = 0.9
    return (imap > 0).astype(np.int32), imap, conf


def decode_deeplab(preds):
    """:488-497: panoptic [1,2,H,W] = (semantics, instance); confidence 1."""
    pan = _np(preds["panoptic"])
    imap = pan[0, 1].astype(np.int32)
    return pan[0, 0].astype(np.int32), imap, np.ones(imap.shape, dtype=np.float32)


def decode_mask2former(preds):
    """:499-510: (semantics, instance, logit); confidence = sigmoid(-logit where instance == 0 else logit), with torch CPU ops."""
    imap = _np(preds[1])
    logit = torch.as_tensor(preds[2]).detach().cpu().float().clone()
    bg = torch.from_numpy(imap == 0)
    logit[bg] = -logit[bg]
    return _np(preds[0]).astype(np.int32), imap.astype(np.int32), torch.sigmoid(logit).numpy().astype(np.float32)


PREDICTION_KINDS = (("unet", decode_unet, ".pkl.bz2"), ("maskrcnn", decode_maskrcnn, ".pkl"), ("deeplab", decode_deeplab, ".pkl"),
                    ("mask2former", decode_mask2former, ".pkl"))


def read_prediction(image_path, preds_name):
    """:425-440: the prediction of the frame `image_path` from `<its folder>/<preds_name>/<stem>.pkl[.bz2]`, decoded by the first of unet / maskrcnn /
    deeplab / mask2former that preds_name contains.  THE FILE IS A PICKLE: load it only from a dataset you trust."""
    for kind, decode, ext in PREDICTION_KINDS:
        if kind in preds_name:
            path = os.path.join(os.path.dirname(image_path), preds_name, os.path.splitext(os.path.basename(image_path))[0] + ext)
            with (bz2.open(path, "rb") if ext.endswith(".bz2") else open(path, "rb")) as f:
                return decode(pickle.load(f))
    raise NotImplementedError("Load predictions for path name %s not implemented" % preds_name)


# ------------------------------------------------------------------------------------------------------------------- coverage rule: the definition
def round_vertices(poly):
    """Step 1: a flat [x0, y0, x1, y1, ...] list -> int64 [n,2] of trunc(5 v + 0.5) in float64."""
    xy = np.asarray(poly, dtype=np.float64).reshape(-1)
    xy = xy[:2 * (len(xy) // 2)].reshape(-1, 2)
    v = np.trunc(COCO_SCALE * xy + 0.5)
    if len(v) and float(np.abs(v).max()) >= COCO_MAX_COORD:
        raise ValueError("a polygon vertex at %g pixels: beyond +-%d" % (float(np.abs(xy).max()), COCO_MAX_COORD // COCO_SCALE))
    return v.astype(np.int64)


def edge_points(verts):
    """Step 2: the boundary points (u, v) int64 [m] of the closed ring through the rounded vertices, all edges in one sequence."""
    n = len(verts)
    us, vs = [], []
    for j in range(n):
        xs, ys = (int(c) for c in verts[j])
        xe, ye = (int(c) for c in verts[(j + 1) % n])
        dx, dy = abs(xe - xs), abs(ye - ys)
        xmajor = dx >= dy
        length = dx if xmajor else dy
        flip = (xs > xe) if xmajor else (ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        d = np.arange(length + 1, dtype=np.int64)
        t = length - d if flip else d
        if length == 0:
            us.append(np.array([xs], dtype=np.int64))
            vs.append(np.array([ys], dtype=np.int64))
        elif xmajor:
            s = np.float64(ye - ys) / np.float64(dx)
            us.append(xs + t)
            vs.append(np.trunc((np.float64(ys) + s * t.astype(np.float64)) + 0.5).astype(np.int64))
        else:
            s = np.float64(xe - xs) / np.float64(dy)
            vs.append(ys + t)
            us.append(np.trunc((np.float64(xs) + s * t.astype(np.float64)) + 0.5).astype(np.int64))
    if not us:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(us), np.concatenate(vs)


def polygon_keys_reference(poly, h, w):
    """Steps 1-3: the sorted keys int64 of one polygon part [x0, y0, x1, y1, ...] in an h x w image."""
    u, v = edge_points(round_vertices(poly))
    if len(u) < 2:
        return np.zeros(0, dtype=np.int64)
    u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
    xd = np.where(u1 < u0, u1, u1 - 1)
    X = (xd - 2) // COCO_SCALE
    keep = (u1 != u0) & ((xd - 2) % COCO_SCALE == 0) & (X >= 0) & (X <= w - 1)
    Y = np.clip((np.minimum(v0, v1) + 2) // COCO_SCALE, 0, h)
    return np.sort((X * h + Y)[keep])


def keys_mask(keys, h, w):
    """Step 4: bool [h,w], pixel (x, y) covered iff the number of keys <= x h + y is odd."""
    count = np.searchsorted(np.asarray(keys, dtype=np.int64), np.arange(h * w, dtype=np.int64), side="right")
    return (count & 1).astype(bool).reshape(w, h).T


def rle_counts(seg):
    """The run lengths of an RLE segmentation dict(size, counts): an uncompressed list, or the compressed string (pycocotools' rleFrString: 5 data bits and
    a continuation bit per character from '0', sign extension from bit 4 of the last, every run from the third on a difference to the run two before)."""
    counts = seg["counts"]
    if not isinstance(counts, (str, bytes)):
        return [int(c) for c in counts]
    data = counts.encode("ascii") if isinstance(counts, str) else counts
    out, p = [], 0
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            c = data[p] - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(out) > 2:
            x += out[-2]
        out.append(x)
    return out


def rle_keys(seg, h, w):
    """The keys of an RLE segmentation: its cumulative run lengths (a zero run gives a key twice, which cancels)."""
    size = [int(v) for v in seg.get("size", (h, w))]
    if size != [h, w]:
        raise ValueError("an RLE segmentation of size %s in an image of %d x %d" % (size, h, w))
    keys = np.cumsum(np.asarray(rle_counts(seg), dtype=np.int64))
    if len(keys) and (int(keys[-1]) > h * w or (np.diff(keys) < 0).any() or int(keys[0]) < 0):
        raise ValueError("an RLE segmentation whose runs do not fit %d x %d pixels" % (h, w))
    return keys


def mask_rle(mask):
    """bool [h,w] -> the uncompressed and the compressed RLE of it (the inverse of rle_keys; what a COCO writer stores)."""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    edges = np.flatnonzero(np.diff(np.concatenate(([False], flat)).astype(np.int8)) != 0)
    counts = np.diff(np.concatenate(([0], edges, [flat.size]))).tolist()
    chars = []
    for i, c in enumerate(counts):
        x = c - counts[i - 2] if i > 2 else c
        more = True
        while more:
            ch = x & 0x1F
            x >>= 5
            more = x != -1 if ch & 0x10 else x != 0
            chars.append(chr((ch | (0x20 if more else 0)) + 48))
    size = [int(mask.shape[0]), int(mask.shape[1])]
    return dict(size=size, counts=counts), dict(size=size, counts="".join(chars))


def segmentation_parts(seg, h, w):
    """A COCO `segmentation` -> [('poly', flat list) | ('keys', int64 keys)]: a list of polygons, or one RLE; empty -> no parts."""
    if not seg:
        return []
    if isinstance(seg, dict):
        return [("keys", rle_keys(seg, h, w))]
    return [("poly", p) for p in seg]


def part_keys(part, h, w):
    return polygon_keys_reference(part[1], h, w) if part[0] == "poly" else part[1]


def polygon_mask_reference(parts, h, w):
    """The coverage bool [h,w] of an annotation whose segmentation is the list of flat polygons `parts` (or one flat polygon): the OR of its parts."""
    if len(parts) and not isinstance(parts[0], (list, tuple, np.ndarray)):
        parts = [parts]
    out = np.zeros((h, w), dtype=bool)
    for p in parts:
        out |= keys_mask(polygon_keys_reference(p, h, w), h, w)
    return out


def image_annotations(coco, image_id, classes):
    """The annotations of an image that :526-527 and :541-542 select (those of the chosen categories, in file order) -> [(label, segmentation)]."""
    return [(classes[a["category_id"]], a.get("segmentation")) for a in coco["anns"].get(image_id, []) if a["category_id"] in classes]


def coco_labels_reference(anns, H0, W0, mip, max_label):
    """agrobot_base.py:524-547 and the nearest shrink for one image: anns = [(label, segmentation)] -> (semantics, instance) int64 [h,w,1].  anns None:
    a frame without labels, -1 everywhere."""
    f = _factor("coco_labels_reference", mip, H0, W0)
    h, w = H0 // f, W0 // f
    if anns is None:
        neg = torch.full((h, w, 1), -1, dtype=torch.int64)
        return neg, neg.clone()
    sem = np.zeros((H0, W0), dtype=np.int64)
    inst = np.zeros((H0, W0), dtype=np.int64)
    for i, (label, seg) in enumerate(anns):
        cover = np.zeros((H0, W0), dtype=bool)
        for part in segmentation_parts(seg, H0, W0):
            cover |= keys_mask(part_keys(part, H0, W0), H0, W0)
        if cover.all():
            sem[:] = 0
        sem = np.minimum(sem + int(label) * cover, int(max_label))
        inst[cover] = i + 1
    return torch.from_numpy(sem[::f, ::f].copy())[..., None], torch.from_numpy(inst[::f, ::f].copy())[..., None]


def part_key_bound(verts):
    """An upper bound of a polygon part's key count from its rounded vertices: within an edge u is monotone, so at most |dX| // 5 + 1 of its steps land
    on a pixel boundary; one more per edge for the joint."""
    if len(verts) == 0:
        return 0
    dx = np.abs(np.roll(verts[:, 0], -1) - verts[:, 0])
    return int((dx // COCO_SCALE + 2).sum())


def may_cover_image(seg, H0, W0):
    """Whether an annotation can cover every pixel: only when the box of its polygons' vertices contains the image (or it is an RLE).  The first column
    needs a vertex at x < 0.5 and the last one at x >= W0 - 0.5 (step 3's xd), rows likewise; the test allows a further half pixel."""
    if isinstance(seg, dict):
        return True
    pts = [np.asarray(p, dtype=np.float64).reshape(-1)[:2 * (len(p) // 2)].reshape(-1, 2) for p in seg or [] if len(p) >= 2]
    if not pts:
        return False
    pts = np.concatenate(pts)
    return bool(pts[:, 0].min() <= 1.0 and pts[:, 1].min() <= 1.0 and pts[:, 0].max() >= W0 - 1.0 and pts[:, 1].max() >= H0 - 1.0)


def coco_tables(frames, H0, W0):
    """What pag_coco_keys / pag_coco_labels read for a chunk: frames = [None | [(label, segmentation)]] -> dict of int32 numpy arrays
    (verts [NV,2] rounded, part_vert_begin [NP+1], point_begin [NV+1] the per-edge point-count prefix sums, part_key_begin [NP+1] from part_key_bound (an RLE
    part: its own count), part_key_count [NP] and keys [NK] holding the RLE parts' keys, ann_part_begin [NA+1], ann_label [NA], ann_cover [NA] = H0 W0
    for an RLE that covers the image, cand = the polygon annotations that need the counting pass, frame_ann_begin [B+1], frame_labelled [B]) and
    max_part_keys, the largest polygon part's bound."""
    if (W0 + 1) * H0 >= 1 << 31:
        raise ValueError("coco_tables: %d x %d pixels do not fit 32-bit keys" % (H0, W0))
    verts, part_vert_begin, part_key_begin, part_key_count, keys = [], [0], [0], [], []
    ann_part_begin, ann_label, ann_cover, cand, frame_ann_begin, frame_labelled = [0], [], [], [], [0], []
    nv, max_part_keys = 0, 0
    for anns in frames:
        frame_labelled.append(0 if anns is None else 1)
        for label, seg in anns or []:
            cover = 0
            for kind, data in segmentation_parts(seg, H0, W0):
                if kind == "poly":
                    v = round_vertices(data)
                    bound = part_key_bound(v)
                    max_part_keys = max(max_part_keys, bound)
                    verts.append(v)
                    nv += len(v)
                    part_key_count.append(0)
                    keys.append(np.zeros(bound, dtype=np.int64))
                else:
                    bound = len(data)
                    part_key_count.append(bound)
                    keys.append(data)
                    runs = np.concatenate((data, [H0 * W0])) if len(data) % 2 else data          # rle_keys: no key beyond H0 W0
                    cover = int((runs[1::2] - runs[0::2]).sum())
                part_vert_begin.append(nv)
                part_key_begin.append(part_key_begin[-1] + bound)
            if not isinstance(seg, dict) and may_cover_image(seg, H0, W0):
                cand.append(len(ann_label))
            ann_label.append(int(label))
            ann_cover.append(cover if cover == H0 * W0 else 0)
            ann_part_begin.append(len(part_key_count))
        frame_ann_begin.append(len(ann_label))
    verts = np.concatenate(verts) if verts else np.zeros((0, 2), dtype=np.int64)
    lengths = np.zeros(len(verts), dtype=np.int64)
    for b, e in zip(part_vert_begin[:-1], part_vert_begin[1:]):
        if e > b:
            nxt = np.roll(verts[b:e], -1, axis=0)
            lengths[b:e] = np.maximum(np.abs(nxt[:, 0] - verts[b:e, 0]), np.abs(nxt[:, 1] - verts[b:e, 1])) + 1
    point_begin = np.concatenate(([0], np.cumsum(lengths)))
    if int(point_begin[-1]) >= 1 << 31 or part_key_begin[-1] >= 1 << 31:
        raise ValueError("coco_tables: more than 2^31 boundary points or keys in one chunk")
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return dict(verts=i32(verts).reshape(-1, 2), part_vert_begin=i32(part_vert_begin), point_begin=i32(point_begin), part_key_begin=i32(part_key_begin),
                part_key_count=i32(part_key_count), keys=i32(np.concatenate(keys) if keys else []), ann_part_begin=i32(ann_part_begin),
                ann_label=i32(ann_label), ann_cover=i32(ann_cover), cand=i32(cand), frame_ann_begin=i32(frame_ann_begin),
                frame_labelled=i32(frame_labelled), max_part_keys=int(max_part_keys))


# -------------------------------------------------------------------------------------------------------------------- frame preparation: the definition
def _u16(depth_raw):
    """The 16-bit depth words as int32 (they are staged as int16 bit patterns)."""
    return depth_raw.to(torch.int32) & 0xFFFF


def depth_metres(depth_raw):
    """float(raw) * 0.001f."""
    return _u16(depth_raw).to(torch.float32) * 0.001


def pred_stats_reference(inst, depth_raw, max_depth, n_ids):
    """inst int32 [B,H0,W0], depth_raw int16 bit patterns [B,H0,W0] -> int32 [B,n_ids,2]: per view and id (total pixels, valid pixels)."""
    B = inst.shape[0]
    d = depth_metres(depth_raw)
    valid = (d > 0) & (d <= torch.tensor(float(max_depth), dtype=torch.float32, device=d.device))
    out = torch.zeros(B, n_ids, 2, dtype=torch.int32, device=inst.device)
    for b in range(B):
        ids = inst[b].reshape(-1).long()
        out[b, :, 0] = torch.bincount(ids, minlength=n_ids)[:n_ids].to(torch.int32)
        out[b, :, 1] = torch.bincount(ids[valid[b].reshape(-1)], minlength=n_ids)[:n_ids].to(torch.int32)
    return out


def keep_ids(counts):
    """int32 [..., 2] (total, valid) -> bool: 2 valid > total."""
    return 2 * counts[..., 1].long() > counts[..., 0].long()


def bilinear_shrink_reference(x, f):
    """float32 [B,H0,W0,C] -> [B,H0/f,W0/f,C]: the module docstring's `shrink`."""
    if f == 1:
        return x.clone()
    o0, o1 = f // 2 - 1, f // 2
    a, b, c, d = x[:, o0::f, o0::f], x[:, o0::f, o1::f], x[:, o1::f, o0::f], x[:, o1::f, o1::f]
    return ((0.25 * a + 0.25 * b) + 0.25 * c) + 0.25 * d


def _u8_table(device):
    """u / 255 for u = 0 .. 255 in IEEE float32 division, computed on the host whatever the device (a device's `x / c` may multiply by the rounded
    reciprocal; the kernel divides)."""
    return torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(device)


def prepare_frames_reference(img_u8, mip, bg_color="white", depth_raw=None, sem=None, inst=None, sem_conf=None, inst_conf=None, counts=None):
    """The frames of a chunk -> dict of the outputs whose inputs are given: imgs float32 [B,h,w,3], masks bool [B,h,w,1], depths float32 [B,h,w,1],
    semantics_pred / instance_pred int64 [B,h,w,1], sem_conf / inst_conf float32 [B,h,w,1].  img_u8 uint8 [B,H0,W0,3 or 4], depth_raw int16 bit patterns,
    sem / inst int32, the confidences float32, all [B,H0,W0]; counts int32 [B,n_ids,2] from pred_stats_reference or None (no depth filter)."""
    B, H0, W0, C0 = img_u8.shape
    f = _factor("prepare_frames_reference", mip, H0, W0)
    out = {}
    v = bilinear_shrink_reference(_u8_table(img_u8.device)[img_u8.long()], f)
    if C0 == 3:
        out["imgs"], out["masks"] = v, torch.ones(B, H0 // f, W0 // f, 1, dtype=torch.bool, device=img_u8.device)
    else:
        rgb, a = v[..., :3], v[..., 3:4]
        rest = 1.0 - a
        rgb = (rgb * a) + rest if bg_color == "white" else rgb - rest
        out["imgs"], out["masks"] = rgb.clamp(0.0, 1.0), a > 0.5
    if depth_raw is not None:
        out["depths"] = bilinear_shrink_reference(depth_metres(depth_raw)[..., None], f)
    flipped = None
    if inst is not None:
        inst2 = inst
        if counts is not None:
            keep = keep_ids(counts)                                                                  # [B, n_ids]
            kept = torch.gather(keep, 1, inst.reshape(B, -1).long()).reshape(inst.shape)
            inst2 = torch.where(kept, inst, torch.zeros_like(inst))
            flipped = (inst != 0) != (inst2 != 0)
        out["instance_pred"] = inst2[:, ::f, ::f].long()[..., None]
        if sem is not None:
            out["semantics_pred"] = (torch.where(inst2 == 0, torch.zeros_like(sem), sem) if counts is not None else sem)[:, ::f, ::f].long()[..., None]
    elif sem is not None:
        out["semantics_pred"] = sem[:, ::f, ::f].long()[..., None]
    for key, conf in (("sem_conf", sem_conf), ("inst_conf", inst_conf)):
        if conf is not None:
            c = torch.where(flipped, torch.ones_like(conf), conf) if flipped is not None else conf
            out[key] = bilinear_shrink_reference(c[..., None], f)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------- decoding
def decode_rgb(path):
    """agrobot_base.py:428: the frame as uint8 [H,W,3], or [H,W,4] when the file has alpha (the reference converts to RGB and never sees one)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("RGBA", "LA", "PA") or (im.mode == "P" and "transparency" in im.info):
            return np.asarray(im.convert("RGBA"), dtype=np.uint8)
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def decode_depth(path):
    """A 16-bit depth PNG -> uint16 [H,W]."""
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im)
    if arr.ndim != 2 or arr.dtype.kind not in "ui" or int(arr.min()) < 0 or int(arr.max()) > 0xFFFF:
        raise ValueError("%s: a depth image is one channel of 16-bit integers, got %s %s" % (path, arr.dtype, arr.shape))
    return arr.astype(np.uint16)


# --------------------------------------------------------------------------------------------------------------------------------------- loader
def plan_frames(root, split, coco, image_sets, classes, dataset_center_idx=0, seq_num_frames=40):
    """-> (paths of the window's frames, path of the centre frame, its annotations [(label, segmentation)] and COCO size (height, width))."""
    def path_of(image_id):
        return os.path.join(root, dataset_rel_path(coco["images"][image_id]["path"]))

    eval_ids = [i for i in image_sets["eval"]]
    kept = keep_eval_frames([path_of(i) for i in eval_ids], list_sequence, seq_num_frames)
    ids_of = {path_of(i): i for i in eval_ids}
    train_paths = [path_of(i) for i in image_sets["train"]]
    if not 0 <= dataset_center_idx < len(kept):
        raise IndexError("load_bup20: dataset_center_idx %d outside the %d eval frames that are %d frames from their sequence's ends"
                         % (dataset_center_idx, len(kept), seq_num_frames + 1))
    center = kept[dataset_center_idx]
    paths = window_paths(center, list_sequence(center), split, seq_num_frames, train_paths, kept)
    if not paths:
        raise RuntimeError("load_bup20: the window about %s holds no frame for split %r" % (center, split))
    md = coco["images"][ids_of[center]]
    return paths, center, image_annotations(coco, md["id"], classes), (int(md["height"]), int(md["width"]))


def load_bup20(root, split, mip=0, bg_color="white", load_modes=(), class_labels=(), dataset_center_idx=0, pose_src="odom", max_depth=-1, scale=None,
               offset=None, model_rescaling="snap_to_bottom", seq_num_frames=40, device="cuda", num_workers=0, use_kernel=True,
               add_noise_to_train_poses=False, dataset_mode="label_window", chunk_bytes=64 << 20, keep_depths=False):
    """The window of split `split` ('train' or 'val') about the dataset_center_idx-th usable eval frame of the BUP20 folder `root` ->
    DeviceMultiviewDataset on `device` with imgs, masks, rays, base_rays and, as the filtered load_modes ask (filter_load_modes), depths, semantics +
    semantics_pred, instance + instance_pred, sem_conf, inst_conf; carrying view_matrices, image_shape, filenames, scale, intrinsics and semantic_info
    exactly like formats.load_nerf_standard's dataset.  The module docstring holds the rules and the deviations from the reference.

    Frames (image, depth where needed, the pickled prediction) are decoded on min(16, num_workers) threads (inline when num_workers <= 0) into one of
    two pinned staging buffers of at most chunk_bytes, copied asynchronously, and prepared on the device per chunk: pag_coco_keys + pag_coco_labels for the
    ground truth, pag_bup20_pred_stats (max_depth > 0) + pag_bup20_prepare for everything from the frames, pag_prepare_views for the rays.  A staging
    buffer is reused only after the event of its own copy has completed.  A polygon part beyond COCO_MAX_PART_KEYS keys is refused by the kernel's entry
    point before any launch; that image's label planes then come from the definition.  On a CPU device, or with use_kernel=False, the definition runs
    throughout.  PREDICTIONS ARE PICKLES: only load a dataset you trust.
    keep_depths: the 'train' split carries `depths` too (filter_load_modes drops it there, as the reference does): the depth carve needs it."""
    import yaml
    from .dataset import DeviceMultiviewDataset
    from .map_export import pinhole_base_rays
    if add_noise_to_train_poses:
        raise NotImplementedError("load_bup20: add_noise_to_train_poses is not implemented")
    if dataset_mode != "label_window":
        raise NotImplementedError("load_bup20: dataset_mode %r is not implemented, only 'label_window'" % (dataset_mode,))
    if bg_color not in ("white", "black"):
        raise ValueError("load_bup20: bg_color %r is neither 'white' nor 'black'" % (bg_color,))
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    root = os.path.expanduser(str(root))
    split = "val" if split == "valid" else split
    window_deltas(seq_num_frames, split)                                   # the split check
    class_labels = list(class_labels) or list(DEFAULT_CLASS_LABELS)
    preds_name, modes = filter_load_modes(load_modes, split, keep_depths)
    json_path, yaml_path = dataset_files(root)
    coco = read_coco(json_path)
    with open(yaml_path) as f:
        image_sets = yaml.safe_load(f)["image_sets"]
    classes = class_map(coco["cats"], class_labels)
    max_label = max(classes.values()) if classes else 0
    paths, center, center_anns, coco_size = plan_frames(root, split, coco, image_sets, classes, int(dataset_center_idx), int(seq_num_frames))
    V = len(paths)
    names = [os.path.basename(p).split(".")[0] for p in paths]

    folder = os.path.dirname(center)
    params = read_params(os.path.join(folder, "params.yaml"))
    if scale is None or offset is None:
        loaded_scale, loaded_offset = load_scale_and_offset(root, model_rescaling)
        scale = loaded_scale if scale is None else scale
        offset = loaded_offset if offset is None else offset
    poses = frame_poses(read_odometry(folder, pose_src), names, os.path.basename(center).split(".")[0], params["extrinsics"])
    c2w, view_matrices = bup20_cameras(scale_and_shift(cv_to_gl(poses), scale, offset))

    first = decode_rgb(paths[0])
    H0, W0, C0 = first.shape
    if (H0, W0) != coco_size and any(p == center for p in paths):
        raise ValueError("load_bup20: %s is %d x %d, the COCO file says %d x %d" % (center, H0, W0, coco_size[0], coco_size[1]))
    f = _factor("load_bup20", mip, H0, W0)
    mip, h, w = int(mip), H0 // f, W0 // f
    fx, fy, x0, y0 = bup20_intrinsics(params["intrinsics"], mip, h, w)
    filter_depth = float(max_depth) > 0
    if filter_depth and H0 * W0 >= 1 << 24:
        raise ValueError("load_bup20: %d x %d pixels: the integer keep rule equals the reference's float32 quotient below 2^24 pixels only" % (H0, W0))
    want_gt = [m for m in ("semantics", "instance") if m in modes]
    want_pred = any(m in modes for m in ("semantics", "instance", "sem_conf", "inst_conf"))
    want_depth = "depths" in modes or (filter_depth and want_pred)
    filter_depth = filter_depth and want_pred

    cuda = device.type == "cuda"
    kernel = cuda and use_kernel
    N0 = H0 * W0
    n_i32 = 3 if want_pred else 0                                          # semantics, instance, confidence (both confidences are one array, :463-510)
    view_bytes = N0 * (4 * n_i32 + (2 if want_depth else 0) + C0)
    per_chunk = max(1, min(V, MAX_CHUNK_VIEWS, int(chunk_bytes) // view_bytes))
    staging = [torch.empty(per_chunk * view_bytes, dtype=torch.uint8, pin_memory=cuda) for _ in range(2 if cuda else 1)]
    events = [None] * len(staging)
    pool = concurrent.futures.ThreadPoolExecutor(min(16, int(num_workers))) if num_workers > 0 else None

    with torch.cuda.device(device) if cuda else _nothing():
        imgs = torch.empty(V, h, w, 3, dtype=torch.float32, device=device)
        masks = torch.empty(V, h, w, 1, dtype=torch.bool, device=device)
        origins, dirs = torch.empty_like(imgs), torch.empty_like(imgs)
        out = {}
        if "depths" in modes:
            out["depths"] = torch.empty(V, h, w, 1, dtype=torch.float32, device=device)
        for m in want_gt:
            out[m] = torch.empty(V, h, w, 1, dtype=torch.int64, device=device)
            out[m + "_pred"] = torch.empty(V, h, w, 1, dtype=torch.int64, device=device)
        for m in ("sem_conf", "inst_conf"):
            if m in modes:
                out[m] = torch.empty(V, h, w, 1, dtype=torch.float32, device=device)
        c2w_dev = c2w.to(device)
        on_device = torch.empty(per_chunk * view_bytes, dtype=torch.uint8, device=device) if cuda else None
        try:
            for k, off in enumerate(range(0, V, per_chunk)):
                n = min(per_chunk, V - off)
                slot = k % len(staging)
                if events[slot] is not None:
                    events[slot].synchronize()                  # the one wait: this buffer's own copy, two chunks ago
                host = staging[slot][:n * view_bytes]

                def carve(buf, n=n):
                    """The chunk's planes in a staging / device buffer: 4-byte planes first, then the 16-bit depth, then the image bytes."""
                    pos, planes = 0, {}
                    if want_pred:
                        for name, dtype in (("sem", torch.int32), ("inst", torch.int32), ("conf", torch.float32)):
                            planes[name] = buf[pos:pos + 4 * n * N0].view(dtype).view(n, H0, W0)
                            pos += 4 * n * N0
                    if want_depth:
                        planes["depth"] = buf[pos:pos + 2 * n * N0].view(torch.int16).view(n, H0, W0)
                        pos += 2 * n * N0
                    planes["img"] = buf[pos:pos + n * N0 * C0].view(n, H0, W0, C0)
                    return planes

                hp = {name: t.numpy() for name, t in carve(host).items()}
                max_id = [0] * n

                def decode(i, off=off, hp=hp, max_id=max_id):
                    path = paths[off + i]
                    arr = first if off + i == 0 else decode_rgb(path)
                    if arr.shape != (H0, W0, C0):
                        raise ValueError("%s: %s pixels and channels, the first frame has %s" % (path, arr.shape, (H0, W0, C0)))
                    hp["img"][i] = arr
                    if want_depth:
                        d = decode_depth(os.path.join(os.path.dirname(path), "depth", os.path.basename(path)))
                        if d.shape != (H0, W0):
                            raise ValueError("%s: the depth image is %s, the frame %d x %d (the reference would resize it; this loader does not)"
                                             % (path, d.shape, H0, W0))
                        hp["depth"][i] = d.view(np.int16)
                    if want_pred:
                        s, m, c = read_prediction(path, preds_name)
                        if s.shape != (H0, W0) or m.shape != (H0, W0) or c.shape != (H0, W0):
                            raise ValueError("%s: a prediction of %s / %s / %s pixels for a frame of %d x %d" % (path, s.shape, m.shape, c.shape, H0, W0))
                        if int(m.min()) < 0:
                            raise ValueError("%s: a negative instance id in the prediction" % path)
                        hp["sem"][i], hp["inst"][i], hp["conf"][i] = s, m, c
                        max_id[i] = int(m.max())

                if pool is None:
                    for i in range(n):
                        decode(i)
                else:
                    list(pool.map(decode, range(n)))
                if cuda:
                    chunk = on_device[:n * view_bytes]
                    chunk.copy_(host, non_blocking=True)
                    events[slot] = torch.cuda.Event()
                    events[slot].record()
                else:
                    chunk = host
                dp = carve(chunk)
                frames = [center_anns if paths[off + i] == center else None for i in range(n)]
                n_ids = max(max_id) + 1
                if kernel:
                    from . import ops
                    if want_gt:
                        _labels_on_device(ops, frames, H0, W0, mip, max_label, off, out.get("semantics"), out.get("instance"))
                    counts = ops.bup20_pred_stats(dp["inst"], dp["depth"], max_depth, n_ids) if filter_depth else None
                    ops.bup20_prepare(dp["img"], mip, bg_color, off, depth_raw=dp.get("depth"), sem=dp.get("sem"), inst=dp.get("inst"),
                                      sem_conf=dp.get("conf"), inst_conf=dp.get("conf"), counts=counts, imgs=imgs, masks=masks, depths=out.get("depths"),
                                      semantics_pred=out.get("semantics_pred"), instance_pred=out.get("instance_pred"), sem_conf_out=out.get("sem_conf"),
                                      inst_conf_out=out.get("inst_conf"))
                    ops.prepare_views(dp["img"], mip, bg_color, off, origins=origins, dirs=dirs, c2w=c2w_dev, intrinsics=(fx, fy, x0, y0))
                else:
                    from .formats import rays_reference
                    for i, anns in enumerate(frames):
                        if want_gt:
                            sem_gt, inst_gt = coco_labels_reference(anns, H0, W0, mip, max_label)
                            for m, plane in (("semantics", sem_gt), ("instance", inst_gt)):
                                if m in out:
                                    out[m][off + i] = plane.to(device)
                    counts = pred_stats_reference(dp["inst"], dp["depth"], max_depth, n_ids) if filter_depth else None
                    got = prepare_frames_reference(dp["img"], mip, bg_color, depth_raw=dp.get("depth"), sem=dp.get("sem"), inst=dp.get("inst"),
                                                   sem_conf=dp.get("conf"), inst_conf=dp.get("conf"), counts=counts)
                    imgs[off:off + n], masks[off:off + n] = got["imgs"], got["masks"]
                    for m in out:
                        if m not in ("semantics", "instance"):
                            out[m][off:off + n] = got[m]
                    r = rays_reference(c2w_dev[off:off + n], w, h, fx, fy, x0, y0)
                    origins[off:off + n], dirs[off:off + n] = r.origins, r.dirs
        finally:
            if pool is not None:
                pool.shutdown()
        data = dict(imgs=imgs, masks=masks, rays=Rays(origins, dirs, 0.0, DEFAULT_FAR), **out)
        base = pinhole_base_rays(w, h, fx, fy, x0, y0, device=device)
        data["base_rays"] = Rays(base.origins, base.dirs, 0.0, DEFAULT_FAR)
        ds = DeviceMultiviewDataset(data, device)
    ds.view_matrices = view_matrices
    ds.image_shape = (h, w)
    ds.filenames = [os.path.basename(p) for p in paths]
    ds.scale = float(scale)
    ds.intrinsics = dict(fx=fx, fy=fy, x0=x0, y0=y0)
    info = semantic_info(class_labels)
    ds.semantic_info = dict(num_classes=info["num_classes"], num_instances=info["num_instances"], things_ids=info["things_ids"], stuff_ids=info["stuff_ids"])
    return ds


def _labels_on_device(ops, frames, H0, W0, mip, max_label, off, semantics, instance):
    """The chunk's ground-truth planes by pag_coco_keys + pag_coco_labels; a frame with a polygon part beyond the sort cap takes the definition."""
    tables = coco_tables(frames, H0, W0)
    if tables["max_part_keys"] > COCO_MAX_PART_KEYS:
        fallback = [i for i, anns in enumerate(frames) if anns is not None and coco_tables([anns], H0, W0)["max_part_keys"] > COCO_MAX_PART_KEYS]
        log.warning("load_bup20: %d frame(s) with a polygon part beyond %d keys take the tensor-op labels", len(fallback), COCO_MAX_PART_KEYS)
        tables = coco_tables([None if i in fallback else anns for i, anns in enumerate(frames)], H0, W0)
    else:
        fallback = []
    dev = ops.coco_upload(tables, (semantics if semantics is not None else instance).device)
    ops.coco_keys(dev, H0, W0)
    ops.coco_labels(dev, H0, W0, mip, max_label, off, semantics=semantics, instance=instance)
    for i in fallback:
        sem_gt, inst_gt = coco_labels_reference(frames[i], H0, W0, mip, max_label)
        if semantics is not None:
            semantics[off + i] = sem_gt.to(semantics.device)
        if instance is not None:
            instance[off + i] = inst_gt.to(instance.device)


# ----------------------------------------------------------------------------------------------------------------------------------------- CLI
def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m pagnerf_amd.bup20", description="A BUP20 folder -> the .npz that python -m pagnerf_amd.train reads")
    ap.add_argument("root", help="the folder with BUP_20.json / CKA_sweet_pepper_2020_summer.json")
    ap.add_argument("--split", default="train", choices=("train", "val"))
    ap.add_argument("--mip", type=int, default=0)
    ap.add_argument("--bg-color", default="white", choices=("white", "black"))
    ap.add_argument("--load-modes", nargs="*", default=[])
    ap.add_argument("--class-labels", nargs="*", default=[])
    ap.add_argument("--dataset-center-idx", type=int, default=0)
    ap.add_argument("--pose-src", default="odom", choices=sorted(ODOMETRY_FILES))
    ap.add_argument("--max-depth", type=float, default=-1.0)
    ap.add_argument("--keep-depths", action="store_true", help="--split train: write the depth images (metres) as well, for the trainer's carve_from_depth")
    ap.add_argument("--model-rescaling", default="snap_to_bottom", choices=("snap_to_bottom", "largest"))
    ap.add_argument("--seq-num-frames", type=int, default=40)
    ap.add_argument("--out", required=True, metavar="FILE.npz")
    ap.add_argument("--num-workers", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    ds = load_bup20(args.root, args.split, mip=args.mip, bg_color=args.bg_color, load_modes=args.load_modes, class_labels=args.class_labels,
                    dataset_center_idx=args.dataset_center_idx, pose_src=args.pose_src, max_depth=args.max_depth, model_rescaling=args.model_rescaling,
                    seq_num_frames=args.seq_num_frames, device=args.device, num_workers=args.num_workers, keep_depths=args.keep_depths)
    with open(os.path.expanduser(args.out), "wb") as f:
        np.savez(f, **dataset_arrays(ds))
    return 0


if __name__ == "__main__":
    sys.exit(main())
