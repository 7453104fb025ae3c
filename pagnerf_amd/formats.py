"""python -m pagnerf_amd.formats ROOT [--split S] [--mip M] [--bg-color C] --out FILE.npz [--num-workers N] [--device D]

NeRF-standard datasets from disk (datasets/formats/nerf_standard.py feeding datasets/multiview_dataset.py:120-132): a folder with `transforms*.json` and
image files in, a DeviceMultiviewDataset out.  The reference decodes every frame, converts it to float (`img_as_float32`), shrinks it (`resize_mip`,
area filter), composites it onto the background, thresholds the alpha into a mask, builds a camera, generates one pinhole ray per pixel on the GPU and
copies everything back to the host to stack it.  Here the decoded uint8 frames go to the device in chunks through two pinned staging buffers, and one
launch per chunk (csrc/prepare.hip) writes the final float image, mask and world rays straight into the dataset's storage.

THE DEFINITION is the tensor-op form in this module (`prepare_views_reference`, `prepare_labels_reference`, `rays_reference`); it serves CPU tensors
(and any device with `use_kernel=False`), and the kernel is held to it: images, masks, labels and ray origins bit for bit, ray directions to 2e-6.

    image   f = 2^mip must divide both sides (cv2.INTER_AREA is an exact block mean only then).  Per channel S = the integer sum of the f x f block,
            v = float32(S) / float32(255 f f), ONE fp32 division.  RGB: v, mask true.  RGBA (:269-282): a = v[3], mask = a > 0.5,
            'white' clamp((rgb * a) + (1 - a), 0, 1), 'black' clamp(rgb - (1 - a), 0, 1): three fp32 roundings in that order, no FMA.
    labels  out[y, x] = src[y f, x f]: torch.nn.functional.interpolate(mode='nearest') at an integer factor (datasets/formats/bup20.py:203-229).
    cameras :177-236 in float64 on the host, rounded to float32 once (`standard_cameras`).
    rays    origin = c2w[:, 3]; dir = normalise(R d), d the camera-frame direction of map_export.pinhole_base_rays at the output size; near 0, far 6 (:239).

PARITY UNPINNED, as map_export.pinhole_base_rays: the ray generator (wisp's generate_centered_pixel_coords / generate_pinhole_rays) and the default
`world_basis` (kaolin's blender_coords(), restated from memory: x' = x, y' = z, z' = -y) are third party and not on the machine this was written on.
Both are arguments or one function, so a pinned value replaces them in one place.

THE LABEL EXTENSION is this package's own, not part of the NeRF-standard / instant-ngp layout: a frame may carry `semantic_path`, `instance_path`,
`semantic_pred_path`, `instance_pred_path`, each an 8-bit grey PNG of the image's size; they become the modes `semantics`, `instance`, `semantics_pred`,
`instance_pred` (int64 [V,h,w,1]).  Top-level `num_classes`, `num_instances`, `things_ids`, `stuff_ids` become `semantic_info`.  A label key on some
frames only is an error.  BUP20's own layout (agrobot_base.py: COCO annotations, detector predictions) is read by bup20.py.
"""
import argparse
import concurrent.futures
import functools
import glob
import json
import logging
import math
import os
import sys

import numpy as np
import torch

from .core import Rays

log = logging.getLogger(__name__)

BLENDER_TO_Y_UP = ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0))      # x' = x, y' = z, z' = -y  (PARITY UNPINNED: kaolin's blender_coords())
LABEL_KEYS = (("semantic_path", "semantics"), ("instance_path", "instance"), ("semantic_pred_path", "semantics_pred"),
              ("instance_pred_path", "instance_pred"))
DEFAULT_FAR = 6.0               # nerf_standard.py:239
MAX_MIP = 8
MAX_CHUNK_VIEWS = 65535         # pag_prepare_views: the chunk's views are the launch's second grid axis


# ------------------------------------------------------------------------------------------------------------------------------ the definition
def _make_block_table(f, device):
    den = 255 * f * f
    return torch.from_numpy(np.arange(den + 1, dtype=np.float32) / np.float32(den)).to(device)


_cached_block_table = functools.lru_cache(maxsize=8)(_make_block_table)


def _block_table(f, device):
    """S / (255 f f) for S = 0 .. 255 f f in IEEE float32 division, computed on the host whatever the device (a device's `x / c` may multiply by the
    rounded reciprocal; the kernel divides).  255 f f < 2^24 up to mip 8, so S and the divisor are exact in float32.  Only the tables up to mip 2
    (16 KB at most) are kept; a larger one - 67 MB at mip 8 - is built for the call and dropped with it."""
    return _cached_block_table(f, device) if f <= 4 else _make_block_table(f, device)


def _factor(name, mip, H0, W0):
    mip = int(mip)
    if not 0 <= mip <= MAX_MIP:
        raise ValueError("%s: mip %d not in [0, %d]" % (name, mip, MAX_MIP))
    f = 1 << mip
    if H0 % f or W0 % f:
        raise ValueError("%s: image size %d x %d is not divisible by 2^mip = %d (the area filter is an exact block mean only then)" % (name, H0, W0, f))
    return f


def prepare_views_reference(src_u8, mip, bg_color):
    """uint8 [B,H0,W0,3 or 4] -> (imgs float32 [B,h,w,3], masks bool [B,h,w,1]) at h = H0 / 2^mip, w = W0 / 2^mip: the module docstring's `image`."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] not in (3, 4):
        raise ValueError("prepare_views_reference: uint8 [B,H0,W0,3 or 4] expected, got %s %s" % (src_u8.dtype, tuple(src_u8.shape)))
    if bg_color not in ("white", "black"):
        raise ValueError("prepare_views_reference: bg_color %r is neither 'white' nor 'black'" % (bg_color,))
    B, H0, W0, C0 = src_u8.shape
    f = _factor("prepare_views_reference", mip, H0, W0)
    h, w = H0 // f, W0 // f
    S = src_u8.reshape(B, h, f, w, f, C0).to(torch.int32).sum((2, 4))
    v = _block_table(f, src_u8.device)[S.long()]
    if C0 == 3:
        return v, torch.ones(B, h, w, 1, dtype=torch.bool, device=src_u8.device)
    rgb, a = v[..., :3], v[..., 3:4]
    rest = 1.0 - a
    rgb = (rgb * a) + rest if bg_color == "white" else rgb - rest
    return rgb.clamp(0.0, 1.0), a > 0.5


def prepare_labels_reference(src_u8, mip):
    """uint8 [B,H0,W0] -> int64 [B,h,w,1], out[y, x] = src[y 2^mip, x 2^mip]."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 3:
        raise ValueError("prepare_labels_reference: uint8 [B,H0,W0] expected, got %s %s" % (src_u8.dtype, tuple(src_u8.shape)))
    f = _factor("prepare_labels_reference", mip, src_u8.shape[1], src_u8.shape[2])
    return src_u8[:, ::f, ::f].long()[..., None]


def standard_cameras(meta, w, h, mip=0, world_basis=BLENDER_TO_Y_UP):
    """The cameras of a transforms JSON (`meta`, its `frames` the views) for w x h images at `mip` (nerf_standard.py:177-236)
    -> fx, fy, x0, y0 (floats), c2w float32 [V,3,4] (camera -> world), view_matrices float32 [V,4,4] (world -> camera).  float64 throughout, rounded once.
    x_fov / y_fov are degrees, camera_angle_x / _y radians: f = 0.5 size / tan(0.5 angle), fy = fx without the y key.  fl_x / fl_y (divided by 2^mip)
    count only without an angle key - where the reference ends with focal 0.  x0 = cx / 2^mip - w // 2, y0 likewise, else 0.
    t = transform_matrix[:3, 3] / aabb_scale * scale + offset (defaults 1.25, 1.0, 0);  c2w = [B R | B t], B = world_basis (None: the identity;
    the default is PARITY UNPINNED, see the module docstring)."""
    f = float(2 ** int(mip))
    if "x_fov" in meta:
        fx = 0.5 * w / math.tan(0.5 * float(meta["x_fov"]) * (math.pi / 180.0))
        fy = 0.5 * h / math.tan(0.5 * float(meta["y_fov"]) * (math.pi / 180.0)) if "y_fov" in meta else fx
    elif "camera_angle_x" in meta:
        fx = 0.5 * w / math.tan(0.5 * float(meta["camera_angle_x"]))
        fy = 0.5 * h / math.tan(0.5 * float(meta["camera_angle_y"])) if "camera_angle_y" in meta else fx
    elif "fl_x" in meta:
        fx = float(meta["fl_x"]) / f
        fy = float(meta["fl_y"]) / f if "fl_y" in meta else fx
    else:
        raise ValueError("standard_cameras: the JSON has none of x_fov, camera_angle_x, fl_x")
    x0 = float(meta["cx"]) / f - w // 2 if "cx" in meta else 0.0
    y0 = float(meta["cy"]) / f - h // 2 if "cy" in meta else 0.0
    for key, what in (("fix_premult", "premultiplied alpha"), ("k1", "distortion"), ("rolling_shutter", "rolling shutter")):      # :207-217
        if key in meta:
            log.warning("The dataset expects %s correction, but the current implementation does not handle this.", what)
    offset = np.asarray(meta.get("offset", [0.0, 0.0, 0.0]), dtype=np.float64)
    scale, aabb_scale = float(meta.get("scale", 1.0)), float(meta.get("aabb_scale", 1.25))
    basis = np.eye(3) if world_basis is None else np.asarray(world_basis, dtype=np.float64).reshape(3, 3)
    V = len(meta["frames"])
    c2w, views = np.zeros((V, 3, 4)), np.zeros((V, 4, 4))
    for i, frame in enumerate(meta["frames"]):
        T = np.asarray(frame["transform_matrix"], dtype=np.float64)
        R = basis @ T[:3, :3]
        t = basis @ (T[:3, 3] / aabb_scale * scale + offset)
        c2w[i, :, :3], c2w[i, :, 3] = R, t
        views[i, :3, :3], views[i, :3, 3], views[i, 3, 3] = R.T, -R.T @ t, 1.0
    return fx, fy, x0, y0, torch.from_numpy(c2w).float(), torch.from_numpy(views).float()


def rays_reference(c2w, w, h, fx, fy, x0=0.0, y0=0.0):
    """World rays of every pixel of the views c2w [V,3,4] -> Rays with [V,h,w,3] fields, in c2w's dtype and on its device: origin = c2w[:, :, 3],
    dir = normalise(R d) with d the camera-frame direction of map_export.pinhole_base_rays (the one statement of the pixel formula); near 0, far 6."""
    from .map_export import pinhole_base_rays
    V = c2w.shape[0]
    d = pinhole_base_rays(w, h, fx, fy, x0, y0, device=c2w.device, dtype=c2w.dtype).dirs                       # [h*w, 3]
    d = (c2w[:, None, :, :3] * d[None, :, None, :]).sum(-1)                                                    # R d: [V, h*w, 3]
    d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    o = c2w[:, None, :, 3].expand(V, h * w, 3)
    return Rays(o.reshape(V, h, w, 3).contiguous(), d.reshape(V, h, w, 3), 0.0, DEFAULT_FAR)


# ------------------------------------------------------------------------------------------------------------------------------------ decoding
def decode_image(path):
    """An image file -> numpy uint8 [H,W], [H,W,3] or [H,W,4].  PIL when it imports (palette and grey + alpha files are expanded to RGBA); otherwise
    visualize.read_png, which reads 8-bit RGB or grey PNGs with filter-0 rows and names that subset in its error for anything else."""
    try:
        from PIL import Image
    except ImportError:
        from .visualize import read_png
        return read_png(path)
    with Image.open(path) as im:
        if im.mode in ("P", "LA", "PA"):
            im = im.convert("RGBA")
        if im.mode not in ("L", "RGB", "RGBA"):
            raise ValueError("%s: only 8-bit grey, RGB and RGBA images are read (PIL mode %r)" % (path, im.mode))
        return np.asarray(im, dtype=np.uint8)


def _resolve(root, name):
    path = os.path.join(root, str(name).replace("\\", "/"))
    return path if os.path.splitext(path)[1] else path + ".png"                # :47-52: no extension means PNG, as nerf-synthetic has it


def transforms_files(root):
    """split -> JSON path, as nerf_standard.py:108-129: one *.json is 'train' alone, three are test / train / val by name."""
    files = sorted(glob.glob(os.path.join(os.path.expanduser(root), "*.json")))
    if len(files) == 1:
        return {"train": files[0]}
    if len(files) != 3:
        raise RuntimeError("Unsupported number of splits, there should be ['test', 'train', 'val']")
    return {s: p for s in ("test", "train", "val") for p in files if s in os.path.basename(p)}


def read_frames(root, split):
    """-> (meta, frames): the JSON of `split`, and per frame whose image file exists a dict(path, basename, transform_matrix, labels {mode: path})."""
    root = os.path.expanduser(root)
    files = transforms_files(root)
    if split not in files:
        raise RuntimeError("Split type ['%s'] unsupported in the dataset provided" % split)
    with open(files[split]) as f:
        meta = json.load(f)
    listed = meta.get("frames") or []
    for key, _ in LABEL_KEYS:
        have = sum(key in fr for fr in listed)
        if have not in (0, len(listed)):
            raise ValueError("%s: %r is present on %d of %d frames; a label image belongs to every frame or to none" % (files[split], key, have, len(listed)))
    frames = []
    for fr in listed:
        path = _resolve(root, fr["file_path"])
        if not os.path.exists(path):        # :54-65: instant-ngp allows frames whose image is missing
            continue
        frames.append(dict(path=path, basename=os.path.basename(os.path.splitext(path)[0]), transform_matrix=fr["transform_matrix"],
                           labels={mode: _resolve(root, fr[key]) for key, mode in LABEL_KEYS if key in fr}))
    if not frames:
        raise RuntimeError("%s: none of the %d frames has its image file" % (files[split], len(listed)))
    return meta, frames


def _as_channels(arr, C0, path, H0, W0):
    """A decoded frame as uint8 [H0,W0,C0]: grey is repeated, a missing alpha is opaque; any other difference is an error."""
    if arr.ndim == 2:
        arr = np.repeat(arr[:, :, None], 3, axis=2)
    if arr.shape[:2] != (H0, W0):
        raise ValueError("%s: %d x %d pixels, the first frame has %d x %d" % (path, arr.shape[0], arr.shape[1], H0, W0))
    if arr.shape[2] == 3 and C0 == 4:
        arr = np.concatenate([arr, np.full((H0, W0, 1), 255, dtype=np.uint8)], axis=2)
    if arr.shape[2] != C0:
        raise ValueError("%s: %d channels, the first frame has %d" % (path, arr.shape[2], C0))
    return arr


def _label_plane(path, H0, W0):
    arr = decode_image(path)
    if arr.ndim != 2 or arr.shape != (H0, W0):
        raise ValueError("%s: a label image is 8-bit grey of the image's size %d x %d, got %s" % (path, H0, W0, arr.shape))
    return arr


# -------------------------------------------------------------------------------------------------------------------------------------- loader
def load_nerf_standard(root, split="train", mip=0, bg_color="white", device="cuda", num_workers=0, world_basis=BLENDER_TO_Y_UP, chunk_bytes=64 << 20,
                       use_kernel=True):
    """The split `split` of the NeRF-standard folder `root` -> DeviceMultiviewDataset on `device` with imgs, masks, rays, base_rays (shared) and the
    label modes of this package's label extension (module docstring), carrying view_matrices, image_shape, filenames, scale, semantic_info and
    `intrinsics` = dict(fx, fy, x0, y0) at the output size (what standard_cameras returned; the rays of further views are made from it).

    Frames are decoded on min(16, num_workers) threads (inline when num_workers <= 0) into one of two pinned uint8 staging buffers of at most
    chunk_bytes (one view when a view is larger), copied asynchronously and prepared on the device by one pag_prepare_views launch (and one
    pag_prepare_labels launch when there are labels) that writes into the final [V,h,w,...] tensors at the chunk's view offset.  A staging buffer is
    reused only after the event of its own copy has completed; nothing else waits for the device.  On a CPU device, or with use_kernel=False, the
    tensor-op forms of this module run instead, and give the same images, masks and labels bit for bit."""
    from .dataset import DeviceMultiviewDataset
    from .map_export import pinhole_base_rays
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if bg_color not in ("white", "black"):
        raise ValueError("load_nerf_standard: bg_color %r is neither 'white' nor 'black'" % (bg_color,))
    meta, frames = read_frames(root, split)
    V = len(frames)
    first = decode_image(frames[0]["path"])
    H0, W0 = first.shape[:2]
    C0 = 4 if first.ndim == 3 and first.shape[2] == 4 else 3
    f = _factor("load_nerf_standard", mip, H0, W0)
    mip, h, w = int(mip), H0 // f, W0 // f
    modes = [mode for _, mode in LABEL_KEYS if mode in frames[0]["labels"]]
    fx, fy, x0, y0, c2w, view_matrices = standard_cameras(dict(meta, frames=frames), w, h, mip, world_basis)

    cuda = device.type == "cuda"
    kernel = cuda and use_kernel
    img_bytes, plane_bytes = H0 * W0 * C0, H0 * W0
    view_bytes = img_bytes + plane_bytes * len(modes)
    per_chunk = max(1, min(V, MAX_CHUNK_VIEWS, int(chunk_bytes) // view_bytes))
    staging = [torch.empty(per_chunk * view_bytes, dtype=torch.uint8, pin_memory=cuda) for _ in range(2 if cuda else 1)]
    events = [None] * len(staging)
    pool = concurrent.futures.ThreadPoolExecutor(min(16, int(num_workers))) if num_workers > 0 else None

    with torch.cuda.device(device) if cuda else _nothing():
        imgs = torch.empty(V, h, w, 3, dtype=torch.float32, device=device)
        masks = torch.empty(V, h, w, 1, dtype=torch.bool, device=device)
        origins, dirs = torch.empty_like(imgs), torch.empty_like(imgs)
        labels = {mode: torch.empty(V, h, w, 1, dtype=torch.int64, device=device) for mode in modes}
        c2w_dev = c2w.to(device)
        on_device = torch.empty(per_chunk * view_bytes, dtype=torch.uint8, device=device) if cuda else None
        try:
            for k, off in enumerate(range(0, V, per_chunk)):
                n = min(per_chunk, V - off)
                slot = k % len(staging)
                if events[slot] is not None:
                    events[slot].synchronize()                  # the one wait: this buffer's own copy, two chunks ago
                host = staging[slot][:n * view_bytes]
                img_np = host[:n * img_bytes].view(n, H0, W0, C0).numpy()
                lab_np = [host[n * img_bytes + p * n * plane_bytes:n * img_bytes + (p + 1) * n * plane_bytes].view(n, H0, W0).numpy() for p in range(len(modes))]

                def decode(i, off=off, img_np=img_np, lab_np=lab_np):
                    fr = frames[off + i]
                    arr = first if off + i == 0 else decode_image(fr["path"])
                    img_np[i] = _as_channels(arr, C0, fr["path"], H0, W0)
                    for p, mode in enumerate(modes):
                        lab_np[p][i] = _label_plane(fr["labels"][mode], H0, W0)

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
                src = chunk[:n * img_bytes].view(n, H0, W0, C0)
                planes = [chunk[n * img_bytes + p * n * plane_bytes:n * img_bytes + (p + 1) * n * plane_bytes].view(n, H0, W0) for p in range(len(modes))]
                if kernel:
                    from . import ops
                    ops.prepare_views(src, mip, bg_color, off, imgs=imgs, masks=masks, origins=origins, dirs=dirs, c2w=c2w_dev, intrinsics=(fx, fy, x0, y0))
                    ops.prepare_labels([(planes[p], labels[mode]) for p, mode in enumerate(modes)], mip, off)
                else:
                    imgs[off:off + n], masks[off:off + n] = prepare_views_reference(src, mip, bg_color)
                    r = rays_reference(c2w_dev[off:off + n], w, h, fx, fy, x0, y0)
                    origins[off:off + n], dirs[off:off + n] = r.origins, r.dirs
                    for p, mode in enumerate(modes):
                        labels[mode][off:off + n] = prepare_labels_reference(planes[p], mip)
        finally:
            if pool is not None:
                pool.shutdown()
        data = dict(imgs=imgs, masks=masks, rays=Rays(origins, dirs, 0.0, DEFAULT_FAR), **labels)
        data["base_rays"] = pinhole_base_rays(w, h, fx, fy, x0, y0, device=device)
        ds = DeviceMultiviewDataset(data, device)
    ds.view_matrices = view_matrices
    ds.image_shape = (h, w)
    ds.filenames = [fr["basename"] for fr in frames]
    ds.scale = float(meta.get("scale", 1.0))
    ds.intrinsics = dict(fx=fx, fy=fy, x0=x0, y0=y0)
    if "num_classes" in meta:
        ds.semantic_info = dict(num_classes=int(meta["num_classes"]), num_instances=int(meta.get("num_instances", 0)),
                                things_ids=[int(v) for v in meta.get("things_ids", [])], stuff_ids=[int(v) for v in meta.get("stuff_ids", [])])
    return ds


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# ----------------------------------------------------------------------------------------------------------------------------------------- CLI
def dataset_arrays(ds):
    """The arrays of the .npz that train.load_npz_dataset reads (the layout in train.py's docstring) for a loaded dataset."""
    h, w = ds.image_shape
    out = {}
    for leaf in ds._leaves:
        a = leaf.src.cpu().numpy()
        out[leaf.key if leaf.field is None else "%s_%s" % (leaf.key, leaf.field)] = a.reshape((ds.num_imgs, h, w, -1) if leaf.per_view else (h, w, -1))
    for key, (lo, hi) in ds._rays_range.items():
        out[key + "_range"] = np.array([lo, hi], dtype=np.float32)
    out["view_matrices"] = ds.view_matrices.numpy()
    out["scale"] = np.float64(ds.scale)
    out["filenames"] = np.array(ds.filenames)
    info = getattr(ds, "semantic_info", None)
    if info is not None:
        out.update(num_classes=np.int64(info["num_classes"]), num_instances=np.int64(info["num_instances"]),
                   things_ids=np.array(info["things_ids"], dtype=np.int64), stuff_ids=np.array(info["stuff_ids"], dtype=np.int64))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m pagnerf_amd.formats", description="A NeRF-standard folder -> the .npz that python -m pagnerf_amd.train reads")
    ap.add_argument("root", help="the folder with transforms*.json")
    ap.add_argument("--split", default="train")
    ap.add_argument("--mip", type=int, default=0)
    ap.add_argument("--bg-color", default="white", choices=("white", "black"))
    ap.add_argument("--out", required=True, metavar="FILE.npz")
    ap.add_argument("--num-workers", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    ds = load_nerf_standard(args.root, split=args.split, mip=args.mip, bg_color=args.bg_color, device=args.device, num_workers=args.num_workers)
    with open(os.path.expanduser(args.out), "wb") as f:
        np.savez(f, **dataset_arrays(ds))
    return 0


if __name__ == "__main__":
    sys.exit(main())
