"""Panoptic point-cloud map export (utils/render_map.py; main_interactive.py:109-129 `--save-map-only` writes its result as nerf_pc.pkl).

Two exports, both streamed: a chunk of rays / lattice points is rendered or queried, reduced to its kept points by ONE ordered-append call
(csrc/map.hip: pag_map_points / pag_map_select - predicate, argmax, unprojection and compaction; no host synchronisation) and dropped.  The
reference keeps every chunk's full RenderBuffer until the end (`rb +=`, :43): at mip 0 on BUP20 shapes the [N, 200] instance buffer alone is 31 GB.

  from views   render_points_at_depth / generate_pc_map_from_views (:82-124, :172-183): every camera's image rendered at `mip`, rays kept by
               density / alpha / hit / depth thresholds, unprojected by the composited depth, labelled by the argmax of the instance channel.
  dense grid   get_dense_occupied_points / generate_pc_map (:46-79, :143-169): the 2^blas_level lattice, points whose density (queried at the
               shifted samples, see below) exceeds min_density, then those whose instance label is not 0.

Capacity policy: the accumulator is sized for the whole ray count / lattice sub-box (32 / 12 bytes per row), so it cannot overflow; a caller
short of memory passes `capacity=`, and an export that keeps more raises with the count it needed (the device counter keeps counting past
the capacity; nothing is written out of bounds).  One synchronisation at the end reads the counter and trims.

Quirks of the reference kept on purpose: `samples = points + (rand / res * 2 - 1)` shifts the query by about -1 instead of
jittering it inside a cell; the density is queried at the shifted samples and the UN-shifted lattice points are kept; `limits` is a strict box.
"""
import pickle

import numpy as np
import torch

from . import ops
from .core import Rays


def pinhole_base_rays(width, height, focal_x, focal_y, x0=0.0, y0=0.0, mip=0, device=None, dtype=torch.float32):
    """Camera-frame rays of one image at `mip` (:83-98: size // 2^mip, intrinsics / 2^mip, pixel centres, identity extrinsics) -> Rays [h*w], row-major
    (y slow).  wisp's generate_centered_pixel_coords / generate_pinhole_rays are third party (RECALLED from the public wisp / kaolin sources, PARITY
    UNPINNED):  px = x + 0.5, py = y + 0.5;  dir = normalise(((px - w/2 - x0) / fx, -(py - h/2 - y0) / fy, -1));  origin = 0.
    Every export below also takes ready-made base rays, so nothing pinned depends on this helper.  dtype: the precision it is evaluated in."""
    f = 2 ** mip
    w, h = int(width // f), int(height // f)
    fx, fy, cx, cy = focal_x / f, focal_y / f, x0 / f, y0 / f
    py, px = torch.meshgrid(torch.arange(h, dtype=dtype, device=device) + 0.5, torch.arange(w, dtype=dtype, device=device) + 0.5,
                            indexing="ij")
    d = torch.stack(((px - w / 2.0 - cx) / fx, -(py - h / 2.0 - cy) / fy, -torch.ones_like(px)), -1).reshape(-1, 3)
    d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    return Rays(torch.zeros_like(d), d)


class MapAccumulator:
    """The append target of the export kernels: points / color f32 [capacity,3], ids i64 [capacity] and the running device counter."""

    def __init__(self, capacity, device, color=True, ids=True):
        self.capacity = int(capacity)
        self.points = torch.empty(self.capacity, 3, device=device)
        self.color = torch.empty(self.capacity, 3, device=device) if color else None
        self.ids = torch.empty(self.capacity, dtype=torch.int64, device=device) if ids else None
        self.count = torch.zeros(1, dtype=torch.int64, device=device)

    def finish(self):
        """The one synchronisation: read the counter, -> (points, color, ids) trimmed to the kept rows."""
        k = int(self.count.item())
        if k > self.capacity:
            raise RuntimeError("map export kept %d points, the accumulator holds %d: pass capacity >= %d" % (k, self.capacity, k))
        return self.points[:k], (self.color[:k] if self.color is not None else None), (self.ids[:k] if self.ids is not None else None)


def _labels_of(labels, inst):
    """-> (inst, ids): the argmax runs in the kernel; a callable (e.g. a mean-shift NeF's predict_clusters) labels the rows itself."""
    if labels == "argmax":
        return inst.reshape(-1, inst.shape[-1]), None
    if not callable(labels):
        raise ValueError("labels must be 'argmax' or a callable f(inst_embedding [n, D]) -> int64 [n]")
    return None, labels(inst.reshape(-1, inst.shape[-1])).reshape(-1).to(torch.int64)


def map_points_from_buffers(pipeline, base_rays, rb, cam_ids, ray0=0, out=None, labels="argmax", min_density=40.0, min_alpha=0.9,
                            depth_range=(0.6, 0.8), channel="inst_embedding"):
    """:107-120 on one RenderBuffer of the rays [ray0, ray0 + n) of the images of `cam_ids` stacked camera after camera (base_rays: ONE image's
    camera-frame rays).  Appends to `out` (a MapAccumulator; made for n rows when None) and returns it; no host synchronisation."""
    idx = pipeline.camera_indices(cam_ids).int()
    n = rb.depth.shape[0]
    dev = rb.depth.device
    if out is None:
        out = MapAccumulator(n, dev)
    inst, ids = _labels_of(labels, getattr(rb, channel))
    ops.map_points(pipeline.camera_extrinsics, idx, base_rays.origins.shape[0], base_rays.origins.reshape(-1, 3).to(dev), base_rays.dirs.reshape(-1, 3).to(dev),
                   ray0, rb.depth, rb.alpha, rb.hit, rb.density, rb.rgb, out.points, out.color, out.ids, out.count, inst=inst, ids=ids,
                   min_density=min_density, min_alpha=min_alpha, depth_min=depth_range[0], depth_max=depth_range[1])
    return out


def _default_cam_ids(pipeline):
    if getattr(pipeline, "cam_id_to_idx", None) is not None:
        return list(pipeline.cam_id_to_idx.keys())                                        # :101
    return list(range(pipeline.camera_extrinsics.shape[0]))


@torch.no_grad()
def render_points_at_depth(pipeline, base_rays=None, intrinsics=None, mip=0, channels=("inst_embedding",), cam_ids=None, render_batch=20000,
                           labels="argmax", capacity=None, **thresholds):
    """:82-124.  base_rays: one image's camera-frame Rays, or intrinsics = dict(width, height, focal_x, focal_y[, x0, y0]) and `mip` for
    pinhole_base_rays.  The stacked rays of all cameras are never materialised: chunk by chunk (the reference's chunks: `render_batch` consecutive
    rays of the stack, across image borders) the rays are transformed, rendered with ['depth', 'density', 'rgb'] + channels, finalised and dropped -
    live memory is O(render_batch x I + kept points), and no host synchronisation is added to those the render itself has.
    -> {'points' f32 [K,3], 'inst_embedding' i64 [K], 'color' f32 [K,3]} on the device.  thresholds: min_density, min_alpha, depth_range."""
    if base_rays is None:
        base_rays = pinhole_base_rays(mip=mip, **intrinsics)
    dev = pipeline.camera_extrinsics.device
    cam_ids = _default_cam_ids(pipeline) if cam_ids is None else cam_ids
    idx = pipeline.camera_indices(cam_ids).int()
    oc, dc = base_rays.origins.reshape(-1, 3).to(dev).float().contiguous(), base_rays.dirs.reshape(-1, 3).to(dev).float().contiguous()
    rpc = oc.shape[0]
    total = rpc * idx.numel()
    out = MapAccumulator(total if capacity is None else capacity, dev)
    render_channels = ["depth", "density", "rgb"] + list(channels)                          # :104
    base = Rays(oc, dc)
    for s in range(0, total, render_batch):
        e = min(s + render_batch, total)
        g = torch.arange(s, e, device=dev)
        b = g % rpc
        rays = pipeline.transform_rays_indexed(oc.index_select(0, b), dc.index_select(0, b), idx.index_select(0, g // rpc))
        rb = pipeline(rays=rays, lod_idx=None, channels=render_channels)
        map_points_from_buffers(pipeline, base, rb, idx.long(), ray0=s, out=out, labels=labels, channel=channels[0], **thresholds)
        del rb, rays
    points, color, ids = out.finish()
    return {"points": points, "inst_embedding": ids, "color": color}


def generate_pc_map_from_views(pipeline, base_rays=None, name="nerf_pc", **kwargs):
    """:172-183 -> [{'points' f32 [K,3], 'inst_embedding' i64 [K], 'color' f32 [K,3], 'name'}] with CPU tensors (what nerf_pc.pkl holds)."""
    rendered = {k: v.detach().cpu() for k, v in render_points_at_depth(pipeline, base_rays, **kwargs).items()}
    rendered["name"] = name
    return [rendered]


def _lattice_box(blas_level, limits):
    """The lattice axis arange(res) / res * 2 - 1 and, per axis, the indices strictly inside `limits` [2,3] = [[min], [max]] (all of them without):
    the box is separable, so the kept sub-box and its size are known on the host."""
    res = 2.0 ** blas_level
    axis = torch.arange(res) / res * 2.0 - 1.0                                            # :56, f32
    if limits is None or torch.as_tensor(limits).numel() == 0:                            # :58
        return res, axis, [torch.arange(int(res))] * 3
    lim = torch.as_tensor(limits, dtype=torch.float32).cpu()
    return res, axis, [torch.nonzero((axis > lim[0, a]) & (axis < lim[1, a])).reshape(-1) for a in range(3)]      # :59-61


@torch.no_grad()
def get_dense_occupied_points(nef, blas_level, min_density=None, limits=None, noise=None, generator=None, render_batch=20000, capacity=None):
    """:46-79 as written -> f32 [K,3] lattice points (x slowest) on the nef's device.  noise: the `torch.rand(P, 3)` of :67 for the P points of the
    (limited) lattice, else drawn per chunk from `generator`.  The density is queried `render_batch` samples at a time."""
    if min_density is None:
        min_density = (0.01 * 512) / np.sqrt(3)                                           # :51-52
    dev = nef.device
    res, axis, keep = _lattice_box(blas_level, limits)
    ax = [axis[k].to(dev) for k in keep]
    nx, ny, nz = (int(k.numel()) for k in keep)
    P = nx * ny * nz
    out = MapAccumulator(P if capacity is None else capacity, dev, color=False, ids=False)
    if noise is not None and tuple(noise.shape) != (P, 3):
        raise ValueError("noise must be [%d, 3] (the points of the limited lattice), got %s" % (P, tuple(noise.shape)))
    for s in range(0, P, render_batch):
        e = min(s + render_batch, P)
        f = torch.arange(s, e, device=dev)
        points = torch.stack((ax[0][f // (ny * nz)], ax[1][(f // nz) % ny], ax[2][f % nz]), -1)
        r = noise[s:e].to(dev) if noise is not None else torch.rand(e - s, 3, device=dev, generator=generator)
        samples = points + (r / res * 2.0 - 1.0)                                          # :67-68: a shift of about -1, as written
        density = nef(coords=samples[:, None], ray_d=None, channels="density")           # :75
        ops.map_select(points, out.points, out.count, value=density.reshape(-1), threshold=min_density)      # :77-79
    return out.finish()[0]


@torch.no_grad()
def generate_pc_map(nef, blas_level, name="nerf_pc", min_density=None, limits=None, channels=("inst_embedding",), labels="argmax", noise=None,
                    generator=None, render_batch=20000):
    """:143-169 -> [{'name', 'points' f32 [K,3], 'instances' i64 [K]}] (CPU tensors): the occupied lattice points whose label is not 0."""
    points = get_dense_occupied_points(nef, blas_level, min_density, limits, noise=noise, generator=generator, render_batch=render_batch)
    P = points.shape[0]
    out = MapAccumulator(P, points.device, color=False)
    for s in range(0, P, render_batch):
        pts = points[s:s + render_batch]
        emb = nef(coords=pts[:, None], ray_d=None, channels=channels[0])                 # :150
        inst, ids = _labels_of(labels, emb)
        ops.map_select(pts, out.points, out.count, inst=inst, ids=ids, ids_out=out.ids)   # :160-165
    pts, _, ids = out.finish()
    return [{"name": name, "points": pts.detach().cpu(), "instances": ids.detach().cpu()}]


def save_map(data, path):
    """The reference's nerf_pc.pkl: a pickle of the list; a path ending in .ply instead gets a little-endian binary PLY of all entries' points
    (x y z float, red green blue uchar when colours exist, instance int)."""
    path = str(path)
    if not path.lower().endswith(".ply"):
        with open(path, "wb") as fh:
            pickle.dump(data, fh)
        return path
    pts = np.concatenate([np.asarray(d["points"], dtype="<f4").reshape(-1, 3) for d in data], 0)
    ids = np.concatenate([np.asarray(d["inst_embedding"] if "inst_embedding" in d else d["instances"]).reshape(-1) for d in data], 0)
    has_color = all("color" in d for d in data)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else []) + [("instance", "<i4")]
    v = np.empty(pts.shape[0], dtype=fields)
    v["x"], v["y"], v["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if has_color:
        col = np.concatenate([np.asarray(d["color"], dtype=np.float32).reshape(-1, 3) for d in data], 0)
        col = np.rint(np.clip(np.nan_to_num(col), 0.0, 1.0) * 255.0).astype(np.uint8)
        v["red"], v["green"], v["blue"] = col[:, 0], col[:, 1], col[:, 2]
    v["instance"] = ids.astype("<i4")
    names = {"<f4": "float", "u1": "uchar", "<i4": "int"}
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % pts.shape[0]
    header += "".join("property %s %s\n" % (names[t], n) for n, t in fields) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
    return path
