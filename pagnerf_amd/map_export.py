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

Beyond the reference: the FUSED VOXEL MAP (csrc/voxelmap.hip; second half of this file).  The views export holds a surface spot once per camera that
saw it, each with that view's own id; VoxelMap / fuse_map reduce such clouds to one row per occupied voxel (mean point and colour, the id most points
voted for, count, agreement), instance_table gives the per-instance table of the result, and `python -m pagnerf_amd.map_export fuse` does both on map
files.  fuse_points_reference / label_table_reference are the tensor-op definitions.  connected_components / clean_map / component_table split the
fused map into connected components of equal-id voxels on the device (floaters dropped, reused ids told apart); their *_reference forms define them.
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


# ------------------------------------------------------------------------------------------- the fused voxel map (csrc/voxelmap.hip)
# Every view contributes one point per kept pixel, labelled by that view's own argmax: a surface spot is in the cloud once per camera that saw it,
# with ids that need not agree.  The fused map has one row per occupied voxel of edge `voxel_size` on the lattice anchored at `origin`: the mean
# position and colour of the voxel's points, the id most of them carry (THE VOTE: every point one vote, the id with the most votes wins, on equal
# votes the smaller id), the number of points and the winner's share of them.  fuse_points_reference is the definition; VoxelMap is the device path.
VOXEL_AXIS_BITS = 21
DROPPED_KEY = 2 ** 63 - 1


def _reference_keys(points, voxel_size, origin, limits):
    """The voxel key of every row in tensor ops (fp32: subtract, divide, floor), DROPPED_KEY for a dropped row."""
    p = points.detach().reshape(-1, 3).float()
    o = torch.as_tensor(origin, dtype=torch.float32, device=p.device).reshape(3)
    v = torch.tensor(float(voxel_size), dtype=torch.float32, device=p.device)
    idx = torch.floor((p - o) / v)
    ok = (torch.isfinite(p) & (idx >= 0) & (idx < 2.0 ** VOXEL_AXIS_BITS)).all(-1)
    if limits is not None and torch.as_tensor(limits).numel() > 0:
        lim = torch.as_tensor(limits, dtype=torch.float32, device=p.device).reshape(2, 3)
        ok = ok & ((p > lim[0]) & (p < lim[1])).all(-1)                                   # the strict box of _lattice_box
    i = torch.where(ok[:, None], idx, torch.zeros_like(idx)).long()
    key = i[:, 2] | (i[:, 1] << VOXEL_AXIS_BITS) | (i[:, 0] << (2 * VOXEL_AXIS_BITS))
    return torch.where(ok, key, torch.full_like(key, DROPPED_KEY))


def _group_mean(values, inv, groups, counts):
    """fp64 sums per group cast to fp32, then one fp32 division by the count."""
    s = torch.zeros(groups, values.shape[1], dtype=torch.float64, device=values.device).index_add_(0, inv, values.double())
    return s.float() / counts.float()[:, None]


def _check_voxel_size(voxel_size):
    v = float(voxel_size)
    if not (v > 0.0 and np.isfinite(np.float32(v)) and np.float32(v) > 0):
        raise ValueError("voxel_size must be a positive finite number, got %r" % (voxel_size,))
    return v


@torch.no_grad()
def fuse_points_reference(points, ids, color=None, voxel_size=2.0 / 256, origin=None, limits=None, min_votes=1):
    """The fused voxel map as tensor ops - the definition (runs wherever its inputs live; sums in fp64).  points f32 [K,3], ids i64 [K], color f32
    [K,3] or None -> {'points' f32 [V,3], 'color' f32 [V,3] (with color), 'instances' i64 [V], 'count' i32 [V], 'agreement' f32 [V], 'voxels' i32
    [V,3], 'voxel_size', 'origin' f32 [3]} with one row per voxel that holds at least min_votes points, in ascending key order (x slowest)."""
    voxel_size = _check_voxel_size(voxel_size)
    origin = (-1.0, -1.0, -1.0) if origin is None else origin
    p = points.detach().reshape(-1, 3).float()
    dev = p.device
    ids = ids.detach().reshape(-1).to(torch.int64)
    keys = _reference_keys(p, voxel_size, origin, limits)
    valid = keys != DROPPED_KEY
    p, ids, keys = p[valid], ids[valid], keys[valid]
    ukeys, inv, cnt = torch.unique(keys, return_inverse=True, return_counts=True)
    V = ukeys.numel()
    out = {"points": _group_mean(p, inv, V, cnt)}
    if color is not None:
        out["color"] = _group_mean(color.detach().reshape(-1, 3).float()[valid], inv, V, cnt)
    # the vote: rows per (voxel, id) pair; unique sorts the pairs by voxel, then by id (signed), so the first pair that reaches a voxel's maximum
    # carries the smallest of the tied ids
    pairs, pc = torch.unique(torch.stack((inv, ids), 1), dim=0, return_counts=True)
    pv, pid = (pairs[:, 0], pairs[:, 1]) if pairs.numel() else (inv[:0], ids[:0])
    best = torch.zeros(V, dtype=torch.int64, device=dev).scatter_reduce_(0, pv, pc, "amax", include_self=False)
    pos = torch.arange(pv.numel(), device=dev)
    first = torch.full((V,), pv.numel(), dtype=torch.int64, device=dev).scatter_reduce_(
        0, pv[pc == best[pv]], pos[pc == best[pv]], "amin", include_self=True)
    out["instances"] = pid[first] if V else ids[:0]
    out["count"] = cnt.to(torch.int32)
    out["agreement"] = best.float() / cnt.float()
    out["voxels"] = torch.stack((ukeys >> (2 * VOXEL_AXIS_BITS), (ukeys >> VOXEL_AXIS_BITS) & (2 ** VOXEL_AXIS_BITS - 1),
                                 ukeys & (2 ** VOXEL_AXIS_BITS - 1)), 1).to(torch.int32)
    keep = cnt >= int(min_votes)
    out = {k: v[keep] for k, v in out.items()}
    out["voxel_size"] = voxel_size
    out["origin"] = torch.as_tensor(origin, dtype=torch.float32, device=dev).reshape(3)
    return out


def _with_volume(table, voxel_size):
    table["volume"] = table["voxels"].double() * float(voxel_size) ** 3
    return table


@torch.no_grad()
def label_table_reference(map, ignore=(0,)):
    """The per-instance table of a fused map as tensor ops - the definition.  -> {'ids' i64 [T], 'voxels' i64 [T], 'observations' i64 [T] (the sum of
    'count'), 'centroid' / 'bbox_min' / 'bbox_max' f32 [T,3] (of the voxel points), 'color' f32 [T,3] (when the map has colour), 'volume' f64 [T] =
    voxels * voxel_size^3}, one row per instance id outside `ignore`, ascending."""
    lab, p = map["instances"].reshape(-1), map["points"].reshape(-1, 3)
    ulab, inv, cnt = torch.unique(lab, return_inverse=True, return_counts=True)
    T = ulab.numel()
    out = {"ids": ulab, "voxels": cnt,
           "observations": torch.zeros(T, dtype=torch.int64, device=lab.device).index_add_(0, inv, map["count"].reshape(-1).long()),
           "centroid": _group_mean(p, inv, T, cnt)}
    idx = inv[:, None].expand(-1, 3)
    out["bbox_min"] = torch.zeros(T, 3, device=p.device).scatter_reduce_(0, idx, p, "amin", include_self=False)
    out["bbox_max"] = torch.zeros(T, 3, device=p.device).scatter_reduce_(0, idx, p, "amax", include_self=False)
    if "color" in map:
        out["color"] = _group_mean(map["color"].reshape(-1, 3), inv, T, cnt)
    keep = torch.ones(T, dtype=torch.bool, device=lab.device)
    for v in ignore:
        keep &= ulab != int(v)
    return _with_volume({k: v[keep] for k, v in out.items()}, map["voxel_size"])


def rows_by_key_and_id(keys, ids, points, color=None):
    """The rows in (key, id) order, rows of equal (key, id) in their given order: a stable sort by id, then a stable sort by key (rocPRIM's radix
    sort through torch.sort; no synchronisation).  -> (keys, ids, points, color) as pag_voxel_fuse takes them."""
    ids, first = torch.sort(ids, stable=True)
    keys, second = torch.sort(keys.index_select(0, first), stable=True)
    order = first.index_select(0, second)
    return keys, ids.index_select(0, second), points.index_select(0, order), (color.index_select(0, order) if color is not None else None)


class VoxelMap:
    """The device path of fuse_points_reference: add() collects chunks of map points (one key launch each, no synchronisation), finish() orders the
    rows by (key, id) with two stable sorts and reduces them in one ordered-append call; its one synchronisation reads the voxel counter.  The result
    does not depend on how the points were split over add() calls, bit for bit.  Outputs are sized for all K rows (52 bytes each) unless
    `capacity` says otherwise; a map of more voxels than that raises with the count it needed."""

    def __init__(self, voxel_size, origin=(-1.0, -1.0, -1.0), limits=None, min_votes=1, device="cuda", capacity=None):
        self.voxel_size = _check_voxel_size(voxel_size)
        self.origin = tuple(float(v) for v in origin)
        self.limits = None if limits is None or torch.as_tensor(limits).numel() == 0 else torch.as_tensor(limits, dtype=torch.float32).reshape(2, 3).cpu()
        self.min_votes = int(min_votes)
        if self.min_votes < 1:
            raise ValueError("min_votes must be at least 1")
        self.device = torch.device(device)
        self.capacity = capacity
        self._origin = torch.tensor(self.origin, dtype=torch.float32, device=self.device)      # made here: finish() copies nothing from the host
        self._chunks = []
        self._color = True

    def add(self, points, ids, color=None):
        points = points.detach().reshape(-1, 3).to(self.device, torch.float32)
        ids = ids.detach().reshape(-1).to(self.device, torch.int64)
        if ids.numel() != points.shape[0] or (color is not None and color.numel() != points.numel()):
            raise ValueError("add: points [k,3], ids [k] and color [k,3] must describe the same rows")
        if color is None:
            self._color = False
        if points.shape[0] == 0:
            return self
        color = color.detach().reshape(-1, 3).to(self.device, torch.float32) if color is not None else None
        self._chunks.append((points, ids, color, ops.voxel_keys(points, self.origin, self.voxel_size, self.limits)))
        return self

    def _empty(self, cap, color):
        dev = self.device
        out = {"points": torch.empty(cap, 3, device=dev)}
        if color:
            out["color"] = torch.empty(cap, 3, device=dev)
        out.update(instances=torch.empty(cap, dtype=torch.int64, device=dev), count=torch.empty(cap, dtype=torch.int32, device=dev),
                   agreement=torch.empty(cap, device=dev), voxels=torch.empty(cap, 3, dtype=torch.int32, device=dev))
        return out

    @torch.no_grad()
    def finish(self):
        K = sum(c[0].shape[0] for c in self._chunks)
        color = self._color and K > 0
        cap = K if self.capacity is None else min(int(self.capacity), K)
        out = self._empty(cap, self._color)
        n = 0
        if K > 0:
            cat = lambda j: self._chunks[0][j] if len(self._chunks) == 1 else torch.cat([c[j] for c in self._chunks])          # noqa: E731
            keys, ids, points, col = rows_by_key_and_id(cat(3), cat(1), cat(0), cat(2) if color else None)
            counter = torch.zeros(1, dtype=torch.int64, device=self.device)
            ops.voxel_fuse(keys, ids, points, col, self.min_votes, out["points"], out.get("color"), out["instances"], out["count"], out["agreement"],
                           out["voxels"], counter)
            n = int(counter.item())                                                         # the one synchronisation
            if n > cap:
                raise RuntimeError("the fused map has %d voxels, the outputs hold %d: pass capacity >= %d" % (n, cap, n))
        out = {k: v[:n] for k, v in out.items()}
        out["voxel_size"] = self.voxel_size
        out["origin"] = self._origin.clone()
        return out


def _entry_ids(d):
    return d["inst_embedding"] if "inst_embedding" in d else d["instances"]


def fuse_map(data, voxel_size, origin=(-1.0, -1.0, -1.0), limits=None, min_votes=1, device="cuda", capacity=None, name="nerf_pc_fused"):
    """The entries of a map list (what generate_pc_map_from_views / generate_pc_map return and nerf_pc.pkl holds: 'points', 'inst_embedding' or
    'instances', optionally 'color') fused into ONE entry with CPU tensors: fuse_points_reference's keys with 'name'.  Ids are taken as they are
    (matching the ids of different training windows is not done here).  device: where it runs; "cpu" is the tensor-op definition."""
    colored = all("color" in d for d in data)
    if torch.device(device).type == "cpu":
        pts = torch.cat([torch.as_tensor(d["points"]).reshape(-1, 3).float() for d in data]) if data else torch.zeros(0, 3)
        ids = torch.cat([torch.as_tensor(_entry_ids(d)).reshape(-1).long() for d in data]) if data else torch.zeros(0, dtype=torch.int64)
        col = torch.cat([torch.as_tensor(d["color"]).reshape(-1, 3).float() for d in data]) if data and colored else None
        fused = fuse_points_reference(pts, ids, col, voxel_size, origin, limits, min_votes)
    else:
        vm = VoxelMap(voxel_size, origin, limits, min_votes, device, capacity)
        for d in data:
            vm.add(torch.as_tensor(d["points"]), torch.as_tensor(_entry_ids(d)), torch.as_tensor(d["color"]) if colored else None)
        fused = vm.finish()
    fused = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in fused.items()}
    fused["name"] = name
    return fused


TABLE_FIELDS = ("ids", "voxels", "observations", "centroid", "bbox_min", "bbox_max", "color", "volume")


@torch.no_grad()
def instance_table(fused, ignore=(0,), device=None, capacity=None):
    """The per-instance table of a fused map (label_table_reference's keys): voxel count, observation total, centroid, bounding box, mean colour
    and volume of every instance id outside `ignore`.  Runs on `device` (default: where the map lives, "cuda" for a CPU map; "cpu" is the tensor-op
    definition): one stable sort by id and one ordered-append call, one synchronisation; the result lives where the map does."""
    home = fused["instances"].device
    dev = torch.device(device) if device is not None else (home if home.type != "cpu" else torch.device("cuda"))
    if dev.type == "cpu":
        cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in fused.items()}
        return {k: (v.to(home) if torch.is_tensor(v) else v) for k, v in label_table_reference(cpu, ignore).items()}
    n = fused["instances"].numel()
    cap = n if capacity is None else min(int(capacity), n)
    has_color = "color" in fused
    out = {"ids": torch.empty(cap, dtype=torch.int64, device=dev), "voxels": torch.empty(cap, dtype=torch.int64, device=dev),
           "observations": torch.empty(cap, dtype=torch.int64, device=dev), "centroid": torch.empty(cap, 3, device=dev),
           "bbox_min": torch.empty(cap, 3, device=dev), "bbox_max": torch.empty(cap, 3, device=dev)}
    if has_color:
        out["color"] = torch.empty(cap, 3, device=dev)
    t = 0
    if n > 0:
        lab, order = torch.sort(fused["instances"].reshape(-1).to(dev), stable=True)
        take = lambda k: fused[k].to(dev).index_select(0, order)                           # noqa: E731
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        ops.label_table(lab, take("points"), take("color") if has_color else None, take("count"), ignore, out["ids"], out["voxels"],
                        out["observations"], out["centroid"], out["bbox_min"], out["bbox_max"], out.get("color"), counter)
        t = int(counter.item())
        if t > cap:
            raise RuntimeError("the table has %d instances, the outputs hold %d: pass capacity >= %d" % (t, cap, t))
    return _with_volume({k: v[:t].to(home) for k, v in out.items()}, fused["voxel_size"])


# ------------------------------------------------------------------------------------------- connected components of the fused map
# An instance id of the fused map is one object only if its voxels are one blob: a few mislabelled voxels far away stretch its box, and the instance
# head may give one id to two distant objects.  The components of equal-id voxels on the lattice separate these: connected_components_reference is
# the definition, connected_components the device path (pag_voxel_components), clean_map drops small components and keeps or splits the rest.
CONNECTIVITIES = {6: 1, 18: 2, 26: 3}                      # neighbours -> the most non-zero components of a neighbour offset
CLEAN_MODES = ("keep", "largest", "split")
MAX_IGNORE = 8
ROW_FIELDS = ("points", "color", "instances", "count", "agreement", "voxels", "component")
_STATUS_TEXT = ((1, "the rows do not ascend strictly by voxel key"), (2, "a voxel index lies outside [0, 2^21)"),
                (4, "a union-find walk exceeded its cap of V + 1 rounds"))


def _check_components_args(connectivity, ignore):
    if connectivity not in CONNECTIVITIES:
        raise ValueError("connectivity must be 6, 18 or 26, got %r" % (connectivity,))
    ignore = tuple(int(v) for v in ignore)
    if len(ignore) > MAX_IGNORE:
        raise ValueError("at most %d ignored ids, got %d" % (MAX_IGNORE, len(ignore)))
    return ignore


def _raise_status(status):
    raise ValueError("connected_components: " + "; ".join(text for bit, text in _STATUS_TEXT if status & bit))


@torch.no_grad()
def connected_components_reference(fused, connectivity=26, same_id=True, ignore=(0,)):
    """The connected components of a fused map - the definition (NumPy on the CPU).  Reads 'voxels' i32 [V,3] (rows strictly ascending by key iz | iy
    << 21 | ix << 42, else ValueError) and 'instances' i64 [V].  Rows whose id is in `ignore` get component 0 and link nothing; two other rows are
    linked when their voxel indices differ by an offset of the neighbourhood (6: faces, 18: and edges, 26: and corners) and - same_id - their ids
    are equal; an index outside [0, 2^21) does not exist.  Components are the transitive closure, numbered 1 .. C by their first row.
    -> {'component' i64 [V], 'components' C}."""
    import itertools
    ignore = _check_components_args(connectivity, ignore)
    vox = np.asarray(torch.as_tensor(fused["voxels"]).cpu()).reshape(-1, 3).astype(np.int64)
    ids = np.asarray(torch.as_tensor(fused["instances"]).cpu()).reshape(-1).astype(np.int64)
    V, lim = ids.shape[0], 2 ** VOXEL_AXIS_BITS
    if vox.shape[0] != V:
        raise ValueError("connected_components: voxels [V,3] and instances [V] must describe the same rows")
    pack = lambda v: v[:, 2] | (v[:, 1] << VOXEL_AXIS_BITS) | (v[:, 0] << (2 * VOXEL_AXIS_BITS))       # noqa: E731
    status = 2 * int(((vox < 0) | (vox >= lim)).any())
    keys = pack(vox)
    status |= int(status == 0 and bool((keys[1:] <= keys[:-1]).any()))
    if status:
        _raise_status(status)
    if V == 0:
        return {"component": torch.zeros(0, dtype=torch.int64), "components": 0}
    live = ~np.isin(ids, np.asarray(ignore, np.int64))
    rows = np.nonzero(live)[0]
    most = CONNECTIVITIES[connectivity]
    ea, eb = [], []
    for off in itertools.product((-1, 0, 1), repeat=3):
        if not off < (0, 0, 0) or sum(o != 0 for o in off) > most:                         # the forward half: every pair of neighbours once
            continue
        nb = vox[rows] + np.asarray(off, np.int64)
        ok = ((nb >= 0) & (nb < lim)).all(1)                                               # per axis: the key arithmetic never borrows
        src, want = rows[ok], pack(nb[ok])
        at = np.minimum(np.searchsorted(keys, want), V - 1)
        hit = (keys[at] == want) & live[at]
        if same_id:
            hit &= ids[at] == ids[src]
        ea.append(src[hit])
        eb.append(at[hit])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    parent = np.arange(V)
    while True:                                                                            # smallest-row propagation: hook the roots, flatten, repeat
        ra, rb = parent[ea], parent[eb]
        if np.array_equal(ra, rb):
            break
        low = np.minimum(ra, rb)
        np.minimum.at(parent, ra, low)
        np.minimum.at(parent, rb, low)
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    is_root = live & (parent == np.arange(V))                                              # a component's root is its first row
    number = np.cumsum(is_root)
    component = np.where(live, number[parent], 0).astype(np.int64)
    return {"component": torch.from_numpy(component), "components": int(is_root.sum())}


@torch.no_grad()
def connected_components(fused, connectivity=26, same_id=True, ignore=(0,), device=None):
    """connected_components_reference on the device (pag_voxel_components: a lock-free union-find over the sorted rows and an ordered append over the
    roots) -> {'component' i64 [V] where the map lives, 'components' C}.  Runs on `device` (default: where the map lives, "cuda" for a CPU map;
    "cpu" selects the definition).  One synchronisation: the read of the count and the status word; a map that breaks the contract raises ValueError."""
    ignore = _check_components_args(connectivity, ignore)
    home = torch.as_tensor(fused["instances"]).device
    dev = torch.device(device) if device is not None else (home if home.type != "cpu" else torch.device("cuda"))
    if dev.type == "cpu":
        out = connected_components_reference(fused, connectivity, same_id, ignore)
        return {"component": out["component"].to(home), "components": out["components"]}
    ids = torch.as_tensor(fused["instances"]).reshape(-1).to(dev, torch.int64)
    vox = torch.as_tensor(fused["voxels"]).reshape(-1, 3).to(dev, torch.int32)
    if vox.shape[0] != ids.numel():
        raise ValueError("connected_components: voxels [V,3] and instances [V] must describe the same rows")
    component = torch.empty(ids.numel(), dtype=torch.int64, device=dev)
    count_status = torch.empty(2, dtype=torch.int64, device=dev)
    ops.voxel_components(vox, ids, connectivity, same_id, ignore, component, count_status)
    count, status = count_status.tolist()                                                  # the one synchronisation
    if status:
        _raise_status(status)
    return {"component": component.to(home), "components": int(count)}


def _clean_args(min_voxels, mode):
    if mode not in CLEAN_MODES:
        raise ValueError("mode must be one of %s, got %r" % (", ".join(CLEAN_MODES), mode))
    if int(min_voxels) < 1:
        raise ValueError("min_voxels must be at least 1")
    return int(min_voxels)


@torch.no_grad()
def clean_map_reference(fused, min_voxels=1, connectivity=26, mode="keep", ignore=(0,)):
    """clean_map on the CPU, row by row - the definition."""
    min_voxels = _clean_args(min_voxels, mode)
    cc = connected_components_reference(fused, connectivity, True, ignore)
    comp, C = cc["component"].numpy(), cc["components"]
    ids = np.asarray(torch.as_tensor(fused["instances"]).cpu()).reshape(-1).astype(np.int64)
    size = np.bincount(comp, minlength=C + 1)
    cid = {}
    for r in range(ids.shape[0]):
        cid.setdefault(int(comp[r]), int(ids[r]))
    alive = [c for c in range(1, C + 1) if size[c] >= min_voxels]
    winner = {}
    for c in alive:                                                                        # per id the most voxels; ascending c: a tie stays with the smaller number
        if cid[c] not in winner or size[c] > size[winner[cid[c]]]:
            winner[cid[c]] = c
    if mode == "largest":
        alive = [c for c in alive if winner[cid[c]] == c]
    new_id = dict(cid)
    if mode == "split":
        nxt = max(int(ids.max()) if ids.size else 0, 0)
        for c in alive:
            if winner[cid[c]] != c:
                nxt += 1
                new_id[c] = nxt
    number = {c: k + 1 for k, c in enumerate(alive)}
    rows = [r for r in range(ids.shape[0]) if comp[r] == 0 or int(comp[r]) in number]
    idx = torch.tensor(rows, dtype=torch.int64)
    out = {k: (torch.as_tensor(v).cpu().index_select(0, idx) if k in ROW_FIELDS else v) for k, v in fused.items()}
    out["instances"] = torch.tensor([int(ids[r]) if comp[r] == 0 else new_id[int(comp[r])] for r in rows], dtype=torch.int64)
    out["component"] = torch.tensor([number.get(int(comp[r]), 0) for r in rows], dtype=torch.int64)
    return out


@torch.no_grad()
def clean_map(fused, min_voxels=1, connectivity=26, mode="keep", ignore=(0,), device=None):
    """A fused map without its floaters, its reused ids told apart: the map's keys plus 'component' i64 [V'], rows still ascending by key.
      1  the components of equal-id voxels (connected_components, same_id)
      2  every row whose component has fewer than min_voxels voxels is dropped; rows with an ignored id never are
      3  mode "keep": ids stay; "largest": per id only the surviving component with the most voxels stays (equal sizes: the smaller component
         number); "split": that component keeps the id, every other surviving component becomes a new instance max(ids of the input, 0) + 1, + 2,
         ... in ascending component number
      4  'component' of the surviving rows is renumbered densely in the same order
    Steps 2 - 4 are tensor ops on C-length tables and one row mask.  Two synchronisations: the component count and the kept rows.  Rows are
    selected, never recomputed.  device as in connected_components ("cpu": clean_map_reference); the result lives where the map does."""
    min_voxels = _clean_args(min_voxels, mode)
    ignore = _check_components_args(connectivity, ignore)
    home = torch.as_tensor(fused["instances"]).device
    dev = torch.device(device) if device is not None else (home if home.type != "cpu" else torch.device("cuda"))
    if dev.type == "cpu":
        cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in fused.items()}
        return {k: (v.to(home) if torch.is_tensor(v) else v) for k, v in clean_map_reference(cpu, min_voxels, connectivity, mode, ignore).items()}
    on_dev = {k: (torch.as_tensor(v).to(dev) if k in ROW_FIELDS else v) for k, v in fused.items()}
    cc = connected_components(on_dev, connectivity, True, ignore, dev)                      # synchronisation 1
    comp, C = cc["component"], cc["components"]
    ids = on_dev["instances"].reshape(-1).to(torch.int64)
    if ids.numel() == 0:
        return dict(fused, component=comp.to(home))
    size = torch.zeros(C + 1, dtype=torch.int64, device=dev).index_add_(0, comp, torch.ones_like(comp))
    cid = torch.zeros(C + 1, dtype=torch.int64, device=dev).scatter_(0, comp, ids)          # one id per component: every row writes the same value
    real = torch.arange(C + 1, device=dev) > 0                                             # entry 0 stands for the ignored rows
    keep = (size >= min_voxels) | ~real
    new_ids = ids
    if mode != "keep" and C > 0:
        # the components ordered by (id, voxels descending, number): two stable sorts; dropped components count as -1 voxels
        _, by_size = torch.sort(torch.where(keep, size, torch.full_like(size, -1))[1:], descending=True, stable=True)
        sorted_id, by_id = torch.sort(cid[1:].index_select(0, by_size), stable=True)
        order = by_size.index_select(0, by_id) + 1
        first = torch.ones(C, dtype=torch.bool, device=dev)
        first[1:] = sorted_id[1:] != sorted_id[:-1]
        winner = torch.zeros(C + 1, dtype=torch.bool, device=dev).index_put_((order,), first) & keep
        if mode == "largest":
            keep = keep & (winner | ~real)
        else:
            extra = keep & ~winner & real
            fresh = ids.max().clamp_min(0) + torch.cumsum(extra.long(), 0)
            new_ids = torch.where(comp > 0, torch.where(extra, fresh, cid).index_select(0, comp), ids)
    kept = keep & real
    number = torch.cumsum(kept.long(), 0) * kept.long()
    rows = torch.nonzero(keep.index_select(0, comp)).reshape(-1)                            # synchronisation 2
    on_dev["instances"], on_dev["component"] = new_ids, number.index_select(0, comp)
    out = {k: (on_dev[k].index_select(0, rows).to(home) if k in ROW_FIELDS else v) for k, v in on_dev.items()}
    return out


@torch.no_grad()
def component_table(fused, device=None, capacity=None):
    """instance_table over the labels 'component' of a map that has them (clean_map's result, or a map with connected_components' 'component' added):
    one row per component other than 0, 'ids' the component number, and a column 'instance' i64 [T] with the id of the component's first row."""
    if "component" not in fused:
        raise ValueError("component_table needs a map with 'component' (clean_map, or connected_components' result added to the map)")
    comp = torch.as_tensor(fused["component"]).reshape(-1).to(torch.int64)
    table = instance_table(dict(fused, instances=comp), ignore=(0,), device=device, capacity=capacity)
    V = comp.numel()
    ids = torch.as_tensor(fused["instances"]).reshape(-1).to(comp.device, torch.int64)
    first_row = torch.full((V + 1,), max(V - 1, 0), dtype=torch.int64, device=comp.device).scatter_reduce_(
        0, comp, torch.arange(V, device=comp.device), "amin", include_self=True)
    where = table["ids"].to(comp.device)
    table["instance"] = (ids.index_select(0, first_row.index_select(0, where)) if V else ids[:0]).to(table["ids"].device)
    return table


def save_instance_table(table, path):
    """One header line, one line per instance: id, voxels, observations, volume, centroid, bounding box and (when present) colour; floats are
    written with repr, so reading them back gives the same values.  A component table (component_table) has the column `instance` after `id`."""
    import csv
    cols = [("id", "ids", None)] + ([("instance", "instance", None)] if "instance" in table else [])
    cols += [("voxels", "voxels", None), ("observations", "observations", None), ("volume", "volume", None)]
    for key, stem in (("centroid", "centroid"), ("bbox_min", "min"), ("bbox_max", "max")):
        cols += [("%s_%s" % (stem, a), key, j) for j, a in enumerate("xyz")]
    if "color" in table:
        cols += [(c, "color", j) for j, c in enumerate(("red", "green", "blue"))]
    arrays = {k: np.asarray(torch.as_tensor(table[k]).cpu()) for _, k, _ in cols}
    with open(str(path), "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow([c for c, _, _ in cols])
        for r in range(arrays["ids"].shape[0]):
            row = [arrays[k][r] if j is None else arrays[k][r, j] for _, k, j in cols]
            w.writerow([repr(v.item()) for v in row])
    return str(path)


def save_map(data, path):
    """The reference's nerf_pc.pkl: a pickle of the list; a path ending in .ply instead gets a little-endian binary PLY of all entries' points
    (x y z float, red green blue uchar when colours exist, instance int; count int and agreement float when every entry is a fused map; component
    int when every entry has component labels)."""
    path = str(path)
    if not path.lower().endswith(".ply"):
        with open(path, "wb") as fh:
            pickle.dump(data, fh)
        return path
    pts = np.concatenate([np.asarray(d["points"], dtype="<f4").reshape(-1, 3) for d in data], 0)
    ids = np.concatenate([np.asarray(d["inst_embedding"] if "inst_embedding" in d else d["instances"]).reshape(-1) for d in data], 0)
    has_color = all("color" in d for d in data)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else []) + [("instance", "<i4")]
    fused = len(data) > 0 and all("count" in d for d in data)
    if fused:
        fields += [("count", "<i4"), ("agreement", "<f4")]
    labelled = len(data) > 0 and all("component" in d for d in data)
    if labelled:
        fields += [("component", "<i4")]
    v = np.empty(pts.shape[0], dtype=fields)
    if labelled:
        v["component"] = np.concatenate([np.asarray(d["component"]).reshape(-1) for d in data], 0).astype("<i4")
    if fused:
        v["count"] = np.concatenate([np.asarray(d["count"]).reshape(-1) for d in data], 0).astype("<i4")
        v["agreement"] = np.concatenate([np.asarray(d["agreement"], dtype="<f4").reshape(-1) for d in data], 0)
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


def main(argv=None):
    """python -m pagnerf_amd.map_export fuse IN.pkl [IN.pkl ...] --voxel-size V [--min-votes N] [--limits x0 y0 z0 x1 y1 z1] --out OUT.ply|OUT.pkl
    [--table OUT.csv] [--min-component N] [--connectivity 6|18|26] [--split keep|largest|split]"""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m pagnerf_amd.map_export")
    sub = ap.add_subparsers(dest="command", required=True)
    fu = sub.add_parser("fuse", help="fuse exported map files into one voxel map",
                        description="Fuses the point clouds of map files (what --save-map and the reference's --save-map-only write: a pickled list of "
                        "dicts with 'points', 'inst_embedding' or 'instances' and optionally 'color') into one voxel map: per occupied voxel the mean "
                        "point and colour, the instance id most points voted for (ties: the smaller id), the point count and the agreement.  Ids are "
                        "taken as they are.  The inputs are pickles: unpickling runs code, so give it files you trust and nothing else.")
    fu.add_argument("inputs", nargs="+", metavar="IN.pkl", help="map files (pickles: trusted files only)")
    fu.add_argument("--voxel-size", type=float, required=True, metavar="V", help="voxel edge in the map's units (the scene cube is [-1, 1]^3)")
    fu.add_argument("--min-votes", type=int, default=1, metavar="N", help="drop voxels that hold fewer than N points")
    fu.add_argument("--limits", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="keep points strictly inside this box")
    fu.add_argument("--origin", type=float, nargs=3, default=(-1.0, -1.0, -1.0), metavar=("X", "Y", "Z"), help="corner the voxel lattice is anchored at")
    fu.add_argument("--ignore", type=int, nargs="*", default=[0], metavar="ID", help="instance ids left out of the table (default: 0)")
    fu.add_argument("--out", required=True, metavar="OUT.ply|OUT.pkl", help="the fused map (a .ply, or a pickle of a one-entry list)")
    fu.add_argument("--table", metavar="OUT.csv", help="also write the per-instance table")
    fu.add_argument("--device", default="cuda", help="where it runs; cpu selects the tensor-op definition")
    fu.add_argument("--min-component", type=int, metavar="N", help="clean the fused map: drop connected components of equal-id voxels that have fewer than "
                    "N voxels (ids of --ignore are left alone); the map gets a component label per voxel and --table becomes the per-component table")
    fu.add_argument("--connectivity", type=int, choices=sorted(CONNECTIVITIES), metavar="6|18|26", help="neighbourhood of the components (default 26)")
    fu.add_argument("--split", choices=CLEAN_MODES, metavar="keep|largest|split", help="an id with several components: keep them (default), keep only the "
                    "largest, or make every further component a new instance")
    args = ap.parse_args(argv)
    data = []
    for path in args.inputs:
        with open(path, "rb") as fh:
            loaded = pickle.load(fh)
        data += loaded if isinstance(loaded, (list, tuple)) else [loaded]
    limits = None if args.limits is None else [args.limits[:3], args.limits[3:]]
    fused = fuse_map(data, args.voxel_size, origin=args.origin, limits=limits, min_votes=args.min_votes, device=args.device)
    clean = args.min_component is not None or args.connectivity is not None or args.split is not None
    if clean:
        fused = clean_map(fused, min_voxels=args.min_component or 1, connectivity=args.connectivity or 26, mode=args.split or "keep",
                          ignore=args.ignore, device=args.device)
    save_map([fused], args.out)
    if args.table:
        table = component_table(fused, device=args.device) if clean else instance_table(fused, ignore=args.ignore, device=args.device)
        save_instance_table(table, args.table)
    print("%d points -> %d voxels: %s" % (sum(int(torch.as_tensor(d["points"]).reshape(-1, 3).shape[0]) for d in data), fused["points"].shape[0], args.out))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
