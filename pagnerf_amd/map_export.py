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
overlap_table / associate_maps / merge_maps / merge_map_sequence match the ids of different training windows' maps by voxel overlap and merge the
maps (`python -m pagnerf_amd.map_export merge`); again the *_reference forms are the definitions.
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


def _home_and_device(a, device):
    """Where map `a` lives, and where a call runs: `device`, else where the map lives, "cuda" for a CPU map."""
    home = torch.as_tensor(a["instances"]).device
    return home, (torch.device(device) if device is not None else (home if home.type != "cpu" else torch.device("cuda")))


def _cpu_map(m):
    return {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in m.items()}


def _to_home(out, home):
    return {k: (v.to(home) if torch.is_tensor(v) else v) for k, v in out.items()}


def _trim(counter, cap, what, cols):
    """The end of an ordered append into columns of `cap` rows: the kept rows (the device counter i64 [1], read here - a synchronisation - or a number
    the caller has read already) -> the columns cut to them.  More rows than fit raises with the capacity it needed; `what` is the caller's
    '... %d ..., ... hold %d' half of the message."""
    k = int(counter.item()) if torch.is_tensor(counter) else int(counter)
    if k > cap:
        raise RuntimeError((what + ": pass capacity >= %d") % (k, cap, k))
    return {name: (v[:k] if v is not None else None) for name, v in cols.items()}


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
        cols = {"points": self.points, "color": self.color, "ids": self.ids}
        return tuple(_trim(self.count, self.capacity, "map export kept %d points, the accumulator holds %d", cols).values())


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

    def add(self, points, ids, color=None, scale=None, offset=None):
        """scale / offset[3]: the chunk's frame; p * scale + offset (fp32: one multiplication, one addition) is what gets keyed and averaged."""
        points = _to_frame(points.detach().reshape(-1, 3).to(self.device, torch.float32), scale, offset)
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
        counter = 0
        if K > 0:
            cat = lambda j: self._chunks[0][j] if len(self._chunks) == 1 else torch.cat([c[j] for c in self._chunks])          # noqa: E731
            keys, ids, points, col = rows_by_key_and_id(cat(3), cat(1), cat(0), cat(2) if color else None)
            counter = torch.zeros(1, dtype=torch.int64, device=self.device)
            ops.voxel_fuse(keys, ids, points, col, self.min_votes, out["points"], out.get("color"), out["instances"], out["count"], out["agreement"],
                           out["voxels"], counter)
        out = _trim(counter, cap, "the fused map has %d voxels, the outputs hold %d", out)     # the one synchronisation
        out["voxel_size"] = self.voxel_size
        out["origin"] = self._origin.clone()
        return out


def _to_frame(points, scale, offset):
    """p * scale + offset in fp32 tensor ops, a multiplication and an addition (no contraction: two launches); the points as they are with both None."""
    if scale is None and offset is None:
        return points
    s = torch.tensor(1.0 if scale is None else float(scale), dtype=torch.float32, device=points.device)
    o = torch.as_tensor((0.0, 0.0, 0.0) if offset is None else offset, dtype=torch.float32).reshape(3).to(points.device)
    return points * s + o


def _entry_ids(d):
    return d["inst_embedding"] if "inst_embedding" in d else d["instances"]


def fuse_map(data, voxel_size, origin=(-1.0, -1.0, -1.0), limits=None, min_votes=1, device="cuda", capacity=None, name="nerf_pc_fused", frames=None):
    """The entries of a map list (what generate_pc_map_from_views / generate_pc_map return and nerf_pc.pkl holds: 'points', 'inst_embedding' or
    'instances', optionally 'color') fused into ONE entry with CPU tensors: fuse_points_reference's keys with 'name'.  Ids are taken as they are:
    the entries must share one numbering (the views of ONE training window do).  Maps of different windows are fused one by one and then joined by
    merge_maps / merge_map_sequence, which match their ids by voxel overlap.  frames: one (scale, offset[3]) per entry, p * scale + offset in fp32
    before the points are keyed (separately normalised windows brought into one frame); None: the points as they are.  device: where it runs;
    "cpu" is the tensor-op definition."""
    colored = all("color" in d for d in data)
    if frames is not None and len(frames) != len(data):
        raise ValueError("frames: one (scale, offset) per entry, got %d for %d entries" % (len(frames), len(data)))
    frames = [(None, None)] * len(data) if frames is None else frames
    if torch.device(device).type == "cpu":
        pts = torch.cat([_to_frame(torch.as_tensor(d["points"]).reshape(-1, 3).float(), *f) for d, f in zip(data, frames)]) if data else torch.zeros(0, 3)
        ids = torch.cat([torch.as_tensor(_entry_ids(d)).reshape(-1).long() for d in data]) if data else torch.zeros(0, dtype=torch.int64)
        col = torch.cat([torch.as_tensor(d["color"]).reshape(-1, 3).float() for d in data]) if data and colored else None
        fused = fuse_points_reference(pts, ids, col, voxel_size, origin, limits, min_votes)
    else:
        vm = VoxelMap(voxel_size, origin, limits, min_votes, device, capacity)
        for d, f in zip(data, frames):
            vm.add(torch.as_tensor(d["points"]), torch.as_tensor(_entry_ids(d)), torch.as_tensor(d["color"]) if colored else None, *f)
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
    home, dev = _home_and_device(fused, device)
    if dev.type == "cpu":
        return _to_home(label_table_reference(_cpu_map(fused), ignore), home)
    n = fused["instances"].numel()
    cap = n if capacity is None else min(int(capacity), n)
    has_color = "color" in fused
    out = {"ids": torch.empty(cap, dtype=torch.int64, device=dev), "voxels": torch.empty(cap, dtype=torch.int64, device=dev),
           "observations": torch.empty(cap, dtype=torch.int64, device=dev), "centroid": torch.empty(cap, 3, device=dev),
           "bbox_min": torch.empty(cap, 3, device=dev), "bbox_max": torch.empty(cap, 3, device=dev)}
    if has_color:
        out["color"] = torch.empty(cap, 3, device=dev)
    counter = 0
    if n > 0:
        lab, order = torch.sort(fused["instances"].reshape(-1).to(dev), stable=True)
        take = lambda k: fused[k].to(dev).index_select(0, order)                           # noqa: E731
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        ops.label_table(lab, take("points"), take("color") if has_color else None, take("count"), ignore, out["ids"], out["voxels"],
                        out["observations"], out["centroid"], out["bbox_min"], out["bbox_max"], out.get("color"), counter)
    out = _trim(counter, cap, "the table has %d instances, the outputs hold %d", out)
    return _with_volume(_to_home(out, home), fused["voxel_size"])


# ------------------------------------------------------------------------------------------- connected components of the fused map
# An instance id of the fused map is one object only if its voxels are one blob: a few mislabelled voxels far away stretch its box, and the instance
# head may give one id to two distant objects.  The components of equal-id voxels on the lattice separate these: connected_components_reference is
# the definition, connected_components the device path (pag_voxel_components), clean_map drops small components and keeps or splits the rest.
CONNECTIVITIES = {6: 1, 18: 2, 26: 3}                      # neighbours -> the most non-zero components of a neighbour offset
CLEAN_MODES = ("keep", "largest", "split")
MAX_IGNORE = 8
ROW_FIELDS = ("points", "color", "instances", "count", "agreement", "voxels", "component")
_STATUS_TEXT = ((1, "the rows do not ascend strictly by voxel key"), (2, "a voxel index lies outside [0, 2^21)"),
                (4, "a union-find walk exceeded its cap of V + 1 rounds"), (8, "an id is missing from the map's id list"),
                (16, "a voxel key occurs more than once in a map"))


def _check_components_args(connectivity, ignore):
    if connectivity not in CONNECTIVITIES:
        raise ValueError("connectivity must be 6, 18 or 26, got %r" % (connectivity,))
    ignore = tuple(int(v) for v in ignore)
    if len(ignore) > MAX_IGNORE:
        raise ValueError("at most %d ignored ids, got %d" % (MAX_IGNORE, len(ignore)))
    return ignore


def _raise_status(status, what="connected_components"):
    raise ValueError(what + ": " + "; ".join(text for bit, text in _STATUS_TEXT if status & bit))


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
    home, dev = _home_and_device(fused, device)
    if dev.type == "cpu":
        return _to_home(connected_components_reference(fused, connectivity, same_id, ignore), home)
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
    home, dev = _home_and_device(fused, device)
    if dev.type == "cpu":
        return _to_home(clean_map_reference(_cpu_map(fused), min_voxels, connectivity, mode, ignore), home)
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


# ------------------------------------------------------------------------------------------- ids across maps: overlap, association, merge
# Every training window has its own instance head, so the ids of two windows' maps are unrelated while the windows overlap in space.  Two fused
# maps on ONE lattice (equal float32(voxel_size), equal origin) are joined by voxel key: overlap_table counts the shared voxels per pair of ids,
# associate_maps matches the ids one to one by the IoU over the CO-OCCUPIED voxels (an instance cut by the window border is not punished for the
# part the other window never saw) with the Hungarian step, merge_maps relabels the second map and unites the rows.  The *_reference forms (NumPy
# on the CPU) are the definitions; the device path is pag_voxel_overlap / pag_overlap_cost / pag_assign_solve / pag_voxel_merge.
MAX_DEVICE_MATCH = 256                                     # active ids per side pag_assign_solve takes


def _np(t, dtype):
    return np.asarray(torch.as_tensor(t).detach().cpu()).astype(dtype)


def _check_same_lattice(a, b, what):
    if np.float32(a["voxel_size"]) != np.float32(b["voxel_size"]):
        raise ValueError("%s: the maps have different voxel_size (%r, %r): they must lie on one lattice" % (what, a["voxel_size"], b["voxel_size"]))
    oa, ob = _np(a["origin"], np.float32).reshape(-1), _np(b["origin"], np.float32).reshape(-1)
    if oa.shape != (3,) or ob.shape != (3,) or not np.array_equal(oa, ob):
        raise ValueError("%s: the maps have different origin (%s, %s): they must lie on one lattice" % (what, oa.tolist(), ob.tolist()))


def _checked_keys(m, what):
    """-> (keys i64 [V], ids i64 [V]) of a fused map, the contract checked with connected_components' status bits and wording."""
    vox, ids = _np(m["voxels"], np.int64).reshape(-1, 3), _np(m["instances"], np.int64).reshape(-1)
    if vox.shape[0] != ids.shape[0]:
        raise ValueError("%s: voxels [V,3] and instances [V] must describe the same rows" % what)
    status = 2 * int(((vox < 0) | (vox >= 2 ** VOXEL_AXIS_BITS)).any())
    keys = vox[:, 2] | (vox[:, 1] << VOXEL_AXIS_BITS) | (vox[:, 0] << (2 * VOXEL_AXIS_BITS))
    status |= int(status == 0 and bool((keys[1:] <= keys[:-1]).any()))
    if status:
        _raise_status(status, what)
    return keys, ids


def _check_match_args(min_iou, ignore):
    ignore = tuple(int(v) for v in ignore)
    if len(ignore) > MAX_IGNORE:
        raise ValueError("at most %d ignored ids, got %d" % (MAX_IGNORE, len(ignore)))
    if not 0.0 <= float(min_iou) <= 1.0:
        raise ValueError("min_iou must lie in [0, 1], got %r" % (min_iou,))
    return float(min_iou), ignore


@torch.no_grad()
def overlap_table_reference(a, b, _what="overlap_table"):
    """The shared voxels of two fused maps per pair of ids - the definition (NumPy on the CPU).  Both maps lie on one lattice (else ValueError) and
    ascend strictly by voxel key (else ValueError, as connected_components).  -> {'ids_a' i64 [Ta], 'ids_b' i64 [Tb]: each map's distinct ids
    ascending (signed), 'table' i64 [Ta,Tb]: the voxel keys present in both maps with id ids_a[i] in a and ids_b[j] in b (ignored ids counted like
    any other), 'shared': the table's sum}."""
    _check_same_lattice(a, b, _what)
    (ka, ia), (kb, ib) = _checked_keys(a, _what), _checked_keys(b, _what)
    ua, sa = np.unique(ia, return_inverse=True)
    ub, sb = np.unique(ib, return_inverse=True)
    _, ra, rb = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    table = np.zeros((ua.shape[0], ub.shape[0]), np.int64)
    np.add.at(table, (sa.reshape(-1)[ra], sb.reshape(-1)[rb]), 1)
    return {"ids_a": torch.from_numpy(ua), "ids_b": torch.from_numpy(ub), "table": torch.from_numpy(table), "shared": int(table.sum())}


def _iou_of_table(table):
    """fp32: (float) t / (float) (r_i + c_j - t) with the sums over ALL columns / rows, 0 where the denominator is 0 (no shared voxel on either side)."""
    den = table.sum(1, keepdims=True) + table.sum(0, keepdims=True) - table
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = table.astype(np.float32) / den.astype(np.float32)
    return np.where(den != 0, iou, np.float32(0.0)).astype(np.float32)


def _active(table, ids_a, ids_b, ignore):
    """The positions of the active ids of either side, ascending: not ignored, a positive entry against a partner that is not ignored."""
    live_a, live_b = ~np.isin(ids_a, np.asarray(ignore, np.int64)), ~np.isin(ids_b, np.asarray(ignore, np.int64))
    pos = (table > 0) & live_a[:, None] & live_b[None, :]
    return np.nonzero(pos.any(1))[0], np.nonzero(pos.any(0))[0]


def _mapping_of_pairs(ids_a, ids_b, pair_pos, ignore):
    """mapping i64 [Tb] from the matched positions [(i, j)]: the partner's id, itself for an ignored id, else a fresh id above every id of both maps,
    in ascending order of the old id."""
    top = max([0] + ([int(ids_a.max())] if ids_a.size else []) + ([int(ids_b.max())] if ids_b.size else []))
    partner = {int(j): int(ids_a[i]) for i, j in pair_pos}
    mapping = np.empty(ids_b.shape[0], np.int64)
    for j, old in enumerate(ids_b.tolist()):
        if j in partner:
            mapping[j] = partner[j]
        elif old in ignore:
            mapping[j] = old
        else:
            top += 1
            mapping[j] = top
    return mapping


@torch.no_grad()
def associate_maps_reference(a, b, min_iou=0.25, ignore=(0,), _what="associate_maps"):
    """The ids of b matched to the ids of a - the definition (NumPy and SciPy on the CPU).  From overlap_table_reference's table, iou[i,j] = table[i,j]
    / (r_i + c_j - table[i,j]) with r_i / c_j the row / column sums over ALL columns / rows (ignored ids included): the IoU over the co-occupied
    voxels, so an instance cut by the window border is not punished for the part the other window never saw.  fp32: two conversions, one division;
    cost = 1.0f - iou.  The ACTIVE ids (not in `ignore`, a positive entry against a partner not in `ignore`), ascending, give the cost sub-matrix
    that scipy.optimize.linear_sum_assignment solves in float64; an assigned pair is MATCHED when table[i,j] > 0 and iou[i,j] >= float32(min_iou).
    ONE TO ONE ONLY: an instance of a that b sees as two keeps the better half, the other half becomes a fresh id (and the other way round).
    -> {'ids_a', 'ids_b', 'table', 'iou' f32 [Ta,Tb], 'pairs' i64 [P,2] = (id_a, id_b) ascending by id_a, 'mapping' i64 [Tb]: the id ids_b[j] takes in
    a's numbering - the matched partner's id, itself for an ignored id, else a fresh id from max(ids_a.max(), ids_b.max(), 0) + 1 upwards in ascending
    order of the old id}."""
    from scipy.optimize import linear_sum_assignment
    min_iou, ignore = _check_match_args(min_iou, ignore)
    out = overlap_table_reference(a, b, _what)
    ids_a, ids_b, table = out["ids_a"].numpy(), out["ids_b"].numpy(), out["table"].numpy()
    iou = _iou_of_table(table)
    act_a, act_b = _active(table, ids_a, ids_b, ignore)
    pairs = []
    if act_a.size and act_b.size:
        cost = np.float32(1.0) - iou[np.ix_(act_a, act_b)]
        rows, cols = linear_sum_assignment(cost.astype(np.float64))
        pairs = [(int(act_a[r]), int(act_b[c])) for r, c in zip(rows, cols)]
        pairs = sorted((i, j) for i, j in pairs if table[i, j] > 0 and iou[i, j] >= np.float32(min_iou))
    out.pop("shared")
    out["iou"] = torch.from_numpy(iou)
    out["pairs"] = torch.tensor([(int(ids_a[i]), int(ids_b[j])) for i, j in pairs], dtype=torch.int64).reshape(-1, 2)
    out["mapping"] = torch.from_numpy(_mapping_of_pairs(ids_a, ids_b, pairs, ignore))
    return out


def relabel_map(m, ids, mapping):
    """The map with every id ids[j] replaced by mapping[j] (ids i64 [T] ascending and holding every id of the map, e.g. associate_maps' 'ids_b' and
    'mapping'); everything else is shared with m.  ValueError for an id of the map that `ids` lacks.  Tensor ops where the map lives."""
    inst = torch.as_tensor(m["instances"]).reshape(-1).to(torch.int64)
    ids = torch.as_tensor(ids).reshape(-1).to(inst.device, torch.int64)
    mapping = torch.as_tensor(mapping).reshape(-1).to(inst.device, torch.int64)
    if ids.numel() != mapping.numel():
        raise ValueError("relabel_map: ids [T] and mapping [T] must have one length")
    if inst.numel() == 0:
        return dict(m, instances=inst)
    if ids.numel() == 0:
        raise ValueError("relabel_map: the map has ids and the list is empty")
    slot = torch.searchsorted(ids, inst).clamp_max(ids.numel() - 1)
    if not bool((ids.index_select(0, slot) == inst).all()):
        raise ValueError("relabel_map: an id of the map is missing from ids")
    return dict(m, instances=mapping.index_select(0, slot))


def _checked_mapping(mapping, ids_b, what):
    mapping = _np(mapping, np.int64).reshape(-1)
    if mapping.shape[0] != ids_b.shape[0]:
        raise ValueError("%s: mapping must hold one id per distinct id of b, ascending (%d), got %d" % (what, ids_b.shape[0], mapping.shape[0]))
    return mapping


@torch.no_grad()
def merge_maps_reference(a, b, mapping=None, min_iou=0.25, ignore=(0,), _what="merge_maps"):
    """Two fused maps on one lattice as one - the definition (NumPy on the CPU).  b is relabelled through `mapping` (i64 [Tb], one id per distinct id
    of b in ascending order; None: associate_maps_reference(a, b, min_iou, ignore)['mapping']).  The result holds the union of the voxel rows in
    ascending key order.  A voxel of one map only is copied bit for bit (b's with its new id).  A voxel of both, cA / cB the counts: count = cA + cB;
    points (and color, kept only when BOTH maps carry it) = (pA * float(cA) + pB * float(cB)) / float(cA + cB) in fp32 in exactly this order, no
    contraction; votes vA = rint(agreementA * cA), vB likewise; equal ids: that id with vA + vB votes; different ids: the id with more votes (ties: the
    smaller id) with its own votes; agreement = float(votes) / float(count).  'component' is dropped (stale after a merge); voxel_size, origin and
    'name' are a's.  A fused row has forgotten its minority votes, so this is NOT the fusion of the two windows' raw points: where the maps disagree
    the losing side's votes for the winner, if any, are lost, and a third id can never win."""
    min_iou, ignore = _check_match_args(min_iou, ignore)
    _check_same_lattice(a, b, _what)
    (ka, ia), (kb, ib) = _checked_keys(a, _what), _checked_keys(b, _what)
    ub, sb = np.unique(ib, return_inverse=True)
    if mapping is None:
        mapping = associate_maps_reference(a, b, min_iou, ignore, _what=_what)["mapping"]
    ib = _checked_mapping(mapping, ub, _what)[sb.reshape(-1)] if ib.size else ib
    keys = np.union1d(ka, kb)
    pa, pb = np.searchsorted(keys, ka), np.searchsorted(keys, kb)
    V = keys.shape[0]
    in_a, in_b = np.zeros(V, bool), np.zeros(V, bool)
    in_a[pa], in_b[pb] = True, True
    both = in_a & in_b
    colored = "color" in a and "color" in b

    def spread(field, dtype, width):
        ca, cb = (np.zeros((V,) + width, dtype) for _ in range(2))
        ca[pa], cb[pb] = _np(a[field], dtype).reshape((-1,) + width), _np(b[field], dtype).reshape((-1,) + width)
        return ca, cb
    cnt_a, cnt_b = spread("count", np.int32, ())
    agr_a, agr_b = spread("agreement", np.float32, ())
    vox_a, vox_b = spread("voxels", np.int32, (3,))
    id_a, id_b = np.zeros(V, np.int64), np.zeros(V, np.int64)
    id_a[pa], id_b[pb] = ia, ib
    total = np.minimum(cnt_a.astype(np.int64) + cnt_b, 2 ** 31 - 1).astype(np.int32)
    fa, fb, fn = cnt_a.astype(np.float32), cnt_b.astype(np.float32), total.astype(np.float32)
    out = {}
    for field in ("points", "color") if colored else ("points",):
        xa, xb = spread(field, np.float32, (3,))
        with np.errstate(all="ignore"):
            mixed = (xa * fa[:, None] + xb * fb[:, None]) / fn[:, None]
        out[field] = torch.from_numpy(np.where(both[:, None], mixed, np.where(in_a[:, None], xa, xb)))
    with np.errstate(all="ignore"):
        va, vb = np.rint(agr_a * fa).astype(np.int64), np.rint(agr_b * fb).astype(np.int64)
        a_wins = (va > vb) | ((va == vb) & (id_a < id_b))
        votes = np.where(id_a == id_b, va + vb, np.where(a_wins, va, vb))
        agreement = votes.astype(np.float32) / fn
    out["instances"] = torch.from_numpy(np.where(both, np.where(a_wins, id_a, id_b), np.where(in_a, id_a, id_b)))
    out["count"] = torch.from_numpy(np.where(both, total, np.where(in_a, cnt_a, cnt_b)))
    out["agreement"] = torch.from_numpy(np.where(both, agreement, np.where(in_a, agr_a, agr_b)).astype(np.float32))
    out["voxels"] = torch.from_numpy(np.where(in_a[:, None], vox_a, vox_b))
    out["voxel_size"] = a["voxel_size"]
    out["origin"] = torch.as_tensor(a["origin"]).detach().cpu().clone()
    if "name" in a:
        out["name"] = a["name"]
    return out


def merge_map_sequence_reference(maps, min_iou=0.25, ignore=(0,)):
    """merge_maps_reference as a left fold over `maps` in the given order; the running map plays a."""
    return _fold(maps, lambda a, b: merge_maps_reference(a, b, None, min_iou, ignore))


def _fold(maps, step):
    maps = list(maps)
    if not maps:
        raise ValueError("merge_map_sequence: no map")
    out = {k: v for k, v in maps[0].items() if k != "component"}
    for m in maps[1:]:
        out = step(out, m)
    return out


def _device_join(a, b, dev, what, combine=True):
    """The device half shared by overlap_table / associate_maps / merge_maps: both maps' rows on `dev`, their distinct ids (synchronisations: the
    lattice check and the sizes of the two lists) and pag_voxel_overlap's keys, slots and table.  The status word is not read here."""
    _check_same_lattice(a, b, what)
    rows = []
    for m in (a, b):
        ids = torch.as_tensor(m["instances"]).reshape(-1).to(dev, torch.int64)
        vox = torch.as_tensor(m["voxels"]).reshape(-1, 3).to(dev, torch.int32)
        if vox.shape[0] != ids.numel():
            raise ValueError("%s: voxels [V,3] and instances [V] must describe the same rows" % what)
        rows.append((vox, ids, torch.unique(ids)))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    j = ops.voxel_overlap(*rows[0], *rows[1], status, combine=combine)
    j.update(ids_a=rows[0][2], ids_b=rows[1][2], status=status)
    return j


@torch.no_grad()
def overlap_table(a, b, device=None):
    """overlap_table_reference on the device (pag_voxel_overlap: the join of the two sorted key columns, the adds combined per wave).  Runs on
    `device` (default: where a lives, "cuda" for a CPU map; "cpu" selects the definition); the result lives where a does.  The synchronisations do not grow with
    the maps (the lattice check, the two id lists, one read of the status word); a map that breaks the contract raises ValueError."""
    home, dev = _home_and_device(a, device)
    if dev.type == "cpu":
        return _to_home(overlap_table_reference(_cpu_map(a), _cpu_map(b)), home)
    j = _device_join(a, b, dev, "overlap_table")
    table = j["table"].long()
    status, shared = torch.stack((j["status"][0].long(), table.sum())).tolist()
    if status:
        _raise_status(status, "overlap_table")
    return {"ids_a": j["ids_a"].to(home), "ids_b": j["ids_b"].to(home), "table": table.to(home), "shared": int(shared)}


def _device_associate(j, min_iou, ignore, dev, what):
    """From the join to the association, all on T-length tables: activity flags and their compaction (tensor ops), pag_overlap_cost, pag_assign_solve,
    the fresh-id numbering and the mapping (tensor ops).  Two reads of device results: (status, active counts) and the solver's status with the pair count."""
    ids_a, ids_b, table = j["ids_a"], j["ids_b"], j["table"]
    Ta, Tb = table.shape
    ign = torch.tensor(ignore if ignore else [0], dtype=torch.int64, device=dev)[:len(ignore)]
    live_a, live_b = ~torch.isin(ids_a, ign), ~torch.isin(ids_b, ign)
    pos = (table > 0) & live_a[:, None] & live_b[None, :]
    on_a, on_b = pos.any(1), pos.any(0)
    status, n_a, n_b = torch.stack((j["status"][0].long(), on_a.sum(), on_b.sum())).tolist()           # synchronisation
    if status:
        _raise_status(status, what)
    if max(n_a, n_b) > MAX_DEVICE_MATCH:
        raise ValueError('%s: %d and %d active ids, the device solver takes %d per side: pass device="cpu"' % (what, n_a, n_b, MAX_DEVICE_MATCH))
    # the active positions ascending, without a data-dependent shape: a stable sort of the flags
    act_a = torch.sort((~on_a).to(torch.uint8), stable=True)[1][:n_a].to(torch.int32)
    act_b = torch.sort((~on_b).to(torch.uint8), stable=True)[1][:n_b].to(torch.int32)
    wide = table.long()
    iou, cost, transposed = ops.overlap_cost(table, wide.sum(1), wide.sum(0), act_a, act_b)
    matched = torch.zeros(Ta, Tb, dtype=torch.bool, device=dev)
    solved = torch.zeros(1, dtype=torch.int32, device=dev)
    if n_a and n_b:
        R, C = cost.shape
        info = torch.tensor([R, 0], dtype=torch.int32, device=dev)
        targets = torch.empty(R, dtype=torch.int64, device=dev)
        ops._call("pag_assign_solve", cost.data_ptr(), 1, R, C, info.data_ptr(), None, targets.data_ptr(), solved.data_ptr(), ops.L.stream())
        rows_of, cols_of = (act_b, act_a) if transposed else (act_a, act_b)
        r, c = rows_of.long(), cols_of.long().index_select(0, (targets - 1).clamp(0, C - 1))
        i, k = (c, r) if transposed else (r, c)
        ok = (table[i, k] > 0) & (iou[i, k] >= torch.tensor(min_iou, dtype=torch.float32, device=dev))
        matched[i, k] = ok
    has_partner = matched.any(0)
    partner = ids_a.index_select(0, matched.to(torch.uint8).argmax(0)) if Ta else ids_b
    fresh = ~has_partner & live_b
    top = torch.stack([t.max() for t in (ids_a, ids_b) if t.numel()] + [torch.zeros((), dtype=torch.int64, device=dev)]).max()
    mapping = torch.where(has_partner, partner, torch.where(fresh, top + torch.cumsum(fresh.long(), 0), ids_b))
    failed, P = torch.stack((solved[0].long(), has_partner.sum())).tolist()                            # synchronisation
    if failed:
        raise RuntimeError("%s: pag_assign_solve did not solve the assignment (status %d)" % (what, failed))
    by_a = matched.any(1)
    rows = torch.sort((~by_a).to(torch.uint8), stable=True)[1][:P]
    pairs = torch.stack((ids_a.index_select(0, rows), ids_b.index_select(0, matched.to(torch.uint8).argmax(1).index_select(0, rows))), 1) if Tb else \
        torch.zeros(0, 2, dtype=torch.int64, device=dev)
    return {"ids_a": ids_a, "ids_b": ids_b, "table": wide, "iou": iou, "pairs": pairs.reshape(-1, 2), "mapping": mapping}


@torch.no_grad()
def associate_maps(a, b, min_iou=0.25, ignore=(0,), device=None):
    """associate_maps_reference on the device: pag_voxel_overlap's table, pag_overlap_cost's fp32 IoU and cost in the definition's op order, the
    Hungarian step by pag_assign_solve (SciPy's algorithm, the same pairs); the T-length bookkeeping is tensor ops.  One to one only, as the
    definition.  Runs on `device` (default: where a lives, "cuda" for a CPU map; "cpu" selects the definition); the result lives where a does.
    Nine synchronisations as torch's debug mode counts them, whatever the maps' size.  More than 256 active ids on either side: ValueError (pass device="cpu"); nothing falls back."""
    min_iou, ignore = _check_match_args(min_iou, ignore)
    home, dev = _home_and_device(a, device)
    if dev.type == "cpu":
        return _to_home(associate_maps_reference(_cpu_map(a), _cpu_map(b), min_iou, ignore), home)
    return _to_home(_device_associate(_device_join(a, b, dev, "associate_maps"), min_iou, ignore, dev, "associate_maps"), home)


@torch.no_grad()
def merge_maps(a, b, mapping=None, min_iou=0.25, ignore=(0,), device=None, capacity=None):
    """merge_maps_reference on the device: the join (pag_voxel_overlap), the association unless `mapping` is given, one stable sort of both maps' keys
    (torch.sort; a's rows first) and pag_voxel_merge, an ordered append over the runs of one or two rows in the definition's op order.  Runs on
    `device` (default: where a lives, "cuda" for a CPU map; "cpu" selects the definition); the result lives where a does.  Outputs are sized for
    all rows of both maps (52 bytes each, 40 without colour) unless `capacity` says otherwise; a merged map of more voxels raises with the count it
    needed.  Ten synchronisations as torch's debug mode counts them, whatever the maps' size (six with `mapping`)."""
    min_iou, ignore = _check_match_args(min_iou, ignore)
    home, dev = _home_and_device(a, device)
    if dev.type == "cpu":
        return _to_home(merge_maps_reference(_cpu_map(a), _cpu_map(b), None if mapping is None else torch.as_tensor(mapping).cpu(), min_iou, ignore), home)
    j = _device_join(a, b, dev, "merge_maps")
    if mapping is None:
        mapping = _device_associate(j, min_iou, ignore, dev, "merge_maps")["mapping"]
    else:
        mapping = torch.as_tensor(mapping).reshape(-1).to(dev, torch.int64)
        if mapping.numel() != j["ids_b"].numel():
            raise ValueError("merge_maps: mapping must hold one id per distinct id of b, ascending (%d), got %d" % (j["ids_b"].numel(), mapping.numel()))
    colored = "color" in a and "color" in b
    kinds = dict(points=torch.float32, color=torch.float32, count=torch.int32, agreement=torch.float32, voxels=torch.int32, instances=torch.int64)
    fields = [k for k in kinds if k != "color" or colored]
    on_dev = [{k: torch.as_tensor(m[k]).to(dev, kinds[k]).reshape((-1, 3) if k in ("points", "color", "voxels") else (-1,)).contiguous() for k in fields}
              for m in (a, b)]
    n = j["keys_a"].numel() + j["keys_b"].numel()
    cap = n if capacity is None else min(int(capacity), n)
    out = {k: torch.empty((cap, 3) if k in ("points", "color", "voxels") else (cap,), dtype=kinds[k], device=dev) for k in fields}
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    keys, order = torch.sort(torch.cat((j["keys_a"], j["keys_b"])), stable=True)
    ops.voxel_merge(keys, order, on_dev[0], on_dev[1], j["slot_b"], mapping.contiguous(), out, counter, j["status"])
    status, rows = torch.stack((j["status"][0].long(), counter[0])).tolist()                           # synchronisation
    if status:
        _raise_status(status, "merge_maps")
    out = _to_home(_trim(rows, cap, "the merged map has %d voxels, the outputs hold %d", out), home)
    out["voxel_size"] = a["voxel_size"]
    out["origin"] = torch.as_tensor(a["origin"]).detach().clone()
    if "name" in a:
        out["name"] = a["name"]
    return out


def merge_map_sequence(maps, min_iou=0.25, ignore=(0,), device=None, capacity=None):
    """merge_maps as a left fold over `maps` in the given order; the running map plays a (merge_map_sequence_reference on the device)."""
    return _fold(maps, lambda a, b: merge_maps(a, b, None, min_iou, ignore, device, capacity))


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
    [--table OUT.csv] [--min-component N] [--connectivity 6|18|26] [--split keep|largest|split]
    python -m pagnerf_amd.map_export merge A.pkl B.pkl [C.pkl ...] --out OUT.ply|OUT.pkl [--voxel-size V] [--frame S X Y Z ...] [--min-iou F]
    [--ignore ID ...] [--table OUT.csv] [--pairs OUT.csv] [--min-component N] [--connectivity 6|18|26] [--split keep|largest|split]"""
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
    me = sub.add_parser("merge", help="match the instance ids of several windows' maps and merge them into one",
                        description="Merges the maps of several training windows into one voxel map with ONE id numbering.  Every input is a fused "
                        "one-entry map (what `fuse` writes as .pkl) or a raw export, which is fused first (--voxel-size is then required).  The maps are "
                        "merged from left to right: the ids of the next map are matched one to one to the ids of the map so far by the IoU over the "
                        "voxels both hold (Hungarian assignment), matched ids take their partner's id, every other id becomes a new one, and the rows "
                        "are united.  Ids that are reused for distant objects match badly: cleaning every input with --min-component / --split split "
                        "before it is matched is the recommended route.  The inputs are pickles: trusted files only.")
    me.add_argument("inputs", nargs="+", metavar="IN.pkl", help="fused maps or raw exports, one per window (pickles: trusted files only)")
    me.add_argument("--voxel-size", type=float, metavar="V", help="voxel edge; required when an input is a raw export")
    me.add_argument("--min-votes", type=int, default=1, metavar="N", help="raw exports: drop voxels that hold fewer than N points")
    me.add_argument("--limits", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="raw exports: keep points strictly inside this box")
    me.add_argument("--origin", type=float, nargs=3, default=(-1.0, -1.0, -1.0), metavar=("X", "Y", "Z"), help="raw exports: corner the voxel lattice is anchored at")
    me.add_argument("--frame", type=float, nargs=4, action="append", metavar=("S", "X", "Y", "Z"), help="once per input, in order: the raw export's "
                    "points become p * S + (X, Y, Z) before they are keyed (separately normalised windows brought into one frame)")
    me.add_argument("--min-iou", type=float, default=0.25, metavar="F", help="least IoU over the co-occupied voxels of a matched pair (default 0.25)")
    me.add_argument("--ignore", type=int, nargs="*", default=[0], metavar="ID", help="instance ids never matched and left out of the table (default: 0)")
    me.add_argument("--out", required=True, metavar="OUT.ply|OUT.pkl", help="the merged map (a .ply, or a pickle of a one-entry list)")
    me.add_argument("--table", metavar="OUT.csv", help="also write the per-instance table of the merged map")
    me.add_argument("--pairs", metavar="OUT.csv", help="also write step, id_a, id_b, shared voxels and iou of every matched pair of every merge step")
    me.add_argument("--device", default="cuda", help="where it runs; cpu selects the definitions")
    me.add_argument("--min-component", type=int, metavar="N", help="clean every input before it is matched: drop connected components of equal-id voxels "
                    "that have fewer than N voxels (recommended, with --split split)")
    me.add_argument("--connectivity", type=int, choices=sorted(CONNECTIVITIES), metavar="6|18|26", help="neighbourhood of the components (default 26)")
    me.add_argument("--split", choices=CLEAN_MODES, metavar="keep|largest|split", help="an id with several components in one input: keep them (default), "
                    "keep only the largest, or make every further component a new instance (recommended: every id is then one blob)")
    args = ap.parse_args(argv)
    if args.command == "merge":
        return _merge_command(args)
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


def _merge_command(args):
    import csv
    if args.frame is not None and len(args.frame) != len(args.inputs):
        raise SystemExit("merge: --frame must be given once per input (%d), got %d" % (len(args.inputs), len(args.frame)))
    limits = None if args.limits is None else [args.limits[:3], args.limits[3:]]
    clean = args.min_component is not None or args.connectivity is not None or args.split is not None
    maps = []
    for n, path in enumerate(args.inputs):
        with open(path, "rb") as fh:
            loaded = pickle.load(fh)
        loaded = list(loaded) if isinstance(loaded, (list, tuple)) else [loaded]
        if len(loaded) == 1 and "voxels" in loaded[0] and "count" in loaded[0]:
            if args.frame is not None and tuple(args.frame[n]) != (1.0, 0.0, 0.0, 0.0):
                raise SystemExit("merge: %s is a fused map already; --frame applies to raw exports (fuse it with the frame instead)" % path)
            m = loaded[0]
        else:
            if args.voxel_size is None:
                raise SystemExit("merge: %s is a raw export: --voxel-size is required to fuse it" % path)
            frame = None if args.frame is None else [(args.frame[n][0], args.frame[n][1:])] * len(loaded)
            m = fuse_map(loaded, args.voxel_size, origin=args.origin, limits=limits, min_votes=args.min_votes, device=args.device, frames=frame)
        if clean:
            m = clean_map(m, min_voxels=args.min_component or 1, connectivity=args.connectivity or 26, mode=args.split or "keep", ignore=args.ignore,
                          device=args.device)
        maps.append(m)
    merged, steps = {k: v for k, v in maps[0].items() if k != "component"}, []
    for n, m in enumerate(maps[1:]):
        found = associate_maps(merged, m, min_iou=args.min_iou, ignore=args.ignore, device=args.device)
        ia, ib = found["ids_a"].tolist(), found["ids_b"].tolist()
        for id_a, id_b in found["pairs"].tolist():
            i, j = ia.index(id_a), ib.index(id_b)
            steps.append([n + 1, id_a, id_b, int(found["table"][i, j]), repr(float(found["iou"][i, j]))])
        merged = merge_maps(merged, m, mapping=found["mapping"], device=args.device)
    merged["name"] = "nerf_pc_merged"
    save_map([merged], args.out)
    if args.table:
        save_instance_table(instance_table(merged, ignore=args.ignore, device=args.device), args.table)
    if args.pairs:
        with open(args.pairs, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["step", "id_a", "id_b", "shared_voxels", "iou"])
            w.writerows(steps)
    print("%d maps, %d matched pairs -> %d voxels: %s" % (len(maps), len(steps), merged["points"].shape[0], args.out))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
