"""Inputs shared by tests/test_carve_host.py and tests/test_gpu_carve.py: ray sets with the walk's edge cases, an analytic sphere seen by six axis
cameras, and a tiny synthetic RGB-D dataset.  Everything is generated from seeds; nothing here runs on the GPU."""
import math

import numpy as np
import torch

DIST_MIN, DIST_MAX = 0.0, 6.0


def _unit(v):
    v = torch.tensor(v, dtype=torch.float32)
    return (v / torch.linalg.norm(v)).tolist()


NAN, INF = float("nan"), float("inf")
# (origin, direction, t_hit): what the issue lists, each at least once
EDGE_RAYS = [
    ((0.1, 0.2, -0.3), _unit((0.3, -0.5, 0.8)), 0.6),          # starts inside the cube
    ((-1.5, -1.2, 0.13), _unit((1.0, 1.0, 0.0)), 1.4),          # one direction component exactly 0
    ((-2.0, 0.3, 0.1), (1.0, 0.0, 0.0), 1.7),                   # two components 0: along a cell row
    ((0.0, 2.0, 0.0), (1.0, 0.0, 0.0), 1.0),                    # a zero component whose slab the origin is outside of: misses
    ((3.0, 3.0, 3.0), _unit((1.0, 0.2, 0.1)), 1.0),             # misses the cube
    ((-3.0, 0.02, 0.05), _unit((1.0, 0.01, 0.02)), 0.5),        # t_hit before the entry (2.0): nothing free, nothing surface without a margin
    ((-3.0, 0.02, 0.05), _unit((1.0, 0.01, 0.02)), 5.9),        # t_hit beyond the exit (4.0): every crossed cell free
    ((-1.7, 0.4, -0.2), _unit((1.0, -0.3, 0.2)), 0.0),          # invalid: 0
    ((-1.7, 0.4, -0.2), _unit((1.0, -0.3, 0.2)), -1.0),         # invalid: negative
    ((-1.7, 0.4, -0.2), _unit((1.0, -0.3, 0.2)), NAN),          # invalid: NaN
    ((-1.7, 0.4, -0.2), _unit((1.0, -0.3, 0.2)), INF),          # invalid: +inf
    ((1.0, 1.0, 1.6), _unit((-1.0, -1.0, -1.0)), 1.5),          # enters through a corner: three equal boundary times
    ((-1.0, -0.5, 0.25), (1.0, 0.0, 0.0), 1.0),                 # starts on a face, runs along cell boundaries (y, z on lattice planes)
]


def ray_set(n, seed):
    """n rays: the edge rays first (as many as fit; for n == 1 the one that starts inside), then random origins in [-1.6, 1.6]^3 - inside and outside
    the cube - with random unit directions, two thirds of them aimed at a point of the cube, and t_hit in (0, 4).  -> origins, dirs [n,3], t_hit [n]."""
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(n, 3, generator=g) * 3.2 - 1.6
    d = torch.randn(n, 3, generator=g)
    aim = torch.rand(n, 3, generator=g) * 1.8 - 0.9
    aimed = torch.rand(n, generator=g) < 0.67
    d = torch.where(aimed[:, None], aim - o, d)
    d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    t = torch.rand(n, generator=g) * 4.0 + 1e-3
    for i, (eo, ed, et) in enumerate(EDGE_RAYS[:n]):
        o[i], d[i], t[i] = torch.tensor(eo), torch.tensor(ed), et
    return o.float().contiguous(), d.float().contiguous(), t.float().contiguous()


def candidates(origins, dirs, level):
    """carve.walk_candidates collected in the oracle's order (ray-major, steps ascending): ray ids, cells int64 [M], t_in, t_out f32 [M]."""
    from pagnerf_amd import carve
    rays, cells, tin, tout = [], [], [], []
    n = origins.shape[0]
    for rec, t_in, t_out, cell in carve.walk_candidates(origins, dirs, DIST_MIN, DIST_MAX, level):
        idx = rec.nonzero().reshape(-1)
        rays.append(idx), cells.append(cell[idx]), tin.append(t_in[idx]), tout.append(t_out[idx])
    rays, cells, tin, tout = torch.cat(rays), torch.cat(cells), torch.cat(tin), torch.cat(tout)
    order = torch.sort(rays, stable=True)[1]                     # within a ray the steps stay in walk order
    assert int(rays.max()) < n
    return rays[order], cells[order], tin[order], tout[order]


# ------------------------------------------------------------------------------------------------------------------------ the analytic sphere
SPHERE_RADIUS = 0.5


def sphere_views(side=12, distance=1.6, half_field=0.42):
    """Six cameras on the axes at `distance` from the origin, looking at it: side x side pixels, unit directions.  -> origins, dirs [6*side*side,3] and
    the exact distance to the sphere of radius 0.5 along each ray (0 where the ray misses it)."""
    u = ((torch.arange(side, dtype=torch.float64) + 0.5) / side * 2 - 1) * half_field
    a, b = torch.meshgrid(u, u, indexing="ij")
    os_, ds_ = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = torch.zeros(side, side, 3, dtype=torch.float64)
            d[..., axis] = -sign
            d[..., (axis + 1) % 3], d[..., (axis + 2) % 3] = a, b
            o = torch.zeros(side * side, 3, dtype=torch.float64)
            o[:, axis] = sign * distance
            os_.append(o), ds_.append((d / torch.linalg.norm(d, dim=-1, keepdim=True)).reshape(-1, 3))
    o, d = torch.cat(os_), torch.cat(ds_)
    bq = (o * d).sum(-1)
    disc = bq * bq - ((o * o).sum(-1) - SPHERE_RADIUS ** 2)
    t = torch.where(disc > 0, -bq - torch.sqrt(disc.clamp_min(0)), torch.zeros_like(bq))
    return o.float(), d.float(), t.float()


# ------------------------------------------------------------------------------------------------------------------- a synthetic RGB-D dataset
SCALE = 0.5                       # scene units per metre


def pinhole_dirs(h, w, field=0.5):
    """Camera-frame directions (x, y, -1) over +-field, NOT normalised (as a depth camera's back-projection has them): [h*w, 3], y slow."""
    ys, xs = torch.meshgrid(((torch.arange(h) + 0.5) / h - 0.5) * 2 * field, ((torch.arange(w) + 0.5) / w - 0.5) * 2 * field, indexing="ij")
    return torch.stack([xs, -ys, -torch.ones_like(xs)], -1).reshape(-1, 3).float()


def down_views(n, height=0.95, radius=0.25, phase=0.0):
    """World -> camera matrices of n cameras at `height` looking down (-z), on a circle of `radius`, each turned a little about the vertical."""
    views = torch.eye(4).repeat(n, 1, 1)
    for i in range(n):
        a = phase + 2 * math.pi * i / n
        yaw = 0.1 * math.sin(3 * a + 0.4)
        R = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        centre = torch.tensor([radius * math.cos(a), radius * math.sin(a), height])
        views[i, :3, :3] = R
        views[i, :3, 3] = -R @ centre
    return views


def world_rays(views, dc):
    """R^T (0 - t) and the normalised R^T d, row-vector form: origins, dirs [V, n, 3]."""
    R, t = views[:, :3, :3], views[:, :3, 3]
    o = torch.matmul(torch.zeros_like(dc)[None] - t[:, None, :], R)
    d = torch.nn.functional.normalize(torch.matmul(dc[None].expand(views.shape[0], -1, -1), R), dim=-1)
    return o.float(), d.float()


def scene_hit(o, d, sphere_radius=0.35, plane_z=-0.4, plane_half=0.9):
    """Distance along unit world rays [n,3] to the first hit of a sphere at the origin over a square of the plane z = plane_z; 0 where neither is hit."""
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - sphere_radius ** 2)
    ts = -b - torch.sqrt(disc.clamp_min(0))
    tp = (plane_z - o[:, 2]) / d[:, 2]
    pp = o + d * tp[:, None]
    hit_p = (tp > 0) & (pp[:, :2].abs().max(-1)[0] < plane_half)
    return torch.where(disc > 0, ts, torch.where(hit_p, tp, torch.zeros_like(tp)))


def z_depth_metres(t, dc):
    """What a depth camera reports for a hit at distance t (scene units) along the pixel's ray: the distance along the optical axis, in metres."""
    return (t * (-dc[:, 2] / torch.linalg.norm(dc, dim=-1))[None] / SCALE).float()


def rgbd_data(views, h, w):
    """The modes of a tiny RGB-D dataset of the sphere-over-plane scene: imgs, depths (z-depth in metres, 0 = no reading), world rays and base rays."""
    dc = pinhole_dirs(h, w)
    o, d = world_rays(views, dc)
    V = views.shape[0]
    t = scene_hit(o.reshape(-1, 3), d.reshape(-1, 3)).reshape(V, -1)
    depths = z_depth_metres(t, dc)
    imgs = (0.5 + 0.5 * torch.sin((o + d * t[..., None]) * 7.0)).float()
    imgs = torch.where(t[..., None] > 0, imgs, torch.ones_like(imgs))
    return dict(imgs=imgs.reshape(V, h, w, 3), depths=depths.reshape(V, h, w, 1), origins=o, dirs=d, base_dirs=dc, t=t)


def rgbd_dataset(views, h, w, device, near=0.0, far=1.9, with_rays=True):
    import pagnerf_amd
    a = rgbd_data(views, h, w)
    data = dict(imgs=a["imgs"], depths=a["depths"], base_rays=pagnerf_amd.Rays(torch.zeros_like(a["base_dirs"]), a["base_dirs"], near, far))
    if with_rays:
        data["rays"] = pagnerf_amd.Rays(a["origins"], a["dirs"], near, far)
    ds = pagnerf_amd.DeviceMultiviewDataset(data, device)
    ds.view_matrices, ds.image_shape, ds.scale = views, (h, w), SCALE
    return ds, a


class StubNef(torch.nn.Module):
    """What carve_occupancy reads of a pipeline's nef: the grid's blas_level."""

    def __init__(self, blas_level):
        super().__init__()
        from pagnerf_amd.grids import OccupancyBLAS
        self.grid = OccupancyBLAS(blas_level)


def bit(bits, cell):
    return (int(bits[cell >> 5]) >> (cell & 31)) & 1


def cell_of(p, level):
    """The lattice cell of points [n,3] in [-1,1]^3, clamped: int64 linear index."""
    R = 2 ** level
    c = torch.floor((p.double() + 1.0) / 2.0 * R).long().clamp(0, R - 1)
    return (c[:, 0] * R + c[:, 1]) * R + c[:, 2]
