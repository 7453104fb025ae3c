"""Carve the occupancy grid from depth images before training (csrc/carve.hip: pag_carve_rays, pag_carve_finish).

An RGB-D dataset knows where free space is before step 0: every valid depth pixel's ray is walked through the grids' 2^blas_level lattice, the cells in
front of the measured surface are marked FREE, the cells within `margin` of it SURFACE, and the two sets are turned into the occupancy bitfield both
marches read (`blas_bits`).  The reference has no such step: this is an addition of this package and nothing here is pinned against it.

THE DEFINITION is the tensor-op form in this module, as elsewhere in the package; it serves CPU and GPU tensors, and the kernels reproduce it bit for bit
(the result is a SET of cells: it does not depend on the order of the rays):

    walk     the candidates (t_in, t_out, cell), t_out > t_in, of oracle/render.py raymarch_voxel() = csrc/render.hip voxel_walk_kernel: the same clip to
             [dist_min, dist_max], first cell, DDA and fp32 roundings in the same order (walk_candidates() below, vectorised over the rays)
    valid    t_hit finite and > 0
    lo, hi   t_hit - margin, t_hit + margin (one fp32 rounding each)
    surface  t_in <= hi and t_out >= lo;   free: not surface and t_out <= lo;   everything else (behind the surface) is left alone
    finish   D = surface dilated `dilate` times by the 26-neighbourhood (max_pool3d 3/1/1: no wrap-around at the faces);
             'hull': ~free | D (a cell no ray observed stays occupied)      'band': D (only the neighbourhood of measured surfaces)
"""
import time

import torch

MODES = {"hull": 0, "band": 1}        # PAG_CARVE_HULL, PAG_CARVE_BAND
MAX_DILATE = 4                         # PAG_CARVE_MAX_DILATE


def num_words(blas_level):
    return max(1, (2 ** int(blas_level)) ** 3 // 32)


def pack_bits(mask):
    """bool [cells] -> int32 [max(1, cells/32)], bit i & 31 of word i >> 5 (the layout of OccupancyBLAS.blas_bits); padding bits 0."""
    mask = mask.reshape(-1).to(torch.bool)
    pad = (-mask.numel()) % 32
    if pad:
        mask = torch.cat([mask, mask.new_zeros(pad)])
    w = (mask.reshape(-1, 32).long() << torch.arange(32, device=mask.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_bits(bits, num_cells):
    """int32 words -> bool [num_cells]."""
    b = bits.reshape(-1).long() & 0xFFFFFFFF
    return ((b[:, None] >> torch.arange(32, device=b.device)) & 1).bool().reshape(-1)[:num_cells]


def walk_candidates(origins, dirs, dist_min, dist_max, blas_level):
    """The voxel walk of oracle/render.py raymarch_voxel() vectorised over the rays: a generator over the 3R + 3 walk steps that yields
    (rec bool [N], t_in f32 [N], t_out f32 [N], cell int64 [N]) - ray i has a candidate in this step iff rec[i].  Every elementwise operation is the
    fp32 one of the scalar form, in its order (tensor / tensor divisions: a division by a Python scalar may become a multiplication by its rounded
    reciprocal on a device).  Ends early once every ray has left the lattice."""
    o, d = origins.reshape(-1, 3).float(), dirs.reshape(-1, 3).float()
    dev = o.device
    R = 2 ** int(blas_level)
    f = lambda v: torch.full((o.shape[0],), float(v), dtype=torch.float32, device=dev)
    cs, one, inf = f(2.0) / f(R), f(1.0), f(float("inf"))
    t0, t1 = f(dist_min), f(dist_max)
    for a in range(3):                                                   # slab test against the cube
        oa, da = o[:, a], d[:, a]
        moving = da != 0
        ta, tb = (-one - oa) / da, (one - oa) / da
        lo, hi = torch.where(ta < tb, ta, tb), torch.where(ta < tb, tb, ta)
        t0 = torch.where(moving, torch.where(t0 >= lo, t0, lo), t0)
        t1 = torch.where(moving, torch.where(t1 <= hi, t1, hi), torch.where((oa < -1.0) | (oa > 1.0), -one, t1))
    alive = t0 < t1
    tm = t0 + (t1 - t0) * f(1e-6)                                        # a point just inside, to pick the first cell
    c, step, tnext, tdelta = [], [], [], []
    for a in range(3):
        oa, da = o[:, a], d[:, a]
        pa = da * tm + oa
        ci = torch.floor((pa + one) / cs)
        ca = torch.where(alive, ci, torch.zeros_like(ci)).clamp(0, R - 1).long()
        pos, neg = da > 0, da < 0
        edge = -one + torch.where(pos, ca + 1, ca).float() * cs
        c.append(ca)
        step.append(pos.long() - neg.long())
        tnext.append(torch.where(pos | neg, (edge - oa) / da, inf))
        tdelta.append(torch.where(pos, cs / da, torch.where(neg, cs / (-da), inf)))
    t, active = t0, alive
    for _ in range(3 * R + 3):
        a0 = (tnext[0] <= tnext[1]) & (tnext[0] <= tnext[2])
        a1 = ~a0 & (tnext[1] <= tnext[2])
        ax = [a0, a1, ~a0 & ~a1]
        tn = torch.where(a0, tnext[0], torch.where(a1, tnext[1], tnext[2]))
        tout = torch.where(tn <= t1, tn, t1)
        yield active & (tout > t), t, tout, (c[0] * R + c[1]) * R + c[2]
        last = tout >= t1
        t = tout
        for k in range(3):
            c[k] = c[k] + torch.where(ax[k], step[k], torch.zeros_like(step[k]))
            tnext[k] = torch.where(ax[k], tnext[k] + tdelta[k], tnext[k])
        cm = torch.where(a0, c[0], torch.where(a1, c[1], c[2]))
        active = active & ~last & (cm >= 0) & (cm < R)
        c = [ck.clamp(0, R - 1) for ck in c]                            # a ray that stepped out is inactive for good: keep its index in range
        if not bool(active.any()):
            break


@torch.no_grad()
def carve_reference(origins, dirs, t_hit, dist_min, dist_max, margin, blas_level, free_bits=None, surface_bits=None):
    """-> (free_bits, surface_bits) int32 [max(1, R^3/32)]: the definition of pag_carve_rays (module docstring).  Given bitfields are OR-ed into
    (new tensors are returned)."""
    if not float(margin) >= 0.0:
        raise ValueError("carve_reference: margin %r is negative or NaN" % (margin,))
    R = 2 ** int(blas_level)
    t_hit = t_hit.reshape(-1).float()
    dev = t_hit.device
    valid = torch.isfinite(t_hit) & (t_hit > 0)
    m = torch.full_like(t_hit, float(margin))
    lo, hi = t_hit - m, t_hit + m
    free = torch.zeros(R ** 3, dtype=torch.bool, device=dev) if free_bits is None else unpack_bits(free_bits, R ** 3).clone()
    surface = torch.zeros(R ** 3, dtype=torch.bool, device=dev) if surface_bits is None else unpack_bits(surface_bits, R ** 3).clone()
    for rec, t_in, t_out, cell in walk_candidates(origins, dirs, dist_min, dist_max, blas_level):
        rec = rec & valid
        s = rec & (t_in <= hi) & (t_out >= lo)
        fr = rec & ~s & (t_out <= lo)
        surface[cell[s]] = True
        free[cell[fr]] = True
    return pack_bits(free), pack_bits(surface)


@torch.no_grad()
def carve_finish_reference(free, surface, blas_level, dilate=1, mode="hull"):
    """-> int32 bits: the definition of pag_carve_finish.  The bits are unpacked, the surface set goes `dilate` times through max_pool3d(kernel 3,
    stride 1, padding 1) - the padding is -inf, so nothing wraps round the cube's faces - and the result is packed again."""
    if mode not in MODES:
        raise ValueError("carve_finish_reference: unknown mode %r (hull / band)" % (mode,))
    if not 0 <= int(dilate) <= MAX_DILATE:
        raise ValueError("carve_finish_reference: dilate %r not in [0, %d]" % (dilate, MAX_DILATE))
    R = 2 ** int(blas_level)
    D = unpack_bits(surface, R ** 3).reshape(1, 1, R, R, R).float()
    for _ in range(int(dilate)):
        D = torch.nn.functional.max_pool3d(D, kernel_size=3, stride=1, padding=1)
    D = D.reshape(-1) > 0
    return pack_bits(D if mode == "band" else (~unpack_bits(free, R ** 3) | D))


def ray_lengths_from_depth(depths, base_dirs, scale, depth_kind="z", max_range=None):
    """A depth image in metres -> the surface distance ALONG each pixel's ray in scene units, 0 (= invalid) where the sensor gave nothing.

    depths [..., n] or [..., n, 1] f32 metres; base_dirs [n, 3] the camera-frame directions of `base_rays` (any length; pag_prepare_views and
    pinhole_base_rays build them with -z forward); scale: scene units per metre (the dataset's `scale`).
      'ray'  t = depth * scale                                        the sensor reports the distance along the ray
      'z'    t = depth * scale * (|d_cam| / (-d_cam.z))               the sensor reports the distance along the optical axis (a depth camera's image)
    Pixels with depth <= 0, a non-finite depth or depth > max_range (metres, optional) give 0.
    The 'z' convention is this package's reading of the sensor (the BUP20 frames come from a depth camera whose images hold z): PARITY UNPINNED.
    Plain tensor ops, no kernel: it is one pass over the image."""
    if depth_kind not in ("z", "ray"):
        raise ValueError("ray_lengths_from_depth: depth_kind %r is neither 'z' nor 'ray'" % (depth_kind,))
    d = depths.float()
    if d.dim() >= 2 and d.shape[-1] == 1 and d.shape[-2] == base_dirs.shape[0]:
        d = d[..., 0]
    if d.shape[-1] != base_dirs.shape[0]:
        raise ValueError("ray_lengths_from_depth: %d depth pixels per view, %d base rays" % (d.shape[-1], base_dirs.shape[0]))
    ok = torch.isfinite(d) & (d > 0)
    if max_range is not None:
        ok = ok & (d <= float(max_range))
    t = d * float(scale)
    if depth_kind == "z":
        bd = base_dirs.float().to(d.device)
        t = t * (torch.linalg.norm(bd, dim=-1) / (-bd[:, 2]))
    return torch.where(ok, t, torch.zeros_like(t))


def _pixels(ds, stride):
    """The pixel indices of every stride-th row and column (all of them for stride 1): int64 [k]."""
    n = ds.num_pixels
    if stride == 1:
        return torch.arange(n, device=ds.device)
    shape = getattr(ds, "image_shape", None)
    if shape is None:
        raise ValueError("carve_occupancy: stride > 1 needs the dataset's `image_shape` (H, W)")
    h, w = int(shape[0]), int(shape[1])
    if h * w != n:
        raise ValueError("carve_occupancy: image_shape %s does not hold the dataset's %d pixels" % ((h, w), n))
    return (torch.arange(0, h, stride, device=ds.device)[:, None] * w + torch.arange(0, w, stride, device=ds.device)[None]).reshape(-1)


@torch.no_grad()
def carve_occupancy(dataset, pipeline, *, margin=None, dilate=1, mode="hull", stride=1, max_range=None, depth_kind="z", views=None, chunk_views=8,
                    scale=None, blas_level=None, use_kernel=None):
    """The occupancy bitfield that the depth images of `dataset` (a DeviceMultiviewDataset with a `depths` mode, f32 metres) leave of the cube:
    -> (bits int32 [max(1, R^3/32)] on the dataset's device, report dict).

    The world rays are pipeline.transform_rays_indexed(base_rays, cam_idx) for a BAPipeline (its CURRENT extrinsics: with pose optimisation these are
    the initial poses, so `margin` has to cover the expected pose error), the dataset's `rays` otherwise; their dist_min / dist_max clip the walk as
    they clip the training march.  `chunk_views` views go into one pag_carve_rays launch; `stride` takes every stride-th pixel per axis; `views`
    restricts the carve to those views.  scale: scene units per metre, default the dataset's `scale`.

    The defaults are chosen from GEOMETRY, not from data: margin = two cell widths (2 * 2 / R scene units: a surface measured anywhere in a cell keeps
    that cell and its neighbours along the ray whatever the sub-cell phase, and the depth's quantisation and a small pose error stay inside it),
    dilate = 1 (the ray through a pixel's centre stands for the pixel's whole footprint, which at the image sizes in use is narrower than a cell, so
    one ring of neighbours covers it), mode 'hull' (nothing that no ray saw is removed).  'band' and stride > 1 trade safety for speed.

    report: valid_pixels, pixels, views, free / surface / occupied (shares of the R^3 cells: marked free, marked surface, set in the result),
    blas_level, margin, seconds (wall clock, device work included).
    On a CUDA dataset the two kernels run (use_kernel=False: the tensor-op definition); a CPU dataset takes the definition."""
    if "depths" not in dataset.modes:
        raise ValueError("carve_occupancy: the dataset has no 'depths' mode (modes: %s).  A BUP20 training window carries none unless it is loaded with "
                         "load_bup20(..., keep_depths=True) - python -m pagnerf_amd.train --carve-from-depth and the YAML key carve_from_depth do that, "
                         "python -m pagnerf_amd.bup20 --split train --keep-depths writes it into the .npz; any other dataset needs a 'depths' array "
                         "[V, H, W, 1] in metres beside its images" % (list(dataset.modes),))
    scale = getattr(dataset, "scale", None) if scale is None else scale
    if scale is None:
        raise ValueError("carve_occupancy: the dataset carries no `scale` (scene units per metre) and no scale= was given")
    if mode not in MODES:
        raise ValueError("carve_occupancy: unknown mode %r (hull / band)" % (mode,))
    if not 0 <= int(dilate) <= MAX_DILATE:
        raise ValueError("carve_occupancy: dilate %r not in [0, %d]" % (dilate, MAX_DILATE))
    if int(stride) < 1 or int(chunk_views) < 1:
        raise ValueError("carve_occupancy: stride and chunk_views must be >= 1")
    is_ba = hasattr(pipeline, "transform_rays_indexed") and "base_rays" in dataset.modes
    if not is_ba and "rays" not in dataset.modes:
        raise ValueError("carve_occupancy: the dataset has no world-frame 'rays' and the pipeline no cameras for its 'base_rays'")
    if blas_level is None:
        blas_level = pipeline.nef.grid.blas_level
    blas_level = int(blas_level)
    R = 2 ** blas_level
    margin = 2 * 2.0 / R if margin is None else float(margin)
    if not margin >= 0.0:
        raise ValueError("carve_occupancy: margin %r is negative or NaN" % (margin,))
    dev = dataset.device
    use_kernel = (dev.type == "cuda") if use_kernel is None else bool(use_kernel)
    start = time.time()
    pix = _pixels(dataset, int(stride))
    depths = dataset.source("depths")
    base_o, base_d = dataset.source("base_rays", "origins"), dataset.source("base_rays", "dirs")
    if depth_kind == "z" and base_d is None:
        raise ValueError("carve_occupancy: depth_kind 'z' needs the dataset's camera-frame 'base_rays'")
    views = torch.arange(dataset.num_imgs) if views is None else torch.as_tensor(views, dtype=torch.int64).reshape(-1).cpu()
    if views.numel() and (int(views.min()) < 0 or int(views.max()) >= dataset.num_imgs):
        raise IndexError("carve_occupancy: view outside [0, %d)" % dataset.num_imgs)
    words = num_words(blas_level)
    free = torch.zeros(words, dtype=torch.int32, device=dev)
    surface = torch.zeros(words, dtype=torch.int32, device=dev)
    valid = torch.zeros((), dtype=torch.int64, device=dev)
    if use_kernel:
        from . import ops
    k = pix.numel()
    for chunk in views.split(int(chunk_views)):
        v = chunk.to(dev)
        t = ray_lengths_from_depth(depths[v][:, pix, 0], base_d[pix] if base_d is not None else depths.new_ones(k, 3), scale, depth_kind, max_range)
        if is_ba:
            cam_idx = v[:, None].expand(-1, k).reshape(-1).to(torch.int32)
            rays = pipeline.transform_rays_indexed(base_o[pix].repeat(len(v), 1), base_d[pix].repeat(len(v), 1), cam_idx)
            o, d, dmin, dmax = rays.origins, rays.dirs, rays.dist_min, rays.dist_max
        else:
            dmin, dmax = dataset.rays_range("rays")
            o, d = dataset.source("rays", "origins")[v][:, pix].reshape(-1, 3), dataset.source("rays", "dirs")[v][:, pix].reshape(-1, 3)
        t = t.reshape(-1).contiguous()
        valid += (t > 0).sum()
        if use_kernel:
            ops.carve_rays(o.detach().float().contiguous(), d.detach().float().contiguous(), t, dmin, dmax, margin, blas_level, free, surface)
        else:
            free, surface = carve_reference(o.detach(), d.detach(), t, dmin, dmax, margin, blas_level, free, surface)
    if use_kernel:
        bits = ops.carve_finish(free, surface, blas_level, dilate, mode)
    else:
        bits = carve_finish_reference(free, surface, blas_level, dilate, mode)
    cells = R ** 3
    share = lambda b: float(unpack_bits(b, cells).sum()) / cells          # reads the device: the report is where the carve waits for it
    report = dict(valid_pixels=int(valid), pixels=int(views.numel() * k), views=int(views.numel()), free=share(free), surface=share(surface),
                  occupied=share(bits), blas_level=blas_level, margin=margin, dilate=int(dilate), mode=mode, stride=int(stride))
    report["seconds"] = time.time() - start
    return bits, report


def report_line(report):
    return ("carved the occupancy from depth: %(valid_pixels)d valid of %(pixels)d pixels in %(views)d views, level %(blas_level)d, margin %(margin).4g, "
            "dilate %(dilate)d, %(mode)s | cells free %(free).1f%% surface %(surface).1f%% -> occupied %(occupied).1f%% | %(seconds).2fs"
            % dict(report, free=100 * report["free"], surface=100 * report["surface"], occupied=100 * report["occupied"]))
