"""The depth carve on the GPU (csrc/carve.hip: pag_carve_rays, pag_carve_finish; pagnerf_amd/carve.py) against the tensor-op definitions, BIT FOR BIT:
the carved sets do not depend on the order of the rays or on scheduling, so torch.equal is the comparison.  The definitions run on the CPU, once per
ray set (cached), and on the GPU once to show that the two agree."""
import functools

import pytest
import torch

import carve_cases as cases
from carve_cases import DIST_MAX, DIST_MIN

pytestmark = pytest.mark.gpu

MARGIN = 0.1


@functools.lru_cache(maxsize=None)
def rays_and_reference(n, level, margin=MARGIN):
    """A ray set and carve_reference's (free, surface) for it, computed once on the CPU and shared (never modified: the tests clone what they change)."""
    from pagnerf_amd import carve
    o, d, t = cases.ray_set(n, seed=1000 * level + n)
    free, surface = carve.carve_reference(o, d, t, DIST_MIN, DIST_MAX, margin, level)
    return o, d, t, free, surface


def run_rays(dev, o, d, t, level, margin=MARGIN, free=None, surface=None):
    from pagnerf_amd import carve, ops
    words = carve.num_words(level)
    free = torch.zeros(words, dtype=torch.int32, device=dev) if free is None else free
    surface = torch.zeros(words, dtype=torch.int32, device=dev) if surface is None else surface
    ops.carve_rays(o.to(dev), d.to(dev), t.to(dev), DIST_MIN, DIST_MAX, margin, level, free, surface)
    return free, surface


# ------------------------------------------------------------------------------------------------------------------------------ pag_carve_rays
@pytest.mark.parametrize("level", [1, 3, 5])           # 8 cells in one word, 16 words, 1024 words
@pytest.mark.parametrize("n", [1, 63, 65, 126, 4096])  # a single lane, partial waves, several workgroups
def test_carve_rays_equals_the_definition(gpu_device, level, n):
    o, d, t, want_free, want_surface = rays_and_reference(n, level)
    free, surface = run_rays(gpu_device, o, d, t, level)
    assert torch.equal(free.cpu(), want_free) and torch.equal(surface.cpu(), want_surface)
    if n >= 63:
        assert int(want_surface.ne(0).sum()) > 0 and int(want_free.ne(0).sum()) > 0


@pytest.mark.parametrize("margin", [0.0, 10.0])        # no band at all, and a band larger than the cube
@pytest.mark.parametrize("level", [3, 5])
def test_carve_rays_margin_extremes(gpu_device, level, margin):
    o, d, t, want_free, want_surface = rays_and_reference(126, level, margin)
    free, surface = run_rays(gpu_device, o, d, t, level, margin)
    assert torch.equal(free.cpu(), want_free) and torch.equal(surface.cpu(), want_surface)
    if margin == 10.0:
        assert not want_free.any() and want_surface.any()


def test_definition_gives_the_same_bits_on_the_gpu(gpu_device):
    """carve_reference with GPU tensors: the tensor-op form is the same fp32 arithmetic on either device."""
    from pagnerf_amd import carve
    o, d, t, want_free, want_surface = rays_and_reference(4096, 5)
    free, surface = carve.carve_reference(o.to(gpu_device), d.to(gpu_device), t.to(gpu_device), DIST_MIN, DIST_MAX, MARGIN, 5)
    assert free.is_cuda and torch.equal(free.cpu(), want_free) and torch.equal(surface.cpu(), want_surface)


def test_identical_rays_equal_one_ray(gpu_device):
    """4096 copies of one ray: every lane of every wave tests and sets the same bits at the same time - the result is the single ray's."""
    o, d, t, _, _ = rays_and_reference(1, 5)
    want_free, want_surface = run_rays(gpu_device, o, d, t, 5)
    assert int(want_surface.ne(0).sum()) > 0 and int(want_free.ne(0).sum()) > 0
    free, surface = run_rays(gpu_device, o.expand(4096, 3).contiguous(), d.expand(4096, 3).contiguous(), t.expand(4096).contiguous(), 5)
    assert torch.equal(free, want_free) and torch.equal(surface, want_surface)
    _, _, _, ref_free, ref_surface = rays_and_reference(1, 5)
    assert torch.equal(free.cpu(), ref_free) and torch.equal(surface.cpu(), ref_surface)


def test_repeat_calls_accumulate(gpu_device):
    """A second call on the same buffers ORs into them, and so does a call on buffers that were never zeroed."""
    from pagnerf_amd import carve
    level = 5
    oa, da, ta, fa, sa = rays_and_reference(126, level)
    ob, db, tb, fb, sb = rays_and_reference(4096, level)
    free, surface = run_rays(gpu_device, oa, da, ta, level)
    run_rays(gpu_device, ob, db, tb, level, free=free, surface=surface)
    assert torch.equal(free.cpu(), fa | fb) and torch.equal(surface.cpu(), sa | sb)
    g = torch.Generator().manual_seed(9)
    f0 = carve.pack_bits(torch.rand(8 ** level, generator=g) < 0.3)
    s0 = carve.pack_bits(torch.rand(8 ** level, generator=g) < 0.3)
    free, surface = run_rays(gpu_device, oa, da, ta, level, free=f0.to(gpu_device), surface=s0.to(gpu_device))
    assert torch.equal(free.cpu(), f0 | fa) and torch.equal(surface.cpu(), s0 | sa)


def test_empty_and_refused_calls(gpu_device):
    from pagnerf_amd import ops
    z = torch.zeros(16, dtype=torch.int32, device=gpu_device)
    e = torch.zeros(0, 3, device=gpu_device)
    ops.carve_rays(e, e, torch.zeros(0, device=gpu_device), 0.0, 6.0, 0.1, 3, z, z.clone())          # N == 0: a no-op
    assert not z.any()
    r = torch.zeros(4, 3, device=gpu_device)
    with pytest.raises(ValueError):
        ops.carve_rays(r, r, torch.ones(4, device=gpu_device), 0.0, 6.0, 0.1, 5, z, z.clone())        # bitfields of another level
    with pytest.raises(RuntimeError, match="margin"):
        ops.carve_rays(r, r, torch.ones(4, device=gpu_device), 0.0, 6.0, -0.1, 3, z, z.clone())
    with pytest.raises(RuntimeError, match="dilate"):
        ops.carve_finish(z, z.clone(), 3, dilate=5)
    with pytest.raises(ValueError):
        ops.carve_finish(z, z.clone(), 3, out=z)                                                       # out aliases an input


# ---------------------------------------------------------------------------------------------------------------------------- pag_carve_finish
@functools.lru_cache(maxsize=None)
def finish_sets(level, kind):
    """(free, surface) bitfields: 'placed' = surface cells at a corner, on a face, on both sides of a word boundary and at the far corner, free at
    50 %; 'random' = surface at 5 % fill, free at 50 %."""
    from pagnerf_amd import carve
    R = 2 ** level
    g = torch.Generator().manual_seed(17 * level + len(kind))
    free = torch.rand(R, R, R, generator=g) < 0.5
    if kind == "random":
        surface = torch.rand(R, R, R, generator=g) < 0.05
    else:
        surface = torch.zeros(R, R, R, dtype=torch.bool)
        surface[0, 0, 0] = surface[R - 1, R - 1, R - 1] = True                 # corners: the first and the last bit
        surface[R // 2, 0, R // 2] = True                                      # on a face
        surface[R // 3, R // 3, min(31, R - 1)] = True                         # the last bit of a word (z = 31 at levels >= 5) ...
        surface[R - 2, R // 2, 32 % R] = True                                  # ... and the first bit of one (z = 32 at level 6, z = 0 below)
    return carve.pack_bits(free.reshape(-1)), carve.pack_bits(surface.reshape(-1))


@functools.lru_cache(maxsize=None)
def finish_reference(level, kind, dilate, mode):
    from pagnerf_amd import carve
    return carve.carve_finish_reference(*finish_sets(level, kind), level, dilate, mode)


# level 6 beyond the issue's list: from R = 64 on a z-row has more than one word, and the dilation crosses word boundaries inside a row
@pytest.mark.parametrize("mode", ["hull", "band"])
@pytest.mark.parametrize("dilate", [0, 1, 2, 4])
@pytest.mark.parametrize("level", [1, 3, 5, 6])
def test_carve_finish_equals_the_definition(gpu_device, level, dilate, mode):
    from pagnerf_amd import carve, ops
    for kind in ("placed", "random"):
        free, surface = finish_sets(level, kind)
        got = ops.carve_finish(free.to(gpu_device), surface.to(gpu_device), level, dilate, mode)
        assert got.dtype == torch.int32 and got.numel() == carve.num_words(level)
        assert torch.equal(got.cpu(), finish_reference(level, kind, dilate, mode)), kind
    if level == 1:
        assert int(got.cpu()) >> 8 == 0                                         # the bits past R^3 of the only word are 0


# ----------------------------------------------------------------------------------------------------------------------------- carve_occupancy
H, W, LEVEL = 12, 16, 5


@pytest.fixture(scope="module")
def rgbd(gpu_device):
    """Two views of 16 x 12 pixels of the sphere-over-plane scene with z-depth images, and the definition's sets for all pixels of both views."""
    from pagnerf_amd import carve
    views = cases.down_views(2)
    ds, a = cases.rgbd_dataset(views, H, W, gpu_device)
    t = carve.ray_lengths_from_depth(a["depths"].reshape(2, -1), a["base_dirs"], cases.SCALE)
    return dict(views=views, ds=ds, a=a, t=t)


def composed(rgbd, origins, dirs, pix=None, dilate=1, mode="hull", margin=2 * 2.0 / 2 ** LEVEL):
    """The reference composed by hand: carve_reference on the given world rays of (the chosen pixels of) both views, then carve_finish_reference."""
    from pagnerf_amd import carve
    origins, dirs, t = origins.cpu(), dirs.cpu(), rgbd["t"]
    if pix is not None:
        origins, dirs, t = origins[:, pix], dirs[:, pix], t[:, pix]
    free, surface = carve.carve_reference(origins.reshape(-1, 3), dirs.reshape(-1, 3), t.reshape(-1), 0.0, 1.9, margin, LEVEL)
    return carve.carve_finish_reference(free, surface, LEVEL, dilate, mode)


def pipeline_rays(rgbd, pipe, dev):
    """The world rays the BAPipeline makes of the base rays, per view: what carve_occupancy walks."""
    a = rgbd["a"]
    n = H * W
    cam = torch.arange(2, device=dev, dtype=torch.int32)[:, None].expand(2, n).reshape(-1)
    with torch.no_grad():
        r = pipe.transform_rays_indexed(torch.zeros(2 * n, 3, device=dev), a["base_dirs"].to(dev).repeat(2, 1), cam)
    return r.origins.reshape(2, n, 3), r.dirs.reshape(2, n, 3)


@pytest.mark.parametrize("kind", ["plain", "ba"])
def test_carve_occupancy_against_the_composed_reference(gpu_device, rgbd, kind):
    import pagnerf_amd
    from pagnerf_amd import carve
    ds, a = rgbd["ds"], rgbd["a"]
    if kind == "ba":
        pipe = pagnerf_amd.BAPipeline(cases.StubNef(LEVEL), rgbd["views"], near=0.0, far=1.9).to(gpu_device)
        origins, dirs = pipeline_rays(rgbd, pipe, gpu_device)
    else:
        pipe = pagnerf_amd.Pipeline(cases.StubNef(LEVEL))
        origins, dirs = a["origins"], a["dirs"]
    bits, rep = carve.carve_occupancy(ds, pipe)
    assert bits.is_cuda and bits.dtype == torch.int32
    assert torch.equal(bits.cpu(), composed(rgbd, origins, dirs))
    assert rep["valid_pixels"] == int((rgbd["t"] > 0).sum()) and rep["pixels"] == 2 * H * W and 0 < rep["occupied"] < 1
    assert torch.equal(carve.carve_occupancy(ds, pipe, chunk_views=1)[0], bits)                     # chunked = unchunked
    assert torch.equal(carve.carve_occupancy(ds, pipe, use_kernel=False)[0], bits)                  # the definition through the same plumbing
    pix = (torch.arange(0, H, 2)[:, None] * W + torch.arange(0, W, 2)[None]).reshape(-1)
    strided, rep2 = carve.carve_occupancy(ds, pipe, stride=2, dilate=2, mode="band", margin=0.07)
    assert torch.equal(strided.cpu(), composed(rgbd, origins, dirs, pix, dilate=2, mode="band", margin=0.07))
    assert rep2["pixels"] == 2 * pix.numel()


def test_bup20_training_window_with_depths_on_the_device(gpu_device, tmp_path):
    """load_bup20(..., keep_depths=True) on the device path (pag_bup20_prepare writes the training window's depths) gives the CPU definition's
    planes, and the carve of that dataset by the kernels equals the carve of the CPU dataset by the definition."""
    import os
    import bup20_scene as S
    import pagnerf_amd
    from pagnerf_amd import carve, train
    root = str(tmp_path / "BUP_20")
    os.makedirs(root)
    S.write_tree(root)
    cfg = dict(mip=1, load_modes=["imgs", "semantics", "instance", "preds_deeplab"], max_depth=1.4, seq_num_frames=S.SEQ_NUM_FRAMES, carve_from_depth=True)
    on_cpu = train.load_dataset(root, "train", cfg, "cpu")
    ds = train.load_dataset(root, "train", cfg, gpu_device)
    assert "depths" in ds.modes and ds.source("depths").is_cuda
    assert torch.equal(ds.source("depths").cpu(), on_cpu.source("depths")) and float(on_cpu.source("depths").max()) > 0
    pipe = pagnerf_amd.Pipeline(cases.StubNef(5))
    for kw in (dict(), dict(margin=0.0, dilate=0)):        # the synthetic folder's depth is per-pixel noise: the default band keeps nearly every seen cell
        bits, rep = carve.carve_occupancy(ds, pipe, **kw)
        want, _ = carve.carve_occupancy(on_cpu, pipe, **kw)
        assert torch.equal(bits.cpu(), want) and rep["valid_pixels"] == int((on_cpu.source("depths") > 0).sum())
        assert rep["free"] > 0 and rep["surface"] > 0 and 0 < rep["occupied"] < 1


# ------------------------------------------------------------------------------------------------------------------------------- the trainer
TH = TW = 24
CFG = dict(nef_type="PanopticDeltaNeF", tracer_type="PanopticPackedRFTracer", grid_type="PermutoGrid", num_lods=8, feature_dim=2, capacity_log_2=12,
           delta_capacity_log_2=12, coarsest_scale=1.0, finest_scale=0.01, blas_level=5, hidden_dim=64, num_layers=1, sem_num_layers=1,
           inst_num_layers=2, sem_softmax=True, inst_softmax=True, panoptic_features_type="delta", view_multires=4, raymarch_type="ray", num_steps=32,
           samples_per_voxel=2, bg_color="white", ray_max_travel=2.0, batch_size=2, num_rays_sampled_per_img=128, render_batch=512, lr=0.001,
           grid_lr_weight=100.0, delta_grid_lr_weight=100.0, rgb_weight=10.0, sem_weight=0.0, inst_weight=0.0, inst_loss=None,
           optimize_extrinsics=True, extrinsics_lr=1e-3, anchor_frame_idxs=[0], epochs=3, save_every=-1, valid_every=-1, prune_at_epoch=1,
           sem_epoch_start=99, inst_epoch_start=99, use_graphs=False)


def run_trainer(dev, log_dir, **over):
    """A tiny RGB-D scene (4 views of 24 x 24 pixels, the sphere over the plane), three epochs of two steps, a prune after epoch 1.  -> the trainer,
    the sample count of every march, and the epochs' total losses."""
    from pagnerf_amd import config
    torch.manual_seed(11)
    views = cases.down_views(4)
    ds, _ = cases.rgbd_dataset(views, TH, TW, dev, with_rays=False)
    ds.semantic_info = dict(num_classes=5, num_instances=16, things_ids=[2, 3, 4], stuff_ids=[0, 1])
    pipe, tr = config.build_from_config(dict(CFG, log_dir=str(log_dir), **over), ds, None, device=dev)
    with torch.no_grad():
        pipe.nef.decoder_density.lout.bias[0] = 2.96          # densities astride the prune threshold, so that the prune keeps some cells and drops others
        for g in (pipe.nef.grid, pipe.nef.delta_grid):
            g.tables.normal_(0.0, 1e-2)
    counts, march = [], pipe.nef.grid.raymarch

    def counted(*args, **kw):
        out = march(*args, **kw)
        counts.append(int(out[0].numel()))
        return out
    pipe.nef.grid.raymarch = counted
    losses = []
    for _ in range(3):
        tr.run_epoch()
        losses.append(tr.log_dict["total_loss"])
    return tr, counts, losses


def test_trainer_carves_before_the_first_step(gpu_device, tmp_path):
    from pagnerf_amd import carve
    tr, counts, losses = run_trainer(gpu_device, tmp_path / "carved", carve_from_depth=True)
    nef = tr.pipeline.nef
    rep = tr.carve_report
    assert rep is not None and rep["views"] == 4 and rep["valid_pixels"] > 0 and not tr._carve_pending
    carved = nef.grid.carve_bits
    assert carved is not None and torch.equal(nef.delta_grid.carve_bits, carved)
    kept = carve.unpack_bits(carved.cpu(), 8 ** 5)
    seen_free = cases.cell_of(torch.tensor([[0.25, 0.0, 0.7]]), 5)               # straight below camera 0 (z = 0.95), well above the sphere (z < 0.35)
    assert not kept[seen_free].any() and 0.02 < rep["occupied"] < 0.98
    on_sphere = cases.cell_of(torch.tensor([[0.0, 0.0, 0.35], [0.3, 0.3, -0.4]]), 5)               # the sphere's top and a point of the plane
    assert kept[on_sphere].all()
    assert tr.epoch == 3 and tr.plan["epoch"] == 2 and all(l == l and abs(l) != float("inf") for l in losses)
    for g in (nef.grid, nef.delta_grid):                                         # after the prune of epoch 1: nothing outside the carve
        assert torch.equal(g.blas_bits & ~g.carve_bits, torch.zeros_like(g.blas_bits))
        assert not g._all_occupied
    sd = tr.state_dict()["pipeline"]
    assert torch.equal(sd["nef.grid.carve_bits"], carved) and torch.equal(sd["nef.delta_grid.carve_bits"], carved)

    plain, plain_counts, plain_losses = run_trainer(gpu_device, tmp_path / "plain")
    assert plain.carve_report is None and plain.pipeline.nef.grid.carve_bits is None
    assert "nef.grid.carve_bits" not in plain.state_dict()["pipeline"]
    assert 0 < counts[0] < plain_counts[0]                                        # the first step marches fewer samples: same rays, same jitter
    assert all(l == l for l in plain_losses)
    assert (plain.pipeline.nef.grid.blas_bits & ~carved).any()                    # the same prune without the carve keeps cells that the carve removed

    path = tr.save_checkpoint(str(tmp_path / "carved" / "model.pth"))            # a carved run's checkpoint into a trainer built the same way
    from pagnerf_amd import config
    ds, _ = cases.rgbd_dataset(cases.down_views(4), TH, TW, gpu_device, with_rays=False)
    ds.semantic_info = dict(num_classes=5, num_instances=16, things_ids=[2, 3, 4], stuff_ids=[0, 1])
    fresh_pipe, fresh = config.build_from_config(dict(CFG, log_dir=str(tmp_path / "resumed"), carve_from_depth=True), ds, None, device=gpu_device)
    fresh.resume(path)
    assert not fresh._carve_pending
    for name in ("grid", "delta_grid"):
        g, src = getattr(fresh_pipe.nef, name), getattr(nef, name)
        assert torch.equal(g.carve_bits.cpu(), src.carve_bits.cpu()) and torch.equal(g.blas_bits.cpu(), src.blas_bits.cpu()) and not g._all_occupied
