"""CPU-side checks of the depth carve (pagnerf_amd/carve.py, csrc/carve.hip): the tensor-op walk against the scalar oracle, properties of the carved
sets that hold by construction, the depth-to-ray-length conversion, OccupancyBLAS.set_carve with its checkpoints, carve_occupancy's plumbing on a CPU
dataset, the trainer's options, and the argument validation of the two entry points (no launch happens without a GPU: every call here is refused)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import carve_cases as cases
from carve_cases import DIST_MAX, DIST_MIN


# ------------------------------------------------------------------------------------------------------------------- the walk against the oracle
@pytest.mark.parametrize("level", [3, 5])
def test_walk_candidates_equal_the_oracle(level):
    """40 random rays and the edge rays: the candidates of carve.walk_candidates are oracle.render.raymarch_voxel's nuggets (no occupancy, one sample
    per nugget) - ray ids and cells exactly, and the sample depth t_in + (t_out - t_in) * 0.5 and the delta t_out - t_in, evaluated in fp32 in the
    oracle's order, bit for bit."""
    from oracle.render import raymarch_voxel
    o, d, _ = cases.ray_set(40 + len(cases.EDGE_RAYS), seed=level)
    ridx, pidx, _, depths, deltas, _ = raymarch_voxel(o, d, DIST_MIN, DIST_MAX, 1, occupancy=None, blas_level=level)
    rays, cells, t_in, t_out = cases.candidates(o, d, level)
    assert ridx.numel() > 200
    assert torch.equal(rays, ridx) and torch.equal(cells, pidx)
    span = t_out - t_in
    assert torch.equal(t_in + span * torch.tensor(0.5), depths.reshape(-1))
    assert torch.equal(span, deltas.reshape(-1))
    per_ray = torch.bincount(ridx, minlength=o.shape[0])
    assert per_ray[3] == 0 and per_ray[4] == 0 and per_ray[0] > 0             # the two misses, the ray from inside


@pytest.mark.parametrize("level", [3, 5])
def test_classification_follows_the_candidates(level):
    """carve_reference's two sets are the candidates classified by the issue's rule, evaluated here per candidate from the walk's own t_in / t_out."""
    from pagnerf_amd import carve
    o, d, t = cases.ray_set(40 + len(cases.EDGE_RAYS), seed=10 + level)
    for margin in (0.0, 0.1, 10.0):
        free, surface = carve.carve_reference(o, d, t, DIST_MIN, DIST_MAX, margin, level)
        rays, cells, t_in, t_out = cases.candidates(o, d, level)
        th = t[rays]
        valid = torch.isfinite(th) & (th > 0)
        lo, hi = th - torch.tensor(margin), th + torch.tensor(margin)
        s = valid & (t_in <= hi) & (t_out >= lo)
        f = valid & ~s & (t_out <= lo)
        want_s, want_f = torch.zeros(8 ** level, dtype=torch.bool), torch.zeros(8 ** level, dtype=torch.bool)
        want_s[cells[s]] = True
        want_f[cells[f]] = True
        assert torch.equal(carve.unpack_bits(surface, 8 ** level), want_s) and torch.equal(carve.unpack_bits(free, 8 ** level), want_f)
        assert not valid[(rays >= 7) & (rays <= 10)].any()                      # t_hit 0, negative, NaN, +inf write nothing
        if margin == 0.0:
            assert not s[rays == 5].any() and not f[rays == 5].any()            # t_hit before the entry
            assert f[rays == 6].all() and (rays == 6).sum() > 0                 # t_hit beyond the exit: every crossed cell is free
        if margin == 10.0:
            assert s[valid].all() and not want_f.any()                          # a margin larger than the cube: everything crossed is surface
    again = carve.carve_reference(o[:5], d[:5], t[:5], DIST_MIN, DIST_MAX, 0.1, level, free, surface)          # ORs into what it is given
    assert torch.equal(again[0] & free, free) and torch.equal(again[1] & surface, surface)


def test_pack_and_unpack_bits():
    from pagnerf_amd import carve
    g = torch.Generator().manual_seed(3)
    for cells in (1, 8, 512, 32768):
        m = torch.rand(cells, generator=g) < 0.5
        bits = carve.pack_bits(m)
        assert bits.dtype == torch.int32 and bits.numel() == max(1, cells // 32)
        assert torch.equal(carve.unpack_bits(bits, cells), m)
    assert carve.num_words(0) == 1 and carve.num_words(1) == 1 and carve.num_words(3) == 16 and carve.num_words(5) == 1024


# ------------------------------------------------------------------------------------------------------------------ properties by construction
@pytest.fixture(scope="module")
def sphere():
    """The sphere of radius 0.5 seen by six axis cameras of 12 x 12 pixels with exact t_hit, carved at level 5 with the default margin (two cells)."""
    from pagnerf_amd import carve
    level = 5
    o, d, t = cases.sphere_views()
    free, surface = carve.carve_reference(o, d, t, DIST_MIN, DIST_MAX, 2 * 2.0 / 2 ** level, level)
    out = {(mode, dil): carve.carve_finish_reference(free, surface, level, dil, mode) for mode in ("hull", "band") for dil in (0, 1)}
    return dict(level=level, o=o, d=d, t=t, free=free, surface=surface, out=out)


def test_sphere_surface_cells_are_kept(sphere):
    from pagnerf_amd import carve
    level, t = sphere["level"], sphere["t"]
    valid = t > 0
    assert 300 < int(valid.sum()) < t.numel()                                    # the cameras see the sphere and the space beside it
    hit = cases.cell_of(sphere["o"][valid] + sphere["d"][valid] * t[valid, None], level)
    for mode in ("hull", "band"):
        kept = carve.unpack_bits(sphere["out"][(mode, 0)], 8 ** level)
        assert kept[hit].all(), mode


def test_sphere_set_relations(sphere):
    from pagnerf_amd import carve
    level, out = sphere["level"], sphere["out"]
    for dil in (0, 1):
        hull, band = out[("hull", dil)], out[("band", dil)]
        assert torch.equal(hull & band, band)                                    # hull contains band
    for mode in ("hull", "band"):
        assert torch.equal(out[(mode, 1)] & out[(mode, 0)], out[(mode, 0)])      # dilate 1 contains dilate 0
        assert not torch.equal(out[(mode, 1)], out[(mode, 0)])
    R = 2 ** level
    centre = ((R // 2) * R + R // 2) * R + R // 2
    assert cases.bit(out[("hull", 1)], centre) == 1 and cases.bit(out[("band", 1)], centre) == 0       # never observed: kept by hull only
    free = carve.unpack_bits(sphere["free"], 8 ** level)
    hull1 = carve.unpack_bits(out[("hull", 1)], 8 ** level)
    assert free.sum() > 1000 and (~hull1).sum() > 500 and not (~hull1 & ~free).any()                    # something is carved, and only what was seen free
    between = cases.cell_of(torch.tensor([[0.0, 0.0, 0.95]]), level)                                     # between the +z camera and the sphere
    assert not hull1[between].any()


def test_finish_reference_small_cases():
    """carve_finish_reference on sets small enough to state: one corner cell at level 1 dilates to the whole 2^3 cube, and nothing wraps round a face."""
    from pagnerf_amd import carve
    one = carve.pack_bits(torch.tensor([True] + [False] * 7))
    zero = torch.zeros(1, dtype=torch.int32)
    assert int(carve.carve_finish_reference(zero, one, 1, 0, "band")) == 1
    assert int(carve.carve_finish_reference(zero, one, 1, 1, "band")) == 0xFF
    assert int(carve.carve_finish_reference(one, zero, 1, 0, "hull")) == 0xFE                            # the bits past R^3 stay 0
    m = torch.zeros(8, 8, 8, dtype=torch.bool)
    m[0, 3, 7] = True
    got = carve.unpack_bits(carve.carve_finish_reference(torch.zeros(16, dtype=torch.int32), carve.pack_bits(m), 3, 1, "band"), 512).reshape(8, 8, 8)
    want = torch.zeros(8, 8, 8, dtype=torch.bool)
    want[0:2, 2:5, 6:8] = True
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        carve.carve_finish_reference(zero, one, 1, 5, "hull")
    with pytest.raises(ValueError):
        carve.carve_finish_reference(zero, one, 1, 1, "shell")


# ---------------------------------------------------------------------------------------------------------------------- depth -> ray length
def test_ray_lengths_from_depth():
    from pagnerf_amd import carve
    from pagnerf_amd.map_export import pinhole_base_rays
    base = pinhole_base_rays(3, 3, 2.0, 2.5)                                     # a 3 x 3 pinhole grid, unit directions with -z forward
    u = (torch.arange(3, dtype=torch.float64) + 0.5 - 1.5)
    py, px = torch.meshgrid(u, u, indexing="ij")
    factor = torch.sqrt((px / 2.0) ** 2 + (py / 2.5) ** 2 + 1.0).reshape(-1)    # |d| / (-d.z) of (x / fx, -y / fy, -1)
    depth = torch.tensor([1.0, 2.0, 0.5, 0.0, -1.0, float("nan"), float("inf"), 3.0, 4.5]).reshape(1, 9, 1)
    t = carve.ray_lengths_from_depth(depth, base.dirs, 0.25, "z")
    assert t.shape == (1, 9)
    ok = torch.tensor([True, True, True, False, False, False, False, True, True])
    want = depth.reshape(-1).double() * 0.25 * factor
    assert torch.allclose(t[0][ok].double(), want[ok], rtol=4e-7, atol=0)       # a few fp32 roundings: the norm, the quotient, two products
    assert (t[0][~ok] == 0).all()                                                # no reading: 0 = invalid
    assert torch.equal(carve.ray_lengths_from_depth(depth, base.dirs * 3.0, 0.25, "z"), t) or \
        torch.allclose(carve.ray_lengths_from_depth(depth, base.dirs * 3.0, 0.25, "z"), t, rtol=4e-7)   # the directions' length does not matter
    r = carve.ray_lengths_from_depth(depth[..., 0], base.dirs, 0.25, "ray")
    assert torch.equal(r[0][ok], depth.reshape(-1)[ok] * 0.25) and (r[0][~ok] == 0).all()
    far = carve.ray_lengths_from_depth(depth, base.dirs, 0.25, "z", max_range=2.5)
    assert (far[0] > 0).tolist() == [True, True, True, False, False, False, False, False, False]
    with pytest.raises(ValueError):
        carve.ray_lengths_from_depth(depth, base.dirs, 0.25, "disparity")
    with pytest.raises(ValueError):
        carve.ray_lengths_from_depth(depth[:, :8], base.dirs, 0.25)


# --------------------------------------------------------------------------------------------------------------------------- OccupancyBLAS
def test_blas_set_carve_and_checkpoints():
    from pagnerf_amd import carve
    from pagnerf_amd.grids import OccupancyBLAS
    g = torch.Generator().manual_seed(5)
    level = 3
    carved = carve.pack_bits(torch.rand(512, generator=g) < 0.6)
    mask = torch.rand(512, generator=g) < 0.5

    plain = OccupancyBLAS(level)
    assert plain.carve_bits is None and "carve_bits" not in plain.state_dict()
    plain.blas_init(mask)
    assert torch.equal(plain.blas_bits, carve.pack_bits(mask))                   # without set_carve: unchanged
    plain.blas_init_bits(carved)
    assert torch.equal(plain.blas_bits, carved)

    grid = OccupancyBLAS(level)
    grid.set_carve(carved)
    assert grid._all_occupied and (grid.blas_bits == -1).all()                   # set_carve alone does not touch the mask
    grid.blas_init(torch.ones(512, dtype=torch.bool))
    assert torch.equal(grid.blas_bits, carved) and not grid._all_occupied        # all ones -> the carve
    grid.blas_init(mask)
    assert torch.equal(grid.blas_bits, carve.pack_bits(mask) & carved)
    grid.blas_init_bits(torch.full((16,), -1, dtype=torch.int32))
    assert torch.equal(grid.blas_bits, carved)
    grid.blas_init_bits(carve.pack_bits(mask))
    assert torch.equal(grid.blas_bits & ~carved, torch.zeros_like(carved))       # a prune cannot re-open carved cells

    sd = grid.state_dict()
    assert torch.equal(sd["carve_bits"], carved)
    fresh = OccupancyBLAS(level)                                                 # a checkpoint with the buffer into a fresh grid
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.carve_bits, carved) and torch.equal(fresh.blas_bits, grid.blas_bits) and not fresh._all_occupied
    fresh.blas_init(torch.ones(512, dtype=torch.bool))
    assert torch.equal(fresh.blas_bits, carved)
    other = OccupancyBLAS(level)                                                 # a checkpoint without it: into a grid without ...
    other.load_state_dict(plain.state_dict())
    assert other.carve_bits is None and torch.equal(other.blas_bits, plain.blas_bits)
    grid.load_state_dict(plain.state_dict())                                     # ... and into a grid with it, which keeps its own
    assert torch.equal(grid.carve_bits, carved) and torch.equal(grid.blas_bits, plain.blas_bits)
    grid.set_carve(None)
    assert grid.carve_bits is None and "carve_bits" not in grid.state_dict()
    with pytest.raises(AssertionError):
        grid.set_carve(carved[:8])


def test_reference_state_dict_leaves_the_carve_out():
    import pagnerf_amd
    from pagnerf_amd.checkpoint import save_reference_state_dict
    nef = pagnerf_amd.PanopticDeltaNeF(grid_type="HashGridTorch", num_lods=4, feature_dim=2, num_classes=3, num_instances=5, sem_num_layers=1,
                                       inst_num_layers=2, panoptic_features_type="delta", blas_level=2, codebook_bitwidth=6)
    for g in (nef.grid, nef.delta_grid):
        g.init_from_resolutions([16, 16, 16, 64])
    before = set(save_reference_state_dict(pagnerf_amd.Pipeline(nef)))
    bits = torch.tensor([0x0F0F0F0F, -1], dtype=torch.int32)
    for g in (nef.grid, nef.delta_grid):
        g.set_carve(bits)
        g.blas_init_bits(bits)
    assert "grid.carve_bits" in nef.state_dict()
    after = save_reference_state_dict(pagnerf_amd.Pipeline(nef))
    assert set(after) == before and not any("carve" in k for k in after)


# ------------------------------------------------------------------------------------------------------------------- carve_occupancy, CPU path
def test_carve_occupancy_on_a_cpu_dataset():
    """The plumbing on CPU tensors, where carve_occupancy takes the tensor-op definition: views, chunks, stride, the report, and the refusals."""
    import pagnerf_amd
    from pagnerf_amd import carve
    level, h, w = 4, 12, 16
    views = cases.down_views(2)
    ds, a = cases.rgbd_dataset(views, h, w, "cpu")
    pipe = pagnerf_amd.Pipeline(cases.StubNef(level))
    bits, rep = carve.carve_occupancy(ds, pipe, dilate=1)
    t = carve.ray_lengths_from_depth(ds.source("depths"), a["base_dirs"], cases.SCALE)
    assert torch.allclose(t, a["t"], rtol=1e-5, atol=1e-6)                      # the z-depth images give back the distances along the rays
    free, surface = carve.carve_reference(a["origins"].reshape(-1, 3), a["dirs"].reshape(-1, 3), t.reshape(-1), 0.0, 1.9, 2 * 2.0 / 16, level)
    assert torch.equal(bits, carve.carve_finish_reference(free, surface, level, 1, "hull"))
    assert rep["valid_pixels"] == int((t > 0).sum()) and rep["pixels"] == 2 * h * w and rep["views"] == 2 and rep["blas_level"] == level
    assert 0 < rep["free"] < 1 and 0 < rep["surface"] < 1 and 0 < rep["occupied"] < 1 and rep["seconds"] >= 0
    assert abs(rep["occupied"] - float(carve.unpack_bits(bits, 4096).sum()) / 4096) < 1e-12
    assert "valid" in carve.report_line(rep)
    chunked, _ = carve.carve_occupancy(ds, pipe, dilate=1, chunk_views=1)
    assert torch.equal(chunked, bits)
    one, rep1 = carve.carve_occupancy(ds, pipe, views=[1], dilate=0, mode="band", margin=0.05)
    f1, s1 = carve.carve_reference(a["origins"][1], a["dirs"][1], t[1], 0.0, 1.9, 0.05, level)
    assert torch.equal(one, carve.carve_finish_reference(f1, s1, level, 0, "band")) and rep1["views"] == 1
    strided, rep2 = carve.carve_occupancy(ds, pipe, stride=2)
    pix = (torch.arange(0, h, 2)[:, None] * w + torch.arange(0, w, 2)[None]).reshape(-1)
    f2, s2 = carve.carve_reference(a["origins"][:, pix].reshape(-1, 3), a["dirs"][:, pix].reshape(-1, 3), t[:, pix].reshape(-1), 0.0, 1.9, 2 * 2.0 / 16, level)
    assert torch.equal(strided, carve.carve_finish_reference(f2, s2, level, 1, "hull")) and rep2["pixels"] == 2 * pix.numel()
    ba = pagnerf_amd.BAPipeline(cases.StubNef(level), views, near=0.0, far=1.9)                      # the cameras' rays instead of the dataset's
    via_ba, _ = carve.carve_occupancy(ds, ba, dilate=1)
    assert float((carve.unpack_bits(via_ba, 4096) != carve.unpack_bits(bits, 4096)).float().mean()) < 0.02      # same rays up to rounding

    no_depth = pagnerf_amd.DeviceMultiviewDataset(dict(imgs=a["imgs"], rays=pagnerf_amd.Rays(a["origins"], a["dirs"], 0.0, 1.9)), "cpu")
    with pytest.raises(ValueError, match="depths"):
        carve.carve_occupancy(no_depth, pipe)
    del ds.scale
    with pytest.raises(ValueError, match="scale"):
        carve.carve_occupancy(ds, pipe)
    assert torch.equal(carve.carve_occupancy(ds, pipe, scale=cases.SCALE)[0], bits)
    for bad in (dict(mode="shell"), dict(dilate=5), dict(margin=-0.1), dict(margin=float("nan")), dict(stride=0), dict(depth_kind="disparity")):
        with pytest.raises(ValueError):
            carve.carve_occupancy(ds, pipe, scale=cases.SCALE, **bad)


# ------------------------------------------------------------------------------------------------------------------------ trainer and options
def test_trainer_and_command_line_options():
    """The options' defaults, and a parsed command line: the --carve-* flags land in the namespace under the trainer's key names, the trainer reads
    them from it, and a command line without them adds no key."""
    import inspect
    from conftest import GOLDEN
    from pagnerf_amd import config, train
    from pagnerf_amd.trainer import PanopticTrainer
    sig = inspect.signature(PanopticTrainer.__init__).parameters
    defaults = dict(carve_from_depth=False, carve_margin=None, carve_dilate=1, carve_mode="hull", carve_stride=1, carve_max_range=None, carve_depth_kind="z")
    assert {k: sig[k].default for k in defaults} == defaults
    assert set(defaults) <= config.known_keys()
    tr = PanopticTrainer(None, None)
    assert tr.carve_from_depth is False and tr._carve_pending is False          # off by default: begin_epoch() never carves

    base = ["--config", os.path.join(GOLDEN, "configs", "best.yaml"), "--dataset", "unused.npz", "--set", "optimize_extrinsics=false"]
    plain = train.config_from_args(train.make_parser().parse_args(base))
    assert not any(k.startswith("carve_") for k in plain)
    tr = PanopticTrainer(None, None, **plain)
    assert not tr._carve_pending and tr.carve == dict(margin=None, dilate=1, mode="hull", stride=1, max_range=None, depth_kind="z")
    argv = base + ["--carve-from-depth", "--carve-margin", "0.2", "--carve-dilate", "2", "--carve-mode", "band", "--carve-stride", "3",
                   "--carve-max-range", "1.5"]
    cfg = train.config_from_args(train.make_parser().parse_args(argv))
    got = {k: v for k, v in cfg.items() if k.startswith("carve_")}
    assert got == dict(carve_from_depth=True, carve_margin=0.2, carve_dilate=2, carve_mode="band", carve_stride=3, carve_max_range=1.5)
    tr = PanopticTrainer(None, None, **cfg)
    assert tr.carve_from_depth and tr._carve_pending
    assert tr.carve == dict(margin=0.2, dilate=2, mode="band", stride=3, max_range=1.5, depth_kind="z")
    only = train.config_from_args(train.make_parser().parse_args(base + ["--carve-stride", "2"]))                # an option alone does not switch it on
    assert only["carve_stride"] == 2 and "carve_from_depth" not in only and not PanopticTrainer(None, None, **only)._carve_pending
    yaml_key = train.config_from_args(train.make_parser().parse_args(base + ["--set", "carve_from_depth=true", "--set", "carve_depth_kind=ray"]))
    tr = PanopticTrainer(None, None, **yaml_key)
    assert tr._carve_pending and tr.carve["depth_kind"] == "ray"
    with pytest.raises(SystemExit):
        train.make_parser().parse_args(base + ["--carve-mode", "shell"])
    for flag in ("--carve-from-depth", "--carve-margin", "--carve-dilate", "--carve-mode", "--carve-stride", "--carve-max-range"):
        assert flag in train.__doc__


# ------------------------------------------------------------------------------------------------------- from a BUP20 folder to the carve
@pytest.fixture(scope="module")
def bup20_tree(tmp_path_factory):
    import bup20_scene as S
    root = str(tmp_path_factory.mktemp("bup20_carve") / "BUP_20")
    os.makedirs(root)
    return root, S.write_tree(root)


def test_bup20_training_window_keeps_depths_for_the_carve(bup20_tree, monkeypatch):
    """The path a user takes: a BUP20 folder loaded as train.load_dataset loads it.  Without carve_from_depth the training window has no `depths`
    (the reference's mode filter) and carve_occupancy says how to get them; with the key it has them - the validation window's own values for the
    same frames' definition - and carve_occupancy accepts the dataset."""
    import bup20_scene as S
    import pagnerf_amd
    from pagnerf_amd import bup20, carve, train
    root, scene = bup20_tree
    assert bup20.filter_load_modes(["semantics", "depths", "preds_deeplab"], "train") == ("preds_deeplab", ["semantics"])
    assert bup20.filter_load_modes(["semantics", "preds_deeplab"], "train", keep_depths=True) == ("preds_deeplab", ["semantics", "depths"])
    assert bup20.filter_load_modes(["semantics", "depths", "preds_deeplab"], "val", keep_depths=True)[1] == ["semantics", "depths"]
    cfg = dict(mip=1, load_modes=["imgs", "semantics", "instance", "preds_deeplab"], max_depth=1.4, seq_num_frames=S.SEQ_NUM_FRAMES)
    pipe = pagnerf_amd.Pipeline(cases.StubNef(3))

    plain = train.load_dataset(root, "train", cfg, "cpu")
    assert "depths" not in plain.modes
    with pytest.raises(ValueError, match="keep_depths"):
        carve.carve_occupancy(plain, pipe)
    assert "depths" not in train.load_dataset(root, "val", dict(cfg, carve_from_depth=True), "cpu").modes       # the key acts on the training window only

    ds = train.load_dataset(root, "train", dict(cfg, carve_from_depth=True), "cpu")
    assert set(ds.modes) == set(plain.modes) | {"depths"} and ds.scale == plain.scale
    for key in plain.modes:                                                      # everything else is what it was
        for field in ((None,) if plain.source(key) is not None else ("origins", "dirs")):
            assert torch.equal(ds.source(key, field), plain.source(key, field)), key
    pos = S.window_positions("train", 6)
    raw = torch.from_numpy(np.stack([scene["depths"][scene["ts"][p]] for p in pos]).view(np.int16))
    img = torch.from_numpy(np.stack([scene["images"][scene["ts"][p]] for p in pos]))
    want = bup20.prepare_frames_reference(img, 1, "white", raw)["depths"]
    h, w = ds.image_shape
    assert torch.equal(ds.source("depths").reshape(len(pos), h, w, 1), want) and float(want.max()) > 0

    bits, rep = carve.carve_occupancy(ds, pipe)
    assert rep["views"] == len(pos) and rep["valid_pixels"] == int((want > 0).sum()) and rep["pixels"] == len(pos) * h * w
    t = carve.ray_lengths_from_depth(ds.source("depths"), ds.source("base_rays", "dirs"), ds.scale)
    free, surface = carve.carve_reference(ds.source("rays", "origins").reshape(-1, 3), ds.source("rays", "dirs").reshape(-1, 3), t.reshape(-1),
                                          *ds.rays_range("rays"), 2 * 2.0 / 8, 3)
    assert torch.equal(bits, carve.carve_finish_reference(free, surface, 3, 1, "hull"))

    calls = []                                                                   # the .npz route: python -m pagnerf_amd.bup20 --keep-depths
    monkeypatch.setattr(bup20, "load_bup20", lambda *a, **k: calls.append(k) or ds)
    monkeypatch.setattr(np, "savez", lambda f, **arrays: calls.append(arrays))
    assert bup20.main([root, "--split", "train", "--keep-depths", "--device", "cpu", "--out", os.devnull]) == 0
    assert calls[0]["keep_depths"] is True and "depths" in calls[1] and "scale" in calls[1]


# ------------------------------------------------------------------------------------------------------------------------------- ABI refusals
@pytest.fixture(scope="module")
def lib():
    from pagnerf_amd import _lib
    from pagnerf_amd.build import LIB
    if not os.path.exists(LIB):
        pytest.skip("libpagnerf_hip.so is not built")
    return _lib.load()


def test_entry_points_are_declared_and_abi_stays_15(lib):
    from pagnerf_amd import _lib
    assert {"pag_carve_rays", "pag_carve_finish"} <= set(_lib.EXPORTS) and lib.pag_abi_version() == 15
    assert (_lib.CARVE_HULL, _lib.CARVE_BAND, _lib.CARVE_MAX_DILATE) == (0, 1, 4)
    C = ctypes
    assert _lib._SIGS["pag_carve_rays"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib._SIGS["pag_carve_finish"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p])


def test_carve_rays_refusals(lib):
    """Every refusal happens before a launch and before a pointer is read: the "buffers" are NULL or an address that must not be touched."""
    from pagnerf_amd import _lib
    P = 0x1000                                                                   # never dereferenced on the host: a refusal comes first
    ok = dict(o=P, d=P, t=P, N=4, dmin=0.0, dmax=6.0, margin=0.1, level=5, free=P, surf=P)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pag_carve_rays(a["o"], a["d"], a["t"], a["N"], a["dmin"], a["dmax"], a["margin"], a["level"], a["free"], a["surf"], None)
    for kw in (dict(N=-1), dict(level=-1), dict(level=11), dict(margin=-0.5), dict(margin=float("nan")), dict(o=None), dict(d=None), dict(t=None),
               dict(free=None), dict(surf=None)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"pag_carve_rays" in lib.pag_last_error_string()
    assert call(N=0, o=None, d=None, t=None, free=None, surf=None) == _lib.OK   # N == 0 is a no-op
    assert call(N=0, margin=-1.0) == _lib.ERR_ARG                                # ... but not with arguments that are wrong anyway


def test_carve_finish_refusals(lib):
    from pagnerf_amd import _lib
    P = 0x1000

    def call(free=P, surf=P, level=5, dilate=1, mode=0, out=P):
        return lib.pag_carve_finish(free, surf, level, dilate, mode, out, None)
    for kw in (dict(level=-1), dict(level=11), dict(dilate=-1), dict(dilate=5), dict(mode=2), dict(mode=-1), dict(free=None), dict(surf=None), dict(out=None)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"pag_carve_finish" in lib.pag_last_error_string()


def test_ops_wrappers_refuse_cpu_tensors():
    from pagnerf_amd import ops
    z = torch.zeros(16, dtype=torch.int32)
    r = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.carve_rays(r, r, torch.ones(4), 0.0, 6.0, 0.1, 3, z, z.clone())
    with pytest.raises(RuntimeError, match="GPU"):
        ops.carve_finish(z, z.clone(), 3)
