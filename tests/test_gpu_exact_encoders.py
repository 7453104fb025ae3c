"""The grid encoders (csrc/encode.hip) on problems whose arithmetic is exact (tests/exact_encoder.py, proved exact on the CPU by
tests/test_exact_encoder_host.py): forward, table gradient (binned and atomic) and position gradient must EQUAL the fp64 reference - torch.equal over the
whole tensor, where the norm bounds of test_gpu_parity.py / test_gpu_sizes.py cannot see one dropped tail tile, one run merged across a boundary it must
not cross or one clipped last slice."""
import numpy as np
import pytest
import torch

import exact_encoder as E

pytestmark = pytest.mark.gpu

KINDS = ("permuto", "hash")
F32, BF16 = torch.float32, torch.bfloat16


def _ops():
    from pagnerf_amd import ops
    return ops


def _spec(p, half_coords=False):
    ops = _ops()
    if p.enc == "permuto":
        return ops.permuto_spec(p.sf, p.shift, p.rows, p.F, half_coords=half_coords)
    return ops.hash_spec(p.res, p.log2_T, p.F, half_coords=half_coords)


def _scale(p):
    return None if p.scale is None else p.scale.tolist()


def _upstream(p, dev, dtype, layout, g=None):
    """The integer upstream gradient as the kernels take it: [M,C] row-major, feature-major, or bf16 XCD8 [8,M,8]."""
    g = torch.from_numpy(p.g if g is None else g)
    if layout == "xcd8":
        return E.to_xcd8(g, p.L, p.F, 0.0).to(dev)
    g = g.to(dtype).to(dev)
    return g.t().contiguous().t() if layout == "features" else g


def _table_grad(p, dev, algo="binned", dtype=F32, layout="rows", mode="set", half_coords=False, g=None):
    """mode 'set': pag_*_encode_bwd_set into NaN-poisoned memory; 'add': pag_*_encode_bwd onto the held table (zeros without one)."""
    ops = _ops()
    xyz = torch.from_numpy(p.xyz).to(dev)
    if mode == "set":
        gt = torch.full((p.L, p.rows, p.F), float("nan"), device=dev)
    else:
        gt = torch.zeros(p.L, p.rows, p.F, device=dev) if p.held is None else torch.from_numpy(p.held).float().to(dev)
    before = ops.BWD_ALGO
    ops.BWD_ALGO = algo
    try:
        ops._encode_bwd(_spec(p, half_coords), xyz, _upstream(p, dev, dtype, layout, g), _scale(p), gt, overwrite=mode == "set")
    finally:
        ops.BWD_ALGO = before
    torch.cuda.synchronize()
    return gt


def _check_table_grad(p, dev, algo, dtype, layout, mode="set", **kw):
    tag = "%s L=%d F=%d rows=%d M=%d %s %s %s %s:" % (p.kind, p.L, p.F, p.rows, p.M, algo, str(dtype)[6:], layout, mode)
    ref = E.reference(p)
    gt = _table_grad(p, dev, algo, dtype, layout, mode, **kw)
    want = ref.gtab if (mode == "set" or p.held is None) else ref.gtab + p.held
    E.assert_bit_equal(tag + " table gradient", gt, want, shift=p.plan.shift)
    if mode == "set":          # untouched rows, cancelled sums and the zero-gradient level come back as +0
        assert not bool((torch.signbit(gt) & (gt == 0)).any()), tag + " -0 in an overwritten table"


def _all_forms(p, dev, layouts=("rows",)):
    """Every (algorithm, gradient dtype, layout) the problem's shape allows."""
    for layout in layouts:
        if layout == "xcd8":
            if ((p.L + 7) // 8) * p.F <= 8:
                _check_table_grad(p, dev, "binned", BF16, "xcd8")
            continue
        for dtype in (F32, BF16):
            _check_table_grad(p, dev, "binned", dtype, layout)
            _check_table_grad(p, dev, "atomic", dtype, layout, mode="add")


# ------------------------------------------------------------------------------------------------------------------------- table gradient
@pytest.mark.parametrize("F", (1, 2, 4))
@pytest.mark.parametrize("kind", ("permuto", "hash", "hash_lo"))
def test_exact_encoder_table_gradient_sizes(gpu_device, kind, F):
    """M = 1, TS - 1, TS, TS + 1, 3 TS + 1 (TS = 1024 / 512 samples per bin tile) x f32 / bf16 gradient x binned / atomic, row-major.  bf16 with F = 2 is the
    packed 8-byte entry: staged through LDS for the permutohedral lattice, written straight to the workspace for the hash grid."""
    for M in E.SIZES[kind]:
        _all_forms(E.problem(kind, 6, F, E.ROWS, M), gpu_device)


def test_exact_encoder_hash_1025_tiles(gpu_device):
    """L = 1, M = 512 * 1024 + 1: 1025 tiles, so reduce wave 0 walks a second group of 64 tiles (holding the one-sample tail tile), 256 slices of ~16 entries
    per tile: chunks that cross four and more tile boundaries."""
    p = E.problem(*E.BIG)
    _check_table_grad(p, gpu_device, "binned", BF16, "rows")
    _check_table_grad(p, gpu_device, "binned", F32, "rows")
    _check_table_grad(p, gpu_device, "atomic", F32, "rows", mode="add")


def test_exact_encoder_permuto_67_tiles(gpu_device):
    """67 tiles and 256 slices: 5 tiles per reduce wave, short segments with hot rows (lds_accumulate's wave pre-sum across tiles), both chunk searches."""
    p = E.problem(*E.MANY_TILES)
    _all_forms(p, gpu_device, ("rows", "xcd8"))


@pytest.mark.parametrize("L", E.XCD8_LEVELS)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_encoder_table_gradient_layouts(gpu_device, kind, L):
    """XCD8-grouped bf16 gradient with 1 .. 4 levels per workgroup, a padded last group (L = 5, 17) and fewer than 8 groups (L = 5), the wave_live skip on the
    zero waves; feature-major f32 / bf16; row-major."""
    for F in (1, 2, 4):
        if ((L + 7) // 8) * F <= 8 and L * F <= 64:
            _all_forms(E.problem(kind, L, F, E.ROWS, E.M_MAIN[kind]), gpu_device, ("xcd8", "features") if F == 2 else ("xcd8",))


@pytest.mark.parametrize("kind", KINDS)
def test_exact_encoder_reduce_geometry(gpu_device, kind):
    """NS = 1, 4 (no multiple of 8), 8 and 16 (the XCD-interleaved block order), a partial last slice, a table smaller than a slice, and the level orders of
    RED_HEAD (L = 1, 2, 3, 24)."""
    for rows, L, F in E.GEOMETRY[kind]:
        _all_forms(E.problem(kind, L, F, rows, E.M_MAIN[kind]), gpu_device, ("rows", "xcd8"))


@pytest.mark.parametrize("kind", KINDS)
def test_exact_encoder_entry_points(gpu_device, kind):
    """pag_*_encode_bwd accumulating onto a held integer table, with and without feat_scale; half_coords on and off give the same bits."""
    case = (kind, 6, 2, E.ROWS, E.M_MAIN[kind])
    for kw in ({}, dict(feat_scale=True), dict(held=True), dict(feat_scale=True, held=True)):
        p = E.problem(*case, **kw)
        for layout, dtype in (("rows", F32), ("rows", BF16), ("xcd8", BF16)):
            _check_table_grad(p, gpu_device, "binned", dtype, layout, mode="add")
            _check_table_grad(p, gpu_device, "binned", dtype, layout, mode="set")
            _check_table_grad(p, gpu_device, "binned", dtype, layout, mode="set", half_coords=True)
        _check_table_grad(p, gpu_device, "atomic", F32, "rows", mode="add")
        _check_table_grad(p, gpu_device, "atomic", BF16, "rows", mode="add", half_coords=True)


@pytest.mark.parametrize("form", ("f32", "xcd8"))
@pytest.mark.parametrize("bad", (float("inf"), float("nan")))
@pytest.mark.parametrize("kind", KINDS)
def test_exact_encoder_nonfinite_upstream(gpu_device, kind, bad, form):
    """One inf / NaN in one level's gradient: every row that level's samples touch is non-finite (what GradScaler's skipped step looks for), every other
    level equals the reference bit for bit."""
    p = E.problem(kind, 8, 2, E.ROWS, E.M_MAIN[kind])
    ref, level, sample = E.reference(p), 1, 5
    g = p.g.copy()
    g[sample, level * p.F] = bad
    dtype, layout = (F32, "rows") if form == "f32" else (BF16, "xcd8")
    others = [l for l in range(p.L) if l != level]
    for algo, mode in (("binned", "set"), ("binned", "add")) + ((("atomic", "add"),) if form == "f32" else ()):
        gt = _table_grad(p, gpu_device, algo, dtype, layout, mode, g=g).cpu()
        tag = "%s %s %s %s %s:" % (kind, bad, form, algo, mode)
        E.assert_bit_equal(tag + " the other levels", gt[others], ref.gtab[others], shift=p.plan.shift)
        touched = E.levels(p)[level].idx[sample] if algo == "atomic" else np.unique(E.levels(p)[level].idx)
        assert not bool(torch.isfinite(gt[level, torch.from_numpy(touched), 0]).any()), tag + " a touched row of the poisoned level is finite"


@pytest.mark.parametrize("kind", KINDS)
def test_exact_encoder_chunks_add_up(gpu_device, kind):
    """The table gradient of a problem equals the sum of the gradients of its two halves, split mid-tile - torch.equal, computed apart and accumulated."""
    p = E.problem(kind, 6, 2, E.ROWS, E.M_MAIN[kind])
    a, b = E.halves(p)
    for dtype, layout in ((F32, "rows"), (BF16, "rows"), (BF16, "xcd8")):
        whole = _table_grad(p, gpu_device, "binned", dtype, layout)
        ga, gb = _table_grad(a, gpu_device, "binned", dtype, layout), _table_grad(b, gpu_device, "binned", dtype, layout)
        assert torch.equal(ga + gb, whole), (kind, dtype, layout)
        E.assert_bit_equal("first half", ga, E.reference(a).gtab, shift=p.plan.shift)
        E.assert_bit_equal("second half", gb, E.reference(b).gtab, shift=p.plan.shift)
        ops = _ops()
        ops._encode_bwd(_spec(b), torch.from_numpy(b.xyz).to(gpu_device), _upstream(b, gpu_device, dtype, layout), None, ga)          # accumulate b onto a
        torch.cuda.synchronize()
        assert torch.equal(ga, whole), (kind, dtype, layout, "accumulated")


# --------------------------------------------------------------------------------------------------------- forward and position gradient
def _forward_and_xyz(p, dev, rays):
    ops = _ops()
    ref = E.reference(p, rays)
    tag = "%s L=%d F=%d M=%d:" % (p.kind, p.L, p.F, p.M)
    spec, scale = _spec(p), _scale(p)
    tab32 = torch.from_numpy(p.tables).float().to(dev)
    xcd8 = ((p.L + 7) // 8) * p.F <= 8
    for tables in (tab32, tab32.half()):
        for out_dtype in (F32, BF16):
            for feature_major in (False, True):
                xyz = torch.from_numpy(p.xyz).to(dev).requires_grad_(True)
                tg = tables.clone().requires_grad_(True)
                out = ops.encode(xyz, tg, spec, feat_scale=scale, out_dtype=out_dtype, feature_major=feature_major)
                assert out.dtype == out_dtype and out.shape == (p.M, p.L * p.F) and (out.stride(1) == p.M or not feature_major or p.M == 1)
                E.assert_bit_equal(tag + " forward %s" % out_dtype, out, ref.out)
                out.backward(_upstream(p, dev, out_dtype, "features" if feature_major else "rows"))
                torch.cuda.synchronize()
                E.assert_bit_equal(tag + " d xyz (%s gradient)" % out_dtype, xyz.grad, ref.dxyz)
                E.assert_bit_equal(tag + " d tables through autograd", tg.grad, ref.gtab, shift=p.plan.shift)
        if xcd8:
            xyz = torch.from_numpy(p.xyz).to(dev).requires_grad_(True)
            out = ops.encode(xyz, tables, spec, feat_scale=scale, layout="xcd8")
            feats, pad = E.from_xcd8(out, p.L, p.F)
            E.assert_bit_equal(tag + " forward XCD8", feats, E.bf16_round(ref.out))
            assert not bool(pad.any()), tag + " XCD8 padding not zero"
            out.backward(_upstream(p, dev, BF16, "xcd8"))
            E.assert_bit_equal(tag + " d xyz (XCD8 gradient)", xyz.grad, ref.dxyz)
            addend = torch.from_numpy(np.random.RandomState(3).randint(-3, 4, size=(8, p.M, 8))).to(BF16)
            with torch.no_grad():
                fused = ops.encode(xyz, tables, spec, feat_scale=scale, layout="xcd8", addend=addend.to(dev))
            want = (E.to_xcd8(torch.from_numpy(E.bf16_round(ref.out)), p.L, p.F, 0.0).double() + addend.double()).numpy()
            E.assert_bit_equal(tag + " forward XCD8 + addend", fused, want)
    ridx, depths, pack_start = rays
    N = len(pack_start) - 1
    for layout in ("rows", "xcd8") if xcd8 else ("rows",):
        origins, dirs = (torch.zeros(N, 3, device=dev, requires_grad=True) for _ in range(2))
        xyz = torch.from_numpy(p.xyz).to(dev).requires_grad_(True)
        tag_rays = (origins, dirs, torch.from_numpy(depths).to(dev), torch.from_numpy(pack_start).to(dev), torch.from_numpy(ridx).to(dev))
        out = ops.encode(xyz, tab32, spec, feat_scale=scale, out_dtype=BF16, layout=layout if layout == "xcd8" else None, rays=tag_rays)
        assert type(out.grad_fn).__name__.startswith("_EncodeRays")
        out.backward(_upstream(p, dev, BF16, layout))
        torch.cuda.synchronize()
        E.assert_bit_equal(tag + " d origins per ray (%s)" % layout, origins.grad, ref.drays[:, :3])
        E.assert_bit_equal(tag + " d dirs per ray (%s)" % layout, dirs.grad, ref.drays[:, 3:])


@pytest.mark.parametrize("F", (1, 2, 4))
@pytest.mark.parametrize("kind", KINDS)
def test_exact_encoder_forward_and_position_gradient_sizes(gpu_device, kind, F):
    """ops.encode forward (f32 / f16 tables; f32, bf16, feature-major, XCD8, XCD8 + addend), pag_*_encode_bwd_xyz and the per-ray pag_*_encode_bwd_rays."""
    for M in E.SIZES[kind]:
        p = E.problem(kind, 6, F, E.ROWS, M)
        _forward_and_xyz(p, gpu_device, E.rays_for(M))


@pytest.mark.parametrize("L,F", ((8, 2), (16, 1)))
@pytest.mark.parametrize("kind", KINDS)
def test_exact_encoder_forward_and_position_gradient_levels(gpu_device, kind, L, F):
    """The same with one and two levels per XCD group filled completely, and with feat_scale."""
    M = E.M_MAIN[kind]
    _forward_and_xyz(E.problem(kind, L, F, E.ROWS, M), gpu_device, E.rays_for(M))
    if (L, F) == (8, 2):
        _forward_and_xyz(E.problem(kind, 6, 2, E.ROWS, M, feat_scale=True, held=True), gpu_device, E.rays_for(M))
