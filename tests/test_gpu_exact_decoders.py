"""The fused decoders (csrc/mlp.hip, mlp_wgrad.hip, mlp_h128.hip, mlp_affine.hip) on problems whose arithmetic is exact (tests/exact_decoder.py,
proved exact on the CPU by tests/test_exact_decoder_host.py).

(a) Without output activation every element of the output, of d x1, d x2 and of every dW / db must EQUAL the fp64 reference: torch.equal over all rows and
columns, where the norm bounds of test_gpu_parity.py / test_gpu_wide_decoder.py cannot see one wrong row, a missing tail tile or a dropped slice.
(b) Behind a sigmoid / softmax head the logits are exact and the output carries the error of exp2 / rcp alone: derived forward bounds (2^-17 relative for
f32, one bf16 ulp for bf16, 2^-15 for per-ray sums) and a per-row backward bound measured on a plain f32 evaluation."""
import types

import numpy as np
import pytest
import torch

import exact_decoder as E

pytestmark = pytest.mark.gpu


def _ops():
    from pagnerf_amd import ops, _lib as L
    return ops, L


def _leaves(p, dev):
    Wg = [w.float().to(dev).requires_grad_(True) for w in p.W]
    bg = [v.float().to(dev).requires_grad_(True) for v in p.b]
    x1g = p.x1.to(dev).requires_grad_(True)
    x2g = None if p.x2 is None else p.x2.to(dev).requires_grad_(True)
    idx = None if p.idx is None else p.idx.to(dev)
    packs = None if p.packs is None else tuple(t.to(dev) for t in p.packs)
    return Wg, bg, x1g, x2g, idx, packs


def _call(family, p, dev, leaves, x1, out_bf16, mode_name, act=None):
    ops, L = _ops()
    Wg, bg, _, x2g, idx, packs = leaves
    kw = dict(x2=x2g, x2_index=idx, in_dim=p.dims[0], out_act=p.out_act if act is None else act, out_dtype=torch.bfloat16 if out_bf16 else torch.float32,
              x1_grouped=p.grouped, x2_packs=packs)
    if family == 128:
        return ops.fused_mlp128(x1, Wg, bg, **kw)
    return ops.fused_mlp(x1, Wg, bg, mode=L.MLP_FP32 if mode_name == "fp32" else L.MLP_MFMA_BF16, **kw)


def _check_input_gradients(tag, p, ref, x1g, x2g):
    in_dim = p.dims[0]
    if p.grouped is not None:
        assert x1g.grad.dtype == torch.bfloat16
        dx, pad = E.from_xcd8(x1g.grad, *p.grouped)
        E.assert_bit_equal(tag + " dx1", dx, ref.dx1)
        E.assert_bit_equal(tag + " dx1 (XCD8 padding)", pad, torch.zeros(pad.shape, dtype=torch.float64))
    else:
        assert x1g.grad.dtype == p.x1.dtype          # d x1 in the input's dtype
        E.assert_bit_equal(tag + " dx1", x1g.grad[:, :p.n1], ref.dx1)
        E.assert_bit_equal(tag + " dx1 (columns >= in_dim)", x1g.grad[:, p.n1:], torch.zeros(p.M, p.x1.shape[1] - p.n1, dtype=torch.float64))
    if x2g is not None:
        E.assert_bit_equal(tag + " dx2", x2g.grad[:, :in_dim - p.n1], ref.dx2)
        E.assert_bit_equal(tag + " dx2 (columns >= in_dim - k1)", x2g.grad[:, in_dim - p.n1:], torch.zeros(p.x2.shape[0], 32 - (in_dim - p.n1), dtype=torch.float64))


def _check_a(dev, family, p, ref, out_bf16, mode_name="bf16"):
    """One exact case, forward and backward, bit for bit."""
    tag = "width %d %s M=%d %s out=%s mode=%s:" % (family, p.dims, p.M, p.form, "bf16" if out_bf16 else "f32", mode_name)
    leaves = _leaves(p, dev)
    Wg, bg, x1g, x2g, idx, packs = leaves
    if p.grouped is not None and family == 128:          # forward only: the XCD8 padding positions hold NaN, which pag_mlp128_fwd must never multiply
        with torch.no_grad():
            quiet = _call(family, p, dev, leaves, E.to_xcd8(p.x.float(), *p.grouped, float("nan")).to(dev), out_bf16, mode_name)
        E.assert_bit_equal(tag + " out (no_grad, NaN padding)", quiet, ref.out)
    out = _call(family, p, dev, leaves, x1g, out_bf16, mode_name)
    assert out.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
    out.backward(p.go.to(dev).to(out.dtype))
    torch.cuda.synchronize()
    E.assert_bit_equal(tag + " out", out, ref.out)
    _check_input_gradients(tag, p, ref, x1g, x2g)
    for i in range(len(Wg)):
        E.assert_bit_equal(tag + " dW%d" % i, Wg[i].grad, ref.dW[i])
        E.assert_bit_equal(tag + " db%d" % i, bg[i].grad, ref.db[i])


# ------------------------------------------------------------------------------------------------------------------------ (a) 128-wide
@pytest.mark.parametrize("n_hidden", (1, 2, 3))
@pytest.mark.parametrize("form,in_dim", E.FORMS_128, ids=lambda v: str(v).replace(" ", ""))
def test_mlp128_exact_full_product(gpu_device, n_hidden, form, in_dim):
    """M = 1037: every out_dim at the ob = 1 / 4 / 7 boundaries x f32 / bf16 output, for this depth and input form."""
    for out_dim in E.OUT_DIMS_128:
        p, ref = E.problem(E.dims_128(n_hidden, in_dim, out_dim), 1037, form)
        for out_bf16 in (False, True):
            _check_a(gpu_device, 128, p, ref, out_bf16)


@pytest.mark.parametrize("M", E.M_OTHER_128)
@pytest.mark.parametrize("corner", range(len(E.CORNERS_128)))
def test_mlp128_exact_sizes(gpu_device, corner, M):
    dims, form, out_bf16 = E.CORNERS_128[corner]
    p, ref = E.problem(dims, M, form)
    _check_a(gpu_device, 128, p, ref, out_bf16)


def test_mlp128_exact_zero_gradient_tiles(gpu_device):
    """Rows [64, 128) of the upstream gradient are zero: the zero-tile early-outs, still bit for bit."""
    dims, form, out_bf16 = E.CORNERS_128[1]
    p, ref = E.problem(dims, 257, form, zero_go_rows=E.ZERO_TILE_ROWS)
    _check_a(gpu_device, 128, p, ref, out_bf16)


def test_mlp128_exact_dx1_accumulate(gpu_device):
    """dx1_accumulate onto an integer-valued held gradient: the sum is exact."""
    ops, L = _ops()
    dev = gpu_device
    p, ref = E.problem((48, 128, 128, 200), 1037, "xcd8")
    Wg, bg, x1g, _, _, _ = _leaves(p, dev)
    out = ops.fused_mlp128(x1g, Wg, bg, out_act=L.ACT_NONE, out_dtype=torch.bfloat16, x1_grouped=p.grouped)
    held = torch.from_numpy(np.random.RandomState(3).randint(-3, 4, size=(p.M, 48)).astype(np.float64))
    want = held + ref.dx1
    assert torch.equal(E.bf16_round(want), want)
    into = E.to_xcd8(held.float(), *p.grouped, 0.0).to(dev)
    dx1, _, dW, db = ops._mlp128_backward(out.grad_fn.state, out.grad_fn.saved_tensors, p.go.to(dev).bfloat16(), dx1_into=into)
    torch.cuda.synchronize()
    assert dx1 is into
    dx, pad = E.from_xcd8(into, *p.grouped)
    E.assert_bit_equal("dx1_accumulate dx1", dx, want)
    E.assert_bit_equal("dx1_accumulate padding", pad, torch.zeros(pad.shape, dtype=torch.float64))
    n = len(Wg)
    for i in range(n):
        E.assert_bit_equal("dx1_accumulate dW%d" % i, dW[i], ref.dW[i])
        E.assert_bit_equal("dx1_accumulate db%d" % i, db[i], ref.db[i])


# ------------------------------------------------------------------------------------------------------------------------- (a) 64-wide
def _with_wgrad_fused(value, fn):
    ops, _ = _ops()
    was = ops.WGRAD_FUSED
    ops.WGRAD_FUSED = value
    try:
        return fn()
    finally:
        ops.WGRAD_FUSED = was


@pytest.mark.parametrize("M", E.M_64)
@pytest.mark.parametrize("mode_name", ("fp32", "bf16"))
def test_mlp64_exact(gpu_device, mode_name, M):
    """Every input form x depth x out_dim (the OB = 1 / 2 / 4 / 7 kernels) at this size and mode; on the MFMA path with ops.WGRAD_FUSED on and off, so that
    the density-like fused kernel and the dz + pag_mlp_wgrad_batch route are each held to the reference."""
    for form, in_dim, out_bf16, modes in E.FORMS_64:
        if mode_name not in modes:
            continue
        for n_layers in (2, 3):
            for out_dim in E.OUT_DIMS_64:
                p, ref = E.problem(E.dims_64(n_layers, in_dim, out_dim), M, form)
                for fused in ((True, False) if mode_name == "bf16" else (True,)):
                    _with_wgrad_fused(fused, lambda: _check_a(gpu_device, 64, p, ref, out_bf16, mode_name + ("" if fused else ", separate wgrad")))


@pytest.mark.parametrize("mode_name,form", (("bf16", "strided"), ("bf16", "strided_bf16"), ("fp32", "strided"), ("fp32", "strided_bf16")))
def test_mlp64_exact_bf16_output_of_a_strided_input(gpu_device, mode_name, form):
    """The dtype pairs of the generic and the parity kernels that E.FORMS_64 leaves out: a bf16 output (and so a bf16 upstream gradient) of a strided f32
    or bf16 input, on both paths; M = 33 is one full tile and a one-row ragged one, the out_dims are those of the OB = 1 / 2 / 4 / 7 kernels."""
    for n_layers in (2, 3):
        for out_dim in E.OUT_DIMS_64:
            p, ref = E.problem(E.dims_64(n_layers, 32 if form == "strided" else 27, out_dim), 33, form)
            _with_wgrad_fused(False, lambda: _check_a(gpu_device, 64, p, ref, True, mode_name))


@pytest.mark.parametrize("fused", (True, False), ids=("fused_wgrad", "separate_wgrad"))
@pytest.mark.parametrize("dims,M", E.GRID_CASES_64, ids=lambda v: str(v).replace(" ", ""))
def test_mlp64_exact_second_grid_round(gpu_device, dims, M, fused):
    """M beyond 768 x 128 (the straight-line forward's grid cap) and beyond 1536 x 128 (mlp_grid's cap): the second round of tiles."""
    p, ref = E.problem(dims, M, "xcd8")
    _with_wgrad_fused(fused, lambda: _check_a(gpu_device, 64, p, ref, True, "bf16" + ("" if fused else ", separate wgrad")))


@pytest.mark.parametrize("fused", (True, False), ids=("fused_wgrad", "separate_wgrad"))
def test_mlp64_exact_zero_gradient_tiles(gpu_device, fused):
    p, ref = E.problem((48, 64, 16), 257, "xcd8", zero_go_rows=E.ZERO_TILE_ROWS)
    _with_wgrad_fused(fused, lambda: _check_a(gpu_device, 64, p, ref, True, "bf16" + ("" if fused else ", separate wgrad")))


@pytest.mark.parametrize("n_out,M", E.AFFINE_CASES)
def test_affine_xcd8_exact(gpu_device, n_out, M):
    ops, _ = _ops()
    dev = gpu_device
    p, ref = E.problem((48, n_out), M, "xcd8")
    tag = "affine_xcd8 n_out=%d M=%d:" % (n_out, M)
    Wg, bg, x1g, _, _, _ = _leaves(p, dev)
    out = ops.affine_xcd8(x1g, Wg[0], bg[0], p.grouped)
    out.backward(p.go.float().to(dev))
    torch.cuda.synchronize()
    E.assert_bit_equal(tag + " out", out, ref.out)
    _check_input_gradients(tag, p, ref, x1g, None)
    E.assert_bit_equal(tag + " dW", Wg[0].grad, ref.dW[0])
    E.assert_bit_equal(tag + " db", bg[0].grad, ref.db[0])


# --------------------------------------------------------------------------------------------------- (b) sigmoid and softmax heads
F32_FORWARD = 2.0 ** -17          # |logit| <= 16: exp2 argument <= ~46, its f32 rounding 46 * 2^-23 = 3.8e-6 relative after the exponential, + ~3 ulp
BF16_FORWARD = 2.0 ** -8          # one bf16 ulp: the rounding itself (2^-9) and a tie moved by the f32 error
COMPOSITE_FORWARD = 2.0 ** -15    # F32_FORWARD + at most 64 non-negative f32 additions


def _check_forward(tag, out, want):
    bound = BF16_FORWARD if out.dtype == torch.bfloat16 else F32_FORWARD
    err = E.forward_rel_error(out, want)
    print("%s forward: worst relative error %.3g (bound %.3g)" % (tag, err, bound))
    assert err <= bound, "%s forward: relative error %g > %g" % (tag, err, bound)


def _check_rows(tag, name, got, want, bound, cap=None):
    """Per row against the fp64 reference with the kernels' rounding points; a bf16 result is held to the reference's own bf16 rounding."""
    if got.dtype == torch.bfloat16:
        want = E.bf16_round(want)
    err, keep = E.row_errors(got, want)
    if cap is not None:
        assert float((~keep).double().mean()) <= cap
    worst = float(err[keep].max()) if bool(keep.any()) else 0.0
    print("%s %s: worst row %.3g (bound %.3g)" % (tag, name, worst, bound))
    assert worst <= bound, "%s %s: row %d off by %g > %g" % (tag, name, int(torch.argmax(err * keep)), worst, bound)


def _check_backward(tag, p, ref, bound, dx1, dx2, gW, gb):
    _check_rows(tag, "dx1", dx1, ref.dx1, bound, cap=E.SMALL_ROW_CAP)
    if dx2 is not None:
        _check_rows(tag, "dx2", dx2, ref.dx2, bound)
    for i in range(len(gW)):
        _check_rows(tag, "dW%d" % i, gW[i], ref.dW[i], bound)
        _check_rows(tag, "db%d" % i, gb[i].reshape(1, -1), ref.db[i].reshape(1, -1), bound)


def _head_reference(family, head, M):
    dims, act, form, out_bf16, max_logit = head
    p, _ = E.problem(dims, M, form, out_act=act, max_logit=max_logit)
    rounded = E.backward_reads_bf16_out(family, dims, out_bf16)
    ref = E.reference(p, round_dz=True, out_bf16=rounded)
    bound, worst, _ = E.backward_bound(p, ref, rounded)
    return p, ref, bound, worst


def _dx1_of(p, x1g):
    return E.from_xcd8(x1g.grad, *p.grouped)[0].to(x1g.grad.dtype) if p.grouped is not None else x1g.grad[:, :p.n1]


@pytest.mark.parametrize("family,head,M", [(128, h, M) for h in E.HEADS_128 for M in E.M_HEADS_128] + [(64, h, M) for h in E.HEADS_64 for M in E.M_HEADS_64],
                         ids=lambda v: str(v).replace(" ", ""))
def test_activated_heads(gpu_device, family, head, M):
    """fused_mlp128 / fused_mlp behind a sigmoid or softmax: exact logits, so the output carries the error of exp2 / rcp alone; the backward per row within
    4 x what a plain f32 evaluation with the same rounding points loses (floor 2^-8)."""
    _check_activated_head(gpu_device, family, head, M)


@pytest.mark.parametrize("dims", ((32, 64, 200), (32, 64, 64, 200)), ids=lambda v: str(v).replace(" ", ""))
def test_wide_softmax_head_of_a_strided_f32_input(gpu_device, dims):
    """The 200-way softmax behind a strided f32 input, two and three layers: no fused backward takes an f32 x1, so the probabilities are rebuilt from the
    statistics by mlp_bwd_wide_mfma with an f32 input gradient - the instantiations E.HEADS_64's XCD8 head never reaches.  Same reference and bounds as
    test_activated_heads; M = 33 is one full tile and a one-row ragged one."""
    _check_activated_head(gpu_device, 64, (dims, E.ACT_SOFTMAX, "strided", True, 8.0), 33)


def _check_activated_head(dev, family, head, M):
    dims, act, form, out_bf16, _ = head
    p, ref, bound, worst = _head_reference(family, head, M)
    tag = "width %d %s act=%d M=%d:" % (family, dims, act, M)
    print("%s f32 evaluation loses %.3g on its worst row -> bound %.3g" % (tag, worst, bound))
    leaves = _leaves(p, dev)
    Wg, bg, x1g, x2g, idx, packs = leaves
    out = _call(family, p, dev, leaves, x1g, out_bf16, "bf16")
    out.backward(p.go.to(dev).to(out.dtype))
    torch.cuda.synchronize()
    _check_forward(tag, out, ref.out)
    _check_backward(tag, p, ref, bound, _dx1_of(p, x1g), None if x2g is None else x2g.grad[:, :dims[0] - p.n1], [w.grad for w in Wg], [v.grad for v in bg])


@pytest.mark.parametrize("M", E.M_HEADS_64)
def test_colour_and_density(gpu_device, M):
    """The density decoder parked (ops.decoder_hold) and evaluated in the colour decoder's launch: its bf16 output and sigma = relu(column 0) bit for bit,
    rgb within the f32 forward bound; the colour decoder's gradients - the sigma gradient added to column 0 inside the kernel - per row."""
    ops, L = _ops()
    dev = gpu_device
    pd, rd = E.problem((48, 64, 16), M, "xcd8")
    pc = E.make_problem((43, 64, 64, 3), M, E.SEED, ("bf16", 16), out_act=E.ACT_SIGMOID, max_logit=4.0, x1_values=rd.out)
    rc = E.reference(pc, round_dz=True)
    E.check_exact(pc, rc)
    bound, worst, _ = E.backward_bound(pc, rc)
    tag = "colour_and_density M=%d:" % M
    Wd, bd, x8g, _, _, _ = _leaves(pd, dev)
    Wc, bc, _, x2g, idx, _ = _leaves(pc, dev)
    hold = ops.decoder_hold()
    try:
        dens = ops.fused_mlp(x8g, Wd, bd, in_dim=48, out_act=L.ACT_NONE, out_dtype=torch.bfloat16, x1_grouped=pd.grouped, hold=hold)
        rgb, sigma = ops.colour_and_density(dens, Wc, bc, x2g, idx, 43, out_act=L.ACT_SIGMOID, out_dtype=torch.float32, producer=hold)
    finally:
        ops.flush_hold(hold)
    assert hold.taken
    dens.retain_grad()
    g_sig = torch.from_numpy(np.random.RandomState(5).randint(-1, 2, size=M).astype(np.float64))
    ((rgb * pc.go.float().to(dev)).sum() + (sigma * g_sig.float().to(dev)).sum()).backward()
    torch.cuda.synchronize()
    E.assert_bit_equal(tag + " density output", dens, rd.out)
    E.assert_bit_equal(tag + " sigma", sigma, torch.relu(rd.out[:, 0]))
    _check_forward(tag, rgb, rc.out)
    want = types.SimpleNamespace(**vars(rc))
    want.dx1 = rc.dx1.clone()
    want.dx1[:, 0] += g_sig * (rd.out[:, 0] > 0)
    print("%s f32 evaluation loses %.3g on its worst row -> bound %.3g" % (tag, worst, bound))
    _check_backward(tag, pc, want, bound, dens.grad, x2g.grad[:, :27], [w.grad for w in Wc], [v.grad for v in bc])
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in Wd + bd + [x8g])


def _rays(M, dev):
    counts = E.rays_for(M, 17)
    N = len(counts)
    rs = np.random.RandomState(19)
    ridx = np.repeat(np.arange(N), counts)
    w = rs.randint(1, 9, size=M) / 64.0                        # dyadic weights and alpha: the upstream gradient alpha * w * g stays bf16
    alpha = 0.5 ** rs.randint(0, 3, size=N)
    t = dict(counts=counts, N=N, ridx=torch.from_numpy(ridx.astype(np.int32)).to(dev), w=torch.from_numpy(w.astype(np.float32)).to(dev),
             alpha=torch.from_numpy(alpha.astype(np.float32)).to(dev), ray_of_pack=torch.arange(N, dtype=torch.int32, device=dev),
             pack_start=torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev))
    t["ridx64"], t["w64"], t["alpha64"] = torch.from_numpy(ridx), torch.from_numpy(w), torch.from_numpy(alpha)
    return t


def _composite_reference(p, rays, g_ray, out_bf16_read):
    """fp64: the per-ray sums alpha * sum w y, and the decoder's gradients under the rank-1 upstream gradient alpha[ray] * w * g[ray]."""
    go = (rays["alpha64"][rays["ridx64"]] * rays["w64"])[:, None] * g_ray[rays["ridx64"]]
    q = E.with_go(p, go)
    ref = E.reference(q, round_dz=True, out_bf16=out_bf16_read)
    comp = torch.zeros(rays["N"], p.dims[-1], dtype=torch.float64).index_add_(0, rays["ridx64"], ref.out * rays["w64"][:, None]) * rays["alpha64"][:, None]
    bound, worst, _ = E.backward_bound(q, ref, out_bf16_read)
    return q, ref, comp, bound, worst


def _check_composite(tag, out, comp, counts, bound=None):
    bound = COMPOSITE_FORWARD if bound is None else bound
    got = out.detach().cpu().double()
    live = torch.from_numpy(counts > 0)
    assert float(got[~live].abs().max()) == 0.0, tag + " an empty ray is not zero"
    err = float(((got[live] - comp[live]).abs() / comp[live]).max())
    print("%s per-ray sums: worst relative error %.3g (bound %.3g)" % (tag, err, bound))
    assert err <= bound, "%s per-ray sums: relative error %g > %g" % (tag, err, bound)


@pytest.mark.parametrize("M", E.M_HEADS_64)
def test_head_composite(gpu_device, M):
    """The 200-way head through ops.head_composite: statistics-only forward, per-ray sums of rebuilt probabilities, rank-1 gradient in the backward."""
    ops, L = _ops()
    dev = gpu_device
    dims, act, form, _, max_logit = E.HEADS_64[0]
    p, _ = E.problem(dims, M, form, out_act=act, max_logit=max_logit)
    rays = _rays(M, dev)
    g_ray = torch.from_numpy(np.random.RandomState(23).randint(-1, 2, size=(rays["N"], dims[-1])).astype(np.float64))
    q, ref, comp, bound, worst = _composite_reference(p, rays, g_ray, E.backward_reads_bf16_out(64, dims, True))
    tag = "head_composite %s M=%d:" % (dims, M)
    Wg, bg, x1g, _, _, _ = _leaves(p, dev)
    out = ops.head_composite(x1g, Wg, bg, rays["w"], rays["alpha"], rays["ridx"], rays["pack_start"], rays["ray_of_pack"], rays["N"], in_dim=dims[0],
                             out_act=L.ACT_SOFTMAX, x1_grouped=p.grouped)
    (out * g_ray.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    _check_composite(tag, out, comp, rays["counts"])
    print("%s f32 evaluation loses %.3g on its worst row -> bound %.3g" % (tag, worst, bound))
    _check_backward(tag, q, ref, bound, _dx1_of(p, x1g), None, [w.grad for w in Wg], [v.grad for v in bg])


@pytest.mark.parametrize("M", E.M_HEADS_64)
def test_head_composite_pair(gpu_device, M):
    """The 200-way and the 6-way head on one input as one node (ops.head_composite_pair): both per-ray sums within the bound, each head's weight gradients
    per row, and the summed input gradient within the two heads' bounds on their own parts plus the one bf16 rounding of the sum."""
    _check_head_pair(gpu_device, M, E.HEADS_64[0])


def test_head_composite_pair_of_two_narrow_heads(gpu_device):
    """A three-layer 6-way head in the wide head's place: the library pairs nothing, so the first head's backward is the three-layer narrow softmax kernel
    and the second head's own launch adds its input gradient to the first one's (dx1_accumulate outside mlp_bwd_pair) - mlp_bwd_fused<3, softmax> and
    <2, softmax, accumulate>, which the shipped pair never launches.  Same references and bounds as test_head_composite_pair, at M = 33."""
    _check_head_pair(gpu_device, 33, ((48, 64, 64, 6), E.ACT_SOFTMAX, "xcd8", False, 2.0))


def _check_head_pair(dev, M, head_a):
    ops, L = _ops()
    (dims_a, _, form, _, ml_a), (dims_b, _, _, _, ml_b) = head_a, E.HEADS_64[1]
    narrow_a = dims_a[-1] <= 64          # then head a's probabilities pass through bf16 as well, before they are summed and for its backward
    pa, _ = E.problem(dims_a, M, form, out_act=E.ACT_SOFTMAX, max_logit=ml_a)
    pb = E.make_problem(dims_b, M, E.SEED, form, out_act=E.ACT_SOFTMAX, max_logit=ml_b, x1_values=pa.x)
    rays = _rays(M, dev)
    rs = np.random.RandomState(29)
    ga = torch.from_numpy(rs.randint(-1, 2, size=(rays["N"], dims_a[-1])).astype(np.float64))
    if narrow_a:
        ga[:, 0], ga[:, 1] = 1.0, -1.0
    gb = torch.from_numpy(rs.randint(-1, 2, size=(rays["N"], 6)).astype(np.float64))
    gb[:, 0], gb[:, 1] = 1.0, -1.0
    qa, ra, ca, bound_a, _ = _composite_reference(pa, rays, ga, E.backward_reads_bf16_out(64, dims_a, True))
    qb, rb, cb, bound_b, _ = _composite_reference(pb, rays, gb, True)          # the narrow head's backward reads its saved bf16 probabilities
    E.check_exact(pb, rb)
    tag = "head_composite_pair %s M=%d:" % (dims_a, M)
    Wa, ba, x1g, _, _, _ = _leaves(pa, dev)
    Wb, bb, _, _, _, _ = _leaves(pb, dev)
    oa, ob = ops.head_composite_pair(x1g, ((Wa, ba, 48), (Wb, bb, 48)), rays["w"], rays["alpha"], rays["ridx"], rays["pack_start"], rays["ray_of_pack"],
                                     rays["N"], x1_grouped=pa.grouped)
    ((oa * ga.float().to(dev)).sum() + (ob * gb.float().to(dev)).sum()).backward()
    torch.cuda.synchronize()
    _check_composite(tag + " wide", oa, ca, rays["counts"], BF16_FORWARD + COMPOSITE_FORWARD if narrow_a else COMPOSITE_FORWARD)
    got_b = ob.detach().cpu().double()
    live = torch.from_numpy(rays["counts"] > 0)
    # the narrow head's probabilities pass through bf16 before they are summed: one bf16 ulp per term
    err_b = float(((got_b[live] - cb[live]).abs() / cb[live]).max())
    print("%s narrow per-ray sums: worst relative error %.3g (bound %.3g)" % (tag, err_b, BF16_FORWARD + COMPOSITE_FORWARD))
    assert err_b <= BF16_FORWARD + COMPOSITE_FORWARD and float(got_b[~live].abs().max()) == 0.0
    for name, W, b, ref, bound in (("wide", Wa, ba, ra, bound_a), ("narrow", Wb, bb, rb, bound_b)):
        for i in range(len(W)):
            _check_rows(tag + " " + name, "dW%d" % i, W[i].grad, ref.dW[i], bound)
            _check_rows(tag + " " + name, "db%d" % i, b[i].grad.reshape(1, -1), ref.db[i].reshape(1, -1), bound)
    got = _dx1_of(pa, x1g).float().cpu().double()
    want = ra.dx1 + rb.dx1
    allowed = bound_a * ra.dx1.norm(dim=1) + bound_b * rb.dx1.norm(dim=1) + 2.0 ** -8 * want.norm(dim=1)
    over = (got - want).norm(dim=1) - allowed
    print("%s summed dx1: worst row uses %.3g of its allowance" % (tag, float(((got - want).norm(dim=1) / allowed.clamp_min(1e-300)).max())))
    assert float(over.max()) <= 0.0, "%s summed dx1: row %d" % (tag, int(torch.argmax(over)))
