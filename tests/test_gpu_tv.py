"""pag_tv_fwd / pag_tv_bwd (csrc/regularizer.hip) on the GPU against the tensor-op form of pagnerf_amd/regularizers.py (the definition) on the same device
tensors and against the reference's values in tests/golden/g17_tv.npz; then through the grids, the instance path of a nef and a traced step (graph and
eager).  Reads only the repository.

Gates (the convention of test_gpu_triplanar.py).  Value: relative distance to the tensor-op form run in fp64 at most 3 x floor + 1e-6, where the floor is the
distance between the form in fp32 and in fp64 on those inputs - computed here from the definition alone and printed.  fp32 gradients: rtol 1e-5 / atol
1e-6 max|g| (an element is at most six terms of like magnitude summed in another order: about 12 fp32 roundings).  Half gradients: the fp32 gradient of the
form rounded to the input dtype, to one unit in the last place (rtol 2^-7 for bf16, 2^-10 for fp16).  Table gradients through the grids: rtol 2e-4 / atol
2e-5 max|g|, the project's gate for atomic-summed table gradients.

The half gate has no absolute term, so it is met only by a backward that rounds as the form's autograd does.  Measured on an MI355X with the first version of
tv_bwd_kernel (terms summed, then scaled once): [6,6,6,200] bf16, power 2, 4 of 43 200 elements off by 2^-24 absolute, relative 1 - elements whose terms cancel
exactly, where that kernel gave 0 and the form 2^-24; power 1 and every fp32 case matched.  The kernel therefore scales every term on its own and adds them in the
form's order (csrc/regularizer.hip)."""
import numpy as np
import pytest
import torch

import test_gpu_parity as T
import tv_cases as TC
from conftest import golden

pytestmark = pytest.mark.gpu

HALF_RTOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


@pytest.fixture(scope="module")
def g17():
    return golden("g17_tv.npz")


def _R():
    from pagnerf_amd import regularizers as R
    return R


def _kernel(x, power, scale=None):
    """-> (value, gradient) through the kernels."""
    R = _R()
    assert R.TV_KERNELS
    xx = x.detach().clone().requires_grad_(True)
    out = R.tv_loss(xx, power)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.device == x.device
    (out if scale is None else scale * out).backward()
    assert xx.grad.dtype == x.dtype and xx.grad.shape == x.shape
    return out.detach(), xx.grad.detach()


def _form(x, power, dtype=None, scale=None):
    """-> (value, gradient) of the tensor-op form; dtype: run it on x converted to that dtype (the gradient is then of that dtype)."""
    R = _R()
    xx = (x.detach() if dtype is None else x.detach().to(dtype)).clone().requires_grad_(True)
    out = R.tv_loss_form(xx, power)
    (out if scale is None else scale * out).backward()
    return out.detach(), xx.grad.detach()


def _grad_gate(got, want, what):
    w = want.float().cpu().numpy()
    np.testing.assert_allclose(got.float().cpu().numpy(), w, rtol=1e-5, atol=1e-6 * float(np.abs(w).max()), err_msg=what)


def _check(x, power, what, g17=None, name=None):
    got_v, got_g = _kernel(x, power)
    form_v, form_g = _form(x, power)                                    # half input: the form on x.float(), gradient cast back to x.dtype
    f32_v, f32_g = _form(x, power, torch.float32)
    f64_v, _ = _form(x, power, torch.float64)
    floor = abs(float(f32_v) - float(f64_v)) / abs(float(f64_v))
    dist = abs(float(got_v) - float(f64_v)) / abs(float(f64_v))
    print("%s power %d: value %.9g  floor (form fp32 vs fp64) %.3e  kernel vs fp64 %.3e" % (what, power, float(got_v), floor, dist))
    assert dist <= 3.0 * floor + 1e-6, (what, power, dist, floor)
    if x.dtype == torch.float32:
        _grad_gate(got_g, f32_g, what)
    else:
        want = f32_g.to(x.dtype).float().cpu().numpy()
        err = np.abs(got_g.float().cpu().numpy() - want) / np.maximum(np.abs(want), 1e-30)
        print("%s power %d: half gradient, largest relative distance to the rounded fp32 gradient %.3e" % (what, power, float(err[want != 0].max())))
        np.testing.assert_allclose(got_g.float().cpu().numpy(), want, rtol=HALF_RTOL[x.dtype], atol=0, err_msg=what)
        assert torch.equal(form_g, f32_g.to(x.dtype))
    if g17 is not None:
        tag = "l%d" % power
        ref = float(g17["%s_%s" % (name, tag)])
        assert abs(float(got_v) - ref) / abs(ref) <= 3.0 * floor + 1e-6, (what, float(got_v), ref)
        if name in TC.GRAD_CASES:
            _grad_gate(got_g, torch.from_numpy(g17["%s_%s_grad" % (name, tag)]), what + " vs g17")
    return got_v, got_g


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("name,seed,shape,dtype", TC.CASES, ids=[c[0] for c in TC.CASES])
def test_kernels_against_the_form_and_the_reference(gpu_device, g17, name, seed, shape, dtype, power):
    x = TC.case(name).to(gpu_device)
    _, g = _check(x, power, name, g17, name)
    if name == "s4445_const" and power == 1:
        _, fg = _form(x, 1)
        assert torch.equal(g == 0, fg == 0) and bool((g == 0).any())                      # sign(0) = 0: the same exact zeros as torch.abs gives


@pytest.mark.parametrize("shape,dtype", [((2, 1, (1 << 20) + 5, 1), torch.float32), ((2, (1 << 20) + 5, 1, 1), torch.float32),
                                         ((3, 5, (1 << 20) + 1, 4), torch.float32), ((2, (1 << 20) + 5, 3, 8), torch.bfloat16)])
def test_long_axes(gpu_device, shape, dtype):
    """An axis of 2^20 points or more: the per-thread carry of the point index is a compare there, not a division."""
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen).to(dtype).to(gpu_device)
    for power in (1, 2):
        _check(x, power, "long %s" % (shape,))


@pytest.mark.parametrize("shape,dtype", [((5, 3, 2, 8), torch.float32), ((3, 3, 3, 16), torch.bfloat16), ((33, 9, 5, 8), torch.float16)])
def test_buffer_that_is_not_16_byte_aligned(gpu_device, shape, dtype):
    """C allows 16-byte channel vectors but the storage offset does not: the single-element kernels, same results as the aligned copy's."""
    n = int(np.prod(shape))
    gen = torch.Generator().manual_seed(n)
    base = torch.randn(n + 1, generator=gen).to(dtype).to(gpu_device)
    x = base[1:].view(shape)
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    for power in (1, 2):
        v, g = _check(x, power, "offset %s" % (shape,))
        v2, g2 = _kernel(x.clone(), power)
        assert x.clone().data_ptr() % 16 == 0
        _grad_gate(g, g2, "offset vs aligned")
        assert abs(float(v) - float(v2)) <= 1e-6 * abs(float(v2))


def test_two_runs_give_the_same_bits(gpu_device):
    for name in ("s331796", "s99948", "s666200_bf16"):
        x = TC.case(name).to(gpu_device)
        for power in (1, 2):
            a, b = _kernel(x, power), _kernel(x, power)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (name, power)


def test_upstream_scalar_is_read_on_the_device(gpu_device):
    """(3.5 * loss).backward(): the gradient is the form's for the same expression; nothing in the forward or the backward synchronises with the host."""
    for name in ("s5437", "s666200_f16"):
        x = TC.case(name).to(gpu_device)
        for power in (1, 2):
            _kernel(x, power)                                                              # library load, allocator warm-up
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                scale = torch.full((), 3.5, device=gpu_device)
                v, g = _kernel(x, power, scale=scale)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            _, want = _form(x, power, torch.float32, scale=3.5)
            _, plain = _kernel(x, power)
            if x.dtype == torch.float32:
                _grad_gate(g, want, name)
            else:
                np.testing.assert_allclose(g.float().cpu().numpy(), want.to(x.dtype).float().cpu().numpy(), rtol=HALF_RTOL[x.dtype], atol=0)
            assert not torch.equal(g, plain)


def test_non_contiguous_input(gpu_device):
    gen = torch.Generator().manual_seed(12)
    base = torch.randn(7, 3, 4, 5, generator=gen).to(gpu_device)
    x = base.permute(3, 2, 1, 0)                                                             # [5,4,3,7], strides reversed
    assert not x.is_contiguous()
    for power in (1, 2):
        xx = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        assert not xx.is_contiguous()
        out = _R().tv_loss(xx, power)
        out.backward()
        v, g = _kernel(x.contiguous(), power)
        assert torch.equal(out.detach(), v) and torch.equal(xx.grad, g)
        _check(x.contiguous(), power, "permuted")


def test_offsets_past_2_31_elements(gpu_device):
    """[1030, 2048, 128, 8] fp16: 2.16e9 elements, so the last slabs sit past element 2^31.  Value against the form summed slab-chunk by slab-chunk in fp64;
    gradient of the last two slabs against the form on the last three (whose gradient there is the whole tensor's, up to the 1 / shape[0] factor)."""
    R = _R()
    d0, rest = 1030, (2048, 128, 8)
    free, _ = torch.cuda.mem_get_info()
    assert free > 24 << 30, "needs 24 GB of free device memory"
    gen = torch.Generator(device=gpu_device).manual_seed(5)
    x = torch.empty((d0,) + rest, dtype=torch.float16, device=gpu_device)
    for i in range(0, d0, 103):
        x[i:i + 103] = torch.randn((min(103, d0 - i),) + rest, generator=gen, device=gpu_device).half()
    slab = x[0].numel()
    assert x.numel() - 2 * slab > 1 << 31                                                     # the last two slabs lie wholly past element 2^31
    total = torch.zeros((), dtype=torch.float64, device=gpu_device)
    for i in range(0, d0, 64):
        c = x[i:min(i + 65, d0)].float()                                                     # one slab of overlap: the x differences that cross chunks
        own = min(64, d0 - i)
        total += (c[1:] - c[:-1]).pow(2).sum(dtype=torch.float64)
        total += (c[:own, 1:] - c[:own, :-1]).pow(2).sum(dtype=torch.float64) + (c[:own, :, 1:] - c[:own, :, :-1]).pow(2).sum(dtype=torch.float64)
        del c
    want = float(total) / d0
    xx = x.requires_grad_(True)
    out = R.tv_l2_loss(xx)
    out.backward()
    got = float(out)
    print("2^31: value %.9g  fp64 chunked %.9g  relative %.3e" % (got, want, abs(got - want) / want))
    assert abs(got - want) / want <= 1e-6                                                    # fp32 partials of <= 96 terms, fp64 from there on
    got_g = xx.grad
    for sl, keep in ((slice(d0 - 3, d0), slice(1, 3)), (slice(0, 3), slice(0, 2))):           # the last two slabs (past 2^31) and the first two
        part = x.detach()[sl].float().requires_grad_(True)
        R.tv_loss_form(part, 2).backward()
        want_g = (part.grad[keep] * (3.0 / d0)).half().float().cpu().numpy()                 # the form divides by its own shape[0] = 3
        assert np.abs(want_g).max() > 0
        rows = got_g[sl][keep].float().cpu().numpy()
        np.testing.assert_allclose(rows, want_g, rtol=2.0 ** -10, atol=2.0 ** -24)           # one fp16 unit in the last place (2^-24: a subnormal's)


# ------------------------------------------------------------------------------------------------------------------------------ through the grids
def _small_grid(kind, dev):
    import pagnerf_amd
    torch.manual_seed(3)
    if kind == "permuto":
        g = pagnerf_amd.PermutoGridHIP(2, capacity_log_2=8, num_lods=4, coarsest_scale=1.0, finest_scale=0.01, blas_level=3)
        g.init_from_scales(tables=torch.randn(4, 256, 2) * 0.1)
    elif kind == "hash":
        g = pagnerf_amd.HashGridHIP(2, codebook_bitwidth=8, blas_level=3)
        g.init_from_resolutions([16, 32, 64])
        with torch.no_grad():
            g.tables.copy_(torch.randn(g.tables.shape) * 0.1)
    else:
        g = pagnerf_amd.TriplanarGridHIP(4, base_lod=1, num_lods=2, feature_std=0.1, feature_bias=0.1, blas_level=3)
    return g.to(dev)


@pytest.mark.parametrize("lattice", ["reference", "step"])
@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("kind", ["permuto", "hash", "triplanar"])
def test_through_the_grids(gpu_device, kind, power, lattice, monkeypatch):
    """grid_tv_l{1,2}_loss(grid.interpolate, n = 4): tables.grad through the kernels equals tables.grad through the tensor-op form (both go through the
    same encode kernels), on the reference's lattice (spacing 1.0) and on a 0.05-spaced one."""
    R = _R()
    grid = _small_grid(kind, gpu_device)
    fn = R.grid_tv_l1_loss if power == 1 else R.grid_tv_l2_loss
    kw = dict(sample_size=0.2, num_dim_samples=4, device=gpu_device)
    if lattice == "step":
        kw.update(step=0.05)
    res = {}
    for kernels in (True, False):
        monkeypatch.setattr(R, "TV_KERNELS", kernels)
        grid.tables.grad = None
        torch.manual_seed(21)
        out = fn(grid.interpolate, **kw)
        out.backward()
        res[kernels] = (float(out), grid.tables.grad.detach().float().cpu().numpy().copy())
    (v1, g1), (v0, g0) = res[True], res[False]
    print("%s power %d %s: value %.9g (kernels) %.9g (form), max|g| %.3e" % (kind, power, lattice, v1, v0, float(np.abs(g0).max())))
    assert np.abs(g0).max() > 0 and abs(v1 - v0) <= 1e-5 * abs(v0)
    np.testing.assert_allclose(g1, g0, rtol=2e-4, atol=2e-5 * float(np.abs(g0).max()))


def test_through_the_instance_path_of_a_nef(gpu_device):
    """The delta terms: lambda x: nef(coords=x, ray_d=None, channels='inst_embedding') on a bf16 PanopticDeltaNeF with the 200-way head, n = 3.  Gradients
    reach delta_grid.tables and decoder_inst; the main grid is read detached and gets none."""
    R = _R()
    nef, _, _, _, _ = T._make_scene(gpu_device, "bf16", N=64, S=16, cap_log2=10)
    for p in nef.parameters():
        p.grad = None
    torch.manual_seed(4)
    out = R.step_tv_terms(nef, delta_grid_tvl1_reg=1e-3, delta_grid_tvl2_reg=2e-3, tv_window_size=0.2, tv_edge_num_samples=3)
    assert out.dim() == 0 and float(out) > 0
    out.backward()
    assert nef.grid.tables.grad is None or float(nef.grid.tables.grad.abs().max()) == 0.0
    assert float(nef.delta_grid.tables.grad.abs().max()) > 0
    got = {n: p.grad for n, p in nef.decoder_inst.named_parameters()}
    assert got and all(g is not None and float(g.abs().max()) > 0 for g in got.values()), {n: g is None for n, g in got.items()}
    for n, p in nef.named_parameters():
        if n.startswith(("decoder_density", "decoder_color", "decoder_semantics")):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
    assert getattr(nef, "_feat_cache", None) is None
    # the same term as the tensor-op form gives it
    kern = nef.delta_grid.tables.grad.detach().clone()
    for p in nef.parameters():
        p.grad = None
    R.TV_KERNELS = False
    try:
        torch.manual_seed(4)
        out0 = R.step_tv_terms(nef, delta_grid_tvl1_reg=1e-3, delta_grid_tvl2_reg=2e-3, tv_window_size=0.2, tv_edge_num_samples=3)
        out0.backward()
    finally:
        R.TV_KERNELS = True
    form = nef.delta_grid.tables.grad.detach()
    print("instance path: value %.9g (kernels) %.9g (form); delta table gradient rel-L2 %.3e" % (float(out), float(out0), T._rel_l2(kern, form)))
    assert abs(float(out) - float(out0)) <= 1e-5 * abs(float(out0))
    np.testing.assert_allclose(kern.cpu().numpy(), form.cpu().numpy(), rtol=2e-4, atol=2e-5 * float(form.abs().max()))


# --------------------------------------------------------------------------------------------------------------------- with a traced step
CH = {"rgb", "depth", "semantics", "inst_embedding"}
TV_KW = dict(grid_tvl1_reg=1e-3, grid_tvl2_reg=2e-3, delta_grid_tvl1_reg=3e-3, delta_grid_tvl2_reg=4e-3, tv_window_size=0.2, tv_edge_num_samples=3)


def _grads(nef):
    from test_gpu_train_step import hip_leaves
    return {k: (v.grad.detach().clone() if v.grad is not None else None) for k, v in hip_leaves(nef).items()}


@pytest.mark.parametrize("use_graphs", [True, False])
def test_tv_terms_compose_with_a_traced_step(gpu_device, use_graphs):
    """(render_loss + step_tv_terms(...)).backward() on 64 rays x 16 samples: every parameter's gradient is the render term's plus the TV terms', taken
    separately; with use_graphs=True the step is a replay (the warm-up traces are done first).  A second step right after it works."""
    import pagnerf_amd
    from test_gpu_train_step import train_loss
    R = _R()
    dev = gpu_device
    N, S = 64, 16
    nef, _, rays, occ, jitter = T._make_scene(dev, "bf16", N=N, S=S, cap_log2=10)
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=S, bg_color="white", use_graphs=use_graphs)
    gen = torch.Generator().manual_seed(9)
    targets = (torch.rand(N, 3, generator=gen).to(dev), torch.randint(0, 6, (N,), generator=gen).to(dev), torch.randint(0, 200, (N,), generator=gen).to(dev))
    jit = jitter.to(dev)

    def render():
        rb = tracer(nef, channels=CH, rays=rays, jitter=jit, stage="train")
        return train_loss(rb.rgb, rb.semantics.float(), rb.inst_embedding.float(), *targets)

    def zero():
        for p in nef.parameters():
            p.grad = None

    for _ in range(3):                                   # eager (learns the count), capture, a replay
        zero()
        render().backward()
    if use_graphs:
        assert tracer._graphs.captures == 1 and tracer._graphs.replays >= 1
    zero()
    render().backward()
    g_render = _grads(nef)
    zero()
    torch.manual_seed(6)
    R.step_tv_terms(nef, **TV_KW).backward()
    g_tv = _grads(nef)
    assert g_tv["grid.tables"] is not None and g_tv["delta_grid.tables"] is not None
    for step in range(2):                                # the composed step, and a second one right after it
        zero()
        before = tracer._graphs.replays if use_graphs else None
        loss = render()
        torch.manual_seed(6)
        total = loss + R.step_tv_terms(nef, **TV_KW)
        total.backward()
        torch.cuda.synchronize()
        if use_graphs:
            assert tracer._graphs.replays == before + 1 and tracer._graphs.captures == 1
        g_both = _grads(nef)
        for name, both in g_both.items():
            a, b = g_render[name], g_tv[name]
            assert both is not None and a is not None, name
            want = (a.float() + b.float()) if b is not None else a.float()
            w = want.cpu().numpy()
            err = float((both.float() - want).abs().max()) / float(np.abs(w).max())
            print("step %d %-24s max|both - (render + tv)| / max|g| %.3e" % (step, name, err))
            np.testing.assert_allclose(both.float().cpu().numpy(), w, rtol=1e-5, atol=1e-6 * float(np.abs(w).max()), err_msg="%s (step %d)" % (name, step))
