"""The per-ray kernels of csrc/render.hip on problems whose arithmetic is exact (tests/exact_composite.py, proved exact on the CPU by
tests/test_exact_composite_host.py): composite_fwd / composite_bwd, the composite_feats_* family and ray_sample_grad must EQUAL the fp64 reference -
torch.equal by value over whole tensors, no tolerance anywhere - where the rtol gates of test_gpu_parity.py / test_gpu_edges.py cannot see one row dropped
from a 5000-sample pack, a carry taken from the wrong lane or a quarter left out of a sum.

Which kernel pag_composite_feats_fwd picks, by the dispatcher's own conditions, and the cases meant for each:

    C <= 16                                                        composite_feats_small_fwd_kernel<f32 | bf16>     C = 1, 7, 16
    bf16, C == 64, base a multiple of 16 bytes                     composite_feats64_bf16_fwd_kernel                C = 64 bf16
    C % 4 == 0, base a multiple of the vector (16 B f32, 8 B bf16) composite_feats_fwd_kernel<f32 | bf16, VEC>      C = 20, 200, 256; C = 64 f32;
                                                                                                                    C = 64 bf16 at base + 8 bytes
    otherwise                                                      composite_feats_fwd_kernel<f32 | bf16, scalar>   C = 17, 30, 63, 65, 201, 255;
                                                                                                                    C = 20 at base + one element"""
import numpy as np
import pytest
import torch

import exact_composite as X

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)


def _ops():
    from pagnerf_amd import ops
    return ops


def _t(x, dev, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev)


def _id(v):
    return str(v).replace(" ", "").replace("torch.", "")


def _table(p, dev):
    """(pack_start, ray_of_pack) the way each form reaches the kernels: the cached identity the march hands out (which ops._one_pack_per_ray recognises),
    ops.packs_from_boundary on the per-sample ray ids, or the permuted table as it is."""
    ops = _ops()
    if p.form == "identity":
        ray_of_pack = ops._ray_iota(p.N, dev)
        assert ops._one_pack_per_ray(ray_of_pack, p.N)
        return _t(p.pack_start, dev, torch.int64), ray_of_pack
    if p.form == "boundary":
        boundary = torch.zeros(p.rows, dtype=torch.bool)
        boundary[:p.M] = torch.from_numpy(p.boundary)
        ridx = torch.zeros(p.rows, dtype=torch.int32)
        ridx[:p.M] = torch.from_numpy(p.ray_of_sample)
        pack_start, ray_of_pack = ops.packs_from_boundary(ridx.to(dev), boundary.to(dev))
        if p.pad:          # a padded batch ends its last pack at the real sample count
            pack_start[-1] = p.M
        assert torch.equal(pack_start.cpu(), torch.from_numpy(p.pack_start)) and torch.equal(ray_of_pack.cpu(), torch.from_numpy(p.ray_of_pack))
        return pack_start, ray_of_pack
    ray_of_pack = _t(p.ray_of_pack, dev, torch.int32)
    assert not ops._one_pack_per_ray(ray_of_pack, p.N)
    return _t(p.pack_start, dev, torch.int64), ray_of_pack


def _rows(p, x):
    """The fp64 reference of a per-sample tensor of a padded batch: zeros in the filler rows."""
    return np.concatenate([x, np.zeros((p.pad,) + x.shape[1:])]) if p.pad else x


# ------------------------------------------------------------------------------------------------------------- pag_composite_fwd / pag_composite_bwd
def _composite(p, dev, rgb=True, depths=True, grad=False):
    sigma, deltas = _t(p.sigma_in, dev).requires_grad_(grad), _t(p.delta_in, dev)
    colour = _t(p.rgb_in, dev).requires_grad_(grad) if rgb else None
    dep = _t(p.depths_in, dev) if depths else None
    pack_start, ray_of_pack = _table(p, dev)
    out = _ops().composite(sigma, colour, deltas, dep, pack_start, ray_of_pack, p.N, bg_white=p.bg_white)
    return sigma, colour, out


def _check_forward(tag, p, out, rgb=True, depths=True):
    r = X.reference(p)
    alpha, hit, out_rgb, out_depth, w = out
    X.assert_bit_equal(tag + " weights", w, _rows(p, r.weights), p, "sample")
    X.assert_bit_equal(tag + " alpha", alpha, r.alpha, p, "ray")
    X.assert_bit_equal(tag + " hit", hit, r.hit, p, "ray")
    assert (out_rgb is not None) == rgb and (out_depth is not None) == depths
    if rgb:
        X.assert_bit_equal(tag + " rgb", out_rgb, r.rgb, p, "ray")
    if depths:
        X.assert_bit_equal(tag + " depth", out_depth, r.depth, p, "ray")


@pytest.mark.parametrize("bg_white", (True, False), ids=("white", "black"))
@pytest.mark.parametrize("table", X.TABLES, ids=_id)
def test_exact_composite_forward(gpu_device, table, bg_white):
    """weights, alpha, hit, rgb, depth; and the launches without colours / without depths (NULL inputs and outputs)."""
    p = X.transmittance(*table, bg_white)
    tag = "%s P %% 4 = %d %s:" % (p.form, p.pmod, "white" if bg_white else "black")
    with torch.no_grad():
        _check_forward(tag, p, _composite(p, gpu_device)[2])
        _check_forward(tag + " rgb=None", p, _composite(p, gpu_device, rgb=False)[2], rgb=False)
        _check_forward(tag + " depths=None", p, _composite(p, gpu_device, depths=False)[2], depths=False)


@pytest.mark.parametrize("bg_white", (True, False), ids=("white", "black"))
@pytest.mark.parametrize("table", X.TABLES, ids=_id)
def test_exact_composite_backward(gpu_device, table, bg_white):
    """d sigma and d rgb under the full upstream gradient and under one on rgb, depth or alpha alone - the others then arrive as None, a NULL pointer."""
    p = X.transmittance(*table, bg_white)
    r = X.reference(p)
    for u in X.UPSTREAM:
        tag = "%s P %% 4 = %d %s upstream %s:" % (p.form, p.pmod, "white" if bg_white else "black", u)
        sigma, colour, (alpha, _hit, out_rgb, out_depth, _w) = _composite(p, gpu_device, grad=True)
        terms = {"rgb": (out_rgb * _t(p.g_rgb, gpu_device)).sum(), "depth": (out_depth * _t(p.g_depth, gpu_device)).sum(),
                 "alpha": (alpha * _t(p.g_alpha, gpu_device)).sum()}
        loss = sum(terms.values()) if u == "full" else terms[u]
        loss.backward()
        X.assert_bit_equal(tag + " d sigma", sigma.grad, r.d_sigma[u], p, "sample")
        X.assert_bit_equal(tag + " d rgb", colour.grad, r.d_rgb[u], p, "sample")


def test_exact_composite_padded_batch(gpu_device):
    """ops.TAIL_ZERO as graphs.py sets it, pack_start[P] < M, NaN in the filler rows of every input: weights, d sigma and d rgb of the fillers are exactly 0."""
    ops = _ops()
    p = X.transmittance("identity", 1, True, pad=X.PAD)
    r = X.reference(p)
    assert int(p.pack_start[-1]) == p.M < p.rows
    ops.TAIL_ZERO = True
    try:
        sigma, colour, out = _composite(p, gpu_device, grad=True)
        _check_forward("padded:", p, out)
        alpha, _hit, out_rgb, out_depth, w = out
        loss = (out_rgb * _t(p.g_rgb, gpu_device)).sum() + (out_depth * _t(p.g_depth, gpu_device)).sum() + (alpha * _t(p.g_alpha, gpu_device)).sum()
        loss.backward()
    finally:
        ops.TAIL_ZERO = False
    assert w.shape[0] == p.rows and not bool(w[p.M:].any()) and not bool(sigma.grad[p.M:].any()) and not bool(colour.grad[p.M:].any())
    X.assert_bit_equal("padded: d sigma", sigma.grad, _rows(p, r.d_sigma["full"]), p, "sample")
    X.assert_bit_equal("padded: d rgb", colour.grad, _rows(p, r.d_rgb["full"]), p, "sample")


# ------------------------------------------------------------------------------------------------- pag_composite_feats_fwd / pag_composite_feats_bwd
def _offset_view(x, elements):
    """A contiguous [M, C] view that starts `elements` elements into a larger buffer."""
    flat = torch.empty(x.numel() + elements + 64, device=x.device, dtype=x.dtype)
    view = flat[elements:elements + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + elements * x.element_size() and flat.data_ptr() % 256 == 0
    return view


def _feats(p, dev, dtype, offset=0, grad=False):
    ops = _ops()
    feats = _t(p.feats_in, dev, dtype)
    if offset:
        feats = _offset_view(feats, offset)
    feats.requires_grad_(grad)
    pack_start, ray_of_pack = _table(p, dev)
    out = ops.composite_feats(feats, _t(p.weights_in, dev), _t(p.alpha, dev), pack_start, ray_of_pack, p.N)
    return feats, out


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", X.feature_cases(), ids=_id)
def test_exact_composite_feats(gpu_device, case, dtype):
    """Forward at every width of every dispatcher branch (table above), f32 and bf16 features; the backward (every row and column, exact zeros under
    alpha = 0, an exact bf16 store) at C = 1, 16, 17, 64, 65, 200, 256 and at the widths that run every table form."""
    p = X.features(*case)
    r = X.reference(p)
    tag = "%s P %% 4 = %d C = %d %s:" % (p.form, p.pmod, p.C, _id(dtype))
    backward = p.C in X.C_BWD + (7, 30)
    with torch.set_grad_enabled(backward):
        feats, out = _feats(p, gpu_device, dtype, grad=backward)
    X.assert_bit_equal(tag + " out", out, r.out, p, "ray", parts=r.parts)
    if backward:
        out.backward(_t(p.g, gpu_device))
        assert feats.grad.dtype == dtype
        X.assert_bit_equal(tag + " d feats", feats.grad, r.d_feats, p, "sample")
        dead = torch.from_numpy(p.alpha[p.ray_of_sample] == 0)
        assert bool(dead.any()) and not bool(feats.grad.cpu()[dead].any()), tag + " rows of rays with alpha = 0"


@pytest.mark.parametrize("table", (("identity", 0), ("boundary", 1), ("permuted", 3)), ids=_id)
def test_exact_composite_feats64_bf16_off_its_alignment(gpu_device, table):
    """64 bf16 channels at a base 8 bytes past a 16-byte boundary: not the dedicated 64-wide kernel (16-byte loads) but the vector kernel (8-byte loads) -
    and the same bits as the aligned call."""
    p = X.features(*table, 64)
    r = X.reference(p)
    with torch.no_grad():
        feats, out = _feats(p, gpu_device, BF16, offset=4)
        assert feats.data_ptr() % 16 == 8
        _, aligned = _feats(p, gpu_device, BF16)
    X.assert_bit_equal("C = 64 bf16 at base + 8 bytes: out", out, r.out, p, "ray", parts=r.parts)
    assert torch.equal(out, aligned)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_exact_composite_feats_one_element_off(gpu_device, dtype):
    """C = 20 at a base one element into a buffer: no multiple of the 4-element vector, so the dispatcher takes the scalar kernel."""
    p = X.features("identity", 1, 20)
    r = X.reference(p)
    with torch.no_grad():
        feats, out = _feats(p, gpu_device, dtype, offset=1)
    assert feats.data_ptr() % (4 * feats.element_size()) == feats.element_size()
    X.assert_bit_equal("C = 20 %s at base + one element: out" % _id(dtype), out, r.out, p, "ray", parts=r.parts)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", X.FEATURE_PAD_CASES, ids=_id)
def test_exact_composite_feats_padded_batch(gpu_device, case, dtype):
    """ops.TAIL_ZERO, NaN features and weights in the filler rows: the outputs are untouched by them and d feats of the fillers is exactly 0."""
    ops = _ops()
    p = X.features(*case, pad=X.PAD)
    r = X.reference(p)
    ops.TAIL_ZERO = True
    try:
        feats, out = _feats(p, gpu_device, dtype, grad=True)
        out.backward(_t(p.g, gpu_device))
    finally:
        ops.TAIL_ZERO = False
    tag = "padded %s C = %d %s:" % (p.form, p.C, _id(dtype))
    X.assert_bit_equal(tag + " out", out, r.out, p, "ray", parts=r.parts)
    assert feats.grad.shape[0] == p.rows and not bool(feats.grad[p.M:].any())
    X.assert_bit_equal(tag + " d feats", feats.grad, _rows(p, r.d_feats), p, "sample")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_exact_composite_features_with_their_own_weights(gpu_device, dtype):
    """_CompositeFeatsWeights (the delta-density tracer's node): one-hot weights computed inside the node at C = 20; out, alpha, d feats and d sigma."""
    ops = _ops()
    p = X.feature_weights("boundary", 3)
    r = X.reference(p)
    dev = gpu_device
    sigma, feats = _t(p.sigma, dev).requires_grad_(), _t(p.feats, dev, dtype).requires_grad_()
    pack_start, ray_of_pack = _table(p, dev)
    out, alpha = ops.composite_features(sigma, _t(p.delta, dev), feats, _t(p.ray_of_sample, dev, torch.int32), pack_start, ray_of_pack, p.N)
    out.backward(_t(p.g, dev))
    tag = "composite_features C = %d %s:" % (p.C, _id(dtype))
    X.assert_bit_equal(tag + " out", out, r.out, p, "ray")
    X.assert_bit_equal(tag + " alpha", alpha, r.alpha, p, "ray")
    X.assert_bit_equal(tag + " d feats", feats.grad, r.d_feats, p, "sample")
    X.assert_bit_equal(tag + " d sigma", sigma.grad, r.d_sigma, p, "sample")


# ------------------------------------------------------------------------------------------------------------------------- pag_ray_sample_grad
@pytest.mark.parametrize("case", X.ray_sample_cases(), ids=_id)
def test_exact_ray_sample_gradient(gpu_device, case):
    """d origins = sum g, d dirs = sum g depth per ray through ops.ray_samples + autograd; samples [M, 3] and [M / 2, 2, 3]; rays without samples get zeros."""
    ops = _ops()
    p = X.ray_samples(*case)
    r = X.reference(p)
    dev = gpu_device
    shape = (p.M, 3) if p.k == 1 else (p.M // p.k, p.k, 3)
    origins, dirs = _t(p.origins, dev).requires_grad_(), _t(p.dirs, dev).requires_grad_()
    pack_start, ray_of_pack = _table(p, dev)
    out = ops.ray_samples(origins, dirs, _t(p.samples, dev).view(shape), _t(p.depths, dev).view(shape[:-1]), pack_start, ray_of_pack)
    assert out.shape == shape
    out.backward(_t(p.g, dev).view(shape))
    tag = "%s P %% 4 = %d k = %d:" % (p.form, p.pmod, p.k)
    X.assert_bit_equal(tag + " d origins", origins.grad, r.d_origins, p, "ray")
    X.assert_bit_equal(tag + " d dirs", dirs.grad, r.d_dirs, p, "ray")
    empty = torch.from_numpy(p.len_of_ray == 0)
    assert bool(empty.any()) and not bool(origins.grad.cpu()[empty].any()) and not bool(dirs.grad.cpu()[empty].any())
