"""SemanticNeF on the CPU (the fp32 tensor-op path) against the reference's golden (g15_semantic_nef.npz, tests/golden/make_golden_semantic.py), its
host logic, and the argument validation of the pag_deep_mlp_* entry points.  No GPU.

The upper part of this file is shared with the fixture's maker and with tests/test_gpu_semantic_nef.py: the seeded weights (they are not stored) and
a plain torch restatement of the network with an `operand_round` hook.  With oracle.decoders.bf16_operands and round_grads=True it is the arithmetic
include/pagnerf_hip.h states for the fused launch: every Linear's input and weight rounded to bf16, every Linear's incoming gradient rounded to bf16
before both of its products, sums in fp32."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden

HIDDEN, CLASSES, N_GOLD = 256, 6, 2048
SEED = 1597          # a draw that meets every condition the fixture's maker asserts (density positive on 92 % of the samples)
TRUNK_IN = [63, 256, 256, 256, 256, 319, 256, 256]


def param_shapes(hidden=HIDDEN, classes=CLASSES):
    """name -> shape, in the order of the reference's named_parameters()."""
    s = {"view_embedder.bands": (10,), "pos_embedder.bands": (10,)}
    for i in range(8):
        n_in = 63 if i == 0 else (hidden + 63 if i == 5 else hidden)
        s["decoder_features.layers.%d.weight" % i] = (hidden, n_in)
        s["decoder_features.layers.%d.bias" % i] = (hidden,)
    s["decoder_features.lout.weight"], s["decoder_features.lout.bias"] = (hidden, hidden), (hidden,)
    s["decoder_density.weight"], s["decoder_density.bias"] = (1, hidden), (1,)
    s["decoder_color.layers.0.weight"], s["decoder_color.layers.0.bias"] = (hidden // 2, hidden + 63), (hidden // 2,)
    s["decoder_color.lout.weight"], s["decoder_color.lout.bias"] = (3, hidden // 2), (3,)
    s["decoder_semantics.layers.0.weight"], s["decoder_semantics.layers.0.bias"] = (hidden // 2, hidden), (hidden // 2,)
    s["decoder_semantics.lout.weight"], s["decoder_semantics.lout.bias"] = (classes, hidden // 2), (classes,)
    return s


# weight variance x fan_in: 2 (He) where a ReLU follows the layer; 1 for lout and the density layer; 0.5 for the two layers that end in logits.  The
# smaller gains on the layers without a ReLU keep the outputs at a scale where ten bf16-operand layers stay inside the maker's rtol = atol = 1.5e-2
# (with He gains throughout, the 4-sigma sample of 2048 x 6 logits sits at 2 - 4e-2 from the fp32 reference).
_GAIN = {"decoder_features.lout.weight": 1.0, "decoder_density.weight": 1.0, "decoder_color.lout.weight": 0.5, "decoder_semantics.lout.weight": 0.5}


def make_weights(seed=SEED, hidden=HIDDEN, classes=CLASSES):
    """He-normal weights (see _GAIN), small uniform biases, density bias 1.0 (nn.Linear's default initialisation leaves the trunk output at 0.14
    absmax, which exercises nothing)."""
    rs = np.random.RandomState(seed)
    w = {}
    for name, shape in param_shapes(hidden, classes).items():
        if name.endswith("bands"):
            continue
        if name.endswith("weight"):
            w[name] = (rs.standard_normal(shape) * np.sqrt(_GAIN.get(name, 2.0) / shape[1])).astype(np.float32)
        else:
            w[name] = rs.uniform(-0.1, 0.1, size=shape).astype(np.float32)
    w["decoder_density.bias"][0] = 1.0
    return w


def make_inputs(seed=SEED, n=N_GOLD):
    rs = np.random.RandomState(seed + 1)
    x = rs.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    d = rs.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return x, d.astype(np.float32)


def make_upstream(seed=SEED, n=N_GOLD, classes=CLASSES):
    rs = np.random.RandomState(seed + 2)
    return {"density": rs.standard_normal((n, 1, 1)).astype(np.float32), "rgb": rs.standard_normal((n, 1, 3)).astype(np.float32),
            "semantics": rs.standard_normal((n, classes)).astype(np.float32)}


def load_weights(nef, w):
    with torch.no_grad():
        for name, p in nef.named_parameters():
            if name in w:
                p.copy_(torch.from_numpy(w[name]))


class _Lin(torch.autograd.Function):
    """F.linear with rounding hooks: rnd on both forward operands; with round_grads the incoming gradient is rounded before both of its products (and
    the bias gradient is the sum of the rounded rows).  dt: accumulation dtype; perm: a permutation of the K axis (the summation order)."""

    @staticmethod
    def forward(ctx, x, W, b, rnd, round_grads, dt, perm):
        xr, Wr = rnd(x).to(dt), rnd(W).to(dt)
        ctx.save_for_backward(xr, Wr)
        ctx.rnd, ctx.round_grads, ctx.dt, ctx.perm = rnd, round_grads, dt, perm
        if perm:
            p = torch.randperm(xr.shape[1], generator=torch.Generator().manual_seed(xr.shape[1]))
            y = xr[:, p] @ Wr[:, p].t()
        else:
            y = xr @ Wr.t()
        return (y + b.to(dt)).float()

    @staticmethod
    def backward(ctx, g):
        xr, Wr = ctx.saved_tensors
        g = (ctx.rnd(g) if ctx.round_grads else g).to(ctx.dt)
        if ctx.perm:
            p = torch.randperm(g.shape[0], generator=torch.Generator().manual_seed(7))
            gW = g[p].t() @ xr[p]
            q = torch.randperm(g.shape[1], generator=torch.Generator().manual_seed(g.shape[1]))
            gx = g[:, q] @ Wr[q]
        else:
            gW, gx = g.t() @ xr, g @ Wr
        return gx.float(), gW.float(), g.sum(0).float(), None, None, None, None


def positional_embed(x, num_freq=10):
    bands = 2.0 ** torch.linspace(0.0, num_freq - 1, num_freq)
    w = (x[:, None, :] * bands[None, :, None]).reshape(x.shape[0], -1)
    return torch.cat([x, torch.sin(w), torch.cos(w)], dim=-1)


def restate(w, x, d, operand_round=None, round_grads=False, dt=torch.float32, perm=False, zero_skip_h=False):
    """The network of pc_nerf/semantic_nerf.py:43-76, :188-224 in plain torch.  w: name -> tensor (requires_grad for gradients); x, d [M,3].
    -> dict(feats [M,H], density [M,1,1], rgb [M,1,3], semantics [M,C], density_pre [M])."""
    rnd = operand_round if operand_round is not None else (lambda t: t)

    def lin(h, name):
        return _Lin.apply(h, w[name + ".weight"], w[name + ".bias"], rnd, round_grads, dt, perm)
    e = positional_embed(x)
    h = e
    for i in range(8):
        if i == 5:
            h = torch.cat([e, torch.zeros_like(h) if zero_skip_h else h], dim=-1)
        h = torch.relu(lin(h, "decoder_features.layers.%d" % i))
    feats = lin(h, "decoder_features.lout")
    pre = lin(feats, "decoder_density")[:, 0]
    hc = torch.relu(lin(torch.cat([feats, positional_embed(-d)], dim=-1), "decoder_color.layers.0"))
    rgb = torch.sigmoid(lin(hc, "decoder_color.lout"))
    hs = torch.relu(lin(feats, "decoder_semantics.layers.0"))
    sem = lin(hs, "decoder_semantics.lout")
    M = x.shape[0]
    return {"feats": feats, "density": torch.relu(pre).reshape(M, 1, 1), "rgb": rgb.reshape(M, 1, 3), "semantics": sem, "density_pre": pre}


def restate_grads(w_np, x, d, up, **kw):
    """Outputs and parameter gradients of `restate` for the upstream gradients `up` (name -> array)."""
    w = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in w_np.items()}
    out = restate(w, torch.from_numpy(x), torch.from_numpy(d), **kw)
    loss = sum((out[c] * torch.from_numpy(up[c])).sum() for c in ("density", "rgb", "semantics"))
    loss.backward()
    return {k: v.detach().numpy() for k, v in out.items()}, {k: v.grad.numpy() for k, v in w.items()}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# The launch-regime cases of tests/test_gpu_semantic_nef_regimes.py: key -> (samples, classes, channels with an upstream gradient).  Their noise floors
# are stored in g15b_semantic_regimes.npz (tests/golden/make_golden_semantic_regimes.py); weights, inputs and upstream gradients come from the seeds.
CHANNELS = ("density", "rgb", "semantics")
M_SLICES, M_PERSIST = 2049, 256 * 256 + 256 + 33
REGIME_CASES = {
    "m2049": (M_SLICES, 6, CHANNELS),
    "m65825": (M_PERSIST, 6, CHANNELS),
    "c1": (M_SLICES, 1, CHANNELS),
    "c16": (M_SLICES, 16, CHANNELS),
    "only_density": (M_SLICES, 6, ("density",)),
    "only_rgb": (M_SLICES, 6, ("rgb",)),
    "only_semantics": (M_SLICES, 6, ("semantics",)),
}
NEAR_ZERO = 0.02


def regime_case(key, seed=SEED):
    """-> (weights, coords, dirs, upstream, plain) of a case for one weight seed: `plain` is the fp32 restatement's outputs, the density upstream is
    zeroed where its |density_pre| < NEAR_ZERO (a ReLU flip there would move a whole term), channels without an upstream gradient hold zeros."""
    M, C, chans = REGIME_CASES[key]
    w = make_weights(seed, classes=C)
    x, d = make_inputs(n=M)
    with torch.no_grad():
        plain = {k: v.numpy() for k, v in restate({k: torch.from_numpy(v) for k, v in w.items()}, torch.from_numpy(x), torch.from_numpy(d)).items()}
    up = make_upstream(seed, n=M, classes=C)
    up["density"][np.abs(plain["density_pre"]) < NEAR_ZERO] = 0.0
    for c in CHANNELS:
        if c not in chans:
            up[c] = np.zeros_like(up[c])
    return w, x, d, up, plain


def wgrad_split(M, C=CLASSES):
    """(tiles, tile pairs, slices, pairs per slice) of the weight-gradient pass for M samples.  The slice count is read off the library's backward
    workspace size (one slab set per slice, 2656 bf16 of dz per sample padded to 256 samples: DESIGN 4.16), so a change of the kernel's constants
    shows here; the 32-sample tile and the pair are the MFMA shape."""
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib as L
    ws = lambda m: int(L.load().pag_deep_mlp_workspace_bytes(m, 256, C, 2))                    # noqa: E731
    pad = lambda m: (m + 255) // 256 * 256                                                     # noqa: E731
    unit = ws(65) - ws(64)                      # 2 -> 3 tiles is 1 -> 2 pairs at the same padded size: one more slab set
    extra = ws(M) - ws(1) - (pad(M) - 256) * 2656 * 2
    assert unit > 0 and extra % unit == 0, (unit, extra)
    ntile = (M + 31) // 32
    npair, n_split = (ntile + 1) // 2, 1 + extra // unit
    return ntile, npair, n_split, -(-npair // n_split)


# ------------------------------------------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def g15():
    return golden("g15_semantic_nef.npz")


def _nef(hidden=HIDDEN, classes=CLASSES, seed=SEED, **kw):
    import pagnerf_amd
    nef = pagnerf_amd.SemanticNeF(num_classes=classes, hidden_dim=hidden, blas_level=3, **kw)
    load_weights(nef, make_weights(seed, hidden, classes))
    return nef


def test_cpu_path_matches_reference_golden(g15):
    nef = _nef()
    x, d = torch.from_numpy(g15["coords"]), torch.from_numpy(g15["dirs"])
    with torch.no_grad():
        out = nef(channels={"density", "rgb", "semantics"}, coords=x[:, None], ray_d=d)
    for c in ("density", "rgb", "semantics"):
        assert tuple(out[c].shape) == tuple(g15[c].shape), c
        np.testing.assert_allclose(out[c].numpy(), g15[c], rtol=1e-5, atol=2e-6, err_msg=c)


def test_parameter_names_and_shapes_are_the_references(g15):
    nef = _nef()
    mine = [(n, tuple(p.shape)) for n, p in nef.named_parameters()]
    ref = list(zip([str(n) for n in g15["param_names"]], [tuple(int(v) for v in s if v >= 0) for s in g15["param_shapes"]]))
    assert mine == ref
    assert mine == list(param_shapes().items())
    assert float(type(nef)(num_classes=3).decoder_density.bias[0]) == 1.0
    assert [n for n, p in nef.named_parameters() if not p.requires_grad] == ["view_embedder.bands", "pos_embedder.bands"]
    assert nef.get_supported_channels() == {"density", "rgb", "semantics"} and nef.get_nef_type() == "panoptic_nef"
    assert nef.grid.num_lods == 1 and nef.grid.active_lods == [0] and not getattr(nef, "accepts_ray_index", False)


def test_channel_selective_forward_return_types():
    nef = _nef()
    x, d = torch.rand(7, 1, 3) * 2 - 1, F.normalize(torch.randn(7, 3), dim=-1)
    with torch.no_grad():
        dens = nef(channels="density", coords=x, ray_d=d)
        lst = nef(channels=["semantics", "density"], coords=x, ray_d=d)
        dct = nef(channels={"rgb", "semantics"}, coords=x, ray_d=d, pidx=None, lod_idx=0)
    assert isinstance(dens, torch.Tensor) and dens.shape == (7, 1, 1)
    assert isinstance(lst, list) and lst[0].shape == (7, CLASSES) and torch.equal(lst[1], dens)
    assert isinstance(dct, dict) and set(dct) == {"rgb", "semantics"} and dct["rgb"].shape == (7, 1, 3) and torch.equal(dct["semantics"], lst[0])
    with pytest.raises(Exception):
        nef(channels={"inst_embedding"}, coords=x, ray_d=d)
    # [batch, num_samples > 1]: one direction per batch entry, repeated over its samples (semantic_nerf.py:209-210)
    xs = torch.rand(3, 4, 3) * 2 - 1
    with torch.no_grad():
        a = nef(channels={"rgb", "density"}, coords=xs, ray_d=d[:3])
        b = nef(channels={"rgb", "density"}, coords=xs.reshape(12, 1, 3), ray_d=d[:3].repeat_interleave(4, 0))
    assert a["rgb"].shape == (3, 4, 3) and a["density"].shape == (3, 4, 1) and torch.equal(a["rgb"].reshape(12, 1, 3), b["rgb"])


def test_skip_layer_reads_the_embedding_in_its_first_columns():
    """Layer 5 reads cat([e, h]): with its h columns (63 ..) zeroed the network must equal the restatement that feeds it zeros for h - and must differ
    when the e columns (.. 62) are zeroed instead, which is what a [h | e] order would have left untouched."""
    nef = _nef()
    w = make_weights()
    x, d = make_inputs(n=64)
    W5 = nef.decoder_features.layers[5].weight
    with torch.no_grad():
        W5[:, 63:] = 0.0
        out = nef(channels={"semantics", "density"}, coords=torch.from_numpy(x)[:, None], ray_d=torch.from_numpy(d))
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    ref = restate(wt, torch.from_numpy(x), torch.from_numpy(d), zero_skip_h=True)
    np.testing.assert_allclose(out["semantics"].numpy(), ref["semantics"].numpy(), rtol=1e-5, atol=2e-6)
    wt2 = dict(wt)
    wt2["decoder_features.layers.5.weight"] = wt["decoder_features.layers.5.weight"].clone()
    wt2["decoder_features.layers.5.weight"][:, :63] = 0.0
    other = restate(wt2, torch.from_numpy(x), torch.from_numpy(d))
    assert rel_l2(other["semantics"].numpy(), ref["semantics"].numpy()) > 1e-2


def test_prune_matches_numpy_restatement():
    nef = _nef()
    R = 8
    rs = np.random.RandomState(3)
    jitter = rs.uniform(0, 1, size=(R ** 3, 3)).astype(np.float32)
    occ0 = rs.uniform(0, 8, size=R ** 3).astype(np.float32)
    nef.grid.occupancy = torch.from_numpy(occ0.copy())
    nef.prune(jitter=torch.from_numpy(jitter))
    ar = np.arange(R)
    pts = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    samples = ((pts + jitter) / np.float32(R) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    wt = {k: torch.from_numpy(v) for k, v in make_weights().items()}
    dens = restate(wt, torch.from_numpy(samples), torch.zeros(R ** 3, 3))["density"].numpy().reshape(-1)
    want = np.maximum(dens, occ0 * np.float32(0.6))
    np.testing.assert_allclose(nef.grid.occupancy.numpy(), want, rtol=1e-5, atol=2e-6)
    thr = (0.01 * 512) / np.sqrt(3)
    clear = np.abs(want - thr) > 1e-4
    mask = nef.grid.occupancy_mask().numpy()
    assert np.array_equal(mask[clear], (want > thr)[clear]) and 0 < mask.sum() < mask.size
    from pagnerf_amd.semantic_nef import sample_unif_sphere
    v = sample_unif_sphere(4096, generator=torch.Generator().manual_seed(0))
    assert v.shape == (4096, 3) and torch.allclose(v.norm(dim=-1), torch.ones(4096), atol=1e-5) and float(v.mean(0).abs().max()) < 0.05


def _cpu_composite(sigma, rgb, deltas, depths, pack_start, ray_of_pack, N, bg_white=True):
    """ops.composite in tensor ops (tracers/panoptic_packed_rf_tracer.py:134-176) for CPU tensors; here every ray has exactly one pack."""
    ps = pack_start.tolist()
    assert ray_of_pack.tolist() == list(range(N))
    rows_a, rows_rgb, rows_d, ws = [], [], [], []
    for ray in range(N):
        s, e = ps[ray], ps[ray + 1]
        tau = sigma[s:e] * deltas[s:e]
        wp = torch.exp(-(torch.cumsum(tau, 0) - tau)) * (1.0 - torch.exp(-tau))
        a = wp.sum()
        rows_a.append(a)
        rc = (wp[:, None] * rgb[s:e]).sum(0)
        rows_rgb.append((1.0 - a) + a * rc if bg_white else a * rc)                    # :158-166: the summed colour is scaled by alpha once more
        rows_d.append((wp * depths[s:e]).sum() if depths is not None else torch.zeros(()))
        ws.append(wp.detach())
    alpha = torch.stack(rows_a)
    return alpha, (alpha.detach() > 0).to(torch.uint8), torch.stack(rows_rgb), torch.stack(rows_d) if depths is not None else None, torch.cat(ws)


def _cpu_composite_feats(feats, weights, alpha, pack_start, ray_of_pack, N):
    rows = [torch.zeros(feats.shape[1]) for _ in range(N)]
    ps = pack_start.tolist()
    for p, ray in enumerate(ray_of_pack.tolist()):
        s, e = ps[p], ps[p + 1]
        rows[ray] = alpha[ray] * (weights[s:e, None] * feats[s:e]).sum(0)
    return torch.stack(rows)


def cpu_trace(nef, rays_o, rays_d, S, channels=("rgb", "depth", "semantics"), stage="train"):
    """PanopticPackedRFTracer.shade on CPU tensors: S evenly spaced samples per ray inside the unit cube, the two compositing ops (GPU only in the
    product) replaced by the tensor-op stand-ins above.  -> dict channel -> tensor."""
    import pagnerf_amd
    from pagnerf_amd import ops
    N = rays_o.shape[0]
    t = (torch.arange(S, dtype=torch.float32) + 0.5) / S * 1.5
    samples = (rays_o[:, None] + rays_d[:, None] * t[None, :, None]).reshape(-1, 1, 3).clamp(-1, 1)
    ridx = torch.arange(N).repeat_interleave(S)
    pack_start = torch.arange(N + 1, dtype=torch.int64) * S
    ray_of_pack = torch.arange(N, dtype=torch.int32)
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=S, bg_color="white")
    real = ops.composite, ops.composite_feats
    ops.composite, ops.composite_feats = _cpu_composite, _cpu_composite_feats
    try:
        return tracer.shade(nef, set(channels), set(), rays_d, N, ridx, ridx.int(), None, samples, t.repeat(N)[:, None], torch.full((N * S, 1), 1.5 / S),
                            pack_start, ray_of_pack, 0, "white", stage)
    finally:
        ops.composite, ops.composite_feats = real


def make_rays(n=24, seed=11):
    rs = np.random.RandomState(seed)
    o = rs.uniform(-0.9, -0.5, size=(n, 3)).astype(np.float32)
    d = rs.uniform(0.2, 1.0, size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy(o), torch.from_numpy(d.astype(np.float32))


def test_trace_through_the_tracer_on_cpu():
    """The tracer's shade() drives the nef the way a training trace does (per-sample ray_d, channels as a set, semantics as raw logits through
    composite_feats); the GPU-only compositing ops are replaced by tensor-op stand-ins, everything else is the product's code."""
    nef = _nef()
    o, d = make_rays()
    out = cpu_trace(nef, o, d, 16)
    assert out["rgb"].shape == (24, 3) and out["depth"].shape == (24, 1) and out["semantics"].shape == (24, CLASSES) and out["alpha"].shape == (24, 1)
    assert torch.isfinite(out["rgb"]).all() and float(out["alpha"].min()) > 0
    (out["rgb"].sum() + out["semantics"].sum()).backward()
    assert nef.decoder_features.layers[0].weight.grad.abs().sum() > 0 and nef.decoder_semantics.lout.weight.grad.abs().sum() > 0


def test_unsupported_widths_take_the_tensor_op_path():
    """hidden_dim 64 / 20 classes / a sin activation are outside the fused path: forward() must agree with the tensor-op form (here: on CPU, where it is
    the only path; tests/test_gpu_semantic_nef.py repeats it on GPU tensors)."""
    import pagnerf_amd
    for hidden, classes, act in ((64, 6, "relu"), (256, 20, "relu"), (128, 3, "sin")):
        nef = pagnerf_amd.SemanticNeF(num_classes=classes, hidden_dim=hidden, activation_type=act, blas_level=2)
        load_weights(nef, make_weights(7, hidden, classes))
        assert not nef.fused_supported()
        x, d = make_inputs(n=33)
        with torch.no_grad():
            out = nef(channels={"density", "rgb", "semantics"}, coords=torch.from_numpy(x)[:, None], ray_d=torch.from_numpy(d))
            ref = nef.tensor_forward(torch.from_numpy(x), torch.from_numpy(d), {"density", "rgb", "semantics"})
        for c in ("density", "rgb", "semantics"):
            assert torch.equal(out[c].reshape(ref[c].shape), ref[c])
        if act == "relu":
            wt = {k: torch.from_numpy(v) for k, v in make_weights(7, hidden, classes).items()}
            np.testing.assert_allclose(out["semantics"].numpy(), restate(wt, torch.from_numpy(x), torch.from_numpy(d))["semantics"].numpy(), rtol=1e-5, atol=2e-6)
    assert _nef().fused_supported()
    with pytest.raises(NotImplementedError):
        pagnerf_amd.SemanticNeF(num_classes=3, activation_type="gelu")


def test_deep_mlp_entry_points_validate_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib as L
    lib = L.load()
    assert lib.pag_deep_mlp_supported(256, 6) == 1 and lib.pag_deep_mlp_supported(256, 16) == 1
    assert lib.pag_deep_mlp_supported(128, 6) == 0 and lib.pag_deep_mlp_supported(256, 17) == 0 and lib.pag_deep_mlp_supported(256, 0) == 0
    assert lib.pag_deep_mlp_workspace_bytes(-1, 256, 6, 0) == -1 and lib.pag_deep_mlp_workspace_bytes(8, 64, 6, 0) == -1
    assert lib.pag_deep_mlp_workspace_bytes(8, 256, 6, 3) == -1 and b"mode" in lib.pag_last_error_string()
    w0, w1, w2 = (lib.pag_deep_mlp_workspace_bytes(5242880, 256, 6, m) for m in (0, 1, 2))
    assert 0 < w0 < 2 ** 21 and w1 - w0 == 5242880 * 2688 * 2 and w2 > 5242880 * 2656 * 2          # bytes per sample of the training step
    a = L.DeepMlpArgs()
    a.hidden, a.num_classes, a.channels = 256, 6, 7
    assert lib.pag_deep_mlp_fwd(ctypes.byref(a), 0, None) == 0 and lib.pag_deep_mlp_bwd(ctypes.byref(a), 0, None) == 0       # M == 0: no-op
    assert lib.pag_deep_mlp_fwd(None, 4, None) == -1 and lib.pag_deep_mlp_fwd(ctypes.byref(a), -1, None) == -1
    assert lib.pag_deep_mlp_fwd(ctypes.byref(a), 4, None) == -1 and b"workspace" in lib.pag_last_error_string()             # NULL workspace
    buf = (ctypes.c_float * 64)()
    one = ctypes.cast(buf, ctypes.c_void_p).value & ~255                # an aligned non-NULL value; refused before it is ever dereferenced
    a.workspace, a.workspace_bytes = one + 256, 64
    assert lib.pag_deep_mlp_fwd(ctypes.byref(a), 4, None) == -1 and b"workspace" in lib.pag_last_error_string()             # short workspace
    a.workspace_bytes = w0
    assert lib.pag_deep_mlp_fwd(ctypes.byref(a), 4, None) == -1 and b"NULL" in lib.pag_last_error_string()                  # NULL coords
    a.hidden = 128
    assert lib.pag_deep_mlp_fwd(ctypes.byref(a), 4, None) == -1 and b"hidden" in lib.pag_last_error_string()
    a.hidden, a.channels = 256, 0
    assert lib.pag_deep_mlp_fwd(ctypes.byref(a), 4, None) == -1 and b"channels" in lib.pag_last_error_string()
    a.channels, a.save = 3, 1
    assert lib.pag_deep_mlp_fwd(ctypes.byref(a), 4, None) == -1 and b"save" in lib.pag_last_error_string()
    a.channels, a.save = 7, 0
    assert lib.pag_deep_mlp_bwd(ctypes.byref(a), 4, None) == -1 and b"workspace" in lib.pag_last_error_string()


def test_fused_path_refuses_a_coords_gradient():
    """The gradient with respect to coords is out of scope for the fused launch: asking for it must raise, not return None silently.  (Checked on the
    host: the guard sits in front of the launch.)"""
    nef = _nef()
    x = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="coords"):
        nef._fused(x, torch.zeros(4, 3), {"density"})


def test_rgb_needs_one_direction_per_batch_entry():
    """coords [B,S,3] go with ray_d [B,3] (semantic_nerf.py:209-210); anything else is refused before a path is chosen, and channels without rgb
    do not need (or touch) ray_d at all."""
    nef = _nef()
    x = torch.from_numpy(make_inputs(n=12)[0]).reshape(4, 3, 3)
    d = torch.from_numpy(make_inputs(n=12)[1])
    with pytest.raises(ValueError, match="ray_d of shape"):
        nef(channels="rgb", coords=x, ray_d=d)                   # per sample where per batch entry is expected
    with pytest.raises(ValueError, match="ray_d of shape"):
        nef(channels={"rgb", "density"}, coords=x, ray_d=None)
    with torch.no_grad():
        a = nef(channels={"density", "semantics"}, coords=x, ray_d=d[:2])      # unused, so its shape does not matter
        b = nef(channels={"density", "semantics"}, coords=x, ray_d=None)
    assert torch.equal(a["density"], b["density"]) and torch.equal(a["semantics"], b["semantics"])


def test_regime_floors_hold_every_case_channel_and_parameter():
    """g15b_semantic_regimes.npz (floors only): every case of REGIME_CASES with its sizes, a floor per output channel and one per parameter of
    param_shapes(classes=C)."""
    g = golden("g15b_semantic_regimes.npz")
    assert sorted(str(k) for k in g["cases"]) == sorted(REGIME_CASES)
    for key, (M, C, chans) in REGIME_CASES.items():
        assert int(g[key + "_M"]) == M and int(g[key + "_C"]) == C, key
        for c in ("feats",) + CHANNELS:
            assert 0.0 < float(g[key + "_floor_" + c]) < 1e-2, (key, c)
        names = [str(n) for n in g[key + "_grad_names"]]
        assert names == sorted(n for n in param_shapes(classes=C) if not n.endswith("bands")), key
        floors = g[key + "_grad_floors"]
        assert floors.shape == (len(names),) and np.isfinite(floors).all() and (floors >= 0).all() and floors.max() < 5e-2, key
        for n, f in zip(names, floors):                  # a head without an upstream gradient has a gradient of exactly zero: no floor
            head = {"decoder_density": "density", "decoder_color": "rgb", "decoder_semantics": "semantics"}.get(n.split(".")[0])
            if head is not None and head not in chans:
                assert f == 0.0, (key, n, f)
            elif n.endswith("weight"):
                assert f > 0.0, (key, n, f)


def test_regime_sizes_sit_in_the_launch_regimes_they_are_named_for():
    """2049 samples: an odd tile count whose last tile holds one sample, two tile pairs per weight-gradient slice, and slices with nothing to do;
    65 825 samples: more 256-sample batches than the 256 workgroups of the persistent kernels, and a short last slice."""
    ntile, npair, n_split, per = wgrad_split(M_SLICES)
    assert ntile % 2 == 1 and M_SLICES % 32 == 1 and per >= 2 and per * (n_split - 1) >= npair and npair % per != 0, (ntile, npair, n_split, per)
    ntile, npair, n_split, per = wgrad_split(M_PERSIST)
    assert per >= 2 and npair % per != 0 and per * (n_split - 1) < npair, (ntile, npair, n_split, per)
    assert (M_PERSIST + 255) // 256 > 256 and M_PERSIST % 256 == 33
    assert wgrad_split(2048)[3] == 1                    # the sizes of tests/test_gpu_semantic_nef.py: at most one pair per slice
