"""The 128-wide decoder family on the GPU (pag_mlp128_fwd / pag_mlp128_bwd through ops.fused_mlp128 and nef.BasicDecoder): op parity against the
tensor-op definition ops.wide_mlp_reference(round_bf16=True) on the CPU, determinism, no_grad, mixed-width and all-128 NeFs, a training trace
against its precision='fp32' self next to the same comparison at width 64, and HIP-graph replay."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CH = {"rgb", "depth", "semantics", "inst_embedding"}


def _ops():
    from pagnerf_amd import ops, _lib as L
    return ops, L


# the two helpers of test_gpu_parity.py::test_fused_mlp_forward_backward
def _rand_mlp(rs, dims):
    W = [torch.from_numpy((rs.standard_normal(size=(dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32)) for i in range(len(dims) - 1)]
    b = [torch.from_numpy((rs.standard_normal(size=(dims[i + 1],)) * 0.1).astype(np.float32)) for i in range(len(dims) - 1)]
    return W, b


def _rel_l2(got, want):
    return float((got - want).norm() / (want.norm() + 1e-20))


def _to_xcd8(x, levels, feats, fill=float("nan")):
    """[M, levels*feats] -> bf16 [8, M, 8]; padding positions hold `fill` (the kernels must never multiply them)."""
    ops, _ = _ops()
    x8 = torch.full((8, x.shape[0], 8), fill)
    for p, c in enumerate(ops.xcd8_columns(levels, feats)):
        if c >= 0:
            x8[p >> 3, :, p & 7] = x[:, c]
    return x8.bfloat16()


def _from_xcd8(x8, levels, feats):
    ops, _ = _ops()
    cols = ops.xcd8_columns(levels, feats)
    out = torch.zeros(x8.shape[1], levels * feats)
    pad = []
    for p, c in enumerate(cols):
        if c >= 0:
            out[:, c] = x8[p >> 3, :, p & 7].float()
        else:
            pad.append(x8[p >> 3, :, p & 7].float())
    return out, torch.stack(pad)


GRID_ROUND = 256 * 256          # _lib.MLP128_BATCH samples x _lib.MLP128_MAX_GRID workgroups: one round of the forward / backward grid

# (dims, out_act, form, out bf16): form "xcd8" | "strided" (f32 x1) | "strided_bf16" | k1 of a strided f32 x1 followed by gathered x2 [50, 32] |
# ("packs", k1): a bf16 x1 followed by x2, with the index's packs handed over (x2_packs: the tracer's form, d x2 through the segmented-sum launch)
CASES = [((48, 128, 16), 0, "xcd8", False), ((48, 128, 16), 0, "strided", False),
         ((43, 128, 128, 3), 1, 16, False), ((43, 128, 128, 128, 3), 1, 16, False),
         ((48, 128, 6), 2, "xcd8", False), ((48, 128, 128, 6), 2, "strided", False),
         ((48, 128, 200), 2, "xcd8", True), ((48, 128, 128, 200), 2, "xcd8", True),
         ((27, 128, 200), 0, "strided", False), ((3, 128, 6), 2, "strided", False)]
# beyond the issue's list: the strided bf16 input / bf16 d x1 paths and the x2_packs branch of d x2, held to the same bounds
EXTRA = [((48, 128, 16), 0, "strided_bf16", False), ((27, 128, 200), 2, "strided_bf16", True), ((43, 128, 128, 3), 1, ("packs", 16), False)]
M_VALUES = (1, 31, 1037, GRID_ROUND + 37)
SIZES = [(c, M) for c in CASES for M in M_VALUES] + [(c, M) for c in EXTRA for M in (31, 1037)]


def _build(rs, dims, form, M, R=50):
    """-> (x1 for the op, grouped, x2, idx, the full [M, in_dim] input as the kernel rounds it, n1 = x1 columns that are real inputs, x2_packs)."""
    in_dim = dims[0]
    if form in ("xcd8", "strided", "strided_bf16"):
        x = torch.from_numpy(rs.standard_normal(size=(M, in_dim)).astype(np.float32))
        if form == "xcd8":
            return _to_xcd8(x, in_dim // 2, 2), (in_dim // 2, 2), None, None, x, in_dim, None
        k1 = 32 if in_dim == 27 else (in_dim + 7) // 8 * 8          # 27 columns padded to 32, 3 to 8
        x1 = torch.full((M, k1), float("nan"))          # columns >= in_dim are ignored, whatever they hold
        x1[:, :in_dim] = x
        return (x1.bfloat16() if form == "strided_bf16" else x1), None, None, None, x, in_dim, None
    k1 = form[1] if isinstance(form, tuple) else form
    x1 = torch.from_numpy(rs.standard_normal(size=(M, k1)).astype(np.float32))
    x2 = torch.zeros(R, 32)
    x2[:, :in_dim - k1] = torch.from_numpy(rs.standard_normal(size=(R, in_dim - k1)).astype(np.float32))
    idx = torch.from_numpy(np.sort(rs.randint(0, R, size=M)).astype(np.int32))
    packs = None
    if isinstance(form, tuple):          # one pack per run of equal indices
        x1 = x1.bfloat16()
        rays, counts = torch.unique_consecutive(idx, return_counts=True)
        packs = (torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)]), rays.int())
    return x1, None, x2, idx, torch.cat([x1.float(), x2[idx.long(), :in_dim - k1]], -1), k1, packs


@pytest.mark.parametrize("case,M", SIZES, ids=lambda v: str(v).replace(" ", ""))
def test_fused_mlp128_forward_backward(gpu_device, case, M):
    ops, L = _ops()
    dev = gpu_device
    dims, act, form, out_bf16 = case
    rs = np.random.RandomState(2)
    W, b = _rand_mlp(rs, dims)
    x1, grouped, x2, idx, xfull, n1, packs = _build(rs, dims, form, M)
    # the kernel rounds inputs and weights to bf16: compare like with like (test_fused_mlp_forward_backward's bf16 case)
    Wt = [w.bfloat16().float().requires_grad_(True) for w in W]
    bt = [v.clone().requires_grad_(True) for v in b]
    xt = xfull.bfloat16().float().requires_grad_(True)
    ref = ops.wide_mlp_reference(xt, Wt, bt, act, round_bf16=True)
    go = torch.from_numpy(rs.standard_normal(size=ref.shape).astype(np.float32))
    if out_bf16:
        go = go.bfloat16().float()
    ref.backward(go)
    Wg = [w.to(dev).requires_grad_(True) for w in W]
    bg = [v.to(dev).requires_grad_(True) for v in b]
    x1g = x1.to(dev).requires_grad_(True)
    x2g = None if x2 is None else x2.to(dev).requires_grad_(True)
    out = ops.fused_mlp128(x1g, Wg, bg, x2=x2g, x2_index=None if idx is None else idx.to(dev), in_dim=dims[0], out_act=act,
                           out_dtype=torch.bfloat16 if out_bf16 else torch.float32, x1_grouped=grouped,
                           x2_packs=None if packs is None else tuple(t.to(dev) for t in packs))
    assert (out.grad_fn.x2_packs is not None) == (packs is not None)
    assert out.shape == ref.shape and out.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
    out.backward(go.to(dev).to(out.dtype))
    torch.cuda.synchronize()
    err = float((out.detach().float().cpu() - ref.detach()).abs().max())
    print("forward max-abs %s M=%d: %.3g" % (dims, M, err))
    assert err < 2e-2, (dims, M, err)
    if grouped is not None:
        dx, pad = _from_xcd8(x1g.grad.cpu(), *grouped)
        assert x1g.grad.dtype == torch.bfloat16 and torch.equal(pad, torch.zeros_like(pad))          # XCD8 padding positions: exactly zero
    else:
        assert x1g.grad.dtype == x1.dtype          # d x1 in the input's dtype
        dx = x1g.grad.float().cpu()[:, :n1]
        assert torch.equal(x1g.grad.float().cpu()[:, n1:], torch.zeros(M, x1.shape[1] - n1))
    checks = [("dx", dx, xt.grad[:, :n1])]
    if x2 is not None:
        want2 = torch.zeros(x2.shape[0], dims[0] - n1).index_add_(0, idx.long(), xt.grad[:, n1:])
        checks.append(("dx2", x2g.grad.cpu()[:, :dims[0] - n1], want2))
        assert torch.equal(x2g.grad.cpu()[:, dims[0] - n1:], torch.zeros(x2.shape[0], 32 - (dims[0] - n1)))
    checks += [("dW%d" % i, Wg[i].grad.cpu(), Wt[i].grad) for i in range(len(W))] + [("db%d" % i, bg[i].grad.cpu(), bt[i].grad) for i in range(len(W))]
    for name, got, want in checks:
        e = _rel_l2(got, want)       # relative L2: a ReLU decision that flips on a last-bit difference moves single entries, not the norm
        print("  %s rel-L2 %.3g" % (name, e))
        assert e < 2e-2, "%s M=%d %s: rel L2 err %g" % (dims, M, name, e)


def _xcd8_problem(dev, dims=(48, 128, 128, 200), act=2, M=1037, seed=4):
    rs = np.random.RandomState(seed)
    W, b = _rand_mlp(rs, dims)
    x = torch.from_numpy(rs.standard_normal(size=(M, dims[0])).astype(np.float32))
    x8 = _to_xcd8(x, dims[0] // 2, 2, fill=0.0).to(dev)
    go = torch.from_numpy(rs.standard_normal(size=(M, dims[-1])).astype(np.float32)).to(dev)
    return [w.to(dev) for w in W], [v.to(dev) for v in b], x8, go, (dims[0] // 2, 2), act


def test_backward_is_deterministic_and_accumulates_dx1(gpu_device):
    ops, L = _ops()
    W, b, x8, go, grouped, act = _xcd8_problem(gpu_device)
    runs = []
    for _ in range(2):
        Wg, bg, xg = [w.clone().requires_grad_(True) for w in W], [v.clone().requires_grad_(True) for v in b], x8.clone().requires_grad_(True)
        out = ops.fused_mlp128(xg, Wg, bg, out_act=act, out_dtype=torch.bfloat16, x1_grouped=grouped)
        out.backward(go.bfloat16())
        runs.append([t.grad.clone() for t in Wg + bg + [xg]])
    for g0, g1 in zip(*runs):
        assert torch.equal(g0, g1)
    # dx1_accumulate: the same backward onto a tensor that already holds a gradient adds to it (two heads on one input)
    Wg, xg = [w.clone().requires_grad_(True) for w in W], x8.clone().requires_grad_(True)
    out = ops.fused_mlp128(xg, Wg, b, out_act=act, out_dtype=torch.bfloat16, x1_grouped=grouped)
    held = torch.randn(x8.shape, device=gpu_device).bfloat16() * (runs[0][-1] != 0)          # padding positions stay zero
    into = held.clone()
    res = ops._mlp128_backward(out.grad_fn.state, out.grad_fn.saved_tensors, go.bfloat16(), dx1_into=into)
    assert res[0] is into
    want = held.float() + runs[0][-1].float()
    assert float((into.float() - want).abs().max()) <= float(want.abs().max()) * 2.0 ** -7          # one bf16 rounding of the sum
    assert not torch.equal(into, held)


def test_no_grad_forward_is_bit_equal_and_saves_nothing(gpu_device):
    ops, L = _ops()
    for dims, act in (((48, 128, 128, 200), 2), ((48, 128, 16), 0)):
        W, b, x8, _, grouped, _ = _xcd8_problem(gpu_device, dims=dims, act=act)
        Wg = [w.clone().requires_grad_(True) for w in W]
        out = ops.fused_mlp128(x8, Wg, b, out_act=act, out_dtype=torch.bfloat16, x1_grouped=grouped)
        assert out.grad_fn is not None and out.grad_fn.saved_tensors[3] is not None
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            quiet = ops.fused_mlp128(x8, Wg, b, out_act=act, out_dtype=torch.bfloat16, x1_grouped=grouped)
        assert torch.equal(quiet, out.detach())
        assert torch.cuda.memory_allocated() - before <= quiet.numel() * 2 + 4096          # the output alone: no workspace


def test_size_refusal_without_allocation(gpu_device):
    """M above PAG_MLP128_MAX_M is refused by the entry points' validation: nothing of that size is allocated or launched."""
    import ctypes
    ops, L = _ops()
    lib = L.load()
    a = L.Mlp128FwdArgs()
    a.x1_dtype, a.k1, a.x1_layout, a.x1_levels, a.x1_feats, a.in_dim, a.n_hidden, a.hidden, a.out_dim = L.BF16, 64, L.LAYOUT_XCD8, 24, 2, 48, 2, 128, 200
    assert lib.pag_mlp128_fwd(ctypes.byref(a), L.MLP128_MAX_M + 1, None) == -1
    assert "M " in lib.pag_last_error_string().decode()
    assert lib.pag_mlp128_workspace_bytes(L.MLP128_MAX_M + 1, 2, 200, 2) == -1


# ---------------------------------------------------------------------------------------------------------------------------- NeFs
def _scene(dev, N=96, S=32, cap_log2=10, seed=0, level=5, **widths):
    """test_gpu_parity._make_scene with decoder widths."""
    import pagnerf_amd
    torch.manual_seed(seed)
    kw = dict(sem_num_layers=1, inst_num_layers=2)
    kw.update(widths)
    nef = pagnerf_amd.PanopticDeltaNeF(grid_type="PermutoGrid", feature_dim=2, num_lods=24, num_classes=6, num_instances=200,
                                       sem_softmax=True, inst_softmax=True, panoptic_features_type="delta", capacity_log_2=cap_log2,
                                       delta_capacity_log_2=cap_log2, coarsest_scale=1.0, finest_scale=1e-4, blas_level=level, precision="bf16", **kw)
    gen = torch.Generator().manual_seed(seed)
    for grid in (nef.grid, nef.delta_grid):
        grid.init_from_scales(random_shift=torch.randn(24, 3, generator=gen) * 10, tables=torch.randn(24, 2 ** cap_log2, 2, generator=gen) * 0.3)
    nef = nef.to(dev)
    o = (torch.rand(N, 3, generator=gen) - 0.5) * 0.6
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    rays = pagnerf_amd.Rays(o.to(dev), d.to(dev), dist_min=0.0, dist_max=2.0)
    occ = torch.rand(2 ** level, 2 ** level, 2 ** level, generator=gen) > 0.35
    for grid in (nef.grid, nef.delta_grid):
        grid.blas_init(occ.reshape(-1))
    return nef, rays, torch.rand(N, S, generator=gen).to(dev)


def _nef_outputs(nef, M, dev, seed=3):
    gen = torch.Generator().manual_seed(seed)
    coords = ((torch.rand(M, 1, 3, generator=gen) - 0.5) * 1.2).to(dev)
    ray_d = torch.nn.functional.normalize(torch.randn(M, 3, generator=gen), dim=-1).to(dev)
    with torch.no_grad():
        return nef(coords=coords, ray_d=ray_d, channels={"density", "rgb", "semantics", "inst_embedding"})


def test_mixed_widths_leave_the_64_wide_path_untouched(gpu_device):
    dev = gpu_device
    narrow, _, _ = _scene(dev)
    mixed, _, _ = _scene(dev, inst_hidden_dim=128)
    for name in ("decoder_density", "decoder_color", "decoder_semantics"):
        getattr(mixed, name).load_state_dict(getattr(narrow, name).state_dict())
    assert mixed.decoder_inst.hidden_dim == 128 and mixed.decoder_semantics.hidden_dim == 64
    assert mixed.can_fuse_panoptic(["semantics"]) and not mixed.can_fuse_panoptic(["inst_embedding"]) and not mixed.can_fuse_panoptic(["inst_embedding", "semantics"])
    M = 1037
    a, b = _nef_outputs(narrow, M, dev), _nef_outputs(mixed, M, dev)
    for ch in ("density", "rgb", "semantics"):
        assert torch.equal(a[ch], b[ch]), ch
    mixed.set_precision("fp32")
    ref = _nef_outputs(mixed, M, dev)["inst_embedding"].float()
    err = float((b["inst_embedding"].float() - ref).abs().max())
    assert err < 3e-2 * max(1.0, float(ref.abs().max())), err


def test_all_128_nef_against_its_fp32_self(gpu_device):
    dev = gpu_device
    nef, _, _ = _scene(dev, hidden_dim=128)
    assert all(getattr(nef, "decoder_" + s).hidden_dim == 128 for s in ("density", "color", "semantics", "inst"))
    assert not nef.can_fuse_panoptic(["semantics"])
    M = 1037
    got = _nef_outputs(nef, M, dev)
    nef.set_precision("fp32")
    ref = _nef_outputs(nef, M, dev)
    for ch in ("density", "rgb", "semantics", "inst_embedding"):
        r = ref[ch].float()
        err = float((got[ch].float() - r).abs().max())
        print("all-128 %s max-abs %.3g (|ref|max %.3g)" % (ch, err, float(r.abs().max())))
        assert err < 3e-2 * max(1.0, float(r.abs().max())), (ch, err)


def _targets(N, dev):
    gen = torch.Generator().manual_seed(9)
    return torch.rand(N, 3, generator=gen).to(dev), torch.randint(0, 6, (N,), generator=gen).to(dev), torch.randint(0, 200, (N,), generator=gen).to(dev)


def _train_loss(rb, gt, sem_gt, inst_gt):
    """test_gpu_train_step.train_loss"""
    F = torch.nn.functional
    loss = 10.0 * torch.abs(rb.rgb - gt).mean()
    loss = loss + 0.1 * F.nll_loss(torch.log(rb.semantics.float() + 1e-27), sem_gt, reduction="none").mean()
    return loss + 1000.0 * F.nll_loss(torch.log(rb.inst_embedding.float() + 1e-27), inst_gt, reduction="none").mean()


def _step(nef, tracer, rays, jitter, targets):
    for p in nef.parameters():
        p.grad = None
    rb = tracer(nef, channels=CH, rays=rays, jitter=jitter, stage="train")
    loss = _train_loss(rb, *targets)
    loss.backward()
    torch.cuda.synchronize()
    return rb, loss.detach().clone(), {k: v.grad.clone() for k, v in nef.named_parameters() if v.grad is not None}


def _group(name):
    return name.split(".")[0] if name.startswith("decoder_") else name.rsplit(".", 1)[0]


def _trace_errors(dev, **widths):
    """rel-L2 of every parameter group's gradient: one eager bf16 training trace against the precision='fp32' trace of the same parameters."""
    import pagnerf_amd
    N, S = 256, 64
    nef, rays, jitter = _scene(dev, N=N, S=S, cap_log2=14, **widths)
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=S, bg_color="white", use_graphs=False)
    targets = _targets(N, dev)
    _, _, got = _step(nef, tracer, rays, jitter, targets)
    nef.set_precision("fp32")
    _, _, want = _step(nef, tracer, rays, jitter, targets)
    assert set(got) == set(want)
    groups = sorted({_group(k) for k in want})
    return {g: _rel_l2(torch.cat([got[k].float().reshape(-1) for k in sorted(want) if _group(k) == g]),
                       torch.cat([want[k].float().reshape(-1) for k in sorted(want) if _group(k) == g])) for g in groups}


def test_training_trace_gradients_against_fp32_within_twice_the_64_wide_error(gpu_device):
    """The 128-wide family may lose at most twice what the 64-wide one loses against the fp32 trace (the sums are twice as long and a flipped
    ReLU moves single entries).  Measured on an MI355X: see DESIGN.md 4.25."""
    e128 = _trace_errors(gpu_device, hidden_dim=128)
    e64 = _trace_errors(gpu_device)
    for g in sorted(e64):
        print("trace gradient rel-L2 %-20s width 128: %.4g   width 64: %.4g" % (g, e128[g], e64[g]))
    for g in sorted(e64):
        assert e128[g] <= 2.0 * e64[g], (g, e128[g], e64[g])


def test_graph_replay_equals_eager_for_a_mixed_width_nef(gpu_device):
    """use_graphs=True over a nef with a 128-wide instance head: the replayed traces equal the eager one bit for bit in the outputs, in the loss and in
    the 128-wide head's own gradients (its weight-gradient slices do not depend on the padded batch size); the other leaves - the 64-wide kernels'
    slabs are cut by the batch size - agree to the 1e-5 of test_gpu_graphs.py."""
    import pagnerf_amd
    dev = gpu_device
    N, S = 96, 32
    nef, rays, jitter = _scene(dev, N=N, S=S, inst_hidden_dim=128)
    targets = _targets(N, dev)
    eager = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=S, bg_color="white", use_graphs=False)
    rb_e, loss_e, g_e = _step(nef, eager, rays, jitter, targets)
    gt = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=S, bg_color="white", use_graphs=True)
    for it in range(3):                    # 0: eager (learns the count), 1: capture, 2: replay
        rb_g, loss_g, g_g = _step(nef, gt, rays, jitter, targets)
        for ch in ("rgb", "alpha", "depth", "semantics", "inst_embedding"):
            assert torch.equal(getattr(rb_g, ch), getattr(rb_e, ch)), (it, ch)
        assert torch.equal(loss_g, loss_e), it
        assert set(g_g) == set(g_e)
        for name, want in g_e.items():
            if name.startswith("decoder_inst."):
                assert torch.equal(g_g[name], want), (it, name)
            else:
                assert _rel_l2(g_g[name].float(), want.float()) < 1e-5, (it, name)
    assert gt._graphs.captures == 1 and gt._graphs.replays >= 1 and gt._graphs.overflows == 0, (gt._graphs.captures, gt._graphs.replays)
