"""pagnerf_amd.loss.SupConLoss (csrc/supcon.hip) on the GPU: the reference's values (tests/golden/g11_supcon.npz), the trainer's full-size shapes,
bitwise determinism, graph capture, memory, bf16 / strided features, and one delta-density training step.

Accuracy rule: the kernel's error against the fp64 restatement (tests/test_supcon_host.py, pinned there to the reference) is at most twice the
reference's own fp32 error on the same data, plus 1e-7 of the values' scale."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_supcon_host import load_case, restated, restated_rows

pytestmark = pytest.mark.gpu


def _rule(kern, ref32, f64, what):
    kern, ref32, f64 = (np.asarray(torch.as_tensor(a).detach().double().cpu()) for a in (kern, ref32, f64))
    if f64.size == 0:
        return
    ek, er, scale = np.abs(kern - f64).max(), np.abs(ref32 - f64).max(), np.abs(f64).max()
    assert ek <= 2 * er + 1e-7 * scale, "%s: kernel error %.3e > 2 x reference error %.3e + 1e-7 x %.3e" % (what, ek, er, scale)


def _grad_rule(kern, ref32, f64, zero_rows, what):
    """The rule on the rows of ordinary features and, separately, on the all-zero rows (their gradient is df / 1e-12)."""
    B, P = f64.shape[:2]
    z = np.zeros((B, P), dtype=bool)
    for b, p in zero_rows:
        z[b, p] = True
    kern, ref32, f64 = (np.asarray(torch.as_tensor(a).detach().double().cpu()) for a in (kern, ref32, f64))
    _rule(kern[~z], ref32[~z], f64[~z], what + " (rows)")
    _rule(kern[z], ref32[z], f64[z], what + " (zero rows)")


def _as_rows(out, mask):
    """SupConLoss's 'none' list (per image [1, |S_b|] or a 0-d zero) -> [B, P] with zeros at the other rows."""
    B, P = mask.shape
    rows = torch.zeros(B, P, device=mask.device)
    for b, o in enumerate(out):
        if o.dim() == 2:
            rows[b][mask[b]] = o[0]
        else:
            assert o.dim() == 0 and float(o) == 0.0
    return rows


def _f64_case(c):
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    mask = torch.from_numpy(c["mask"]) if c["mask"] is not None else None
    out = restated(x, torch.from_numpy(c["labels"]), mask, c["T"], c["Tb"], c["pn"], c["reduction"])
    (out * torch.as_tensor(np.asarray(c["g"]), dtype=torch.float64)).sum().backward()
    return out.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("name", [str(n) for n in golden("g11_supcon.npz")["names"]])
def test_supcon_matches_reference_golden(gpu_device, name):
    from pagnerf_amd.loss import SupConLoss
    c = load_case(golden("g11_supcon.npz"), name)
    dev = gpu_device
    x = torch.from_numpy(c["x"]).to(dev).requires_grad_(True)
    labels = torch.from_numpy(c["labels"]).to(dev)
    mask = torch.from_numpy(c["mask"]).to(dev) if c["mask"] is not None else None
    out = SupConLoss(temperature=c["T"], base_temperature=c["Tb"], pn_ratio=c["pn"])(x, labels, reduction=c["reduction"], anchor_mask=mask)
    if isinstance(out, list):
        out = _as_rows(out, mask)
    assert tuple(out.shape) == c["loss"].shape and out.dtype == torch.float32
    g = torch.as_tensor(np.asarray(c["g"]), device=dev)
    (out * g).sum().backward()
    v64, g64 = _f64_case(c)
    _rule(out, c["loss"], v64, name + " value")
    _grad_rule(x.grad, c["grad"], g64, c["zero_rows"], name + " gradient")
    if c["mask"] is not None:
        grad = x.grad.cpu().numpy()
        assert not grad[~c["mask"]].any(), "non-anchor rows must get an exactly zero gradient"
        for b in range(c["mask"].shape[0]):
            if not c["mask"][b].any() or np.unique(c["labels"][b][c["mask"][b]]).size < 2:
                assert not grad[b].any(), "skipped image %d must get an exactly zero gradient" % b


def _trainer_inputs(dev, D, masked, dtype=torch.float32, seed=0):
    gen = torch.Generator().manual_seed(seed)
    B, P = 6, 4096
    x = torch.randn(B, P, D, generator=gen)
    if D == 6:
        x = torch.softmax(2.0 * x, -1) + 1e-27
        labels = torch.randint(0, 6, (B, P), generator=gen)
    else:
        labels = torch.randint(0, 40, (B, P), generator=gen)
    mask = (torch.rand(B, P, generator=gen) > 0.15) if masked else None
    return x.to(dev, dtype), labels.to(dev), (mask.to(dev) if masked else None)


@pytest.mark.parametrize("D,masked", [(200, True), (6, False)])
def test_supcon_full_size_against_fp64(gpu_device, D, masked):
    """B = 6, P = 4096: D = 200 with ~15 % of the rays masked out (the instance call), D = 6 without a mask (the semantic call)."""
    from pagnerf_amd.loss import SupConLoss
    x, labels, mask = _trainer_inputs(gpu_device, D, masked)
    fn = SupConLoss(temperature=0.07, pn_ratio=0.5 if masked else 0.3)
    res = {}
    for kind, xx in (("kernel", x), ("f32", x), ("f64", x.double())):
        xx = xx.detach().clone().requires_grad_(True)
        if kind == "kernel":
            out = fn(xx, labels, reduction="mean", anchor_mask=mask)
        else:
            out = restated(xx, labels, mask, 0.07, 0.07, fn_pn(fn), "mean")
        out.backward()
        res[kind] = (out.detach(), xx.grad)
    _rule(res["kernel"][0], res["f32"][0], res["f64"][0], "value")
    _grad_rule(res["kernel"][1], res["f32"][1], res["f64"][1], [], "gradient")


def fn_pn(fn):
    """pn_ratio back from the module's weights (pos_weight < 1 iff pn_ratio < 0.5)."""
    return fn.pos_weight / 2 if fn.pos_weight < 1 else 1 - fn.neg_weight / 2


def test_supcon_is_bitwise_deterministic(gpu_device):
    from pagnerf_amd.loss import SupConLoss
    x, labels, mask = _trainer_inputs(gpu_device, 200, True, seed=1)
    outs = []
    for _ in range(2):
        xx = x.clone().requires_grad_(True)
        out = SupConLoss()(xx, labels, anchor_mask=mask)
        out.backward()
        outs.append((out.detach(), xx.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_supcon_graph_capture_replays_like_eager(gpu_device):
    """No host synchronisation on the 'mean' path: forward + backward captured once and replayed on new inputs equals eager bitwise."""
    from pagnerf_amd.loss import SupConLoss
    fn = SupConLoss(pn_ratio=0.3)
    x, labels, mask = _trainer_inputs(gpu_device, 200, True, seed=2)
    sx, sl, sm = x.clone().requires_grad_(True), labels.clone(), mask.clone()

    def step():
        out = fn(sx, sl, reduction="mean", anchor_mask=sm)
        return out, torch.autograd.grad(out, sx)[0]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_grad = step()
    for seed in (3, 4):
        x2, l2, m2 = _trainer_inputs(gpu_device, 200, True, seed=seed)
        with torch.no_grad():
            sx.copy_(x2)
            sl.copy_(l2)
            sm.copy_(m2)
        graph.replay()
        xe = x2.clone().requires_grad_(True)
        e_out = fn(xe, l2, reduction="mean", anchor_mask=m2)
        e_grad = torch.autograd.grad(e_out, xe)[0]
        torch.cuda.synchronize()
        assert torch.equal(g_out, e_out) and torch.equal(g_grad, e_grad), seed


def test_supcon_memory_is_linear_in_rays(gpu_device):
    from pagnerf_amd.loss import SupConLoss
    x, labels, mask = _trainer_inputs(gpu_device, 200, True, seed=5)
    x.requires_grad_(True)
    fn = SupConLoss()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn(x, labels, anchor_mask=mask)
    grad = torch.autograd.grad(out, x)[0]
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise <= 4 * x.numel() * x.element_size() + (1 << 20), rise
    assert grad.shape == x.shape


def test_supcon_bf16_and_strided_features(gpu_device):
    """bf16 features through a strided [B, P, D] view of a [B P, D + 8] buffer: fp32 loss, bf16 gradient at the view's elements, under the rule
    against the f32 restatement of the same bf16 values (the reference's fp32 error taken on those values)."""
    from pagnerf_amd.loss import SupConLoss
    dev = gpu_device
    gen = torch.Generator().manual_seed(7)
    B, P, D = 3, 700, 200
    base = torch.randn(B * P, D + 8, generator=gen).to(dev, torch.bfloat16).requires_grad_(True)
    labels = torch.randint(0, 9, (B, P), generator=gen).to(dev)
    mask = (torch.rand(B, P, generator=gen) > 0.2).to(dev)
    view = base[:, 4:4 + D].reshape(B, P, D)
    assert view.stride() == (P * (D + 8), D + 8, 1)
    out = SupConLoss(pn_ratio=0.8)(view, labels, reduction="sum", anchor_mask=mask)
    out.backward()
    assert out.dtype == torch.float32 and base.grad.dtype == torch.bfloat16
    assert not base.grad[:, :4].any() and not base.grad[:, 4 + D:].any()
    xv = view.detach().float()
    res = {}
    for kind, xx in (("f32", xv), ("f64", xv.double())):
        xx = xx.clone().requires_grad_(True)
        o = restated(xx, labels, mask, 0.07, 0.07, 0.8, "sum")
        o.backward()
        res[kind] = (o.detach(), xx.grad)
    _rule(out, res["f32"][0], res["f64"][0], "bf16 value")
    g = base.grad[:, 4:4 + D].reshape(B, P, D).float()
    # the gradient is rounded to bf16 on the way out: compare against the fp64 gradient at bf16's resolution
    g64 = res["f64"][1].float()
    assert torch.all((g - g64).abs() <= 2 * (res["f32"][1] - g64).abs().max() + 2 ** -7 * g64.abs().amax(-1, keepdim=True) + 1e-7 * g64.abs().max())


def test_supcon_dd_train_step(gpu_device):
    """PanopticDDensityNeF + PanopticDDensityPackedRFTracer with a raw 200-wide instance head on the bf16 path: rendered loss + inst_weight x
    SupConLoss.  The instance decoder's gradients equal those of the same step with the fp64-restated loss (cast to fp32) under the rule."""
    import pagnerf_amd
    from pagnerf_amd.loss import SupConLoss
    dev = gpu_device
    torch.manual_seed(11)
    nef = pagnerf_amd.PanopticDDensityNeF(grid_type="HashGridTorch", feature_dim=2, num_lods=8, num_classes=6, num_instances=200,
                                          sem_num_layers=1, sem_softmax=True, inst_num_layers=2, inst_softmax=False,
                                          delta_num_layers=1, delta_hidden_dim=64, codebook_bitwidth=12, blas_level=3, precision="bf16").to(dev)
    gen = torch.Generator().manual_seed(12)
    for g in (nef.grid, nef.delta_grid):
        g.init_from_resolutions([16] * 7 + [256])
        g.tables.data.copy_(torch.randn(g.tables.shape, generator=gen).to(dev) * 0.5)
    with torch.no_grad():
        nef.decoder_density.lout.bias[0] = 3.0
    tracer = pagnerf_amd.PanopticDDensityPackedRFTracer(raymarch_type="ray", num_steps=32, bg_color="white")
    B, R = 2, 256
    rays = pagnerf_amd.Rays(((torch.rand(B * R, 3, generator=gen) - 0.5) * 0.5).to(dev),
                            torch.nn.functional.normalize(torch.randn(B * R, 3, generator=gen), dim=-1).to(dev), 0.0, 2.0)
    gt = torch.rand(B * R, 3, generator=gen).to(dev)
    inst_gts = torch.randint(0, 6, (B, R), generator=gen).to(dev)
    inst_mask = (torch.rand(B, R, generator=gen) > 0.15).to(dev)
    inst_weight = 0.1
    fn = SupConLoss(temperature=0.07, pn_ratio=0.5)
    grads = {}
    for kind in ("kernel", "f32", "f64"):
        nef.zero_grad(set_to_none=True)
        rb = tracer(nef, channels={"rgb", "depth", "semantics", "inst_embedding"}, rays=rays, stage="train")
        emb = rb.inst_embedding.reshape(B, -1, rb.inst_embedding.shape[-1])
        assert emb.shape[-1] == 200
        if kind == "kernel":
            inst = fn(emb, inst_gts, reduction="mean", anchor_mask=inst_mask)
        else:
            dt = torch.float64 if kind == "f64" else torch.float32
            inst = restated(emb.to(dt), inst_gts, inst_mask, 0.07, 0.07, 0.5, "mean").float()
        loss = torch.abs(rb.rgb - gt).mean() + inst_weight * inst
        loss.backward()
        grads[kind] = {n: p.grad.detach().clone() for n, p in nef.decoder_inst.named_parameters()}
    for n in grads["kernel"]:
        assert torch.isfinite(grads["kernel"][n]).all() and float(grads["kernel"][n].abs().sum()) > 0, n
        _rule(grads["kernel"][n], grads["f32"][n], grads["f64"][n], "decoder_inst." + n)
