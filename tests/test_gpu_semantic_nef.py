"""SemanticNeF's fused launch (mlp_deep.hip) on the GPU against the reference's golden and against the bf16-operand restatement of
tests/test_semantic_nef_host.py, within the noise floors stored in g15_semantic_nef.npz (tests/golden/make_golden_semantic.py).

Gates: the forward stays within rtol = atol = 3e-2 of the fp32 golden per channel (the project's bf16 tolerance) and its rel-L2 distance to the
bf16-operand / fp32-accumulate restatement is at most 3 x the stored floor (the floor is the distance between two summation orders of that very
arithmetic; orderings differ from each other by up to 1.4 x and the GPU adds its own sin / cos / exp); every parameter gradient likewise, plus 1e-6.
Gradients are never compared with fp32: ReLU flips put the bf16 arithmetic 10 - 20 % away from it."""
import numpy as np
import pytest
import torch

from conftest import golden
import test_semantic_nef_host as H
from oracle.decoders import bf16_operands

pytestmark = pytest.mark.gpu
ALL = {"density", "rgb", "semantics"}


@pytest.fixture(scope="module")
def g15():
    return golden("g15_semantic_nef.npz")


def _nef(dev, **kw):
    return H._nef(**kw).to(dev)


def _restated(g15):
    w = H.make_weights()
    up = {c: g15["up_" + c] for c in ALL}
    return H.restate_grads(w, g15["coords"], g15["dirs"], up, operand_round=bf16_operands, round_grads=True)


def test_forward_matches_golden_and_restatement(gpu_device, g15):
    nef = _nef(gpu_device)
    x, d = torch.from_numpy(g15["coords"]).to(gpu_device), torch.from_numpy(g15["dirs"]).to(gpu_device)
    with torch.no_grad():
        out = nef(channels=ALL, coords=x[:, None], ray_d=d)
    ref, _ = _restated(g15)
    for c in sorted(ALL):
        got = out[c].float().cpu().numpy()
        assert got.shape == g15[c].shape, c
        dist, floor = H.rel_l2(got, ref[c]), float(g15["floor_" + c])
        print("%-10s max|gpu - golden| %.3e   rel-L2 to the bf16 restatement %.3e   floor %.3e (x %.2f)" % (
            c, float(np.abs(got - g15[c]).max()), dist, floor, dist / floor))
        np.testing.assert_allclose(got, g15[c], rtol=3e-2, atol=3e-2, err_msg=c)
        assert dist <= 3.0 * floor, (c, dist, floor)


def test_parameter_gradients_within_noise_floor(gpu_device, g15):
    nef = _nef(gpu_device)
    x, d = torch.from_numpy(g15["coords"]).to(gpu_device), torch.from_numpy(g15["dirs"]).to(gpu_device)
    out = nef(channels=ALL, coords=x[:, None], ray_d=d)
    loss = sum((out[c] * torch.from_numpy(g15["up_" + c]).to(gpu_device)).sum() for c in ALL)
    loss.backward()
    _, ref = _restated(g15)
    floors = dict(zip([str(n) for n in g15["grad_names"]], g15["grad_floors"].tolist()))
    grads = {n: p.grad.float().cpu().numpy() for n, p in nef.named_parameters() if p.requires_grad}
    assert set(grads) == set(ref) == set(floors)
    bad = []
    for n in sorted(grads):
        dist = H.rel_l2(grads[n], ref[n])
        print("%-40s rel-L2 %.3e   floor %.3e (x %.2f)" % (n, dist, floors[n], dist / max(floors[n], 1e-30)))
        if not dist <= 3.0 * floors[n] + 1e-6:
            bad.append((n, dist, floors[n]))
    assert not bad, bad


@pytest.mark.parametrize("M", [0, 1, 33, 1000])
def test_sizes_and_tails(gpu_device, g15, M):
    """M = 0, one sample, one sample past a tile, and a size that is no multiple of the tile (32) or of the workgroup's batch (256): the first M rows
    of the golden batch give the first M rows of its outputs, forward and backward."""
    nef = _nef(gpu_device)
    x, d = torch.from_numpy(g15["coords"][:M]).to(gpu_device), torch.from_numpy(g15["dirs"][:M]).to(gpu_device)
    out = nef(channels=ALL, coords=x[:, None], ray_d=d)
    assert out["density"].shape == (M, 1, 1) and out["rgb"].shape == (M, 1, 3) and out["semantics"].shape == (M, H.CLASSES)
    for c in ALL:
        np.testing.assert_allclose(out[c].detach().float().cpu().numpy(), g15[c][:M], rtol=3e-2, atol=3e-2, err_msg=c)
    sum(out[c].sum() for c in ALL).backward()
    if M == 0:
        assert all(p.grad is None or float(p.grad.abs().sum()) == 0.0 for p in nef.parameters())
        return
    w = H.make_weights()
    up = {"density": np.ones((M, 1, 1), np.float32), "rgb": np.ones((M, 1, 3), np.float32), "semantics": np.ones((M, H.CLASSES), np.float32)}
    _, ref = H.restate_grads(w, g15["coords"][:M], g15["dirs"][:M], up, operand_round=bf16_operands, round_grads=True)
    for n, p in nef.named_parameters():
        if p.requires_grad:
            assert torch.isfinite(p.grad).all(), n
    # a coarse gate at these sizes (few samples: single ReLU flips weigh more than in the 2048-sample floors): the big matrices within 5 %
    for n in ("decoder_features.layers.0.weight", "decoder_features.layers.5.weight", "decoder_features.lout.weight", "decoder_color.layers.0.weight",
              "decoder_semantics.lout.weight", "decoder_density.weight", "decoder_semantics.lout.bias"):
        g = dict(nef.named_parameters())[n].grad.float().cpu().numpy()
        assert H.rel_l2(g, ref[n]) < 5e-2, (n, H.rel_l2(g, ref[n]))


def test_density_only_no_grad_is_bit_identical(gpu_device, g15):
    nef = _nef(gpu_device)
    x, d = torch.from_numpy(g15["coords"]).to(gpu_device), torch.from_numpy(g15["dirs"]).to(gpu_device)
    with torch.no_grad():
        dens = nef(channels="density", coords=x[:, None], ray_d=d)
        full = nef(channels=ALL, coords=x[:, None], ray_d=d)
        sem = nef(channels=["semantics"], coords=x[:, None], ray_d=None)[0]
    assert torch.equal(dens, full["density"]) and torch.equal(sem, full["semantics"])
    train = nef(channels=ALL, coords=x[:, None], ray_d=d)          # the training launch (saves its activations) computes the same values
    for c in ALL:
        assert torch.equal(train[c].detach(), full[c]), c


def test_two_runs_give_bit_identical_gradients(gpu_device, g15):
    x, d = torch.from_numpy(g15["coords"]).to(gpu_device), torch.from_numpy(g15["dirs"]).to(gpu_device)
    runs = []
    for _ in range(2):
        nef = _nef(gpu_device)
        out = nef(channels=ALL, coords=x[:, None], ray_d=d)
        sum((out[c] * torch.from_numpy(g15["up_" + c]).to(gpu_device)).sum() for c in ALL).backward()
        runs.append({n: p.grad.clone() for n, p in nef.named_parameters() if p.requires_grad})
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]), n


def test_unsupported_widths_agree_with_tensor_ops_on_gpu(gpu_device):
    import pagnerf_amd
    nef = pagnerf_amd.SemanticNeF(num_classes=20, hidden_dim=64, blas_level=2).to(gpu_device)
    x, d = H.make_inputs(n=100)
    x, d = torch.from_numpy(x).to(gpu_device), torch.from_numpy(d).to(gpu_device)
    with torch.no_grad():
        out = nef(channels=ALL, coords=x[:, None], ray_d=d)
        ref = nef.cpu().tensor_forward(x.cpu(), d.cpu(), ALL)
    for c in ALL:
        np.testing.assert_allclose(out[c].reshape(ref[c].shape).cpu().numpy(), ref[c].numpy(), rtol=1e-4, atol=1e-5, err_msg=c)
    with pytest.raises(RuntimeError, match="coords"):
        _nef(gpu_device)(channels=ALL, coords=x[:, None].clone().requires_grad_(True), ray_d=d)


def test_traced_training_step_is_eager_and_matches_cpu_trace(gpu_device, g15):
    """A stage='train' trace through PanopticPackedRFTracer: the nef does not take the graph path (no accepts_ray_index) and the rendered channels match
    the CPU path's trace of the same samples within the forward gate (rtol = atol = 3e-2).  The CPU trace is fp32, so its gradients are only a coarse
    check here (finite everywhere, head and lout matrices within 30 %): the gradient gate proper is test_parameter_gradients_within_noise_floor."""
    import pagnerf_amd
    from pagnerf_amd.graphs import GraphRunner
    S, N = 16, 24
    o, d = H.make_rays(N)
    cpu_nef = H._nef()
    ref = H.cpu_trace(cpu_nef, o, d, S)
    (ref["rgb"].sum() + ref["semantics"].sum()).backward()
    nef = _nef(gpu_device)
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=S, bg_color="white", use_graphs=True)
    rays = pagnerf_amd.Rays(o.to(gpu_device), d.to(gpu_device), 0.0, 1.5)
    assert not GraphRunner.eligible(tracer, nef, {"rgb", "depth", "semantics"}, set(), rays, "train")
    # the same samples as the CPU trace: shade() on them (the march itself is the grid's, tested elsewhere)
    t = (torch.arange(S, dtype=torch.float32) + 0.5) / S * 1.5
    samples = (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 1, 3).clamp(-1, 1).to(gpu_device)
    ridx = torch.arange(N, device=gpu_device).repeat_interleave(S)
    pack_start = (torch.arange(N + 1, dtype=torch.int64) * S).to(gpu_device)
    ray_of_pack = torch.arange(N, dtype=torch.int32, device=gpu_device)
    out = tracer.shade(nef, {"rgb", "depth", "semantics"}, set(), rays.dirs, N, ridx, ridx.int(), None, samples, t.repeat(N)[:, None].to(gpu_device),
                       torch.full((N * S, 1), 1.5 / S, device=gpu_device), pack_start, ray_of_pack, 0, "white", "train")
    for c in ("rgb", "depth", "semantics", "alpha"):
        np.testing.assert_allclose(out[c].detach().float().cpu().numpy(), ref[c].detach().numpy(), rtol=3e-2, atol=3e-2, err_msg=c)
    (out["rgb"].sum() + out["semantics"].sum()).backward()
    # and a whole trace() with the march, eagerly
    rb = tracer(nef, channels={"rgb", "depth", "semantics"}, rays=rays, stage="train")
    assert rb.rgb.shape == (N, 3) and rb.semantics.shape == (N, H.CLASSES) and torch.isfinite(rb.rgb).all()
    cg = dict(cpu_nef.named_parameters())
    for n, p in nef.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    # gradients against fp32 only as a coarse check (bf16 sits 10 - 20 % from fp32 on trunk gradients: the header); the exact gate is the test above
    for n in ("decoder_semantics.lout.weight", "decoder_color.lout.weight", "decoder_features.lout.weight"):
        assert H.rel_l2(dict(nef.named_parameters())[n].grad.cpu().numpy(), cg[n].grad.numpy()) < 0.3, n


def test_batched_coords_with_one_direction_per_ray(gpu_device, g15):
    """The reference's argument form: coords [B,S,3] with ray_d [B,3] (semantic_nerf.py:209-210).  The training launch always runs the colour head, so
    it must get one direction per SAMPLE whatever channels were asked for: with gradients enabled and channels without rgb the B-row ray_d is not handed
    to the kernel (it would read B * S rows of it).  Values equal the flat call's bits; the gradients of a density + semantics loss equal the bits of
    the all-channel flat call with the same loss, and the colour head's gradients are exactly zero."""
    B, S = 8, 5
    x = torch.from_numpy(g15["coords"][:B * S]).to(gpu_device)
    d = torch.from_numpy(g15["dirs"][:B]).to(gpu_device)
    d_flat = d[:, None].repeat(1, S, 1).reshape(-1, 3)
    up_d = torch.from_numpy(g15["up_density"][:B * S]).to(gpu_device)
    up_s = torch.from_numpy(g15["up_semantics"][:B * S]).to(gpu_device)
    with torch.no_grad():
        flat = _nef(gpu_device)(channels=ALL, coords=x[:, None], ray_d=d_flat)
    nef = _nef(gpu_device)
    out = nef(channels={"density", "semantics"}, coords=x.reshape(B, S, 3), ray_d=d)
    assert set(out) == {"density", "semantics"} and out["density"].shape == (B, S, 1) and out["semantics"].shape == (B * S, H.CLASSES)
    assert torch.equal(out["density"].detach().reshape(-1), flat["density"].reshape(-1)) and torch.equal(out["semantics"].detach(), flat["semantics"])
    ((out["density"].reshape(-1) * up_d.reshape(-1)).sum() + (out["semantics"] * up_s).sum()).backward()
    ref = _nef(gpu_device)
    o2 = ref(channels=ALL, coords=x[:, None], ray_d=d_flat)
    ((o2["density"].reshape(-1) * up_d.reshape(-1)).sum() + (o2["semantics"] * up_s).sum()).backward()
    rg = dict(ref.named_parameters())
    for n, p in nef.named_parameters():
        if not p.requires_grad:
            continue
        if n.startswith("decoder_color"):
            assert float(p.grad.abs().max()) == 0.0, n
        else:
            assert float(p.grad.abs().max()) > 0.0 and torch.equal(p.grad, rg[n].grad), n
    # all channels on the batched form: the directions are repeated per sample, with and without gradients
    full = _nef(gpu_device)(channels=ALL, coords=x.reshape(B, S, 3), ray_d=d)
    assert full["rgb"].shape == (B, S, 3) and torch.equal(full["rgb"].detach().reshape(-1, 3), flat["rgb"].reshape(-1, 3))
    with torch.no_grad():
        dens = _nef(gpu_device)(channels="density", coords=x.reshape(B, S, 3), ray_d=d)
    assert torch.equal(dens.reshape(-1), flat["density"].reshape(-1))


def test_launch_refuses_directions_that_are_not_per_sample(gpu_device, g15):
    from pagnerf_amd.semantic_nef import deep_forward
    nef = _nef(gpu_device)
    lins = nef.linears()
    W, b = [l.weight.detach().float().contiguous() for l in lins], [l.bias.detach().float().contiguous() for l in lins]
    x, d = torch.from_numpy(g15["coords"][:64]).to(gpu_device), torch.from_numpy(g15["dirs"][:8]).to(gpu_device)
    with pytest.raises(ValueError, match="one direction per sample"):
        deep_forward(x, d, H.CLASSES, 7, W, b)
    with pytest.raises(ValueError, match="one direction per sample"):
        deep_forward(x, None, H.CLASSES, 2, W, b)
    with pytest.raises(ValueError, match="ray_d of shape"):
        nef(channels=ALL, coords=x.reshape(8, 8, 3), ray_d=d[:4])


def test_second_backward_raises_a_clear_error(gpu_device, g15):
    nef = _nef(gpu_device)
    x, d = torch.from_numpy(g15["coords"][:64]).to(gpu_device), torch.from_numpy(g15["dirs"][:64]).to(gpu_device)
    out = nef(channels=ALL, coords=x[:, None], ray_d=d)
    loss = sum(out[c].sum() for c in ALL)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
