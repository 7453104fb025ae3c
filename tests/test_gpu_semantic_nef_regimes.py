"""SemanticNeF's fused launch (mlp_deep.hip) in the launch regimes and at the class counts tests/test_gpu_semantic_nef.py does not reach: the
persistent kernels' second batch (more than 256 x 256 samples), weight-gradient slices of several tile pairs / of none / with an odd tile count, 1 and
16 classes, upstream gradients on one channel only (the others NULL), and every channel mask under no_grad.

Cases and their seeds: tests/test_semantic_nef_host.py::REGIME_CASES; noise floors: g15b_semantic_regimes.npz
(tests/golden/make_golden_semantic_regimes.py).  Gates, as in tests/test_gpu_semantic_nef.py: outputs elementwise rtol = atol = 3e-2 against the plain
fp32 restatement; output rel-L2 to the bf16-operand restatement <= 3 x the case's stored floor; every parameter gradient's rel-L2 to the bf16-operand
restatement <= 3 x its stored floor + 1e-6.  Every ratio is printed before it is asserted.  The CPU restatement of a case is computed once per module
and never modified; the 65 825-row launch runs once and is shared too."""
import numpy as np
import pytest
import torch

from conftest import golden
import test_semantic_nef_host as H
from oracle.decoders import bf16_operands

pytestmark = pytest.mark.gpu
ALL = set(H.CHANNELS)
HEAD_OF = {"density": "decoder_density.", "rgb": "decoder_color.", "semantics": "decoder_semantics."}


@pytest.fixture(scope="module")
def g15b():
    return golden("g15b_semantic_regimes.npz")


_CPU, _BIG = {}, {}


def _case(key):
    """The CPU side of a case: inputs, upstream gradients, the plain fp32 outputs and the bf16-operand restatement's outputs and gradients."""
    if key not in _CPU:
        w, x, d, up, plain = H.regime_case(key)
        out, grads = H.restate_grads(w, x, d, up, operand_round=bf16_operands, round_grads=True)
        _CPU[key] = {"x": x, "d": d, "up": up, "plain": plain, "out": out, "grads": grads}
    return _CPU[key]


def _launch(dev, key, zeros_for_the_rest=False):
    """One training launch and backward of a case.  The loss is built from the case's channels only, so autograd hands None - a NULL pointer - for
    the others; with zeros_for_the_rest they get explicit zero tensors instead.
    -> (outputs of the training launch, outputs under no_grad, parameter gradients), on the device."""
    c, (M, C, chans) = _case(key), H.REGIME_CASES[key]
    nef = H._nef(classes=C).to(dev)
    x, d = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["d"]).to(dev)
    with torch.no_grad():
        quiet = nef(channels=ALL, coords=x[:, None], ray_d=d)
    out = nef(channels=ALL, coords=x[:, None], ray_d=d)
    loss = sum((out[ch] * torch.from_numpy(c["up"][ch]).to(dev)).sum() for ch in H.CHANNELS if ch in chans)
    if zeros_for_the_rest:
        loss = loss + sum((out[ch] * torch.zeros_like(out[ch])).sum() for ch in H.CHANNELS if ch not in chans)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in nef.named_parameters() if p.requires_grad}
    return {ch: v.detach() for ch, v in out.items()}, quiet, grads


def _big(dev):
    """The 65 825-row launch, once per module."""
    if not _BIG:
        _BIG["train"], _BIG["quiet"], _BIG["grads"] = _launch(dev, "m65825")
    return _BIG


def _check_outputs(key, out, g15b, what):
    c, (M, C, _) = _case(key), H.REGIME_CASES[key]
    shapes = {"density": (M, 1, 1), "rgb": (M, 1, 3), "semantics": (M, C)}
    bad = []
    for ch in H.CHANNELS:
        got = out[ch].float().cpu().numpy()
        assert got.shape == shapes[ch] and np.isfinite(got).all(), (key, ch, got.shape)
        dist, floor = H.rel_l2(got, c["out"][ch]), float(g15b[key + "_floor_" + ch])
        print("%-8s %-9s %-10s max|gpu - fp32| %.3e   rel-L2 to the bf16 restatement %.3e   floor %.3e (x %.2f)" % (
            key, what, ch, float(np.abs(got - c["plain"][ch]).max()), dist, floor, dist / floor))
        np.testing.assert_allclose(got, c["plain"][ch], rtol=3e-2, atol=3e-2, err_msg="%s %s %s" % (key, what, ch))
        if not dist <= 3.0 * floor:
            bad.append((ch, dist, floor))
    assert not bad, (key, what, bad)


def _check_grads(key, grads, g15b):
    c, C = _case(key), H.REGIME_CASES[key][1]
    floors = dict(zip([str(n) for n in g15b[key + "_grad_names"]], g15b[key + "_grad_floors"].tolist()))
    assert set(grads) == set(c["grads"]) == set(floors)
    bad = []
    for n in sorted(grads):
        got = grads[n].float().cpu().numpy()
        assert got.shape == H.param_shapes(classes=C)[n] and np.isfinite(got).all(), (key, n, got.shape)
        dist = H.rel_l2(got, c["grads"][n])
        print("%-8s %-40s rel-L2 %.3e   floor %.3e (x %.2f of 3 x floor + 1e-6)" % (key, n, dist, floors[n], dist / (3.0 * floors[n] + 1e-6)))
        if not dist <= 3.0 * floors[n] + 1e-6:
            bad.append((n, dist, floors[n]))
    assert not bad, (key, bad)


def _print_plain_sums(key, grads):
    """decoder_density.bias and decoder_semantics.lout.bias are plain fp32 sums of the bf16-rounded per-sample dz.  Printed for the record: their
    distance from the float64 sum of those terms beside chain . 2^-24 . sum|terms|, where chain = 64 . per + n_split is the longest sequential fp32
    addition of the weight-gradient pass (64 samples per tile pair, `per` pairs per slice) plus the finish pass over the slices."""
    c = _case(key)
    _, _, n_split, per = H.wgrad_split(H.REGIME_CASES[key][0])
    chain = 64 * per + n_split
    alive = torch.from_numpy(c["out"]["density_pre"] > 0).double()[:, None]
    terms = {"decoder_density.bias": torch.from_numpy(c["up"]["density"]).reshape(-1, 1).bfloat16().double() * alive,
             "decoder_semantics.lout.bias": torch.from_numpy(c["up"]["semantics"]).bfloat16().double()}
    for n, t in terms.items():
        err = (grads[n].double().cpu() - t.sum(0)).abs()
        bound = chain * 2.0 ** -24 * t.abs().sum(0)
        print("%-8s %-30s max|gpu - float64 sum| %.3e   chain %d: smallest bound %.3e (largest error / bound %.1e)" % (
            key, n, float(err.max()), chain, float(bound.min()), float((err / bound).max())))


@pytest.mark.parametrize("key", ["m2049", "m65825"])
def test_regimes_forward_and_every_parameter_gradient(gpu_device, g15b, key):
    """2049 samples: 65 tiles (odd, the last one holds one sample) in 33 pairs over 32 slices - two pairs per slice in slices 0 .. 15, one in slice
    16, none in slices 17 .. 31.  65 825 samples: 258 batches over 256 workgroups, so workgroups 0 and 1 walk a second batch (layer 0 staged over the
    last head's image, the PE scratch reused), and 33 pairs per slice with a short last slice.  The forward under the training launch and under
    no_grad, and every parameter gradient, within the gates of the header."""
    M = H.REGIME_CASES[key][0]
    ntile, npair, n_split, per = H.wgrad_split(M)
    print("%s: %d tiles, %d pairs, %d slices of %d pairs" % (key, ntile, npair, n_split, per))
    assert per >= 2, (ntile, npair, n_split, per)
    if key == "m2049":
        assert ntile % 2 == 1 and M % 32 == 1 and per * (n_split - 1) >= npair and npair % per != 0, (ntile, npair, n_split, per)    # an empty slice
        train, quiet, grads = _launch(gpu_device, key)
    else:
        assert (M + 255) // 256 > 256 and npair % per != 0, (M, npair, per)
        big = _big(gpu_device)
        train, quiet, grads = big["train"], big["quiet"], big["grads"]
    _check_outputs(key, train, g15b, "training")
    _check_outputs(key, quiet, g15b, "no_grad")
    _print_plain_sums(key, grads)
    _check_grads(key, grads, g15b)


def test_outputs_do_not_depend_on_the_position_in_the_launch(gpu_device):
    """A sample's outputs depend on that sample alone: it sits on one lane and every dot product runs in the same k order.  The rows of the 65 825
    launch in workgroup 0's first batch (0 .. 255), in its second batch (65536 .. 65791) and in the ragged tail (65792 .. 65824), launched alone as
    one 545-row batch, give the same bits - with and without saved activations."""
    big, c = _big(gpu_device), _case("m65825")
    M = H.REGIME_CASES["m65825"][0]
    assert M == 65825
    rows = torch.cat([torch.arange(0, 256), torch.arange(65536, 65792), torch.arange(65792, M)])
    assert rows.numel() == 545
    nef = H._nef().to(gpu_device)
    x, d = torch.from_numpy(c["x"])[rows].contiguous().to(gpu_device), torch.from_numpy(c["d"])[rows].contiguous().to(gpu_device)
    with torch.no_grad():
        quiet = nef(channels=ALL, coords=x[:, None], ray_d=d)
    train = nef(channels=ALL, coords=x[:, None], ray_d=d)
    rows = rows.to(gpu_device)
    for what, small, large in (("no_grad", quiet, big["quiet"]), ("training", train, big["train"])):
        for ch in H.CHANNELS:
            a, b = small[ch].detach(), large[ch][rows]
            differ = (a != b).reshape(545, -1).any(1)
            print("%-9s %-10s rows that differ: %d of 545 (first batch %d, second batch %d, tail %d)" % (
                what, ch, int(differ.sum()), int(differ[:256].sum()), int(differ[256:512].sum()), int(differ[512:].sum())))
            assert torch.equal(a, b), (what, ch)


def test_two_runs_at_65825_samples_give_bit_identical_gradients(gpu_device):
    """The slabs are added in slice order and nothing is accumulated with atomics: a second run gives the first one's bits."""
    first = _big(gpu_device)["grads"]
    _, _, second = _launch(gpu_device, "m65825")
    assert set(first) == set(second)
    for n in first:
        assert torch.equal(first[n], second[n]), n


@pytest.mark.parametrize("key", ["c1", "c16"])
def test_class_counts(gpu_device, g15b, key):
    """1 and 16 classes (the ends of what pag_deep_mlp_supported accepts): the semantic output layer is a 32-row padded block whose rows >= C are
    masked in the forward store, in the backward's g_sem load and in the packed and transposed weight images."""
    M, C, _ = H.REGIME_CASES[key]
    train, quiet, grads = _launch(gpu_device, key)
    assert train["semantics"].shape == (M, C) and quiet["semantics"].shape == (M, C)
    assert grads["decoder_semantics.lout.weight"].shape == (C, 128) and grads["decoder_semantics.lout.bias"].shape == (C,)
    _check_outputs(key, train, g15b, "training")
    _check_outputs(key, quiet, g15b, "no_grad")
    _check_grads(key, grads, g15b)


@pytest.mark.parametrize("channel", H.CHANNELS)
def test_upstream_gradient_on_one_channel_only(gpu_device, g15b, channel):
    """The loss is built from one channel, so the backward gets NULL for the two others: the same bits as with explicit zero tensors for them, within
    the gates of the restatement with that upstream, and exactly zero on the heads that received nothing."""
    key = "only_" + channel
    _, _, grads = _launch(gpu_device, key)
    _, _, zeros = _launch(gpu_device, key, zeros_for_the_rest=True)
    for n in grads:
        assert torch.equal(grads[n], zeros[n]), n
    _check_grads(key, grads, g15b)
    for other in H.CHANNELS:
        for n in grads:
            if n.startswith(HEAD_OF[other]):
                peak = float(grads[n].abs().max())
                assert (peak == 0.0) == (other != channel), (n, peak)
    assert all(float(g.abs().max()) > 0.0 for n, g in grads.items() if n.startswith("decoder_features."))


def test_every_channel_mask_under_no_grad(gpu_device):
    """All seven masks through deep_forward at 289 samples (two batches, a one-sample last tile): every channel a mask asks for has the bits of the
    all-channel launch, every other one comes back None.  `rgb` alone skips the density / semantics stage altogether."""
    from pagnerf_amd.semantic_nef import deep_forward, CH_BITS
    M = 289
    nef = H._nef().to(gpu_device)
    lins = nef.linears()
    W, b = [l.weight.detach().float().contiguous() for l in lins], [l.bias.detach().float().contiguous() for l in lins]
    x, d = H.make_inputs(n=M)
    x, d = torch.from_numpy(x).to(gpu_device), torch.from_numpy(d).to(gpu_device)
    full = dict(zip(H.CHANNELS, deep_forward(x, d, H.CLASSES, 7, W, b)[:3]))
    w = {k: torch.from_numpy(v) for k, v in H.make_weights().items()}
    with torch.no_grad():
        plain = H.restate(w, x.cpu(), d.cpu())
    for ch, shape in (("density", (M,)), ("rgb", (M, 3)), ("semantics", (M, H.CLASSES))):
        assert full[ch].shape == shape
        np.testing.assert_allclose(full[ch].cpu().numpy(), plain[ch].reshape(shape).numpy(), rtol=3e-2, atol=3e-2, err_msg=ch)
    for mask in range(1, 7):
        got = dict(zip(H.CHANNELS, deep_forward(x, d, H.CLASSES, mask, W, b)[:3]))
        for ch in H.CHANNELS:
            if mask & CH_BITS[ch]:
                assert got[ch] is not None and torch.equal(got[ch], full[ch]), (mask, ch)
            else:
                assert got[ch] is None, (mask, ch)
