"""CPU-side checks of pagnerf_amd.loss.SupConLoss (csrc/supcon.hip): the reference's constructor signature, no CPU fallback, argument validation of the
pag_supcon_* entry points before any launch, and the tensor-op restatement the GPU tests compare against, pinned to the reference's own values
(tests/golden/g11_supcon.npz, tests/golden/make_golden_supcon.py)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from conftest import golden


def case_features(seed, B, P, D, kind):
    """The features of a g11 case (same function as make_golden_supcon.py)."""
    z = np.random.RandomState(seed).standard_normal(size=(B, P, D))
    if kind == "probs":
        e = np.exp(2.0 * z - (2.0 * z).max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True)).astype(np.float32) + np.float32(1e-27)
    return z.astype(np.float32)


def load_case(z, name):
    seed, B, P, D, probs, masked = (int(v) for v in z[name + "_meta"])
    x = case_features(seed, B, P, D, "probs" if probs else "normal")
    for b, p in z[name + "_zero_rows"]:
        x[b, p] = 0.0
    T, Tb, pn = (float(v) for v in z[name + "_params"])
    return dict(x=x, labels=z[name + "_labels"], mask=z[name + "_mask"] if masked else None, T=T, Tb=Tb, pn=pn,
                reduction=str(z[name + "_reduction"]), g=z[name + "_g"], loss=z[name + "_loss"], grad=z[name + "_grad"], zero_rows=z[name + "_zero_rows"])


def restated_rows(x, labels, anchor_mask, T, Tb, pn_ratio):
    """Per-row supervised-contrastive loss [B, P] (0 at non-anchors and in skipped images) of features x [B, P, D] in x's dtype, written from the formula
    (SupConLoss's docstring) with tensor ops, one image at a time; differentiable with respect to x."""
    pw, nw = min(1.0, 2 * pn_ratio), min(1.0, 2 * (1 - pn_ratio))
    B, P = x.shape[:2]
    f = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    rows = []
    for b in range(B):
        sel = anchor_mask[b] if anchor_mask is not None else torch.ones(P, dtype=torch.bool, device=x.device)
        fb, lb = f[b][sel], labels[b][sel]
        if anchor_mask is not None and (int(sel.sum()) == 0 or lb.unique().numel() < 2):
            rows.append(torch.zeros(P, dtype=x.dtype, device=x.device))
            continue
        n = fb.shape[0]
        A = fb @ fb.T / T
        logits = A - A.max(1, keepdim=True).values.detach()
        off = 1.0 - torch.eye(n, dtype=x.dtype, device=x.device)
        lse = torch.log((torch.exp(logits) * off).sum(1, keepdim=True))
        pos = (lb[:, None] == lb[None, :]).to(x.dtype) * off
        s = (pos * (pw * logits - nw * lse)).sum(1) / (pos.sum(1) + 1e-16)
        row = torch.zeros(P, dtype=x.dtype, device=x.device).masked_scatter(sel, -(T / Tb) * s)
        rows.append(row)
    return torch.stack(rows)


def restated(x, labels, anchor_mask, T, Tb, pn_ratio, reduction):
    """The value SupConLoss returns, in the reference's shapes ('none' with anchor_mask: [B, P] with zeros instead of the per-image list)."""
    rows = restated_rows(x, labels, anchor_mask, T, Tb, pn_ratio)
    if reduction == "none":
        return rows
    if anchor_mask is None:
        return rows.sum() if reduction == "sum" else rows.mean()
    if reduction == "sum":
        return rows.sum().reshape(1)
    return (rows.sum(1) / anchor_mask.sum().clamp(min=1)).sum().reshape(1)


def backward_with(out, g):
    """out.backward with the fixture's upstream gradient (a scalar, or [B, P] for 'none')."""
    g = torch.as_tensor(np.asarray(g), dtype=out.dtype, device=out.device)
    (out * g).sum().backward()


def test_supcon_loss_has_the_reference_constructor():
    from pagnerf_amd.loss import SupConLoss
    params = list(inspect.signature(SupConLoss.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("temperature", 0.07), ("contrast_mode", "all"), ("base_temperature", 0.07), ("pn_ratio", 0.5)]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params)
    m = SupConLoss(temperature=0.1, pn_ratio=0.8)
    assert m.pos_weight == 1 and abs(m.neg_weight - 0.4) < 1e-12
    import pagnerf_amd
    assert "SupConLoss" in pagnerf_amd.__doc__


def test_supcon_loss_refuses_cpu_tensors_and_simclr():
    from pagnerf_amd.loss import SupConLoss
    x, lab = torch.randn(2, 8, 4), torch.zeros(2, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SupConLoss()(x, lab)
    with pytest.raises(NotImplementedError):
        SupConLoss()(x, None)


def test_supcon_entry_points_validate_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib
    lib = _lib.load()
    need = lib.pag_supcon_workspace_bytes(6, 4096, 200)
    assert need >= 6 * 4096 * 208 * 4 and lib.pag_supcon_workspace_bytes(1, 8, 513) == 0
    buf = ctypes.c_void_p(256)                     # never dereferenced: every call below must fail its checks first
    ok = (buf, 0, 2, 100, 16, 1600, 16, buf, None, 0.07, 0.07, 1.0, 1.0, buf, need, buf, None)

    def fwd(**kw):
        names = ["x", "dtype", "B", "P", "D", "img", "row", "lab", "mask", "T", "Tb", "pw", "nw", "ws", "nbytes", "loss", "st"]
        a = dict(zip(names, ok))
        a.update(kw)
        return lib.pag_supcon_fwd(*[a[n] for n in names])

    assert fwd(B=0) == -1 and b"sizes" in lib.pag_last_error_string()
    assert fwd(D=0) == -1 and fwd(D=513) == -1 and fwd(P=0) == -1
    assert fwd(row=8) == -1                                               # row_stride < D
    assert fwd(dtype=1) == -1 and b"dtype" in lib.pag_last_error_string()
    assert fwd(T=0.0) == -1 and fwd(Tb=-1.0) == -1
    assert fwd(x=None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert fwd(lab=None) == -1 and fwd(ws=None) == -1 and fwd(loss=None) == -1
    assert fwd(nbytes=64) == -1 and b"workspace" in lib.pag_last_error_string()
    assert lib.pag_supcon_bwd(0, 0, 100, 16, 0.07, 0.07, 1.0, 1.0, buf, need, buf, buf, None) == -1
    assert lib.pag_supcon_bwd(1, 2, 100, 16, 0.07, 0.07, 1.0, 1.0, buf, need, buf, buf, None) == -1 and b"dtype" in lib.pag_last_error_string()
    assert lib.pag_supcon_bwd(0, 2, 100, 16, 0.07, 0.07, 1.0, 1.0, buf, need, None, buf, None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert lib.pag_supcon_bwd(0, 2, 100, 16, 0.07, 0.07, 1.0, 1.0, buf, 64, buf, buf, None) == -1 and b"workspace" in lib.pag_last_error_string()


@pytest.mark.parametrize("name", [str(n) for n in golden("g11_supcon.npz")["names"]])
def test_restatement_reproduces_reference_golden(name):
    """The fp32 restatement above against the reference's fp32 values: value and gradient."""
    c = load_case(golden("g11_supcon.npz"), name)
    x = torch.from_numpy(c["x"]).requires_grad_(True)
    mask = torch.from_numpy(c["mask"]) if c["mask"] is not None else None
    out = restated(x, torch.from_numpy(c["labels"]), mask, c["T"], c["Tb"], c["pn"], c["reduction"])
    assert tuple(out.shape) == c["loss"].shape
    np.testing.assert_allclose(out.detach().numpy(), c["loss"], rtol=2e-5, atol=2e-5)
    backward_with(out, c["g"])
    ref = c["grad"]
    scale = np.abs(ref).max(-1, keepdims=True) + 1e-30
    assert np.all(np.abs(x.grad.numpy() - ref) <= 2e-4 * scale), name
    if mask is not None:
        assert not x.grad.numpy()[~c["mask"]].any()
