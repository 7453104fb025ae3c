#!/usr/bin/env python3
"""Generate g11_supcon.npz by running the REFERENCE's loss/sup_contrastive.py::SupConLoss (imported unmodified from the reference checkout) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_supcon.py

The fixture holds, per case, the inputs that are not regenerated (labels, anchor masks, the upstream gradient, the rows zeroed after generation), the
reference's fp32 value(s) of the loss and its autograd gradient with respect to the features.  The features themselves are regenerated from the seed
stored with each case by `case_features` (tests/test_supcon_host.py has the same function).

Cases: D in {6 (the semantic call's softmax probabilities + 1e-27), 16, 200}; P not a multiple of 64; pn_ratio 0.5 / 0.3 / 0.8; base_temperature !=
temperature; the three reductions with and without anchor_mask; an image without anchors, an image whose anchors all share one label, labels held by a
single ray (rows without positives) and all-zero feature rows.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PAGNERF_REFERENCE", "/root/reference")
sys.path.insert(0, REF)


def case_features(seed, B, P, D, kind):
    """float32 [B, P, D]: standard normal, or ("probs") softmax(2 z) computed in float64 plus float32(1e-27) - the semantic call's input."""
    z = np.random.RandomState(seed).standard_normal(size=(B, P, D))
    if kind == "probs":
        e = np.exp(2.0 * z - (2.0 * z).max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True)).astype(np.float32) + np.float32(1e-27)
    return z.astype(np.float32)


# name, seed, B, P, D, kind, temperature, base_temperature, pn_ratio, reduction, masked
CASES = [
    ("sem_mean", 1100, 2, 100, 6, "probs", 0.07, 0.07, 0.5, "mean", False),
    ("sem_none", 1101, 2, 100, 6, "probs", 0.07, 0.07, 0.3, "none", False),
    ("inst16_mean", 1102, 3, 200, 16, "normal", 0.07, 0.07, 0.5, "mean", True),
    ("inst16_sum", 1103, 3, 200, 16, "normal", 0.1, 0.07, 0.8, "sum", True),
    ("inst16_none", 1104, 3, 200, 16, "normal", 0.07, 0.07, 0.3, "none", True),
    ("flat16_sum", 1105, 2, 150, 16, "normal", 0.07, 0.1, 0.8, "sum", False),
    ("inst200_mean", 1106, 2, 130, 200, "normal", 0.07, 0.07, 0.3, "mean", True),
    ("flat200_none", 1107, 2, 130, 200, "normal", 0.07, 0.05, 0.8, "none", False),
]


def make_case(rs, B, P, D, kind, masked):
    """labels, anchor mask and the rows to zero.  Masked cases: image 0 has ~30 % of its rays masked out, a few singleton labels and an all-zero row;
    image 1 has no anchors; image 2 (when there is one) has anchors that all share one label."""
    if kind == "probs":
        labels = rs.randint(0, D, size=(B, P)).astype(np.int64)
    else:
        labels = rs.choice([0, 3, 4, 17, 1005, 1 << 40], size=(B, P)).astype(np.int64)
        labels[0, :3] = [7001, 7002, 7003]                        # labels of one ray: rows without positives
    mask = np.ones((B, P), dtype=bool)
    zero_rows = [(0, 5)]
    if masked:
        mask[0] = rs.uniform(size=P) > 0.3
        mask[0, :6] = True
        if B > 1:
            mask[1] = False                                       # no anchors
        if B > 2:
            mask[2] = labels[2] == 4                              # one label among the anchors
    else:
        zero_rows.append((B - 1, P - 1))
    return labels, mask, np.array(zero_rows, dtype=np.int64)


def main():
    from loss.sup_contrastive import SupConLoss
    save = {"names": np.array([c[0] for c in CASES])}
    for name, seed, B, P, D, kind, T, Tb, pn, red, masked in CASES:
        rs = np.random.RandomState(seed + 1)
        labels, mask, zero_rows = make_case(rs, B, P, D, kind, masked)
        x = case_features(seed, B, P, D, kind)
        for b, p in zero_rows:
            x[b, p] = 0.0
        g = rs.standard_normal(size=(B, P)).astype(np.float32) if red == "none" else np.float32(rs.uniform(0.5, 2.0))
        xt = torch.from_numpy(x).requires_grad_(True)
        fn = SupConLoss(temperature=T, base_temperature=Tb, pn_ratio=pn)
        out = fn(xt, torch.from_numpy(labels), reduction=red, anchor_mask=torch.from_numpy(mask) if masked else None)
        if isinstance(out, list):                                 # 'none' with anchor_mask: per image [1, |S_b|] or a 0-d zero
            loss = np.zeros((B, P), np.float32)
            total = 0
            for b, o in enumerate(out):
                if o.dim() == 2:
                    loss[b, mask[b]] = o.detach().numpy()[0]
                    total = total + (o[0] * torch.from_numpy(g[b][mask[b]])).sum()
            total.backward()
        elif red == "none":
            loss = out.detach().numpy()
            (out * torch.from_numpy(g)).sum().backward()
        else:
            loss = out.detach().numpy().astype(np.float32)
            (out * float(g)).sum().backward()
        meta = np.array([seed, B, P, D, 1 if kind == "probs" else 0, 1 if masked else 0], np.int64)
        save.update({f"{name}_meta": meta, f"{name}_params": np.array([T, Tb, pn], np.float64), f"{name}_reduction": np.array(red),
                     f"{name}_labels": labels, f"{name}_mask": mask, f"{name}_zero_rows": zero_rows, f"{name}_g": np.asarray(g, np.float32),
                     f"{name}_loss": loss, f"{name}_grad": xt.grad.numpy()})
    np.savez_compressed(os.path.join(HERE, "g11_supcon.npz"), **save)


if __name__ == "__main__":
    main()
