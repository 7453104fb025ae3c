#!/usr/bin/env python3
"""Generate g15b_semantic_regimes.npz: the noise floors of the launch-regime cases of tests/test_gpu_semantic_nef_regimes.py.  CPU only; reads nothing
but this repository.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_semantic_regimes.py

The method of make_golden_semantic.py: per case (tests/test_semantic_nef_host.py::REGIME_CASES) and per weight seed SEED, SEED + 10, SEED + 20, the
rel-L2 distance from the bf16-operand / fp32-accumulate restatement to the same restatement accumulated in fp64 with the summation axes permuted, per
output channel and per parameter gradient; the largest over the seeds is stored.  The density upstream is zeroed where the plain fp32 restatement's
|density_pre| < 0.02.  Only floors are stored: weights, inputs and upstream gradients are drawn from the seeds by the test as they are here.  The
GPU test allows three times the floor (+ 1e-6 on gradients).
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_semantic_nef_host as H                                    # noqa: E402
from oracle.decoders import bf16_operands                             # noqa: E402

OUT = ("feats",) + H.CHANNELS


def case_floors(key):
    floors_out, floors_grad = {}, {}
    for seed in (H.SEED, H.SEED + 10, H.SEED + 20):
        w, x, d, up, plain = H.regime_case(key, seed)
        if seed == H.SEED:                                        # the conditions make_golden_semantic.py asserts on the inputs the test runs
            near, pos = float((np.abs(plain["density_pre"]) < H.NEAR_ZERO).mean()), float((plain["density_pre"] > 0).mean())
            print("%-15s M %6d C %2d: near-zero density share %.3f, positive share %.3f" % ((key,) + H.REGIME_CASES[key][:2] + (near, pos)))
            assert near <= 0.10, (key, near)
            assert 0.20 <= pos <= 0.95, (key, pos)
        o32, g32 = H.restate_grads(w, x, d, up, operand_round=bf16_operands, round_grads=True)
        o64, g64 = H.restate_grads(w, x, d, up, operand_round=bf16_operands, round_grads=True, dt=torch.float64, perm=True)
        for c in OUT:
            floors_out[c] = max(floors_out.get(c, 0.0), H.rel_l2(o32[c], o64[c]))
        for k in g32:
            floors_grad[k] = max(floors_grad.get(k, 0.0), H.rel_l2(g32[k], g64[k]))
        print("    seed %d floors: feats %.2e density %.2e rgb %.2e sem %.2e | grad min %.2e max %.2e" % (
            seed, floors_out["feats"], floors_out["density"], floors_out["rgb"], floors_out["semantics"], min(floors_grad.values()),
            max(floors_grad.values())))
    return floors_out, floors_grad


def main():
    out = {"cases": np.array(sorted(H.REGIME_CASES))}
    for key, (M, C, _) in H.REGIME_CASES.items():
        fo, fg = case_floors(key)
        names = sorted(fg)
        assert names == sorted(n for n in H.param_shapes(classes=C) if not n.endswith("bands"))
        out[key + "_M"], out[key + "_C"] = np.int64(M), np.int64(C)
        for c in OUT:
            out[key + "_floor_" + c] = np.float64(fo[c])
        out[key + "_grad_names"] = np.array(names)
        out[key + "_grad_floors"] = np.array([fg[k] for k in names], dtype=np.float64)
        for n in ("decoder_density.bias", "decoder_density.weight", "decoder_semantics.lout.bias", "decoder_features.layers.0.weight"):
            print("    %-36s %.3e" % (n, fg[n]))
    path = os.path.join(HERE, "g15b_semantic_regimes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 64_000


if __name__ == "__main__":
    main()
