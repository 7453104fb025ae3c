#!/usr/bin/env python3
"""Generate g17_tv.npz by running the REFERENCE's loss/regularizers.py (imported unmodified from the reference checkout; it needs only torch) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tv.py

tv_l1_loss / tv_l2_loss: for every case of tests/tv_cases.py the reference's value (`<name>_l1`, `<name>_l2`), and for GRAD_CASES its autograd gradient
(`<name>_l1_grad`, `<name>_l2_grad`).  The inputs are regenerated from the seeds by tv_cases.case_values; half cases hand the reference the rounded values
as fp32, which is how this project defines the term for half inputs.
grid_tv_l1_loss / grid_tv_l2_loss: the fixed analytic encoder of tv_cases.grid_encoder, n = 4, device 'cpu', torch.manual_seed(GRID_SEED) before each call:
the coordinates the encoder received (`grid_coords`, the same for both) and the two losses.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PAGNERF_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

import tv_cases as TC


def main():
    from loss import regularizers as R
    save = {"names": np.array([c[0] for c in TC.CASES]), "grad_names": np.array(TC.GRAD_CASES)}
    for name, seed, shape, dtype in TC.CASES:
        for tag, fn in (("l1", R.tv_l1_loss), ("l2", R.tv_l2_loss)):
            x = TC.case(name).float().requires_grad_(True)
            out = fn(x)
            save["%s_%s" % (name, tag)] = np.float32(out.detach().numpy())
            if name in TC.GRAD_CASES:
                out.backward()
                save["%s_%s_grad" % (name, tag)] = x.grad.numpy()
    for tag, fn in (("l1", R.grid_tv_l1_loss), ("l2", R.grid_tv_l2_loss)):
        seen = []
        torch.manual_seed(TC.GRID_SEED)
        out = fn(TC.grid_encoder(seen), sample_size=TC.GRID_SAMPLE_SIZE, num_dim_samples=TC.GRID_N, device="cpu")
        assert len(seen) == 1
        if "grid_coords" in save:
            assert np.array_equal(save["grid_coords"], seen[0].numpy())
        save["grid_coords"] = seen[0].numpy()
        save["grid_%s" % tag] = np.float32(out.detach().numpy())
    save["grid_meta"] = np.array([TC.GRID_SEED, TC.GRID_N], np.int64)
    save["grid_sample_size"] = np.float64(TC.GRID_SAMPLE_SIZE)
    np.savez_compressed(os.path.join(HERE, "g17_tv.npz"), **save)


if __name__ == "__main__":
    main()
