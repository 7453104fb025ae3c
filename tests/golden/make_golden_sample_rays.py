#!/usr/bin/env python3
"""Generate g18_sample_rays.npz by running the REFERENCE's datasets/transforms/ray_sampler.py::SampleRays (loaded unmodified from the reference checkout
by file path; it needs only torch) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sample_rays.py

Two calls under torch.manual_seed(SEED): the single-image mode (every mode [35, C], num_samples 8) and the batch mode (every mode [3, 35, C],
num_samples 12 -> 4 rays per image).  `rays` is a stand-in for wisp's Rays (origins / dirs, .shape, indexing, .contiguous()), as the g15 / g16 makers
use stand-ins for the third-party classes.  Channel 0 of `imgs` holds the pixel index, so the reference's random choice can be read back from its output.
Saved: the inputs (`<mode>_in_<key>`), the reference's outputs (`<mode>_out_<key>`, the two fields of rays as `rays.origins` / `rays.dirs`), the
input and output key lists.  The excluded keys (cameras, cameras_ts, filenames) are part of the inputs' key list only.
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PAGNERF_REFERENCE", "/root/reference")
SEED, N, SINGLE_K, BATCH, BATCH_SAMPLES = 18, 35, 8, 3, 12


class Rays:
    """Stand-in for wisp.core.Rays: what SampleRays touches."""

    def __init__(self, origins, dirs):
        self.origins, self.dirs = origins, dirs

    @property
    def shape(self):
        return self.origins.shape[:-1]

    def __getitem__(self, idx):
        return Rays(self.origins[idx], self.dirs[idx])

    def contiguous(self):
        return Rays(self.origins.contiguous(), self.dirs.contiguous())


def inputs(lead, gen):
    """Every mode of a BUP20 item with the leading axes `lead` = (35,) or (3, 35); imgs[..., 0] = the pixel index."""
    rnd = lambda *c: torch.rand(*lead, *c, generator=gen)
    imgs = rnd(4)
    imgs[..., 0] = torch.arange(lead[-1], dtype=torch.float32).expand(*lead)
    return {"imgs": imgs,
            "semantics": torch.randint(0, 6, (*lead, 1), generator=gen),
            "instance": torch.randint(0, 200, (*lead, 1), generator=gen),
            "sem_conf": rnd(1), "inst_conf": rnd(1).half(),
            "masks": torch.rand(*lead, 1, generator=gen) > 0.5,
            "depths": rnd(1).double(),
            "rays": Rays(rnd(3), rnd(3)),
            "cameras": "not indexable", "cameras_ts": 7, "filenames": "frame_0007"}


def main():
    spec = importlib.util.spec_from_file_location("ref_ray_sampler", os.path.join(REF, "datasets", "transforms", "ray_sampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gen = torch.Generator().manual_seed(SEED)
    save = {"meta": np.array([SEED, N, SINGLE_K, BATCH, BATCH_SAMPLES], np.int64)}
    for tag, lead, k in (("single", (N,), SINGLE_K), ("batch", (BATCH, N), BATCH_SAMPLES)):
        data = inputs(lead, gen)
        torch.manual_seed(SEED)
        out = mod.SampleRays(k)(data)
        save[tag + "_in_keys"] = np.array(list(data))
        save[tag + "_out_keys"] = np.array(list(out))
        for kind, d in (("in", data), ("out", out)):
            for key, v in d.items():
                if isinstance(v, Rays):
                    save["%s_%s_%s.origins" % (tag, kind, key)] = v.origins.numpy()
                    save["%s_%s_%s.dirs" % (tag, kind, key)] = v.dirs.numpy()
                elif isinstance(v, torch.Tensor):
                    save["%s_%s_%s" % (tag, kind, key)] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "g18_sample_rays.npz"), **save)


if __name__ == "__main__":
    main()
