#!/usr/bin/env python3
"""Generate g16_panoptic_lifting.npz from the REFERENCE's pc_nerf/panoptic_lifting.py and grids/tensorf.py (imported unmodified from the reference
checkout) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_panoptic_lifting.py

Third-party modules are the stand-ins of make_golden.install_stubs() plus those make_golden_semantic.reference_class() adds; the reference class also
gets a no-op init_embedder (the stand-in BaseNeuralField calls one).  The grid is shrunk by constructing the reference's TensoRF with small arguments
(resolutions 16, 19, .. 28: an odd step), not by editing it.  Weights are not stored: tests/test_panoptic_lifting_host.py draws them from a seeded
RandomState, and this maker imports that helper.  The fixture holds the inputs, the reference's four channels and sigma_feature, seeded upstream
gradients (the density one zeroed where |sigma_feature| < 1e-4, next to the blocks make_upstream zeroes), every parameter's gradient from the
reference's autograd, the names and shapes of named_parameters(), one plane and one line after step_upsample_vm_grid(), and the NOISE FLOORS: per
output and per parameter gradient, the largest rel-L2 distance over three weight seeds between the reference run in fp32 and the same run in fp64.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden as MG                                              # noqa: E402,F401  (puts the repository and the reference on sys.path)
import make_golden_semantic as MS                                     # noqa: E402
import test_panoptic_lifting_host as H                                # noqa: E402


def reference_classes():
    MS.reference_class()
    from grids.tensorf import TensoRF
    from pc_nerf.panoptic_lifting import PanopticLiftingNeF
    PanopticLiftingNeF.init_embedder = lambda self: None
    return PanopticLiftingNeF, TensoRF


def build(Ref, Grid, w, dtype=torch.float32):
    ref = Ref(**H.NEF_KW)
    ref.grid = Grid(**H.GRID_KW)
    ref = ref.to(dtype)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            p.copy_(torch.from_numpy(w[n]).to(dtype))
    return ref


def run(ref, x, d, up, dtype=torch.float32):
    """-> outputs (numpy, with sigma_feature), parameter gradients (numpy)."""
    xt, dt = torch.from_numpy(x).to(dtype), torch.from_numpy(d).to(dtype)
    ref.zero_grad()
    out = ref(channels=set(H.CHANNELS), coords=xt[:, None], ray_d=dt)
    with torch.no_grad():
        sigma = ref.grid.interpolate(xt[:, None], 0)[0].reshape(-1)
    res = {c: out[c].detach().numpy() for c in H.CHANNELS}
    res["sigma_feature"] = sigma.numpy()
    grads = None
    if up is not None:
        sum((out[c] * torch.from_numpy(up[c]).to(dtype)).sum() for c in H.CHANNELS).backward()
        grads = {n: p.grad.detach().numpy() for n, p in ref.named_parameters()}
    return res, grads


def upstream_for(Ref, Grid, w, x, d, seed):
    up = H.make_upstream(seed)
    sigma = run(build(Ref, Grid, w), x, d, None)[0]["sigma_feature"]
    near = np.abs(sigma) < H.ZERO_EPS
    assert near.mean() <= 0.02, near.mean()
    up["density"][near] = 0.0
    return up


def main():
    Ref, Grid = reference_classes()
    x, d = H.make_inputs()
    w = H.make_weights()
    ref = build(Ref, Grid, w)
    names = [n for n, _ in ref.named_parameters()]
    shapes = [tuple(p.shape) for _, p in ref.named_parameters()]
    assert list(zip(names, shapes)) == list(H.param_shapes().items()), list(zip(names, shapes))
    assert ref.get_supported_channels() == set(H.CHANNELS) and ref.grid.resolutions == H.RESOLUTIONS
    up = upstream_for(Ref, Grid, w, x, d, H.SEED)
    gold, grads = run(ref, x, d, up)
    shapes_out = {c: tuple(gold[c].shape) for c in H.CHANNELS}
    assert shapes_out == {"density": (H.N_GOLD, 1, 1), "rgb": (H.N_GOLD, 3), "semantics": (H.N_GOLD, 1, H.CLASSES),
                          "inst_embedding": (H.N_GOLD, 1, H.INSTANCES)}, shapes_out
    pos = float((gold["density"] > 0).mean())
    assert 0.2 <= pos <= 0.8, pos
    # the numpy restatement of the host tests agrees with the reference's grid
    np.testing.assert_allclose(H.np_vm_sigma(w, x), gold["sigma_feature"], rtol=1e-5, atol=2e-6)
    # noise floors: fp32 against fp64, the largest over three weight seeds
    floors_out, floors_grad = {}, {}
    for seed in (H.SEED, H.SEED + 10, H.SEED + 20):
        ws = H.make_weights(seed)
        ups = upstream_for(Ref, Grid, ws, x, d, seed)
        o32, g32 = run(build(Ref, Grid, ws), x, d, ups)
        o64, g64 = run(build(Ref, Grid, ws, torch.float64), x, d, ups, torch.float64)
        worst = 0.0
        for c in H.CHANNELS:
            floors_out[c] = max(floors_out.get(c, 0.0), H.rel_l2(o32[c], o64[c]))
            assert np.allclose(o32[c], o64[c], rtol=1e-5, atol=2e-6), c
        for k in g32:
            floors_grad[k] = max(floors_grad.get(k, 0.0), H.rel_l2(g32[k], g64[k]))
            worst = max(worst, float(np.abs(g32[k] - g64[k]).max()))
            assert np.allclose(g32[k], g64[k], rtol=2e-4, atol=2e-5), k
        print("seed %d floors: %s | grad min %.2e max %.2e (max |diff| %.2e)" % (
            seed, {c: "%.2e" % floors_out[c] for c in H.CHANNELS}, min(floors_grad.values()), max(floors_grad.values()), worst))
    for k in sorted(floors_grad):
        print("  floor %-42s %.2e" % (k, floors_grad[k]))
    ref.grid.step_upsample_vm_grid()
    assert ref.grid.current_resolution == H.RESOLUTIONS[1]
    out = {"coords": x, "dirs": d, "sigma_feature": gold["sigma_feature"]}
    for c in H.CHANNELS:
        out[c] = gold[c]
        out["up_" + c] = up[c]
        out["floor_" + c] = np.float64(floors_out[c])
    out["param_names"] = np.array(names)
    out["param_shapes"] = np.array([list(s) + [-1] * (4 - len(s)) for s in shapes], dtype=np.int64)
    out["grad_names"] = np.array(names)
    out["grad_floors"] = np.array([floors_grad[k] for k in names], dtype=np.float64)
    for k in names:
        out["grad_" + k] = grads[k]
    out["upsampled_density_plane_0"] = ref.grid.features.density_plane[0].detach().numpy()
    out["upsampled_app_line_1"] = ref.grid.features.app_line[1].detach().numpy()
    path = os.path.join(HERE, "g16_panoptic_lifting.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
