#!/usr/bin/env python3
"""Generate g15_semantic_nef.npz from the REFERENCE's pc_nerf/semantic_nerf.py (imported unmodified from the reference checkout) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_semantic.py

Third-party modules are the stand-ins of make_golden.install_stubs() plus: a skip-aware BasicDecoder (wisp's BasicDecoder(skip=[5]): layer 5 reads
cat([x, h]) - the column order is recalled from upstream), a plain BLASGrid and what grids/occtree.py imports (OctreeAS.init_dense,
kaolin.ops.spc.unbatched_get_level_points: the dense lattice of the level).  Weights are not stored: tests/test_semantic_nef_host.py draws them from a
seeded RandomState, and this maker imports that helper.  The fixture holds the inputs, the reference's three channels, seeded upstream gradients (the
density one zeroed where the reference's pre-activation density is within 0.02 of zero), the names and shapes of named_parameters() and the NOISE
FLOORS: per output and per parameter gradient, the largest rel-L2 distance over three weight seeds from the bf16-operand / fp32-accumulate restatement
to the same restatement accumulated in fp64 with the K axis permuted.  The GPU test allows three times that.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden as MG                                              # noqa: E402  (puts the repository and the reference on sys.path)
import test_semantic_nef_host as H                                    # noqa: E402
from oracle.decoders import bf16_operands                             # noqa: E402


class SkipBasicDecoder(nn.Module):
    def __init__(self, input_dim, output_dim, activation, bias, layer=nn.Linear, num_layers=1, hidden_dim=128, skip=[]):
        super().__init__()
        self.activation, self.skip = activation, list(skip)
        self.layers = nn.ModuleList([layer(input_dim if i == 0 else (hidden_dim + input_dim if i in self.skip else hidden_dim), hidden_dim, bias=bias)
                                     for i in range(num_layers)])
        self.lout = layer(hidden_dim, output_dim, bias=bias)

    def forward(self, x):
        h = x
        for i, l in enumerate(self.layers):
            if i in self.skip and i > 0:
                h = torch.cat([x, h], dim=-1)
            h = self.activation(l(h))
        return self.lout(h)


class BLASGrid(nn.Module):
    pass


class OctreeAS:
    def init_dense(self, level):
        R = 2 ** level
        ar = torch.arange(R, dtype=torch.int16)
        self.points = torch.stack(torch.meshgrid(ar, ar, ar, indexing="ij"), -1).reshape(-1, 3)
        self.octree, self.prefix, self.pyramid = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32)


def reference_class():
    MG.install_stubs()
    grids = sys.modules["wisp.models.grids"]
    grids.BasicDecoder, grids.BLASGrid = SkipBasicDecoder, BLASGrid
    MG._mod("wisp.ops.spc").sample_spc = None
    MG._mod("wisp.ops.grid")
    MG._mod("wisp.models.decoders").BasicDecoder = SkipBasicDecoder
    MG._mod("kaolin.ops")
    MG._mod("kaolin.ops.spc").unbatched_get_level_points = lambda points, pyramid, level: points
    MG._mod("wisp.accelstructs").OctreeAS = OctreeAS
    from pc_nerf.semantic_nerf import SemanticNeF
    return SemanticNeF


def main():
    Ref = reference_class()
    ref = Ref(num_classes=H.CLASSES, hidden_dim=H.HIDDEN, activation_type="relu", layer_type="none", blas_level=3)
    names = [n for n, _ in ref.named_parameters()]
    shapes = [tuple(p.shape) for _, p in ref.named_parameters()]
    assert list(zip(names, shapes)) == list(H.param_shapes().items())
    assert float(ref.decoder_density.bias[0]) == 1.0 and ref.get_supported_channels() == {"density", "rgb", "semantics"}
    w = H.make_weights()
    H.load_weights(ref, w)
    x, d = H.make_inputs()
    xt, dt = torch.from_numpy(x), torch.from_numpy(d)
    with torch.no_grad():
        gold = ref(channels={"density", "rgb", "semantics"}, coords=xt[:, None], ray_d=dt)
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    plain = H.restate(wt, xt, dt)
    for c in ("density", "rgb", "semantics"):
        assert tuple(gold[c].shape) == tuple(plain[c].shape), c
        np.testing.assert_allclose(plain[c].numpy(), gold[c].numpy(), rtol=1e-5, atol=1e-5, err_msg=c)
    # both ReLU sides in every layer, density positive on 20 - 95 % of the samples
    e = H.positional_embed(xt)
    h = e
    for i in range(8):
        if i == 5:
            h = torch.cat([e, h], -1)
        z = torch.nn.functional.linear(h, wt["decoder_features.layers.%d.weight" % i], wt["decoder_features.layers.%d.bias" % i])
        frac = float((z > 0).float().mean())
        assert 0.05 < frac < 0.95, (i, frac)
        h = torch.relu(z)
    pos = float((plain["density_pre"] > 0).float().mean())
    assert 0.20 <= pos <= 0.95, pos
    bf = H.restate(wt, xt, dt, operand_round=bf16_operands)
    for c in ("density", "rgb", "semantics"):
        np.testing.assert_allclose(bf[c].numpy(), gold[c].numpy(), rtol=1.5e-2, atol=1.5e-2, err_msg=c)
    up = H.make_upstream()
    near = np.abs(plain["density_pre"].numpy()) < 0.02
    assert near.mean() <= 0.10, near.mean()
    up["density"][near] = 0.0
    # noise floors over three weight seeds
    floors_out, floors_grad = {}, {}
    for seed in (H.SEED, H.SEED + 10, H.SEED + 20):
        ws = H.make_weights(seed)
        pre = H.restate({k: torch.from_numpy(v) for k, v in ws.items()}, xt, dt)["density_pre"].numpy()
        ups = {k: v.copy() for k, v in H.make_upstream(seed).items()}
        ups["density"][np.abs(pre) < 0.02] = 0.0
        o32, g32 = H.restate_grads(ws, x, d, ups, operand_round=bf16_operands, round_grads=True)
        o64, g64 = H.restate_grads(ws, x, d, ups, operand_round=bf16_operands, round_grads=True, dt=torch.float64, perm=True)
        for c in ("feats", "density", "rgb", "semantics"):
            floors_out[c] = max(floors_out.get(c, 0.0), H.rel_l2(o32[c], o64[c]))
        for k in g32:
            floors_grad[k] = max(floors_grad.get(k, 0.0), H.rel_l2(g32[k], g64[k]))
        print("seed %d floors: feats %.2e density %.2e rgb %.2e sem %.2e | grad min %.2e max %.2e" % (
            seed, floors_out["feats"], floors_out["density"], floors_out["rgb"], floors_out["semantics"], min(floors_grad.values()), max(floors_grad.values())))
    o32, g32 = H.restate_grads(w, x, d, up, operand_round=bf16_operands, round_grads=True)
    _, gfp = H.restate_grads(w, x, d, up)
    print("bf16-operand restatement vs fp32: outputs", {c: "%.2e" % H.rel_l2(o32[c], plain[c].numpy()) for c in ("feats", "density", "rgb", "semantics")})
    print("                                  grads  min %.2e max %.2e" % (min(H.rel_l2(g32[k], gfp[k]) for k in g32), max(H.rel_l2(g32[k], gfp[k]) for k in g32)))
    out = {"coords": x, "dirs": d}
    for c in ("density", "rgb", "semantics"):
        out[c] = gold[c].numpy()
        out["up_" + c] = up[c]
        out["floor_" + c] = np.float64(floors_out[c])
    out["floor_feats"] = np.float64(floors_out["feats"])
    out["param_names"] = np.array(names)
    out["param_shapes"] = np.array([list(s) + [-1] * (2 - len(s)) for s in shapes], dtype=np.int64)
    gnames = sorted(floors_grad)
    out["grad_names"] = np.array(gnames)
    out["grad_floors"] = np.array([floors_grad[k] for k in gnames], dtype=np.float64)
    path = os.path.join(HERE, "g15_semantic_nef.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 400_000


if __name__ == "__main__":
    main()
