#!/usr/bin/env python3
"""Generate g14_map.npz from the REFERENCE's utils/render_map.py and utils/outlier_rejection.py (imported unmodified from the reference checkout) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_map.py

Third-party modules the two files import are replaced by stand-ins: wisp.ops.raygen (the "generated" rays are the case's base rays), wisp.core.Rays,
kaolin.render.camera (Camera / CameraExtrinsics / PinholeIntrinsics; extrinsics.inv_transform_rays(o, d) = (R^T (o - t), R^T d)); Tensor.cuda keeps
tensors on the CPU.  The pipeline stand-in returns the case's seeded buffers chunk by chunk and the nef stand-in seeded density / instance rows
(tests/test_map_export_host.py generates both), which pins everything after the render: masks, argmax, unprojection, order, the `+=` chunk join, the
limits box, the noise shift and both compactions.  The fixture holds the small inputs, base rays, view matrices and the reference's outputs; instance
rows and colours are regenerated from the seeds by the tests.  The maker asserts the cases' conditions and that the numpy restatement of the host
test reproduces every case.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PAGNERF_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_map_export_host as H                                     # noqa: E402


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod


class Rays:
    def __init__(self, origins, dirs):
        self.origins, self.dirs = origins, dirs

    @classmethod
    def stack(cls, rays):
        return cls(torch.stack([r.origins for r in rays]), torch.stack([r.dirs for r in rays]))

    def reshape(self, *dims):
        return Rays(self.origins.reshape(*dims), self.dirs.reshape(*dims))


class Intrinsics:
    def __init__(self, width, height, params=None, near=0.0, far=6.0):
        self.width, self.height, self.near, self.far = width, height, near, far
        self._params = torch.tensor([[1.0, 1.0, float(width), float(width)]]) if params is None else params

    def parameters(self):
        return self._params


class Extrinsics:
    def __init__(self, view):
        self.R, self.t = view[:, :3, :3], view[:, :3, 3]

    @classmethod
    def from_view_matrix(cls, view):
        return cls(view.reshape(-1, 4, 4))

    def inv_transform_rays(self, o, d):
        return torch.matmul(o - self.t[:, None, :], self.R), torch.matmul(d, self.R)      # row-vector form of R^T (o - t), R^T d


class Camera:
    def __init__(self, extrinsics, intrinsics):
        self.extrinsics, self.intrinsics = extrinsics, intrinsics

    def __len__(self):
        return self.extrinsics.R.shape[0]

    def to(self, *a, **k):
        return self


class Buffers:
    """RenderBuffer stand-in: named [n, ...] channels, `+=` concatenates along the ray axis."""

    def __init__(self, **ch):
        self.__dict__.update(ch)

    def __iadd__(self, other):
        for k, v in other.__dict__.items():
            self.__dict__[k] = torch.cat([self.__dict__[k], v], 0)
        return self


class Packs:
    def __init__(self, n):
        self.n = n

    def split(self, size):
        return [(s, min(s + size, self.n)) for s in range(0, self.n, size)]


class ViewsPipeline:
    def __init__(self, name, base):
        c = H.VIEWS_CASES[name]
        self.data = {k: torch.from_numpy(v) for k, v in H.views_inputs(name).items()}
        self.cameras = Camera(Extrinsics(self.data["view"]), Intrinsics(c["w"], c["h"]))
        self.cam_id_to_idx = {"cam%d" % i: i for i in range(c["cams"])}
        self.base, self.chunks = base, []

    def transform_rays(self, base_rays, cam_ids):
        assert base_rays.origins.shape == (len(cam_ids),) + tuple(self.base.origins.shape)
        return Packs(base_rays.origins.shape[0] * base_rays.origins.shape[1])

    def __call__(self, rays, lod_idx, channels):
        s, e = rays
        assert channels == ["depth", "density", "rgb", "inst_embedding"]
        self.chunks.append((s, e))
        return Buffers(**{k: self.data[k][s:e] for k in ("depth", "density", "rgb", "inst_embedding", "alpha", "hit")})


class DenseNef:
    def __init__(self, name):
        c = H.DENSE_CASES[name]
        self.I = c["I"]
        self.rs_density, self.rs_inst = np.random.RandomState(c["seed"]), np.random.RandomState(c["seed"] + 100)
        self.queried = []

    def __call__(self, coords, ray_d, channels):
        n = coords.shape[0]
        assert coords.shape[1:] == (1, 3) and ray_d is None
        if channels == ["density"]:
            self.queried.append(coords[:, 0].clone())
            return [torch.from_numpy(H.dense_density(self.rs_density, n)).reshape(n, 1, 1)]
        assert channels == ["inst_embedding"]
        return [torch.from_numpy(H.dense_inst(self.rs_inst, n, self.I))]


def reference_module(current):
    for name in ("kaolin", "kaolin.render", "wisp", "wisp.ops"):
        _stub(name)
    _stub("kaolin.render.camera", Camera=Camera, CameraExtrinsics=Extrinsics, PinholeIntrinsics=Intrinsics)
    _stub("wisp.core", Rays=Rays)
    _stub("wisp.ops.raygen", generate_centered_pixel_coords=lambda *a, **k: None, generate_pinhole_rays=lambda cam, grid: current["base"])
    torch.Tensor.cuda = lambda self, *a, **k: self
    from utils import render_map
    return render_map


def main():
    current = {}
    M = reference_module(current)
    out = {}
    for name, c in H.VIEWS_CASES.items():
        bo, bd = H.base_rays_np(c["h"], c["w"])
        current["base"] = Rays(torch.from_numpy(bo), torch.from_numpy(bd))
        pipe = ViewsPipeline(name, current["base"])
        res = M.generate_pc_map_from_views(pipe, name="nerf_pc", channels=["inst_embedding"], mip=0)[0]
        assert res["name"] == "nerf_pc" and pipe.chunks[0][1] == min(H.RENDER_BATCH, pipe.chunks[-1][1])
        d = H.views_inputs(name)
        kept, pts, ids, col = H.np_views(d, bo, bd, **H.THRESHOLDS)
        assert np.array_equal(ids, res["inst_embedding"].numpy()) and col.tobytes() == res["color"].numpy().tobytes(), name
        np.testing.assert_allclose(pts, res["points"].numpy(), rtol=1e-5, atol=1e-6)
        if name != "none_kept":
            assert 0.05 < kept.size / d["hit"].size < 0.5, name
            terms = H.np_views_mask(d, **H.THRESHOLDS)
            for i in range(5):
                assert (np.logical_and.reduce([t for j, t in enumerate(terms) if j != i]) & ~terms[i]).any(), (name, i)
        for k in ("density", "alpha", "depth", "hit", "view"):
            out[name + "/" + k] = d[k]
        out[name + "/base_origins"], out[name + "/base_dirs"] = bo, bd
        out[name + "/kept"] = kept
        out[name + "/points"] = res["points"].numpy()
        out[name + "/inst_embedding"] = res["inst_embedding"].numpy()
        out[name + "/color"] = res["color"].numpy()
        print("views %-22s rays %6d chunks %d kept %d" % (name, d["hit"].size, len(pipe.chunks), kept.size))
    real_rand = torch.rand
    for name, c in H.DENSE_CASES.items():
        limits = torch.tensor(c["limits"], dtype=torch.float32) if c["limits"] is not None else torch.zeros(0)
        drawn = []

        def rand(*a, **k):
            drawn.append(real_rand(*a, **k))
            return drawn[-1]
        torch.manual_seed(c["seed"])
        torch.rand = rand
        try:
            nef = DenseNef(name)
            occ = M.get_dense_occupied_points(nef, c["level"], c["min_density"], limits)
            noise = drawn[0].clone()
            nef2 = DenseNef(name)
            res = M.generate_pc_map(nef2, c["level"], name="nerf_pc", min_density=c["min_density"], limits=limits, channels=["inst_embedding"])[0]
        finally:
            torch.rand = real_rand
        P, my_occ, my_pts, my_ids = H.np_dense(name)
        lattice = H.np_lattice(c["level"], c["limits"])
        res_n = np.float32(2.0 ** c["level"])
        samples = torch.cat(nef.queried).numpy()                                          # the density was queried at points + (rand / res * 2 - 1)
        assert samples.tobytes() == (lattice + (noise.numpy() / res_n * np.float32(2.0) - np.float32(1.0))).astype(np.float32).tobytes(), name
        assert noise.shape == (P, 3) and my_occ.tobytes() == occ.numpy().tobytes() and my_pts.tobytes() == res["points"].numpy().tobytes(), name
        assert np.array_equal(my_ids, res["instances"].numpy()) and res["name"] == "nerf_pc", name
        out[name + "/lattice_size"] = np.int64(P)
        out[name + "/noise"] = noise.numpy()
        out[name + "/occupied"] = occ.numpy()
        out[name + "/points"] = res["points"].numpy()
        out[name + "/instances"] = res["instances"].numpy()
        print("dense %-26s lattice %6d occupied %6d map %6d" % (name, P, occ.shape[0], res["points"].shape[0]))
    path = os.path.join(HERE, "g14_map.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
