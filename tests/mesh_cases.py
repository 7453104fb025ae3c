"""The surface-nets cases shared by tests/test_mesh_host.py and tests/test_gpu_mesh.py: small analytic fields (the largest 33^3), built once.
case(name) -> (field f32 [nx,ny,nz] CPU tensor, iso, lo, h); reference(name) -> surface_nets_reference's result of the case, computed once, shared and
never written to."""
import numpy as np
import torch

CENTRE = (0.03, -0.05, 0.02)
SPHERE_VOLUME = 4.0 / 3.0 * np.pi * 0.6 ** 3
TORUS_VOLUME = 2.0 * np.pi ** 2 * 0.55 * 0.25 ** 2
NONFINITE_POINTS = {(13, 8, 8): float("nan"), (8, 3, 8): float("inf"), (8, 8, 13): float("-inf")}      # next to sphere17's surface, far from each other

CASES = ("sphere17", "sphere33", "torus17", "torus33", "odd_box", "plane", "one_point", "border", "equal_iso", "nonfinite", "noise", "empty", "full",
         "sphere33_crop")
CROP = ((5, 30), (2, 25), (9, 33))                         # sphere33_crop: the index sub-box [lo, hi) per axis; index0 is its lo corner

_CASES, _REFERENCES = {}, {}


def _grid(shape, d):
    """Lattice coordinates i / d * 2 - 1 per axis (float64; spacing h = 2 / d) -> x, y, z [nx,ny,nz]."""
    return np.meshgrid(*[np.arange(n, dtype=np.float64) / d * 2.0 - 1.0 for n in shape], indexing="ij")


def _sphere(shape, d, centre=CENTRE, radius=0.6):
    x, y, z = _grid(shape, d)
    return radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)


def _torus(n):
    x, y, z = _grid((n, n, n), n - 1)
    return 0.25 - np.sqrt((np.sqrt((x - 0.01) ** 2 + (y + 0.02) ** 2) - 0.55) ** 2 + (z - 0.03) ** 2)


def _build(name):
    if name in ("sphere17", "sphere33"):
        n = int(name[6:])
        return _sphere((n, n, n), n - 1), 0.0, -1.0, 2.0 / (n - 1)
    if name in ("torus17", "torus33"):
        n = int(name[5:])
        return _torus(n), 0.0, -1.0, 2.0 / (n - 1)
    if name == "odd_box":                                  # 4896 cells, 17 442 edge rows: no multiple of 64 or 256; nx, ny, nz all different
        return _sphere((18, 17, 19), 16), 0.0, -1.0, 2.0 / 16
    if name == "plane":
        return np.broadcast_to(3.0 - np.arange(6, dtype=np.float64)[:, None, None], (6, 5, 7)).copy(), 0.5, -1.0, 0.25
    if name == "one_point":
        f = np.zeros((5, 5, 5))
        f[2, 2, 2] = 1.0
        return f, 0.5, -1.0, 0.5
    if name == "border":                                   # the surface leaves the lattice: an open mesh
        return _sphere((9, 9, 9), 8, centre=(-1.0, -1.0, -1.0), radius=0.9), 0.0, -1.0, 0.25
    if name == "equal_iso":                                # values equal to iso count as inside
        return np.random.default_rng(5).integers(0, 3, (7, 8, 6)).astype(np.float64), 1.0, -1.0, 0.25
    if name == "nonfinite":
        f = _sphere((17, 17, 17), 16)
        for p, v in NONFINITE_POINTS.items():
            f[p] = v
        return f, 0.0, -1.0, 2.0 / 16
    if name == "noise":                                    # seed 13: all 256 sign configurations of a cell, the non-manifold ones included
        return np.random.default_rng(13).uniform(-1.0, 1.0, (12, 11, 13)), 0.0, -1.0, 0.2
    if name in ("empty", "full"):
        return np.full((5, 4, 6), -1.0 if name == "empty" else 1.0), 0.0, -1.0, 0.5
    if name == "sphere33_crop":
        f, iso, lo, h = _build("sphere33")
        return f[tuple(slice(a, b) for a, b in CROP)], iso, lo, h
    raise KeyError(name)


def case(name):
    if name not in _CASES:
        f, iso, lo, h = _build(name)
        _CASES[name] = (torch.from_numpy(np.ascontiguousarray(f).astype(np.float32)), iso, lo, h)
    return _CASES[name]


def index0(name):
    return tuple(a for a, _ in CROP) if name == "sphere33_crop" else (0, 0, 0)


def reference(name):
    """The definition's result on the CPU, computed once and shared."""
    from pagnerf_amd import surface_nets_reference
    if name not in _REFERENCES:
        f, iso, lo, h = case(name)
        _REFERENCES[name] = surface_nets_reference(f, iso, lo, h, index0(name))
    return _REFERENCES[name]


def bits(t):
    """f32 tensor -> its bit patterns (so that equal means bit-equal: -0 != 0, NaN == the same NaN)."""
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_same_mesh(got, want, what=""):
    for k in ("faces", "cell_vertex"):
        assert got[k].dtype == torch.int32 and tuple(got[k].shape) == tuple(want[k].shape), (what, k, got[k].dtype, tuple(got[k].shape), tuple(want[k].shape))
        assert torch.equal(got[k].cpu(), want[k]), (what, k)
    for k in ("vertices", "normals"):
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == tuple(want[k].shape), (what, k, tuple(got[k].shape), tuple(want[k].shape))
        differ = (bits(got[k]) != bits(want[k])).nonzero()
        assert differ.numel() == 0, (what, k, "first differing element", differ[0].tolist(), got[k].cpu()[tuple(differ[0])].item(),
                                     want[k][tuple(differ[0])].item())
