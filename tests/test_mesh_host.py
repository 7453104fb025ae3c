"""CPU checks of the surface-mesh export's definition and host layer (pagnerf_amd/mesh.py): surface_nets_reference is the yardstick of the device
kernels (tests/test_gpu_mesh.py), so it is checked here on its own - against closed forms, the counts that follow from the sign pattern alone, and
the topology and volume of analytic shapes."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_cases as C


def _report(name):
    from pagnerf_amd import mesh_report
    return mesh_report(C.reference(name))


def _f32(x):
    return np.float32(x)


def test_plane_has_the_closed_form():
    """f[i,j,k] = 3 - i at iso 0.5 on 6 x 5 x 7: the cells i = 2 are cut in the middle of their four x edges."""
    f, iso, lo, h = C.case("plane")
    out = C.reference("plane")
    j, k = np.meshgrid(np.arange(4), np.arange(6), indexing="ij")
    want = np.empty((24, 3), np.float32)
    # the definition's two roundings, formed here: (float(index) + local) * h + lo with local = (0.5, 0.5, 0.5)
    for x, idx in enumerate((np.full(24, 2), j.reshape(-1), k.reshape(-1))):
        want[:, x] = (idx.astype(np.float32) + _f32(0.5)) * _f32(h) + _f32(lo)
    assert out["vertices"].dtype == torch.float32 and np.array_equal(out["vertices"].numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(out["normals"], torch.tensor([1.0, 0.0, 0.0]).repeat(24, 1))
    cv = out["cell_vertex"]
    assert cv.dtype == torch.int32 and tuple(cv.shape) == (5, 4, 6)
    assert torch.equal(cv[2], torch.arange(24, dtype=torch.int32).reshape(4, 6)) and (cv[:2] == -1).all() and (cv[3:] == -1).all()
    # one quad per x edge (2,j,k) -> (3,j,k) with 1 <= j <= 3, 1 <= k <= 5, in (j, k) order; P = (2,j,k) is inside: the order is kept.
    # a = 0, u = y, v = z: the cells (j-1,k-1), (j,k-1), (j,k), (j-1,k) of the layer
    vid = lambda a, b: a * 6 + b                                                        # noqa: E731
    faces = []
    for jj in range(1, 4):
        for kk in range(1, 6):
            q = [vid(jj - 1, kk - 1), vid(jj, kk - 1), vid(jj, kk), vid(jj - 1, kk)]
            faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    assert out["faces"].dtype == torch.int32 and out["faces"].tolist() == faces
    v = out["vertices"].double()
    n = torch.cross(v[out["faces"][:, 1].long()] - v[out["faces"][:, 0].long()], v[out["faces"][:, 2].long()] - v[out["faces"][:, 0].long()], dim=-1)
    assert (n[:, 0] > 0).all() and (n[:, 1:] == 0).all()                                 # from inside (small x) to outside


def test_one_point_is_a_closed_cube():
    r = _report("one_point")
    assert (r["vertices"], r["faces"], r["edges"]) == (8, 12, 18)
    assert r["closed"] and r["oriented"] and r["euler"] == 2 and r["volume"] > 0


# the counts follow from the sign pattern and the rules alone; the volume bounds are the issue's (surface nets shrink a convex shape), and the value
# beside each bound is what the committed definition measures
@pytest.mark.parametrize("name,V,F,euler,volume,bound,measured", [
    ("sphere17", 438, 872, 2, C.SPHERE_VOLUME, 0.06, -0.0491),
    ("sphere33", 1740, 3476, 2, C.SPHERE_VOLUME, 0.02, -0.0124),
    ("torus17", 504, 1008, 0, C.TORUS_VOLUME, 0.11, -0.0918),
    ("torus33", 2006, 4012, 0, C.TORUS_VOLUME, 0.03, -0.0233),
])
def test_analytic_shapes(name, V, F, euler, volume, bound, measured):
    r = _report(name)
    out = C.reference(name)
    assert (r["vertices"], r["faces"]) == (V, F)
    assert r["closed"] and r["oriented"] and r["euler"] == euler
    error = r["volume"] / volume - 1.0
    print(name, "volume error %.4f" % error)
    assert abs(error) < bound and abs(error - measured) < 5e-4, error
    v, f = out["vertices"].double(), out["faces"].long()
    fn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=-1)
    assert ((fn * out["normals"].double()[f[:, 0]]).sum(-1) > 0).all()                   # every face normal agrees with its first vertex's normal
    assert torch.allclose(out["normals"].norm(dim=-1), torch.ones(V), atol=1e-6)


def test_the_definition_is_quick():
    """The 33^3 case in well under a second (some 10 ms alone).  One thread and the best of five: the suite's other workers share the machine, and a
    thread pool that waits for busy cores measures them, not the definition."""
    import time
    from pagnerf_amd import surface_nets_reference
    f, iso, lo, h = C.case("sphere33")
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        best = float("inf")
        for _ in range(5):
            t = time.perf_counter()
            surface_nets_reference(f, iso, lo, h)
            best = min(best, time.perf_counter() - t)
    finally:
        torch.set_num_threads(threads)
    assert best < 0.5, best


def _edge_uses(faces):
    f = faces.long()
    a, b = torch.cat((f[:, 0], f[:, 1], f[:, 2])), torch.cat((f[:, 1], f[:, 2], f[:, 0]))
    return torch.unique(torch.minimum(a, b) * (1 << 32) + torch.maximum(a, b), return_counts=True)[1]


def test_border_is_open_and_stays_inside_the_lattice():
    out, r = C.reference("border"), _report("border")
    assert r["vertices"] > 0 and r["faces"] > 0 and not r["closed"]
    uses = _edge_uses(out["faces"])
    assert ((uses == 1) | (uses == 2)).all() and (uses == 1).any()
    V = out["vertices"].shape[0]
    assert out["faces"].min() >= 0 and out["faces"].max() < V                            # a cell outside the lattice has no vertex to refer to
    cv = out["cell_vertex"]
    assert tuple(cv.shape) == (8, 8, 8) and torch.equal(cv[cv >= 0].reshape(-1), torch.arange(V, dtype=torch.int32))


def test_values_equal_to_iso_are_inside():
    f, iso, lo, h = C.case("equal_iso")
    out = C.reference("equal_iso")
    inside = f >= iso
    active = torch.zeros(6, 7, 5, dtype=torch.int32)
    for bx in (0, 1):
        for by in (0, 1):
            for bz in (0, 1):
                active += inside[bx:6 + bx, by:7 + by, bz:5 + bz]
    assert (f == iso).any() and torch.equal(out["cell_vertex"] >= 0, (active > 0) & (active < 8))
    assert torch.isfinite(out["vertices"]).all() and torch.isfinite(out["normals"]).all()


def test_nonfinite_points_take_their_cells_out_and_nothing_else():
    f, iso, lo, h = C.case("nonfinite")
    out, clean = C.reference("nonfinite"), C.reference("sphere17")
    assert torch.isfinite(out["vertices"]).all() and torch.isfinite(out["normals"]).all()
    bad = torch.zeros(16, 16, 16, dtype=torch.bool)                                      # cells with a non-finite corner
    for (i, j, k) in C.NONFINITE_POINTS:
        bad[max(i - 1, 0):i + 1, max(j - 1, 0):j + 1, max(k - 1, 0):k + 1] = True
    assert bad.sum() == 24 and (out["cell_vertex"][bad] == -1).all() and (clean["cell_vertex"][bad] >= 0).any()
    assert torch.equal(out["cell_vertex"][~bad] >= 0, clean["cell_vertex"][~bad] >= 0)
    # the clean mesh without the bad cells' vertices and the faces that touch them, renumbered
    keep_vertex = torch.ones(clean["vertices"].shape[0], dtype=torch.bool)
    keep_vertex[clean["cell_vertex"][bad & (clean["cell_vertex"] >= 0)].long()] = False
    renumber = torch.cumsum(keep_vertex, 0).to(torch.int32) - 1
    keep_face = keep_vertex[clean["faces"].long()].all(-1)
    keep_face = keep_face.reshape(-1, 2).all(-1).repeat_interleave(2)                    # a quad goes as a whole
    assert torch.equal(C.bits(out["vertices"]), C.bits(clean["vertices"][keep_vertex]))
    assert torch.equal(C.bits(out["normals"]), C.bits(clean["normals"][keep_vertex]))
    assert torch.equal(out["faces"], renumber[clean["faces"][keep_face].long()])
    assert 0 < out["faces"].shape[0] < clean["faces"].shape[0]


@pytest.mark.parametrize("name", ["empty", "full"])
def test_no_surface_no_mesh(name):
    out = C.reference(name)
    assert tuple(out["vertices"].shape) == (0, 3) and tuple(out["normals"].shape) == (0, 3) and tuple(out["faces"].shape) == (0, 3)
    assert out["faces"].dtype == torch.int32 and (out["cell_vertex"] == -1).all() and tuple(out["cell_vertex"].shape) == (4, 3, 5)


def test_noise_holds_every_sign_configuration():
    f, iso, lo, h = C.case("noise")
    inside = (f >= iso).to(torch.int64)
    code = torch.zeros(11, 10, 12, dtype=torch.int64)
    for c, (bx, by, bz) in enumerate((x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)):
        code += inside[bx:11 + bx, by:10 + by, bz:12 + bz] << c
    assert torch.unique(code).numel() == 256
    out = C.reference("noise")
    assert torch.equal(out["cell_vertex"] >= 0, (code > 0) & (code < 255))
    uses = _edge_uses(out["faces"])
    assert out["faces"].max() < out["vertices"].shape[0] and uses.max() > 2              # non-manifold edges are there


def test_a_crop_is_the_same_surface():
    """sphere33 cut to an index sub-box with index0 = the box's corner: the cells of the crop give the full lattice's vertices, bit for bit, and the
    faces whose four cells lie in the crop."""
    full, crop = C.reference("sphere33"), C.reference("sphere33_crop")
    (x0, x1), (y0, y1), (z0, z1) = C.CROP
    cv_full, cv_crop = full["cell_vertex"][x0:x1 - 1, y0:y1 - 1, z0:z1 - 1], crop["cell_vertex"]
    assert torch.equal(cv_full >= 0, cv_crop >= 0) and 0 < (cv_crop >= 0).sum() < full["vertices"].shape[0]
    ids = cv_full[cv_full >= 0].long()                                                   # cell order is kept by the crop
    assert torch.equal(C.bits(crop["vertices"]), C.bits(full["vertices"][ids])) and torch.equal(C.bits(crop["normals"]), C.bits(full["normals"][ids]))
    to_crop = torch.full((full["vertices"].shape[0],), -1, dtype=torch.int32)
    to_crop[ids] = torch.arange(ids.numel(), dtype=torch.int32)
    mapped = to_crop[full["faces"].long()]
    inside = (mapped >= 0).all(-1).reshape(-1, 2).all(-1).repeat_interleave(2)
    assert torch.equal(crop["faces"], mapped[inside])


def test_surface_nets_with_device_cpu_is_the_definition():
    from pagnerf_amd import surface_nets
    f, iso, lo, h = C.case("odd_box")
    C.assert_same_mesh(surface_nets(f, iso, lo, h, device="cpu"), C.reference("odd_box"), "odd_box")
    want = C.reference("sphere17")                                                        # the same sphere on the larger lattice
    assert C.reference("odd_box")["faces"].shape == want["faces"].shape and torch.equal(C.bits(C.reference("odd_box")["vertices"]), C.bits(want["vertices"]))


def test_save_and_load_round_trip(tmp_path):
    from pagnerf_amd import load_mesh, save_mesh
    out = C.reference("torus17")
    V = out["vertices"].shape[0]
    gen = torch.Generator().manual_seed(3)
    color = torch.rand(V, 3, generator=gen) * 1.4 - 0.2                                  # values outside [0, 1] are clipped
    color[0, 0] = float("nan")
    mesh = dict(name="m", vertices=out["vertices"], normals=out["normals"], faces=out["faces"], color=color,
                instances=torch.randint(0, 200, (V,), generator=gen), semantics=torch.randint(0, 6, (V,), generator=gen))
    path = save_mesh(mesh, tmp_path / "mesh.ply")
    header = open(path, "rb").read(600).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert header[:3] == ["ply", "format binary_little_endian 1.0", "element vertex %d" % V]
    assert "element face %d" % out["faces"].shape[0] in header and header[-2] == "property list uchar int vertex_indices"
    assert [l.split()[-1] for l in header if l.startswith("property") and "list" not in l] == [
        "x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "instance", "semantic"]
    back = load_mesh(path)
    assert torch.equal(C.bits(back["vertices"]), C.bits(out["vertices"])) and torch.equal(C.bits(back["normals"]), C.bits(out["normals"]))
    assert back["faces"].dtype == torch.int32 and torch.equal(back["faces"], out["faces"])
    assert torch.equal(back["instances"], mesh["instances"]) and torch.equal(back["semantics"], mesh["semantics"])
    want = np.rint(np.clip(np.nan_to_num(color.numpy()), 0.0, 1.0) * 255.0).astype(np.uint8)
    assert back["color"].dtype == torch.uint8 and np.array_equal(back["color"].numpy(), want)
    plain = load_mesh(save_mesh({k: mesh[k] for k in ("vertices", "normals", "faces")}, tmp_path / "plain.ply"))
    assert sorted(plain) == ["faces", "normals", "vertices"] and torch.equal(plain["faces"], out["faces"])
    empty = C.reference("empty")
    back = load_mesh(save_mesh(empty, tmp_path / "empty.ply"))
    assert tuple(back["vertices"].shape) == (0, 3) and tuple(back["faces"].shape) == (0, 3)


def test_argument_errors():
    from pagnerf_amd import extract_mesh, surface_nets, surface_nets_reference
    for fn in (surface_nets_reference, lambda *a: surface_nets(*a, device="cpu"), surface_nets):
        with pytest.raises(ValueError, match="nx, ny, nz"):
            fn(torch.zeros(4, 4), 0.0, -1.0, 0.5)
        with pytest.raises(ValueError, match="at least 2 points"):
            fn(torch.zeros(4, 1, 4), 0.0, -1.0, 0.5)
        with pytest.raises(ValueError, match="2\\^31 cells"):
            fn(torch.zeros(1).expand(2 ** 16 + 1, 2 ** 15 + 1, 2), 0.0, -1.0, 0.5)         # a view: no memory behind it
    with pytest.raises(ValueError, match="index0"):
        surface_nets_reference(torch.zeros(3, 3, 3), 0.0, -1.0, 0.5, index0=(0, -1, 0))
    with pytest.raises(ValueError, match="labels must be"):
        extract_mesh(None, labels="mode")
    with pytest.raises(ValueError, match="channels"):
        extract_mesh(None, channels=("rgb",))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib
    return _lib.load()


def test_mesh_entry_points_resolve_and_refuse_bad_arguments(lib):
    from pagnerf_amd import _lib
    assert {"pag_mesh_workspace_bytes", "pag_mesh_vertices", "pag_mesh_faces"} <= set(_lib.EXPORTS) and lib.pag_abi_version() == 15
    size = lib.pag_mesh_workspace_bytes
    assert 0 < size(17, 17, 17) < size(33, 33, 33) < size(257, 257, 257) < size(1025, 1025, 1025)
    assert size(257, 257, 257) >= (257 ** 3 * 3 + 255) // 256 * 12                        # an i64 and an i32 per block of 256 edge rows
    assert size(1, 5, 5) == 0 and size(5, 5, 0) == 0 and size(-3, 5, 5) == 0
    assert size(2 ** 16 + 1, 2 ** 15 + 1, 2) == 0                                          # 2^31 cells
    assert size(1291, 1291, 1291) == 0 and size(1128, 1128, 1128) == 0 and size(1127, 1127, 1127) > 0      # 2^32 edge rows and more
    buf = (ctypes.c_float * 64)()
    cnt = (ctypes.c_int64 * 1)()
    lo, idx = (ctypes.c_float * 3)(-1.0, -1.0, -1.0), (ctypes.c_int * 3)(0, 0, 0)
    big = 1 << 40

    def vertices(nx=3, ny=3, nz=3, field=buf, lo=lo, idx=idx, out=buf, cap=4, cv=buf, count=cnt, ws=buf, ws_bytes=big):
        return lib.pag_mesh_vertices(field, nx, ny, nz, 0.0, lo, 0.5, idx, out, out, cap, cv, count, ws, ws_bytes, None)
    assert vertices(nx=1) == -1 and b"2 points" in lib.pag_last_error_string()
    assert vertices(nx=2 ** 16 + 1, ny=2 ** 15 + 1, nz=2) == -1 and b"2^31 cells" in lib.pag_last_error_string()
    assert vertices(cap=-1) == -1 and vertices(lo=None) == -1 and vertices(idx=None) == -1
    assert vertices(field=None) == -1 and vertices(cv=None) == -1 and vertices(count=None) == -1 and vertices(out=None) == -1
    assert vertices(idx=(ctypes.c_int * 3)(0, -1, 0)) == -1 and b"index0" in lib.pag_last_error_string()
    assert vertices(ws=None) == -1 and vertices(ws_bytes=8) == -1 and b"workspace" in lib.pag_last_error_string()

    def faces(nx=3, ny=3, nz=3, field=buf, cv=buf, out=buf, cap=4, count=cnt, ws=buf, ws_bytes=big):
        return lib.pag_mesh_faces(field, nx, ny, nz, 0.0, cv, out, cap, count, ws, ws_bytes, None)
    assert faces(nz=1) == -1 and b"2 points" in lib.pag_last_error_string()
    assert faces(cap=-1) == -1 and faces(field=None) == -1 and faces(cv=None) == -1 and faces(count=None) == -1 and faces(out=None) == -1
    assert faces(ws_bytes=8) == -1 and b"workspace" in lib.pag_last_error_string()


def test_mesh_ops_refuse_cpu_tensors():
    from pagnerf_amd import ops
    f = torch.zeros(3, 3, 3)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ops.mesh_vertices(f, 0.0, (-1.0,) * 3, 0.5, (0, 0, 0), None, None, torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ops.mesh_faces(f, 0.0, torch.zeros(8, dtype=torch.int32), None, torch.zeros(1, dtype=torch.int64))
