"""GPU checks of the surface-mesh export (pagnerf_amd/mesh.py on csrc/mesh.hip: pag_mesh_vertices / pag_mesh_faces) against the CPU definition
surface_nets_reference on the cases of mesh_cases.py.  faces and cell_vertex are integers; vertices and normals are compared BIT FOR BIT: the op order
is fixed, mesh.hip is built without contraction, and division and square root are the correctly rounded ones."""
import types
import warnings

import numpy as np
import pytest
import torch

import mesh_cases as C

pytestmark = pytest.mark.gpu


def _run(name, dev, **kw):
    from pagnerf_amd import surface_nets
    f, iso, lo, h = C.case(name)
    return surface_nets(f.to(dev), iso, lo, h, C.index0(name), **kw)


@pytest.mark.parametrize("name", C.CASES)
def test_the_device_mesh_is_the_definition(gpu_device, name):
    from pagnerf_amd import surface_nets
    want = C.reference(name)
    got = _run(name, gpu_device)
    assert all(got[k].is_cuda for k in ("vertices", "normals", "faces", "cell_vertex"))
    C.assert_same_mesh(got, want, name)
    f, iso, lo, h = C.case(name)
    back = surface_nets(f, iso, lo, h, C.index0(name), device=gpu_device)                 # a CPU field: there and back
    assert not any(back[k].is_cuda for k in back)
    C.assert_same_mesh(back, want, name + " from the CPU")


@pytest.mark.parametrize("name", ["sphere33", "noise", "odd_box"])
def test_two_runs_give_the_same_bits(gpu_device, name):
    first, second = _run(name, gpu_device), _run(name, gpu_device)
    for k in ("vertices", "normals"):
        assert torch.equal(C.bits(first[k]), C.bits(second[k]))
    assert torch.equal(first["faces"], second["faces"]) and torch.equal(first["cell_vertex"], second["cell_vertex"])


@pytest.mark.parametrize("name", ["odd_box", "noise"])
def test_capacity(gpu_device, name):
    want = C.reference(name)
    V, F = want["vertices"].shape[0], want["faces"].shape[0]
    C.assert_same_mesh(_run(name, gpu_device, capacity=(V, F)), want, name)
    C.assert_same_mesh(_run(name, gpu_device, capacity=(V + 7, F + 5)), want, name)
    with pytest.raises(RuntimeError, match="kept %d vertices, the buffers hold %d" % (V, V - 1)):
        _run(name, gpu_device, capacity=(V - 1, F))
    with pytest.raises(RuntimeError, match="kept %d faces, the buffers hold %d" % (F, F - 1)):
        _run(name, gpu_device, capacity=(V, F - 1))


@pytest.mark.parametrize("name", ["odd_box", "noise"])
def test_nothing_is_written_past_the_capacity(gpu_device, name):
    """The outputs are the first rows of larger, pattern-filled tensors; the capacity is one vertex / one quad short: the counters still count
    everything, the rows that fit are the definition's, and every byte past the capacity keeps the pattern."""
    from pagnerf_amd import ops
    f, iso, lo, h = C.case(name)
    want = C.reference(name)
    V, F = want["vertices"].shape[0], want["faces"].shape[0]
    dev = gpu_device
    f = f.to(dev)
    PAT_F, PAT_I = 12345.5, -77
    big_v, big_n = torch.full((V + 64, 3), PAT_F, device=dev), torch.full((V + 64, 3), PAT_F, device=dev)
    big_f = torch.full((F + 64, 3), PAT_I, dtype=torch.int32, device=dev)
    cell_vertex = torch.full((want["cell_vertex"].numel() + 64,), PAT_I, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    cv = cell_vertex[:want["cell_vertex"].numel()]
    for cap_v, cap_f in ((V - 1, F - 1), (V - 1, F - 2), (0, 0)):
        for t, pat in ((big_v, PAT_F), (big_n, PAT_F), (big_f, PAT_I), (cell_vertex, PAT_I)):
            t.fill_(pat)
        count.zero_()
        ops.mesh_vertices(f, iso, (lo,) * 3, h, C.index0(name), big_v[:cap_v], big_n[:cap_v], cv, count[0:1])
        ops.mesh_faces(f, iso, cv, big_f[:cap_f], count[1:2])
        assert count.tolist() == [V, F // 2]
        assert torch.equal(C.bits(big_v[:cap_v]), C.bits(want["vertices"][:cap_v])) and torch.equal(C.bits(big_n[:cap_v]), C.bits(want["normals"][:cap_v]))
        assert (big_v[cap_v:] == PAT_F).all() and (big_n[cap_v:] == PAT_F).all()
        whole = cap_f // 2 * 2                                                             # a quad that does not fit whole is not written
        assert torch.equal(big_f[:whole].cpu(), want["faces"][:whole]) and (big_f[whole:] == PAT_I).all()
        assert torch.equal(cv.cpu(), want["cell_vertex"].reshape(-1)) and (cell_vertex[cv.numel():] == PAT_I).all()     # every cell's slot, fit or not


def _reported_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return out, [w for w in seen if "called a synchronizing" in str(w.message)]


def test_host_synchronisations(gpu_device):
    """Two reads by default (the vertex count sizes the buffers, the last read trims the faces), one with capacity=."""
    want = C.reference("sphere17")
    _run("sphere17", gpu_device)                                                           # warm up: allocator, library load
    f = C.case("sphere17")[0].to(gpu_device)
    from pagnerf_amd import surface_nets
    got, syncs = _reported_syncs(lambda: surface_nets(f, 0.0, -1.0, 2.0 / 16))
    C.assert_same_mesh(got, want)
    assert len(syncs) == 2, [str(w.message) for w in syncs]
    cap = (want["vertices"].shape[0], want["faces"].shape[0])
    got, syncs = _reported_syncs(lambda: surface_nets(f, 0.0, -1.0, 2.0 / 16, capacity=cap))
    C.assert_same_mesh(got, want)
    assert len(syncs) == 1, [str(w.message) for w in syncs]


# ----------------------------------------------------------------------------------------------- the nef
_SCENE = {}


def _nef(dev):
    """The parity tests' small nef, built once."""
    import test_gpu_parity as T
    if "nef" not in _SCENE:
        _SCENE["nef"] = T._make_scene(dev, "bf16", N=8, S=32)[0]
    return _SCENE["nef"]


class _BlobNef:
    """The small nef with its density set by hand to a blob - 20 * (0.55 - |p - c|), clamped at 0 - so that the surface at density 2 is a sphere of
    radius 0.45 whatever the random tables hold; every other channel is the nef's own."""
    CENTRE = (0.05, -0.1, 0.08)

    def __init__(self, nef):
        self.nef, self.device = nef, nef.device

    def get_supported_channels(self):
        return self.nef.get_supported_channels()

    def __call__(self, coords=None, ray_d=None, channels=None):
        if channels == "density":
            c = torch.tensor(self.CENTRE, device=coords.device)
            return torch.relu(20.0 * (0.55 - torch.linalg.norm(coords.float() - c, dim=-1, keepdim=True)))
        return self.nef(coords=coords, ray_d=ray_d, channels=channels)


def _lattice_points(res, keep, dev):
    axis = torch.arange(res + 1, dtype=torch.float32) / float(res) * 2.0 - 1.0
    ax = [axis[k].to(dev) for k in keep]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def test_density_lattice_is_the_direct_query(gpu_device):
    from pagnerf_amd import density_lattice
    nef = _nef(gpu_device)
    res = 16
    with torch.no_grad():
        pts = _lattice_points(res, [torch.arange(res + 1)] * 3, gpu_device)
        want = nef(coords=pts[:, None], ray_d=None, channels="density").reshape(res + 1, res + 1, res + 1).float()
    field, lo, h, index0 = density_lattice(nef, res)
    assert field.is_cuda and field.dtype == torch.float32 and (lo, h, index0) == (-1.0, 2.0 / res, (0, 0, 0))
    assert want.max() > 0 and torch.equal(C.bits(field), C.bits(want))
    assert torch.equal(C.bits(density_lattice(nef, res, batch=1000)[0]), C.bits(want))
    # a strict box: -0.5 and 0.75 are lattice coordinates (indices 4 and 14) and stay out
    limits = torch.tensor([[-0.5, -0.3, -1.5], [0.75, 0.3, 0.1]])
    keep = [torch.arange(5, 14), torch.arange(6, 11), torch.arange(0, 9)]
    cut, lo, h, index0 = density_lattice(nef, res, limits=limits, batch=1000)
    assert index0 == (5, 6, 0) and tuple(cut.shape) == (9, 5, 9)
    assert torch.equal(C.bits(cut), C.bits(want[5:14, 6:11, 0:9]))
    with torch.no_grad():
        direct = nef(coords=_lattice_points(res, keep, gpu_device)[:, None], ray_d=None, channels="density").reshape(9, 5, 9).float()
    assert torch.equal(C.bits(cut), C.bits(direct))


@pytest.mark.parametrize("density", ["blob", "field"])
def test_extract_mesh(gpu_device, density):
    from pagnerf_amd import density_lattice, extract_mesh, mesh_report, surface_nets
    nef = _nef(gpu_device)
    res = 16
    if density == "blob":
        nef, iso = _BlobNef(nef), 2.0
    else:                                                                                  # the nef's own field, cut at the median of its positive values
        own = density_lattice(nef, res)[0]
        iso = float(own[own > 0].median())
    mesh = extract_mesh(nef, resolution=res, min_density=iso, name="m")
    V, F = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    assert mesh["name"] == "m" and V > 50 and F > 50 and mesh["vertices"].is_cuda
    assert mesh["faces"].dtype == torch.int32 and mesh["faces"].min() >= 0 and mesh["faces"].max() < V
    if density == "blob":
        r = mesh_report(mesh)
        # surface nets shrink a sphere by about (h / r)^2 of its volume: 5 % at mesh_cases' sphere17 (r = 4.8 h), so about 9 % at r = 3.6 h
        assert r["closed"] and r["oriented"] and r["euler"] == 2 and abs(r["volume"] / (4.0 / 3.0 * np.pi * 0.45 ** 3) - 1.0) < 0.15
        assert (mesh["normals"] != 0).any(-1).all()
    v, n = mesh["vertices"], mesh["normals"]
    with torch.no_grad():
        inst = nef(coords=v[:, None], ray_d=None, channels="inst_embedding").float().reshape(V, -1)
        sem = nef(coords=v[:, None], ray_d=None, channels="semantics").float().reshape(V, -1)
        ray_d = -n
        ray_d[(n == 0).all(-1)] = torch.tensor([0.0, 0.0, -1.0], device=gpu_device)       # a camera looking straight at the surface
        rgb = nef(coords=v[:, None], ray_d=ray_d, channels="rgb").float().reshape(V, 3)
    assert mesh["instances"].dtype == torch.int64 and torch.equal(mesh["instances"], torch.argmax(inst, -1))
    assert mesh["semantics"].dtype == torch.int64 and torch.equal(mesh["semantics"], torch.argmax(sem, -1))
    assert torch.equal(C.bits(mesh["color"]), C.bits(rgb))
    chunked = extract_mesh(nef, resolution=res, min_density=iso, batch=97, name="m")
    for k in ("vertices", "normals", "color"):
        assert torch.equal(C.bits(chunked[k]), C.bits(mesh[k])), k
    for k in ("faces", "instances", "semantics"):
        assert torch.equal(chunked[k], mesh[k]), k
    # the definition on the same field gives the same mesh
    field, lo, h, index0 = density_lattice(nef, res)
    C.assert_same_mesh(surface_nets(field, iso, lo, h, index0), surface_nets(field.cpu(), iso, lo, h, index0, device="cpu"), density)
    assert torch.equal(C.bits(surface_nets(field, iso, lo, h, index0)["vertices"]), C.bits(v))
    # a callable labels the instances itself; a channel that was not asked for is not there
    by_hand = extract_mesh(nef, resolution=res, min_density=iso, color=False, channels=("inst_embedding",), labels=lambda e: torch.argmax(e.float(), -1) + 1)
    assert torch.equal(by_hand["instances"], mesh["instances"] + 1) and "semantics" not in by_hand and "color" not in by_hand


def test_a_channel_the_nef_lacks(gpu_device):
    from pagnerf_amd import extract_mesh
    nef = _BlobNef(_nef(gpu_device))
    nef.get_supported_channels = lambda: {"density", "rgb", "inst_embedding"}
    mesh = extract_mesh(nef, resolution=8, min_density=2.0, color=False)                   # the default channels: what the nef has
    assert "instances" in mesh and "semantics" not in mesh
    with pytest.raises(ValueError, match="semantics"):
        extract_mesh(nef, resolution=8, min_density=2.0, color=False, channels=("inst_embedding", "semantics"))


def test_save_mesh_of_the_train_command(gpu_device, tmp_path, capsys):
    """train.save_mesh (--save-mesh) on a stand-in trainer that holds the nef alone: a PLY that load_mesh reads, and the report line of that mesh."""
    from pagnerf_amd import extract_mesh, load_mesh, mesh_report, train
    from pagnerf_amd import mesh as M
    nef = _BlobNef(_nef(gpu_device))
    trainer = types.SimpleNamespace(pipeline=types.SimpleNamespace(nef=nef))
    path = train.save_mesh(trainer, str(tmp_path / "mesh.ply"), resolution=16, min_density=2.0)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    back = load_mesh(path)
    want = extract_mesh(nef, resolution=16, min_density=2.0)
    assert torch.equal(C.bits(back["vertices"]), C.bits(want["vertices"])) and torch.equal(back["faces"], want["faces"].cpu())
    assert torch.equal(back["instances"], want["instances"].cpu()) and torch.equal(back["semantics"], want["semantics"].cpu())
    assert back["color"].dtype == torch.uint8 and tuple(back["color"].shape) == (want["vertices"].shape[0], 3)
    report = mesh_report(back)
    assert report["vertices"] == want["vertices"].shape[0] and report["faces"] == want["faces"].shape[0]
    assert line == M.report_line(mesh_report(want)) and line.startswith("mesh: %d vertices, %d faces" % (report["vertices"], report["faces"]))
