"""CPU side of the map export (pagnerf_amd/map_export.py on csrc/map.hip): the seeded inputs of the g14_map.npz cases (made from the reference's
utils/render_map.py by tests/golden/make_golden_map.py, which imports the generators below), a numpy restatement of render_points_at_depth :107-120
and get_dense_occupied_points / generate_pc_map :46-79, :143-169 pinned to that fixture, argument refusal of the new entry points, save_map and
pinhole_base_rays.  The GPU tests compare the device against the same fixture."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

from conftest import golden

RENDER_BATCH = 20000
THRESHOLDS = dict(min_density=40.0, min_alpha=0.9, depth_range=(0.6, 0.8))

# name -> cameras, image height / width, instance channels, kind of instance rows
VIEWS_CASES = {
    "chunk_inside_image": dict(seed=1401, cams=3, h=88, w=80, I=200, kind="plain"),       # 21 120 rays: the 20 000 boundary falls inside image 2
    "ties_and_nan": dict(seed=1402, cams=3, h=24, w=32, I=200, kind="ties"),
    "six_channels": dict(seed=1403, cams=2, h=24, w=32, I=6, kind="plain"),
    "none_kept": dict(seed=1404, cams=2, h=8, w=8, I=6, kind="no_hit"),
}
# name -> blas level, limits [[min], [max]] or None, min_density (None: the default), instance channels
DENSE_CASES = {
    "level4_all": dict(seed=1411, level=4, limits=None, min_density=None, I=200),
    "level5_limits": dict(seed=1412, level=5, limits=[[-0.5, -0.3, -1.0], [0.5, 0.25, 0.1]], min_density=None, I=6),
    "level4_limits_on_lattice": dict(seed=1413, level=4, limits=[[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]], min_density=3.5, I=200),
    "level4_nothing_occupied": dict(seed=1414, level=4, limits=None, min_density=100.0, I=6),
}


# ----------------------------------------------------------------------------------------------- seeded inputs
def view_matrices(rs, C):
    """[C,4,4] f32 world -> camera matrices: a random rotation (QR) and a small translation."""
    out = np.zeros((C, 4, 4), np.float32)
    for c in range(C):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out[c, :3, :3] = q
        out[c, :3, 3] = rs.uniform(-0.3, 0.3, 3)
        out[c, 3, 3] = 1.0
    return out


def base_rays_np(h, w):
    """One image's camera-frame rays [h*w,3] (origins, unit dirs), f32: pixel centres through a pinhole of focal length w."""
    py, px = np.meshgrid(np.arange(h, dtype=np.float32) + 0.5, np.arange(w, dtype=np.float32) + 0.5, indexing="ij")
    d = np.stack(((px - w / 2) / w, -(py - h / 2) / w, -np.ones_like(px)), -1).reshape(-1, 3).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    return np.zeros_like(d), d


def views_inputs(name):
    """The rendered buffers of a views case, all rays of all cameras: dict of f32 / bool arrays from the case's seed."""
    c = VIEWS_CASES[name]
    rs = np.random.RandomState(c["seed"])
    N, I = c["cams"] * c["h"] * c["w"], c["I"]
    view = view_matrices(rs, c["cams"])
    d = dict(view=view,
             density=rs.gamma(2.0, 40.0, N).astype(np.float32)[:, None],
             alpha=rs.uniform(0.7, 1.0, N).astype(np.float32)[:, None],
             depth=rs.uniform(0.5, 0.9, N).astype(np.float32)[:, None],
             hit=rs.rand(N) > 0.1,
             rgb=rs.rand(N, 3).astype(np.float32))
    inst = rs.rand(N, I).astype(np.float32)
    if c["kind"] == "ties":
        inst = (np.round(inst * 8) / 8).astype(np.float32)                                # 9 distinct values over 200 columns: the maximum is tied
        rows = np.nonzero(rs.rand(N) < 0.05)[0]
        inst[rows, rs.randint(0, I, rows.size)] = np.nan
        inst[rows[::2], rs.randint(0, I, rows[::2].size)] = np.nan                        # two NaNs in a row: the first one wins
        inst[rows[1::7]] = np.nan                                                         # a row of NaNs only
        inst[::11, 0] = -0.0
    if c["kind"] == "no_hit":
        d["hit"] = np.zeros(N, bool)
    d["inst_embedding"] = inst
    return d


def dense_density(rs, n):
    """The next n density values of a dense case's nef stand-in (sequential draws: the same whatever the chunking)."""
    return (rs.rand(n) * 6.0).astype(np.float32)


def dense_inst(rs, n, I):
    """The next n instance rows: uniform, with column 0 lifted above the others in about 40 % of the rows (label 0 = dropped)."""
    a = rs.rand(n, I + 1)
    inst = a[:, :I].astype(np.float32)
    inst[:, 0] += (a[:, I] < 0.4).astype(np.float32)
    return inst


# ----------------------------------------------------------------------------------------------- numpy restatement
def np_argmax(inst):
    """torch.argmax(dim=-1): the first index of the maximum, a NaN counting as the maximum."""
    nan = np.isnan(inst)
    with np.errstate(invalid="ignore"):
        plain = np.argmax(np.where(nan, -np.inf, inst), axis=-1)
    return np.where(nan.any(-1), np.argmax(nan, axis=-1), plain).astype(np.int64)


def np_views_mask(d, min_density=40.0, min_alpha=0.9, depth_range=(0.6, 0.8)):
    terms = [d["density"][:, 0] > np.float32(min_density), d["alpha"][:, 0] > np.float32(min_alpha), d["hit"].astype(bool),
             d["depth"][:, 0] < np.float32(depth_range[1]), d["depth"][:, 0] > np.float32(depth_range[0])]
    return terms


def np_views(d, base_o, base_d, **thresholds):
    """:107-120 -> (kept ray indices, points f32 [K,3], ids i64 [K], colours f32 [K,3])."""
    terms = np_views_mask(d, **thresholds)
    mask = np.logical_and.reduce(terms)
    C, n = d["view"].shape[0], base_o.shape[0]
    R, t = d["view"][:, :3, :3].astype(np.float64), d["view"][:, :3, 3].astype(np.float64)
    o = np.broadcast_to(base_o[None].astype(np.float64), (C, n, 3))
    p_cam = base_d[None].astype(np.float64) * d["depth"].astype(np.float64).reshape(C, n, 1)
    pts = np.einsum("cnk,ckj->cnj", o - t[:, None], R) + np.einsum("cnk,ckj->cnj", p_cam, R)       # R^T (o - t) + R^T (d depth), row-vector form
    kept = np.nonzero(mask)[0]
    return kept, pts.reshape(-1, 3)[kept].astype(np.float32), np_argmax(d["inst_embedding"][kept]), d["rgb"][kept]


def np_lattice(level, limits):
    """:56-63 -> the (limited) lattice points f32 [P,3], x slowest."""
    res = np.float32(2.0 ** level)
    axis = (np.arange(int(res), dtype=np.float32) / res * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    pts = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    if limits is not None:
        lim = np.asarray(limits, np.float32)
        m = np.logical_and.reduce([(pts[:, a] > lim[0, a]) & (pts[:, a] < lim[1, a]) for a in range(3)])
        pts = pts[m]
    return pts


def dense_min_density(c):
    return (0.01 * 512) / np.sqrt(3) if c["min_density"] is None else c["min_density"]


def np_dense(name):
    """get_dense_occupied_points + generate_pc_map of a dense case -> (lattice size P, occupied points, map points, instances)."""
    c = DENSE_CASES[name]
    lattice = np_lattice(c["level"], c["limits"])
    dens = dense_density(np.random.RandomState(c["seed"]), lattice.shape[0])
    occ = lattice[dens > np.float32(dense_min_density(c))]
    ids = np_argmax(dense_inst(np.random.RandomState(c["seed"] + 100), occ.shape[0], c["I"]))
    return lattice.shape[0], occ, occ[ids != 0], ids[ids != 0]


# ----------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", sorted(VIEWS_CASES))
def test_restatement_equals_reference_views(name):
    g = golden("g14_map.npz")
    c = VIEWS_CASES[name]
    d = views_inputs(name)
    for k in ("density", "alpha", "depth", "hit", "view"):                                # the small inputs are in the fixture, bit for bit
        assert np.array_equal(d[k], g[name + "/" + k]), k
    bo, bd = g[name + "/base_origins"], g[name + "/base_dirs"]
    assert bo.shape == (c["h"] * c["w"], 3)
    kept, pts, ids, col = np_views(d, bo, bd, **THRESHOLDS)
    assert np.array_equal(kept, g[name + "/kept"])
    assert np.array_equal(ids, g[name + "/inst_embedding"]) and g[name + "/inst_embedding"].dtype == np.int64
    assert col.tobytes() == g[name + "/color"].tobytes()
    np.testing.assert_allclose(pts, g[name + "/points"], rtol=1e-5, atol=1e-6)
    if name != "none_kept":
        share = kept.size / d["hit"].size
        assert 0.05 < share < 0.5, share
        terms = np_views_mask(d, **THRESHOLDS)
        for i in range(5):                                                                # every term alone rejects a ray the other four accept
            others = np.logical_and.reduce([t for j, t in enumerate(terms) if j != i])
            assert (others & ~terms[i]).any(), i
    else:
        assert kept.size == 0


def test_views_fixture_covers_ties_nan_and_the_chunk_boundary():
    d = views_inputs("ties_and_nan")
    kept = golden("g14_map.npz")["ties_and_nan/kept"]
    rows = d["inst_embedding"][kept]
    nan = np.isnan(rows)
    assert (nan.sum(-1) == 1).any() and (nan.sum(-1) >= 2).any() and nan.all(-1).any()
    clean = rows[~nan.any(-1)]
    assert ((clean == clean.max(-1, keepdims=True)).sum(-1) > 1).any()                    # tied maxima among the kept rows
    c = VIEWS_CASES["chunk_inside_image"]
    n = c["h"] * c["w"]
    assert RENDER_BATCH % n != 0 and RENDER_BATCH < c["cams"] * n


@pytest.mark.parametrize("name", sorted(DENSE_CASES))
def test_restatement_equals_reference_dense(name):
    g = golden("g14_map.npz")
    P, occ, pts, ids = np_dense(name)
    assert P == int(g[name + "/lattice_size"])
    assert occ.tobytes() == g[name + "/occupied"].tobytes() and occ.shape == g[name + "/occupied"].shape
    assert pts.tobytes() == g[name + "/points"].tobytes() and pts.shape == g[name + "/points"].shape
    assert np.array_equal(ids, g[name + "/instances"])
    if name == "level4_nothing_occupied":
        assert occ.shape[0] == 0
    else:
        assert 0 < pts.shape[0] < occ.shape[0] < P


# ----------------------------------------------------------------------------------------------- entry points without a device
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib
    return _lib.load()


def test_map_entry_points_refuse_bad_arguments(lib):
    buf = (ctypes.c_float * 64)()
    cnt = (ctypes.c_int64 * 1)()
    assert lib.pag_map_workspace_bytes(0) == 0 and lib.pag_map_workspace_bytes((1 << 31) + 1) == 0
    assert lib.pag_map_workspace_bytes(20000) >= 20000 * 4
    big = 1 << 40

    def points(n=4, params=buf, C=2, n_cam=2, rpc=8, ray0=0, inst=buf, I=6, stride=6, ids=None, out=buf, cap=4, count=cnt, ws=buf, ws_bytes=big,
               depth=buf):
        return lib.pag_map_points(params, C, buf, n_cam, rpc, buf, buf, ray0, n, depth, buf, buf, buf, buf, inst, I, stride, ids, 40.0, 0.9, 0.6, 0.8,
                                  out, buf, buf, cap, count, ws, ws_bytes, None)
    assert points(n=0) == 0 and points(n=0, params=None, inst=None, out=None, count=None, ws=None, ws_bytes=0) == 0      # no ray: nothing to do
    assert points(n=-1) == -1
    assert points(ray0=13) == -1 and b"outside" in lib.pag_last_error_string()             # rays [13, 17) of 2 x 8
    assert points(C=0) == -1 and points(rpc=0) == -1 and points(cap=-1) == -1
    assert points(I=0) == -1 and points(I=1025, stride=1025) == -1 and points(stride=5) == -1
    assert points(ids=buf) == -1 and b"either" in lib.pag_last_error_string()
    assert points(inst=None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert points(params=None) == -1 and points(depth=None) == -1 and points(out=None) == -1 and points(count=None) == -1
    assert points(ws=None) == -1 and points(ws_bytes=8) == -1 and b"workspace" in lib.pag_last_error_string()

    def select(n=4, pin=buf, value=buf, inst=None, I=0, stride=0, ids=None, out=buf, cap=4, count=cnt, ws=buf, ws_bytes=big):
        return lib.pag_map_select(pin, n, value, 0.5, inst, I, stride, ids, out, None, cap, count, ws, ws_bytes, None)
    assert select(n=0) == 0 and select(n=0, pin=None, value=None, out=None, count=None, ws=None, ws_bytes=0) == 0
    assert select(n=-1) == -1 and select(cap=-1) == -1
    assert select(value=None) == -1 and b"predicate" in lib.pag_last_error_string()
    assert select(pin=None) == -1 and select(out=None) == -1 and select(count=None) == -1
    assert select(value=None, inst=buf, I=6, stride=4) == -1 and select(value=None, inst=buf, I=6, stride=6, ids=buf) == -1
    assert select(ws_bytes=8) == -1 and b"workspace" in lib.pag_last_error_string()


def test_map_export_refuses_cpu_tensors():
    from pagnerf_amd import ops
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.map_select(z, z.clone(), torch.zeros(1, dtype=torch.int64), value=torch.zeros(4))


# ----------------------------------------------------------------------------------------------- host helpers
def test_save_map_pickle_and_ply(tmp_path):
    from pagnerf_amd import save_map
    pts = torch.tensor([[0.5, -1.0, 2.0], [1.5, 0.25, -3.0]])
    data = [{"points": pts, "inst_embedding": torch.tensor([7, 199]), "color": torch.tensor([[1.0, 0.5, 0.0], [0.2, 2.0, -1.0]]), "name": "nerf_pc"}]
    p = save_map(data, tmp_path / "nerf_pc.pkl")
    back = pickle.load(open(p, "rb"))
    assert back[0]["name"] == "nerf_pc" and torch.equal(back[0]["points"], pts) and torch.equal(back[0]["inst_embedding"], data[0]["inst_embedding"])
    raw = open(save_map(data, tmp_path / "map.ply"), "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 2"]
    assert lines[3:] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
                         "property int instance"]
    v = np.frombuffer(body, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3), ("instance", "<i4")])
    assert v.shape == (2,) and v[1]["xyz"].tolist() == [1.5, 0.25, -3.0] and v[1]["rgb"].tolist() == [51, 255, 0] and v[1]["instance"] == 199
    assert v[0]["rgb"].tolist() == [255, 128, 0] and v[0]["instance"] == 7
    dense = [{"name": "nerf_pc", "points": pts, "instances": torch.tensor([3, 4])}]         # generate_pc_map's structure: no colours
    raw = open(save_map(dense, tmp_path / "dense.ply"), "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"red" not in head and len(body) == 2 * 16


def test_pinhole_base_rays():
    from pagnerf_amd import pinhole_base_rays
    rays = pinhole_base_rays(1280, 720, 1000.0, 1000.0, mip=2)
    assert rays.origins.shape == (180 * 320, 3) and rays.dirs.shape == (180 * 320, 3) and not rays.origins.any()
    assert torch.allclose(rays.dirs.norm(dim=-1), torch.ones(180 * 320), atol=1e-6)
    odd = pinhole_base_rays(5, 3, 4.0, 4.0)                                              # odd sizes: the centre pixel looks down -z
    assert odd.dirs.shape == (15, 3) and torch.equal(odd.dirs[1 * 5 + 2], torch.tensor([0.0, 0.0, -1.0]))
    assert odd.dirs[0, 0] < 0 < odd.dirs[0, 1] and odd.dirs[14, 0] > 0 > odd.dirs[14, 1]    # x right, y up, first pixel top left
    assert torch.allclose(odd.dirs[1 * 5 + 3, :2] / -odd.dirs[1 * 5 + 3, 2], torch.tensor([0.25, 0.0]))
