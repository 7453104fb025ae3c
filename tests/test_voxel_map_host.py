"""Host-side checks of the fused voxel map (pagnerf_amd/map_export.py): the tensor-op definitions fuse_points_reference / label_table_reference
against a brute-force Python dict, the rules at the edges (ties, id range, floor below the origin, faces, non-finite rows, the strict box,
min_votes, K = 0 / 1), the entry points' argument checks without a device, the PLY and CSV writers, and fuse_map on a list of entries."""
import csv
import ctypes
import pickle

import numpy as np
import pytest
import torch

import voxel_map_cases as C


def _ref(points, ids, color=None, **kw):
    from pagnerf_amd import fuse_points_reference
    return fuse_points_reference(torch.as_tensor(points, dtype=torch.float32), torch.as_tensor(ids, dtype=torch.int64),
                                 None if color is None else torch.as_tensor(color, dtype=torch.float32), **kw)


@pytest.mark.parametrize("seed,kw", [(0, {}), (1, dict(min_votes=2)), (2, dict(limits=[[-0.5, -0.5, -0.5], [0.5, 0.75, 1.0]])),
                                     (3, dict(origin=(-0.3, -0.2, -0.1)))])
def test_references_equal_a_brute_force_dict(seed, kw):
    from pagnerf_amd import label_table_reference
    rs = np.random.RandomState(seed)
    K = 300
    pts = torch.from_numpy(rs.uniform(-1, 1, (K, 3)).astype(np.float32))
    ids = torch.from_numpy(C.IDS[rs.randint(0, 5, K)])
    col = torch.from_numpy(rs.rand(K, 3).astype(np.float32))
    for color in (col, None):
        got = _ref(pts, ids, color, voxel_size=0.5, **kw)
        want = C.brute_fuse(pts, ids, color, 0.5, **kw)
        assert 8 < want["count"].numel() <= 64 and int(want["count"].max()) > 3
        C.assert_same(got, want, C.FUSED_KEYS, kw)
        assert got["voxel_size"] == 0.5 and torch.equal(got["origin"], torch.tensor(kw.get("origin", C.ORIGIN)))
        for ignore in ((0,), (), (0, -5, 3)):
            table = label_table_reference(got, ignore=ignore)
            C.assert_same(table, C.brute_table(got, ignore), C.TABLE_KEYS, ignore)
            assert table["volume"].dtype == torch.float64 and torch.equal(table["volume"], table["voxels"].double() * 0.125)


def test_ties_go_to_the_smaller_id_and_ids_are_int64():
    p = torch.tensor([[0.1, 0.1, 0.1]] * 6)
    big, neg = (1 << 31) + 3, -5
    out = _ref(p, [7, 3, 7, 3, 9, 9], voxel_size=0.5)                                       # three ids, two votes each
    assert out["instances"].tolist() == [3] and out["count"].tolist() == [6] and out["agreement"].tolist() == [np.float32(2) / np.float32(6)]
    assert _ref(p, [big, neg, big, neg, 0, 1], voxel_size=0.5)["instances"].tolist() == [neg]       # signed comparison: -5 < 2^31 + 3
    assert _ref(p, [big, 1 << 40, 1 << 40, big, 0, 1], voxel_size=0.5)["instances"].tolist() == [big]
    assert _ref(p, [big, 1 << 40, 1 << 40, big, 1 << 40, 1], voxel_size=0.5)["instances"].tolist() == [1 << 40]     # a majority beats a smaller id
    assert _ref(p, [neg] * 6, voxel_size=0.5)["agreement"].tolist() == [1.0]


def test_floor_faces_non_finite_rows_and_the_strict_box():
    v = 0.25
    o = (-1.0, -1.0, -1.0)
    inside = [-0.9, -0.9, -0.9]
    out = _ref([inside, [-1.0 - v / 2, -0.9, -0.9]], [1, 2], voxel_size=v, origin=o)        # floor(-0.5) = -1: dropped, not voxel 0
    assert out["voxels"].tolist() == [[0, 0, 0]] and out["instances"].tolist() == [1] and out["count"].tolist() == [1]
    out = _ref([[-0.75, -1.0, -0.5], [-0.76, -0.99, -0.51]], [1, 2], voxel_size=v, origin=o)      # a point on a face belongs to the upper voxel
    assert out["voxels"].tolist() == [[0, 0, 1], [1, 0, 2]] and out["instances"].tolist() == [2, 1]
    bad = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [4.0e6, 0, 0], inside]
    out = _ref(bad, [1, 2, 3, 4, 5], voxel_size=v, origin=o)                                # 4e6 / 0.25 is beyond 2^21 cells
    assert out["instances"].tolist() == [5] and torch.equal(out["points"], torch.tensor([inside]))
    box = [[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]]
    pts = [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, -0.5, 0.0], [0.0, 0.0, 0.4999], [0.8, 0.0, 0.0]]
    out = _ref(pts, [1, 2, 3, 4, 5], voxel_size=v, origin=o, limits=box)                     # on the box's faces: outside
    assert sorted(out["instances"].tolist()) == [1, 4]
    assert sorted(_ref(pts, [1, 2, 3, 4, 5], voxel_size=v, origin=o, limits=torch.zeros(0))["instances"].tolist()) == [1, 2, 3, 4, 5]
    with pytest.raises(ValueError):
        _ref(pts, [1, 2, 3, 4, 5], voxel_size=0.0)
    with pytest.raises(ValueError):
        _ref(pts, [1, 2, 3, 4, 5], voxel_size=-1.0)


def test_min_votes_and_tiny_inputs():
    from pagnerf_amd import label_table_reference
    p = [[0.1, 0.1, 0.1]] * 3 + [[-0.6, 0.1, 0.1]] * 2 + [[0.6, 0.6, 0.6]]
    ids = [1, 1, 2, 3, 3, 4]
    assert _ref(p, ids, voxel_size=0.5)["count"].tolist() == [2, 3, 1]
    assert _ref(p, ids, voxel_size=0.5, min_votes=2)["instances"].tolist() == [3, 1]
    assert _ref(p, ids, voxel_size=0.5, min_votes=3)["count"].tolist() == [3] and _ref(p, ids, voxel_size=0.5, min_votes=4)["count"].numel() == 0
    empty = _ref(torch.zeros(0, 3), torch.zeros(0), torch.zeros(0, 3), voxel_size=0.5)
    assert empty["points"].shape == (0, 3) and empty["color"].shape == (0, 3) and empty["voxels"].shape == (0, 3) and empty["instances"].dtype == torch.int64
    assert empty["count"].dtype == torch.int32 and label_table_reference(empty)["centroid"].shape == (0, 3)
    one = _ref([[0.3, -0.2, 0.9]], [-7], [[0.5, 0.25, 1.0]], voxel_size=0.5)
    assert torch.equal(one["points"], torch.tensor([[0.3, -0.2, 0.9]])) and torch.equal(one["color"], torch.tensor([[0.5, 0.25, 1.0]]))
    assert one["voxels"].tolist() == [[2, 1, 3]] and one["agreement"].tolist() == [1.0]
    t = label_table_reference(one)
    assert t["ids"].tolist() == [-7] and torch.equal(t["bbox_min"], t["bbox_max"]) and torch.equal(t["centroid"], one["points"])


# ----------------------------------------------------------------------------------------------- entry points without a device
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib
    return _lib.load()


def test_voxel_entry_points_refuse_bad_arguments(lib):
    buf = (ctypes.c_float * 64)()
    f3 = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    cnt = (ctypes.c_int64 * 1)()
    ign = (ctypes.c_int64 * 1)(0)
    big = 1 << 40
    assert lib.pag_voxel_workspace_bytes(0) == 0 and lib.pag_voxel_workspace_bytes(-3) == 0 and lib.pag_voxel_workspace_bytes((1 << 31) + 1) == 0
    assert lib.pag_voxel_workspace_bytes(20000) >= (20000 + 255) // 256 * 12

    def keys(n=4, points=buf, origin=f3, v=0.5, out=buf):
        return lib.pag_voxel_keys(points, n, origin, v, None, out, None)
    assert keys(n=0) == 0 and keys(n=0, points=None, out=None) == 0
    assert keys(n=-1) == -1 and keys(n=(1 << 31) + 1) == -1
    assert keys(v=0.0) == -1 and b"voxel_size" in lib.pag_last_error_string()
    assert keys(v=-0.5) == -1 and keys(v=float("nan")) == -1 and keys(v=float("inf")) == -1 and keys(n=0, v=0.0) == -1
    assert keys(points=None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert keys(out=None) == -1 and keys(origin=None) == -1

    def fuse(n=4, k=buf, ids=buf, points=buf, color=buf, votes=1, out=buf, color_out=buf, cap=4, count=cnt, ws=buf, ws_bytes=big):
        return lib.pag_voxel_fuse(k, ids, points, color, n, votes, out, color_out, out, out, out, out, cap, count, ws, ws_bytes, None)
    assert fuse(n=0) == 0 and fuse(n=0, k=None, ids=None, points=None, color=None, out=None, color_out=None, count=None, ws=None, ws_bytes=0) == 0
    assert fuse(n=-1) == -1 and fuse(cap=-1) == -1 and fuse(votes=0) == -1 and b"min_votes" in lib.pag_last_error_string()
    assert fuse(k=None) == -1 and fuse(ids=None) == -1 and fuse(points=None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert fuse(out=None) == -1 and fuse(count=None) == -1 and fuse(color_out=None) == -1
    assert fuse(ws=None) == -1 and fuse(ws_bytes=8) == -1 and b"workspace" in lib.pag_last_error_string()

    def table(n=4, labels=buf, points=buf, color=buf, vc=buf, ignore=ign, n_ignore=1, out=buf, color_out=buf, cap=4, count=cnt, ws=buf, ws_bytes=big):
        return lib.pag_label_table(labels, points, color, vc, n, ignore, n_ignore, out, out, out, out, out, out, color_out, cap, count, ws, ws_bytes, None)
    assert table(n=0) == 0 and table(n=0, labels=None, points=None, color=None, vc=None, out=None, color_out=None, count=None, ws=None, ws_bytes=0) == 0
    assert table(n=-1) == -1 and table(cap=-1) == -1
    assert table(n_ignore=9) == -1 and b"ignored" in lib.pag_last_error_string() and table(n_ignore=-1) == -1 and table(ignore=None) == -1
    assert table(labels=None) == -1 and table(points=None) == -1 and table(vc=None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert table(out=None) == -1 and table(count=None) == -1 and table(color_out=None) == -1
    assert table(ws=None) == -1 and table(ws_bytes=8) == -1 and b"workspace" in lib.pag_last_error_string()


def test_voxel_ops_refuse_cpu_tensors():
    from pagnerf_amd import VoxelMap, instance_table, ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.voxel_keys(torch.zeros(4, 3), (-1.0, -1.0, -1.0), 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        VoxelMap(0.5, device="cpu").add(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        VoxelMap(0.0)
    assert instance_table(_ref(torch.zeros(0, 3), torch.zeros(0), voxel_size=0.5), device="cpu")["ids"].numel() == 0


# ----------------------------------------------------------------------------------------------- writers
def _old_ply_bytes(data):
    """save_map's PLY as it was written before the fused map existed, restated."""
    pts = np.concatenate([np.asarray(d["points"], dtype="<f4").reshape(-1, 3) for d in data], 0)
    ids = np.concatenate([np.asarray(d["inst_embedding"] if "inst_embedding" in d else d["instances"]).reshape(-1) for d in data], 0)
    has_color = all("color" in d for d in data)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else []) + [("instance", "<i4")]
    v = np.empty(pts.shape[0], dtype=fields)
    v["x"], v["y"], v["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if has_color:
        col = np.concatenate([np.asarray(d["color"], dtype=np.float32).reshape(-1, 3) for d in data], 0)
        col = np.rint(np.clip(np.nan_to_num(col), 0.0, 1.0) * 255.0).astype(np.uint8)
        v["red"], v["green"], v["blue"] = col[:, 0], col[:, 1], col[:, 2]
    v["instance"] = ids.astype("<i4")
    names = {"<f4": "float", "u1": "uchar", "<i4": "int"}
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % pts.shape[0]
    header += "".join("property %s %s\n" % (names[t], n) for n, t in fields) + "end_header\n"
    return header.encode("ascii") + v.tobytes()


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[2].startswith("element vertex ")
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    fields = [(l.split()[2], types[l.split()[1]]) for l in lines[3:]]
    v = np.frombuffer(body, dtype=fields)
    assert v.shape == (int(lines[2].split()[2]),)
    return v


def test_save_map_ply_with_and_without_the_fused_properties(tmp_path):
    from pagnerf_amd import fuse_map, save_map
    cloud, _ = C.exact_case("ties_300")
    data = [{"points": cloud["points"], "inst_embedding": cloud["ids"] % 1000, "color": cloud["color"], "name": "nerf_pc"}]
    dense = [{"name": "nerf_pc", "points": cloud["points"][:50], "instances": cloud["ids"][:50] % 1000}]
    for old in (data, dense, data + data):                                                 # today's dicts: byte for byte what they were
        assert open(save_map(old, tmp_path / "old.ply"), "rb").read() == _old_ply_bytes(old)
    for entries in (data, dense):
        fused = fuse_map(entries, cloud["voxel_size"], device="cpu")
        v = _read_ply(save_map([fused], tmp_path / "fused.ply"))
        want = ["x", "y", "z"] + (["red", "green", "blue"] if "color" in fused else []) + ["instance", "count", "agreement"]
        assert list(v.dtype.names) == want and v.shape[0] == fused["count"].numel() > 0
        assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), fused["points"].numpy())
        assert np.array_equal(v["instance"], fused["instances"].numpy()) and np.array_equal(v["count"], fused["count"].numpy())
        assert v["agreement"].tobytes() == fused["agreement"].numpy().tobytes()
        if "color" in fused:
            assert np.array_equal(v["red"], np.rint(fused["color"].numpy()[:, 0] * 255.0).astype(np.uint8))
        back = pickle.load(open(save_map([fused], tmp_path / "fused.pkl"), "rb"))
        assert back[0]["name"] == "nerf_pc_fused" and torch.equal(back[0]["agreement"], fused["agreement"])


def test_instance_table_csv_round_trip(tmp_path):
    from pagnerf_amd import label_table_reference, save_instance_table
    for color in (True, False):
        table = label_table_reference(C.exact_table_map([3, 1, 7, 2, 30], 5, color=color), ignore=())
        rows = list(csv.reader(open(save_instance_table(table, tmp_path / "t.csv"), newline="")))
        head = ["id", "voxels", "observations", "volume"] + ["%s_%s" % (s, a) for s in ("centroid", "min", "max") for a in "xyz"]
        assert rows[0] == head + (["red", "green", "blue"] if color else []) and len(rows) == 1 + 5
        body = np.array([[float(x) for x in r] for r in rows[1:]])
        assert [int(r[0]) for r in rows[1:]] == table["ids"].tolist() == [-6, -3, 0, 3, 6]
        assert [int(r[1]) for r in rows[1:]] == [3, 1, 7, 2, 30] and [int(r[2]) for r in rows[1:]] == table["observations"].tolist()
        assert np.array_equal(body[:, 3], table["volume"].numpy())
        for j, k in enumerate(("centroid", "bbox_min", "bbox_max") + (("color",) if color else ())):
            assert np.array_equal(body[:, 4 + 3 * j:7 + 3 * j].astype(np.float32), table[k].numpy()), k


def test_fuse_map_on_a_list_equals_the_reference_on_the_concatenation(tmp_path):
    from pagnerf_amd import fuse_map, instance_table, label_table_reference, map_export, save_map
    a, _ = C.exact_case("ties_300")
    b = C.random_cloud(K=400, cells=4, seed=3)
    views = {"points": a["points"], "inst_embedding": a["ids"], "color": a["color"], "name": "nerf_pc"}
    dense = {"points": b["points"].numpy(), "instances": b["ids"].numpy(), "name": "window_2"}     # what generate_pc_map holds; arrays are read too
    kw = dict(origin=(-1.0, -1.0, -1.25), min_votes=2, limits=[[-0.9, -0.9, -0.9], [0.9, 0.9, 0.9]])
    fused = fuse_map([views, dense], 0.125, device="cpu", **kw)
    want = _ref(torch.cat([a["points"], b["points"]]), torch.cat([a["ids"], b["ids"]]), voxel_size=0.125, **kw)
    assert "color" not in fused and fused["name"] == "nerf_pc_fused" and fused["voxel_size"] == 0.125
    C.assert_same(fused, want, C.FUSED_KEYS)
    both = fuse_map([views, dict(views, points=views["points"] * 0.5)], 0.125, device="cpu", name="x")
    want = _ref(torch.cat([a["points"], a["points"] * 0.5]), torch.cat([a["ids"]] * 2), torch.cat([a["color"]] * 2), voxel_size=0.125)
    C.assert_same(both, want, C.FUSED_KEYS)
    assert both["name"] == "x" and 0 < both["count"].numel() < 2 * a["ids"].numel()
    C.assert_same(instance_table(both, device="cpu"), label_table_reference(both), C.TABLE_KEYS)
    # the command line on pickled map files, the tensor-op definition selected
    p1, p2 = save_map([views], tmp_path / "a.pkl"), save_map([dict(views, points=views["points"] * 0.5)], tmp_path / "b.pkl")
    assert map_export.main(["fuse", p1, p2, "--voxel-size", "0.125", "--out", str(tmp_path / "o.pkl"), "--table", str(tmp_path / "o.csv"),
                            "--device", "cpu"]) == 0
    back = pickle.load(open(tmp_path / "o.pkl", "rb"))
    C.assert_same(back[0], want, C.FUSED_KEYS)
    assert len(list(csv.reader(open(tmp_path / "o.csv", newline="")))) == 1 + label_table_reference(both)["ids"].numel()
