"""CPU checks of the map merge (pagnerf_amd/map_export.py: overlap_table / associate_maps / merge_maps and their *_reference definitions): the
definitions against a second form over dicts and sets and against results written down by hand, the assignment against exhaustive search, the
`merge` command line, the unchanged `fuse` files, and the argument validation of the new entry points without a device."""
import csv
import ctypes
import pickle

import numpy as np
import pytest
import torch

import map_components_cases as C
import map_merge_cases as M


def _ids(out, i, j):
    return out["ids_a"].tolist().index(i), out["ids_b"].tolist().index(j)


@pytest.mark.parametrize("name", M.PAIRS + ["many_257"])
def test_the_association_equals_the_second_form_and_the_hand_results(name):
    from pagnerf_amd import associate_maps, associate_maps_reference, overlap_table_reference
    a, b, kw = M.pair(name)
    ignore = (0,)
    out = associate_maps_reference(a, b, **kw)
    ids_a, ids_b, shared = M.brute_table(a, b)
    assert out["ids_a"].tolist() == ids_a and out["ids_b"].tolist() == ids_b and out["table"].dtype == torch.int64
    assert {(ids_a[i], ids_b[j]): int(out["table"][i, j]) for i in range(len(ids_a)) for j in range(len(ids_b)) if out["table"][i, j]} == shared
    table = overlap_table_reference(a, b)
    assert torch.equal(table["table"], out["table"]) and table["shared"] == sum(shared.values())
    iou = M.brute_iou(ids_a, ids_b, shared)
    assert out["iou"].dtype == torch.float32 and out["iou"].shape == (len(ids_a), len(ids_b))
    assert all(out["iou"][i, j].numpy().view(np.int32) == iou[(x, y)].view(np.int32) for i, x in enumerate(ids_a) for j, y in enumerate(ids_b))
    # the pairs: matched entries only, one to one, above the bound; the mapping follows from them
    pairs = [tuple(p) for p in out["pairs"].tolist()]
    assert pairs == sorted(pairs) and len({p[0] for p in pairs}) == len(pairs) == len({p[1] for p in pairs})
    bound = np.float32(kw.get("min_iou", 0.25))
    assert all(shared.get(p, 0) > 0 and iou[p] >= bound and p[0] not in ignore and p[1] not in ignore for p in pairs)
    partner = {j: i for i, j in pairs}
    fresh = max(ids_a + ids_b + [0])
    for j, new in zip(ids_b, out["mapping"].tolist()):
        if j in partner:
            assert new == partner[j]
        elif j in ignore:
            assert new == j
        else:
            fresh += 1
            assert new == fresh
    want = M.EXPECT.get(name, {})
    if "pairs" in want:
        assert pairs == want["pairs"] and out["mapping"].tolist() == want["mapping"]
    if "shared" in want:
        assert table["shared"] == want["shared"]
    for i, j, n in want.get("entries", ()):
        assert int(out["table"][_ids(out, i, j)]) == n
    if "iou_of_pairs" in want:
        assert all(float(out["iou"][_ids(out, *p)]) == want["iou_of_pairs"] for p in pairs)
    # the assignment is optimal: its total cost over ALL assigned pairs (matched or not) is the exhaustive minimum
    best, act_a, act_b = M.brute_best_cost(ids_a, ids_b, shared, iou, ignore)
    if best is not None and max(len(act_a), len(act_b)) <= 6:
        from scipy.optimize import linear_sum_assignment
        cost = np.array([[np.float32(1.0) - iou[(i, j)] for j in act_b] for i in act_a], np.float64)
        rows, cols = linear_sum_assignment(cost)
        assert cost[rows, cols].sum() == best
        assigned = {(act_a[r], act_b[c]) for r, c in zip(rows, cols)}
        assert set(pairs) == {p for p in assigned if shared.get(p, 0) > 0 and iou[p] >= bound}
    got = associate_maps(a, b, device="cpu", **kw)                                         # the public form with device="cpu" is the definition
    C.assert_same(got, out, M.RESULT_KEYS, name)


def test_the_named_cases_say_what_they_are_meant_to():
    from pagnerf_amd import associate_maps_reference
    out = associate_maps_reference(*M.pair("one_over_two")[:2])
    assert float(out["iou"][_ids(out, 1, 3)]) == 0.75 and float(out["iou"][_ids(out, 1, 4)]) == 0.25     # the smaller half is at the bound and still loses
    a, b, kw = M.pair("background")
    out = associate_maps_reference(a, b, **kw)
    i, j = _ids(out, 1, 2)
    assert float(out["iou"][i, j]) == np.float32(3) / np.float32(10) and int(out["table"][i].sum()) == 10      # 3 / 3 = 1 without the background
    assert out["pairs"].shape == (0, 2) and out["pairs"].dtype == torch.int64
    a, b, kw = M.pair("threshold")
    out = associate_maps_reference(a, b, **kw)
    assert float(out["iou"][_ids(out, 1, 3)]) == 0.5 and float(out["iou"][_ids(out, 2, 4)]) == np.float32(1) / np.float32(3)
    assert associate_maps_reference(a, b, min_iou=0.3)["pairs"].tolist() == [[1, 3], [2, 4]]
    for name in ("equal_iou", "equal_iou_mirrored"):
        out = associate_maps_reference(*M.pair(name)[:2])
        assert out["iou"].flatten().tolist() == [0.5, 0.5] and out["pairs"].shape == (1, 2)
    assert associate_maps_reference(*M.pair("five_by_two")[:2])["table"].shape == (5, 2)
    out = associate_maps_reference(*M.pair("many_257")[:2])
    assert out["pairs"].shape == (257, 2) and out["mapping"].tolist() == list(range(257, 0, -1))
    out = associate_maps_reference(*M.pair("wave_pairs")[:2])
    assert out["pairs"].shape[0] == 64 + 2 + 1 + 3 + 7 + 16 + 33 and int(out["table"].sum()) == 512


def test_ignored_ids_and_argument_checks():
    from pagnerf_amd import associate_maps_reference, merge_maps, relabel_map
    a, b, _ = M.pair("signed_ids")
    out = associate_maps_reference(a, b, ignore=(0, 7))                                    # 7 is ignored on both sides: BIG of a and -3 of b lose their partners
    assert out["pairs"].tolist() == [[-3, M.BIG]] and out["mapping"].tolist() == [M.BIG + 1, M.BIG + 2, 0, M.BIG + 3, 7, -3]
    out = associate_maps_reference(a, b, ignore=())
    assert [0, 0] in out["pairs"].tolist()
    with pytest.raises(ValueError, match="min_iou"):
        associate_maps_reference(a, b, min_iou=1.5)
    with pytest.raises(ValueError, match="ignored"):
        associate_maps_reference(a, b, ignore=tuple(range(9)))
    with pytest.raises(ValueError, match="mapping"):
        merge_maps(a, b, mapping=torch.tensor([1, 2]), device="cpu")
    moved = relabel_map(b, out["ids_b"], out["ids_b"] + 100)
    assert torch.equal(moved["instances"], b["instances"] + 100) and moved["points"] is b["points"]
    with pytest.raises(ValueError, match="missing"):
        relabel_map(b, out["ids_b"][1:], out["ids_b"][1:])


def test_broken_contracts_raise_with_their_cause():
    from pagnerf_amd import associate_maps, merge_maps, overlap_table
    for name, (a, b, text) in M.contract_pairs().items():
        for fn in (overlap_table, associate_maps, merge_maps):
            with pytest.raises(ValueError, match=text):
                fn(a, b, device="cpu")


def _new_ids(out):
    return dict(zip(out["ids_b"].tolist(), out["mapping"].tolist()))


@pytest.mark.parametrize("name", M.PAIRS)
def test_the_merge_equals_the_second_form(name):
    from pagnerf_amd import associate_maps_reference, merge_maps_reference
    a, b, kw = M.pair(name)
    got = merge_maps_reference(a, b, **kw)
    rows = M.brute_merge(a, b, _new_ids(associate_maps_reference(a, b, **kw)))
    M.assert_rows(got, rows, name)
    assert bool((np.diff(C.key_of(got["voxels"].numpy())) > 0).all()) and got["voxel_size"] == a["voxel_size"] and torch.equal(got["origin"], a["origin"])
    if name == "disjoint":                                                                 # the plain union: every row of either map, bit for bit
        assert got["count"].numel() == a["count"].numel() + b["count"].numel()
        assert sorted(got["points"].flatten().tolist()) == sorted(torch.cat((a["points"], b["points"])).flatten().tolist())


@pytest.mark.parametrize("color_a,color_b,component", [(True, True, False), (True, False, False), (False, True, True), (True, True, True)])
def test_the_merge_cases_by_hand(color_a, color_b, component):
    from pagnerf_amd import merge_maps, merge_maps_reference
    a, b, mapping, want = M.merge_case(color_a, color_b, component)
    got = merge_maps_reference(a, b, mapping)
    assert got["instances"].tolist() == want["instances"] and got["count"].tolist() == want["count"]
    assert torch.equal(got["agreement"], torch.tensor(want["votes"], dtype=torch.float32) / torch.tensor(want["count"], dtype=torch.float32))
    assert ("color" in got) == (color_a and color_b) and "component" not in got
    M.assert_rows(got, M.brute_merge(a, b, {0: 0, 3: 3, 4: 4}), "merge case")
    # singles are copied bit for bit, rows of both maps are not
    assert torch.equal(got["points"][:4], a["points"][:4]) and torch.equal(got["points"][-3:], b["points"][-3:])
    assert not torch.equal(got["points"][4:10], a["points"][4:10]) and torch.equal(got["voxels"][4:10], a["voxels"][4:10])
    C.assert_same(merge_maps(a, b, mapping, device="cpu"), got, M.MERGED_KEYS)
    swapped = merge_maps_reference(a, b, torch.tensor([0, 4, 3]))                          # b's 3 and 4 change places: row 0 goes to b's 5 votes, the votes add on rows 1, 2 and 4
    assert swapped["instances"].tolist()[4:10] == [4, 3, 3, 3, 3, 0] and swapped["agreement"][5] == torch.tensor(6.0) / torch.tensor(7.0)


def test_three_windows_in_a_chain_share_one_id():
    from pagnerf_amd import merge_map_sequence, merge_map_sequence_reference, merge_maps_reference
    maps = M.chain()
    got = merge_map_sequence_reference(maps)
    column = got["voxels"][:, 0] == 3
    assert int(column.sum()) == 22 and got["instances"][column].unique().tolist() == [2]   # w1's id runs through all three windows
    assert sorted(got["instances"].unique().tolist()) == [2, 5, 8, 9] and got["count"].numel() == 22 + 4 + 4 + 3
    C.assert_same(got, merge_maps_reference(merge_maps_reference(maps[0], maps[1]), maps[2]), M.MERGED_KEYS)
    C.assert_same(merge_map_sequence(maps, device="cpu"), got, M.MERGED_KEYS)
    assert "component" not in merge_map_sequence_reference([dict(maps[0], component=torch.zeros(14, dtype=torch.int64))])
    with pytest.raises(ValueError, match="no map"):
        merge_map_sequence_reference([])


def frame_clouds():
    """Case 22: the same 40 lattice points in two frames: the second cloud is the first scaled by 1/2 and moved, so (2, offset) brings it back exactly."""
    vox = C.blob((3, 5, 2), (5, 4, 2))
    p = torch.from_numpy(((vox + 0.5) * (2.0 / 32) - 1.0).astype(np.float32))
    offset = (0.25, -0.5, 0.125)
    q = (p - torch.tensor(offset)) * 0.5                                                   # exact in fp32: dyadic values
    ids = torch.from_numpy(np.where(vox[:, 0] < 5, 1, 2))
    col = torch.from_numpy((np.arange(vox.size).reshape(-1, 3) % 257 / 256.0).astype(np.float32))
    return [{"points": p, "inst_embedding": ids, "color": col}, {"points": q, "inst_embedding": ids, "color": col}], [(1.0, (0.0, 0.0, 0.0)), (2.0, offset)]


def test_frames_bring_two_clouds_onto_the_same_voxels():
    from pagnerf_amd import fuse_map
    data, frames = frame_clouds()
    fused = fuse_map(data, 2.0 / 32, device="cpu", frames=frames)
    assert fused["count"].tolist() == [2] * 40 and torch.equal(fused["points"], fuse_map(data[:1], 2.0 / 32, device="cpu")["points"])
    apart = fuse_map(data, 2.0 / 32, device="cpu")
    assert apart["count"].numel() > 40
    same = fuse_map(data, 2.0 / 32, device="cpu", frames=None)
    C.assert_same(same, apart, C.MAP_KEYS)
    with pytest.raises(ValueError, match="frames"):
        fuse_map(data, 2.0 / 32, device="cpu", frames=frames[:1])


# ----------------------------------------------------------------------------------------------- the command line
def _window_clouds():
    """Two raw exports on the 2/64 lattice: the chain's first two windows as points at the voxel centres, every third point twice."""
    out = []
    for m in M.chain()[:2]:
        vox, ids = m["voxels"].numpy().astype(np.int64), m["instances"].numpy()
        vox, ids = np.concatenate([vox, vox[::3]]), np.concatenate([ids, ids[::3]])
        out.append([{"points": torch.from_numpy(((vox + 0.5) * (2.0 / 64) - 1.0).astype(np.float32)), "inst_embedding": torch.from_numpy(ids), "name": "nerf_pc"}])
    return out


def test_merge_command_round_trip(tmp_path):
    from pagnerf_amd import associate_maps_reference, fuse_map, label_table_reference, map_export, merge_maps_reference, save_map
    clouds = _window_clouds()
    raw = [save_map(c, tmp_path / ("w%d.pkl" % n)) for n, c in enumerate(clouds)]
    fused = [fuse_map(c, 2.0 / 64, device="cpu") for c in clouds]
    want = merge_maps_reference(*fused)
    base = ["merge"] + raw + ["--voxel-size", str(2.0 / 64), "--device", "cpu"]
    assert map_export.main(base + ["--out", str(tmp_path / "m.pkl"), "--pairs", str(tmp_path / "p.csv"), "--table", str(tmp_path / "t.csv")]) == 0
    back = pickle.load(open(tmp_path / "m.pkl", "rb"))
    assert len(back) == 1 and back[0]["name"] == "nerf_pc_merged"
    C.assert_same(back[0], want, M.MERGED_KEYS)
    found = associate_maps_reference(*fused)
    rows = list(csv.reader(open(tmp_path / "p.csv", newline="")))
    assert rows[0] == ["step", "id_a", "id_b", "shared_voxels", "iou"] and rows[1:] == [["1", "2", "7", "4", "1.0"]] and found["pairs"].tolist() == [[2, 7]]
    assert open(tmp_path / "t.csv", newline="").read() == _table_csv_text_no_color(label_table_reference(want))
    # fused inputs give the same map; a .ply is written; cleaning flags are taken
    one = save_map([fused[0]], tmp_path / "f0.pkl")
    assert map_export.main(["merge", one, raw[1], "--voxel-size", str(2.0 / 64), "--device", "cpu", "--out", str(tmp_path / "n.pkl")]) == 0
    C.assert_same(pickle.load(open(tmp_path / "n.pkl", "rb"))[0], want, M.MERGED_KEYS)
    flags = ["--min-component", "2", "--split", "split", "--min-iou", "0.5", "--ignore", "0", "5"]
    assert map_export.main(base + flags + ["--out", str(tmp_path / "c.ply")]) == 0
    from test_voxel_map_host import _read_ply
    v = _read_ply(tmp_path / "c.ply")
    assert "component" not in v.dtype.names and v.shape[0] == want["count"].numel()
    with pytest.raises(SystemExit):
        map_export.main(["merge"] + raw + ["--device", "cpu", "--out", str(tmp_path / "x.pkl")])               # a raw export without --voxel-size
    with pytest.raises(SystemExit):
        map_export.main(base + ["--frame", "1", "0", "0", "0", "--out", str(tmp_path / "x.pkl")])                # one frame for two inputs
    shifted = ["--frame", "1", "0", "0", "0", "--frame", "1", "0", "0", str(6 * 2.0 / 64)]                    # the second window moved 6 voxels up
    assert map_export.main(base + shifted + ["--out", str(tmp_path / "s.pkl")]) == 0
    assert pickle.load(open(tmp_path / "s.pkl", "rb"))[0]["count"].numel() == 28 > want["count"].numel()           # nothing is shared any more


def _table_csv_text_no_color(t):
    head = ["id", "voxels", "observations", "volume"] + ["%s_%s" % (s, a) for s in ("centroid", "min", "max") for a in "xyz"]
    lines = [",".join(head)]
    for r in range(t["ids"].numel()):
        row = [t["ids"][r], t["voxels"][r], t["observations"][r], t["volume"][r]] + [t[k][r, j] for k in ("centroid", "bbox_min", "bbox_max") for j in range(3)]
        lines.append(",".join(repr(v.item()) for v in row))
    return "\r\n".join(lines) + "\r\n"


def test_the_fuse_command_writes_the_files_it_wrote_before(tmp_path):
    """`fuse` on one input, through the command line that now also knows `merge`, against the restatement of the files as they were."""
    from pagnerf_amd import fuse_map, label_table_reference, map_export, save_map
    from test_map_components_host import _cloud_of_the_clean_case, _fused_ply_bytes, _table_csv_text
    src = save_map(_cloud_of_the_clean_case(), tmp_path / "nerf_pc.pkl")
    fused = fuse_map(_cloud_of_the_clean_case(), 2.0 / 64, device="cpu")
    assert map_export.main(["fuse", src, "--voxel-size", str(2.0 / 64), "--device", "cpu", "--out", str(tmp_path / "o.ply"), "--table", str(tmp_path / "o.csv")]) == 0
    assert open(tmp_path / "o.ply", "rb").read() == _fused_ply_bytes(fused)
    assert open(tmp_path / "o.csv", newline="").read() == _table_csv_text(label_table_reference(fused))
    assert map_export.main(["fuse", src, "--voxel-size", str(2.0 / 64), "--device", "cpu", "--out", str(tmp_path / "o.pkl")]) == 0
    back = pickle.load(open(tmp_path / "o.pkl", "rb"))
    assert sorted(back[0]) == sorted(fused) and all(torch.equal(back[0][k], fused[k]) for k in C.MAP_KEYS if k in fused)


# ----------------------------------------------------------------------------------------------- the entry points without a device
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib
    return _lib.load()


def test_merge_entry_points_refuse_bad_arguments(lib):
    buf = (ctypes.c_int64 * 64)()
    err = lib.pag_last_error_string

    def overlap(na=4, nb=4, Ta=2, Tb=2, va=buf, ia=buf, ua=buf, vb=buf, ib=buf, ub=buf, ka=buf, sa=buf, kb=buf, sb=buf, table=buf, status=buf):
        return lib.pag_voxel_overlap(va, ia, na, ua, Ta, vb, ib, nb, ub, Tb, 1, ka, sa, kb, sb, table, status, None)
    assert overlap(na=-1) == -1 and b"rows" in err() and overlap(na=1 << 30, nb=1 << 30) == -1
    assert overlap(Ta=5) == -1 and b"Ta" in err() and overlap(Tb=-1) == -1 and overlap(na=1 << 20, nb=1 << 20, Ta=1 << 16, Tb=1 << 16) == -1
    assert overlap(status=None) == -1 and b"status" in err()
    for k in ("va", "ia", "ua", "ka", "sa", "vb", "ib", "ub", "kb", "sb"):
        assert overlap(**{k: None}) == -1 and b"NULL" in err(), k
    assert overlap(Ta=0) == -1 and overlap(table=None) == -1 and b"table" in err()

    def cost(Ta=3, Tb=4, n_a=2, n_b=2, table=buf, rs=buf, cs=buf, aa=buf, ab=buf, iou=buf, out=buf):
        return lib.pag_overlap_cost(table, rs, cs, Ta, Tb, aa, n_a, ab, n_b, iou, out, None)
    assert cost(Ta=0, n_a=0) == 0 and cost(Ta=0, n_a=0, table=None, rs=None, cs=None, aa=None, ab=None, iou=None, out=None) == 0
    assert cost(Ta=-1) == -1 and b"Ta" in err() and cost(Ta=1 << 16, Tb=1 << 16) == -1
    assert cost(n_a=4) == -1 and b"active" in err() and cost(n_b=-1) == -1
    assert cost(table=None) == -1 and cost(rs=None) == -1 and cost(cs=None) == -1 and cost(iou=None) == -1 and b"NULL" in err()
    assert cost(aa=None) == -1 and cost(ab=None) == -1 and cost(out=None) == -1 and b"NULL" in err()

    big = 1 << 40
    names = ("keys", "order", "pa", "ca", "ia", "na_", "aa", "va", "pb", "cb", "sb", "mp", "nb_", "ab", "vb", "po", "co", "io", "no", "ao", "vo", "count", "status", "ws")

    def merge(na=4, nb=4, Tb=2, cap=8, ws_bytes=big, **kw):
        p = {k: kw.get(k, buf) for k in names}
        return lib.pag_voxel_merge(p["keys"], p["order"], na, nb, p["pa"], p["ca"], p["ia"], p["na_"], p["aa"], p["va"], p["pb"], p["cb"], p["sb"], p["mp"], Tb,
                                   p["nb_"], p["ab"], p["vb"], p["po"], p["co"], p["io"], p["no"], p["ao"], p["vo"], cap, p["count"], p["status"], p["ws"],
                                   ws_bytes, None)
    assert merge(na=0, nb=0, Tb=0) == 0 and merge(na=0, nb=0, Tb=0, **{k: None for k in names}) == 0
    assert merge(na=-1) == -1 and b"rows" in err() and merge(na=1 << 30, nb=1 << 30) == -1 and merge(cap=-1) == -1 and merge(Tb=5) == -1
    for k in ("keys", "order", "count", "status", "pa", "ia", "na_", "aa", "va", "pb", "sb", "mp", "nb_", "ab", "vb", "po", "io", "no", "ao", "vo"):
        assert merge(**{k: None}) == -1 and b"NULL" in err(), k
    assert merge(ca=None) == -1 and b"colour" in err() and merge(cb=None) == -1
    assert merge(ws=None) == -1 and b"workspace" in err() and merge(ws_bytes=lib.pag_voxel_workspace_bytes(8) - 1) == -1


def test_merge_ops_refuse_cpu_tensors():
    from pagnerf_amd import ops
    z = lambda *s, d=torch.int64: torch.zeros(*s, dtype=d)                                  # noqa: E731
    with pytest.raises(RuntimeError, match="GPU"):
        ops.voxel_overlap(z(4, 3, d=torch.int32), z(4), z(1), z(4, 3, d=torch.int32), z(4), z(1), z(1, d=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.overlap_cost(z(2, 2, d=torch.int32), z(2), z(2), z(1, d=torch.int32), z(1, d=torch.int32))
