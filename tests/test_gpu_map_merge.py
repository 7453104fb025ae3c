"""GPU checks of the map merge (pagnerf_amd/map_export.py on csrc/voxelmap.hip: pag_voxel_overlap / pag_overlap_cost / pag_voxel_merge, and
pag_assign_solve) against the CPU definitions on the shared cases.  Every float operation is specified with its order: all comparisons are for
equality, integers equal and floats bit for bit."""
import warnings

import numpy as np
import pytest
import torch

import map_components_cases as C
import map_merge_cases as M

pytestmark = pytest.mark.gpu

_REFERENCES = {}


def _reference(name):
    """The definitions' results of a pair, computed once and shared."""
    from pagnerf_amd import associate_maps_reference, merge_maps_reference, overlap_table_reference
    if name not in _REFERENCES:
        a, b, kw = M.pair(name)
        _REFERENCES[name] = (a, b, kw, overlap_table_reference(a, b), associate_maps_reference(a, b, **kw), merge_maps_reference(a, b, **kw))
    return _REFERENCES[name]


def _to(m, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in m.items()}


def _bits_equal(got, want, keys, what):
    C.assert_same(got, want, keys, what)
    for k in keys:                                                                         # torch.equal holds -0.0 == 0.0: compare the bits as well
        if k in want and want[k].dtype == torch.float32:
            assert torch.equal(got[k].cpu().view(torch.int32), want[k].view(torch.int32)), (what, k)


@pytest.mark.parametrize("name", M.PAIRS)
def test_table_association_and_merge_equal_the_definitions(gpu_device, name):
    from pagnerf_amd import associate_maps, merge_maps, overlap_table
    a, b, kw, table, found, merged = _reference(name)
    da, db = _to(a, gpu_device), _to(b, gpu_device)
    got = overlap_table(da, db)
    assert got["table"].is_cuda and got["shared"] == table["shared"]
    _bits_equal(got, table, ("ids_a", "ids_b", "table"), name)
    got = associate_maps(da, db, **kw)
    assert got["mapping"].is_cuda and got["pairs"].is_cuda
    _bits_equal(got, found, M.RESULT_KEYS, name)
    got = merge_maps(da, db, **kw)
    assert got["points"].is_cuda and got["voxel_size"] == a["voxel_size"]
    _bits_equal(got, merged, M.MERGED_KEYS, name)
    # CPU maps with the device named: the results come home
    home = associate_maps(a, b, device=gpu_device, **kw)
    assert not home["mapping"].is_cuda
    _bits_equal(home, found, M.RESULT_KEYS, name)
    home = merge_maps(a, b, device=gpu_device, **kw)
    assert not home["points"].is_cuda
    _bits_equal(home, merged, M.MERGED_KEYS, name)


@pytest.mark.parametrize("name", ["big_pair", "wave_pairs", "same_permuted"])
def test_two_runs_give_the_same_bits_with_and_without_the_combining(gpu_device, name):
    from pagnerf_amd import merge_maps, ops
    a, b, kw, table, found, merged = _reference(name)
    da, db = _to(a, gpu_device), _to(b, gpu_device)
    first, second = merge_maps(da, db, **kw), merge_maps(da, db, **kw)
    for k in M.MERGED_KEYS:
        if k in first:
            assert torch.equal(first[k], second[k]), k
    status = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    rows = (da["voxels"], da["instances"], da["instances"].unique(), db["voxels"], db["instances"], db["instances"].unique())
    for combine in (True, False, True):
        j = ops.voxel_overlap(*rows, status, combine=combine)
        assert torch.equal(j["table"].cpu().long(), table["table"]) and int(status) == 0, combine
    if name == "big_pair":
        assert int(j["table"].max()) == 4166 and int(j["table"].sum()) == 4166


def test_more_active_ids_than_the_device_solver_takes(gpu_device):
    from pagnerf_amd import associate_maps, merge_maps
    a, b, _ = M.pair("many_257")
    for fn in (associate_maps, merge_maps):
        with pytest.raises(ValueError, match='device="cpu"'):
            fn(_to(a, gpu_device), _to(b, gpu_device))
    out = associate_maps(_to(a, gpu_device), _to(b, gpu_device), device="cpu")              # the definition, and the result still lives with the map
    assert out["pairs"].is_cuda and out["pairs"].shape == (257, 2)


def test_ignore_sets_and_given_mappings(gpu_device):
    from pagnerf_amd import associate_maps, associate_maps_reference, merge_maps, merge_maps_reference
    a, b, _ = M.pair("signed_ids")
    for ignore in ((0, 7), (), (0,), (5, -8, 0)):
        _bits_equal(associate_maps(_to(a, gpu_device), _to(b, gpu_device), ignore=ignore), associate_maps_reference(a, b, ignore=ignore), M.RESULT_KEYS, ignore)
    a, b, kw = M.pair("threshold")
    for min_iou in (0.3, 0.5, 0.51, 0.0, 1.0):
        _bits_equal(associate_maps(a, b, min_iou=min_iou, device=gpu_device), associate_maps_reference(a, b, min_iou=min_iou), M.RESULT_KEYS, min_iou)
    for color_a, color_b, component in ((True, True, False), (True, False, False), (False, True, True), (True, True, True)):
        a, b, mapping, want = M.merge_case(color_a, color_b, component)
        for m in (mapping, torch.tensor([0, 4, 3])):
            got = merge_maps(_to(a, gpu_device), _to(b, gpu_device), mapping=m.to(gpu_device))
            _bits_equal(got, merge_maps_reference(a, b, m), M.MERGED_KEYS, (color_a, color_b, component))
            assert ("color" in got) == (color_a and color_b) and "component" not in got
        assert got["instances"].tolist()[4:10] == [4, 3, 3, 3, 3, 0]
    got = merge_maps(_to(a, gpu_device), _to(b, gpu_device), mapping=mapping)
    assert got["instances"].tolist() == want["instances"] and got["count"].tolist() == want["count"]
    with pytest.raises(RuntimeError, match="capacity >= 13"):
        merge_maps(_to(a, gpu_device), _to(b, gpu_device), mapping=mapping, capacity=12)
    with pytest.raises(ValueError, match="mapping"):
        merge_maps(_to(a, gpu_device), _to(b, gpu_device), mapping=torch.tensor([1, 2]))


def test_contract_violations_raise_through_the_status_word(gpu_device):
    """The rows are read as data: nothing is accessed out of range, the status word reports what was wrong."""
    from pagnerf_amd import associate_maps, merge_maps, overlap_table
    for name, (a, b, text) in M.contract_pairs().items():
        for fn in (overlap_table, associate_maps, merge_maps):
            with pytest.raises(ValueError, match=text):
                fn(_to(a, gpu_device), _to(b, gpu_device))
    a, b, kw, table, found, merged = _reference("window_cut")                              # the next call starts from a clean status word
    _bits_equal(merge_maps(_to(a, gpu_device), _to(b, gpu_device)), merged, M.MERGED_KEYS, "after")


def test_a_chain_of_three_windows(gpu_device):
    from pagnerf_amd import merge_map_sequence, merge_map_sequence_reference
    maps = M.chain()
    want = merge_map_sequence_reference(maps)
    got = merge_map_sequence([_to(m, gpu_device) for m in maps])
    assert got["instances"].is_cuda
    _bits_equal(got, want, M.MERGED_KEYS, "chain")
    _bits_equal(merge_map_sequence(maps, device=gpu_device), want, M.MERGED_KEYS, "chain, cpu maps")


def test_frames_on_the_device(gpu_device):
    from pagnerf_amd import VoxelMap, fuse_map
    from test_map_merge_host import frame_clouds
    data, frames = frame_clouds()
    want = fuse_map(data, 2.0 / 32, device="cpu", frames=frames)
    got = fuse_map(data, 2.0 / 32, device=gpu_device, frames=frames)
    assert got["count"].tolist() == [2] * 40
    C.assert_same(got, want, ("instances", "count", "agreement", "voxels", "points", "color"))
    C.assert_same(fuse_map(data, 2.0 / 32, device=gpu_device, frames=None), fuse_map(data, 2.0 / 32, device=gpu_device), C.MAP_KEYS)
    vm = VoxelMap(2.0 / 32, device=gpu_device)
    for d, (s, o) in zip(data, frames):
        vm.add(d["points"], d["inst_embedding"], d["color"], scale=s, offset=o)
    C.assert_same(_to(vm.finish(), "cpu"), want, ("instances", "count", "agreement", "voxels", "points", "color"))


def test_end_to_end_two_windows(gpu_device):
    """Points -> VoxelMap -> clean_map(split) -> associate_maps -> merge_maps -> instance_table on the device, and the same route through the CPU forms."""
    from pagnerf_amd import (VoxelMap, associate_maps, associate_maps_reference, clean_map, clean_map_reference, fuse_points_reference, instance_table,
                             label_table_reference, merge_maps, merge_maps_reference)
    parts = [(C.blob((x, 3, 3), (3, 3, 3)), i) for x, i in ((0, 1), (5, 1), (10, 2), (15, 3), (20, 4))] + [(C.blob((0, 8, 8), (24, 2, 1)), 0)]
    vox, ids = np.concatenate([v for v, _ in parts]), np.concatenate([np.full(v.shape[0], i) for v, i in parts])       # id 1 is used for two blobs
    size = 2.0 / 32
    windows = []
    for lo, hi, perm in ((0, 17, [0, 1, 2, 3, 4]), (8, 24, [0, 3, 4, 2, 1])):                 # the blob at x = 15 is cut by the first window
        keep = (vox[:, 0] >= lo) & (vox[:, 0] < hi)
        v, i = vox[keep], np.array(perm)[ids[keep]]
        v, i = np.concatenate([v, v[::2]]), np.concatenate([i, i[::2]])                    # every second voxel is seen twice
        windows.append((torch.from_numpy(((v + 0.5) * size - 1.0).astype(np.float32)), torch.from_numpy(i)))
    dev_maps = [clean_map(VoxelMap(size, device=gpu_device).add(p.to(gpu_device), i.to(gpu_device)).finish(), mode="split") for p, i in windows]
    cpu_maps = [clean_map_reference(fuse_points_reference(p, i, voxel_size=size), mode="split") for p, i in windows]
    for d, c in zip(dev_maps, cpu_maps):
        # a voxel holds one point or the same point twice: p / 1 and (p + p) / 2 are exact, so the means are equal bit for bit in either sum order
        C.assert_same(d, c, ("points", "instances", "count", "agreement", "voxels", "component"))
    found, want = associate_maps(*dev_maps), associate_maps_reference(*cpu_maps)
    _bits_equal(found, want, M.RESULT_KEYS, "end to end")
    assert found["pairs"].shape[0] == 2 and found["mapping"].numel() == 4
    merged, want = merge_maps(*dev_maps), merge_maps_reference(*cpu_maps)
    _bits_equal(merged, want, M.MERGED_KEYS, "end to end")
    table, want_table = instance_table(merged), label_table_reference(want)
    # the centroid is left to the instance table's own tests: it is an fp32 sum over many voxels in the kernel's order, not the definition's fp64 sum
    C.assert_same(table, want_table, ("ids", "voxels", "observations", "bbox_min", "bbox_max", "volume"))


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


def test_host_synchronisations_do_not_grow_with_the_map(gpu_device):
    """The counts torch's synchronisation debug mode reports for a map of 57 voxels and one of 4196 are the same; the launches alone report none."""
    from pagnerf_amd import associate_maps, merge_maps, ops
    counts = {}
    for name in ("window_cut", "big_pair"):
        a, b, kw, table, found, merged = _reference(name)
        da, db = _to(a, gpu_device), _to(b, gpu_device)
        associate_maps(da, db), merge_maps(da, db)                                          # warm up: allocator, library load
        _, s1 = _reported_syncs(lambda: associate_maps(da, db))
        _, s2 = _reported_syncs(lambda: merge_maps(da, db))
        _, s3 = _reported_syncs(lambda: merge_maps(da, db, mapping=found["mapping"].to(gpu_device)))
        counts[name] = (len(s1), len(s2), len(s3))
        print("synchronisations of associate_maps / merge_maps / merge_maps with a mapping on %s: %s" % (name, counts[name]))
    assert counts["window_cut"] == counts["big_pair"] and max(counts["big_pair"]) <= 12, counts
    ua, ub = da["instances"].unique(), db["instances"].unique()
    status = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        j = ops.voxel_overlap(da["voxels"], da["instances"], ua, db["voxels"], db["instances"], ub, status)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(j["table"].cpu().long(), table["table"])


def test_the_merge_command_on_the_device(gpu_device, tmp_path):
    import pickle
    from pagnerf_amd import fuse_map, map_export, merge_maps_reference, save_map
    from test_map_merge_host import _window_clouds
    clouds = _window_clouds()
    raw = [save_map(c, tmp_path / ("w%d.pkl" % n)) for n, c in enumerate(clouds)]
    want = merge_maps_reference(*[fuse_map(c, 2.0 / 64, device="cpu") for c in clouds])
    assert map_export.main(["merge"] + raw + ["--voxel-size", str(2.0 / 64), "--device", str(gpu_device), "--out", str(tmp_path / "m.pkl")]) == 0
    back = pickle.load(open(tmp_path / "m.pkl", "rb"))[0]
    assert not back["points"].is_cuda
    C.assert_same(back, want, ("instances", "count", "agreement", "voxels", "points"))
