"""GPU checks of the fused map's connected components (pagnerf_amd/map_export.py on csrc/voxelmap.hip: pag_voxel_components) against the CPU
definitions connected_components_reference / clean_map_reference on the same maps.  Every output is an integer or a selected row: all comparisons
are for equality."""
import warnings

import numpy as np
import pytest
import torch

import map_components_cases as C

pytestmark = pytest.mark.gpu

_REFERENCES = {}


def _reference(name):
    """The definition's result of a case, computed once and shared."""
    from pagnerf_amd import connected_components_reference
    if name not in _REFERENCES:
        m, kw = C.case(name)
        _REFERENCES[name] = (m, kw, connected_components_reference(m, **kw))
    return _REFERENCES[name]


def _to(m, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in m.items()}


def _same_components(got, want, what=""):
    assert got["components"] == want["components"], (what, got["components"], want["components"])
    assert got["component"].dtype == torch.int64 and torch.equal(got["component"].cpu(), want["component"]), what


@pytest.mark.parametrize("name", C.CASES_1_TO_9)
def test_components_equal_the_definition(gpu_device, name):
    from pagnerf_amd import connected_components
    m, kw, want = _reference(name)
    got = connected_components(_to(m, gpu_device), **kw)
    assert got["component"].is_cuda and isinstance(got["components"], int)
    _same_components(got, want, name)
    back = connected_components(m, device=gpu_device, **kw)                                # a CPU map: the labels come back to the CPU
    assert not back["component"].is_cuda
    _same_components(back, want, name)


@pytest.mark.parametrize("name", ["one_id_26", "five_ids_2_6_any", "serpentine", "x_line", "bridge_18"])
def test_two_runs_give_the_same_bits(gpu_device, name):
    from pagnerf_amd import connected_components
    m, kw, want = _reference(name)
    on_device = _to(m, gpu_device)
    first, second = connected_components(on_device, **kw), connected_components(on_device, **kw)
    assert first["components"] == second["components"] and torch.equal(first["component"], second["component"])
    _same_components(second, want, name)


def test_a_map_from_voxelmap_finish_and_the_same_map_through_the_cpu(gpu_device):
    from pagnerf_amd import VoxelMap, connected_components, connected_components_reference
    vox, ids = C.lattice(2, 5)
    twice = np.concatenate([vox, vox[::2]])                                                # every second voxel holds two points with the same id
    pts = torch.from_numpy(((twice + 0.5) * (2.0 / 32) - 1.0).astype(np.float32))
    fused = VoxelMap(2.0 / 32, device=gpu_device).add(pts.to(gpu_device), torch.from_numpy(np.concatenate([ids, ids[::2]])).to(gpu_device)).finish()
    assert fused["voxels"].is_cuda and torch.equal(fused["voxels"].cpu(), C.make_map(vox, ids)["voxels"])
    cpu = _to(fused, "cpu")
    for conn in (6, 18, 26):
        want = connected_components_reference(cpu, connectivity=conn)
        _same_components(connected_components(fused, connectivity=conn), want, conn)
        _same_components(connected_components(_to(cpu, gpu_device), connectivity=conn), want, conn)
        _same_components(connected_components(cpu, connectivity=conn, device=gpu_device), want, conn)


@pytest.mark.parametrize("mode", ["keep", "largest", "split"])
def test_clean_map_equals_the_definition(gpu_device, mode):
    from pagnerf_amd import clean_map, clean_map_reference
    tie = C.make_map(*C.clean_voxels(first=(2, 3, 2)))
    for what, m, kw in (("case 10", C.make_map(*C.clean_voxels()), dict(min_voxels=2)), ("case 10, a tie", tie, dict(min_voxels=2)),
                        ("case 10, nothing dropped", tie, dict(min_voxels=1)), ("case 10, everything dropped", tie, dict(min_voxels=13)),
                        ("case 2", C.case("five_ids_0_26_same")[0], dict(min_voxels=3)), ("case 2, 6 neighbours", C.case("five_ids_1_6_same")[0], dict(min_voxels=3, connectivity=6)),
                        ("case 2, id 3 ignored", C.case("five_ids_3_18_same")[0], dict(min_voxels=3, connectivity=18, ignore=(0, 3)))):
        want = clean_map_reference(m, mode=mode, **kw)
        got = clean_map(_to(m, gpu_device), mode=mode, **kw)
        assert got["component"].is_cuda and got["voxel_size"] == m["voxel_size"] and torch.equal(got["origin"].cpu(), m["origin"])
        C.assert_same(got, want, C.MAP_KEYS, (what, mode))                                 # integers equal, floats bit for bit: rows are only selected
        C.assert_same(clean_map(m, mode=mode, device=gpu_device, **kw), want, C.MAP_KEYS, (what, mode, "cpu map"))
        assert bool((np.diff(C.key_of(want["voxels"].numpy())) > 0).all())
    assert 0 < want["component"].numel() < m["instances"].numel()
    empty = clean_map(_to(C.case("empty")[0], gpu_device), mode=mode)
    assert empty["component"].shape == (0,) and empty["points"].shape == (0, 3)


def test_component_table_on_the_device(gpu_device):
    from pagnerf_amd import clean_map, component_table, label_table_reference
    import voxel_map_cases as V
    m = C.make_map(*C.clean_voxels())
    out = clean_map(_to(m, gpu_device), min_voxels=2, mode="split")
    table = component_table(out)
    cpu = _to(out, "cpu")
    want = label_table_reference(dict(cpu, instances=cpu["component"]), ignore=(0,))
    assert table["ids"].is_cuda
    V.assert_same(table, want, ("ids", "voxels", "observations", "bbox_min", "bbox_max", "volume"))
    for k, src in (("centroid", "points"), ("color", "color")):                              # fp32 sums in the kernel's order: the derived bound of the fusion's tests
        mean, bound = V.run_mean_bound(cpu[src], cpu["component"], 3)
        assert bool(((table[k].cpu().double() - mean[1:]).abs() <= bound[1:]).all()), k
    assert table["instance"].tolist() == [5, 6] and table["voxels"].tolist() == [40, 12]


def test_contract_violations_raise_through_the_status_word(gpu_device):
    """The rows are read as data: nothing is accessed out of range, the status word reports what was wrong."""
    from pagnerf_amd import clean_map, connected_components
    maps = C.contract_maps()
    for name, text in (("order", "ascend"), ("duplicate", "ascend"), ("beyond", r"outside \[0, 2\^21\)"), ("negative", r"outside \[0, 2\^21\)")):
        with pytest.raises(ValueError, match=text):
            connected_components(_to(maps[name], gpu_device))
    with pytest.raises(ValueError, match="ascend"):
        clean_map(_to(maps["order"], gpu_device), min_voxels=2)
    m, kw, want = _reference("contact_26")                                                 # the next call starts from a clean status word
    _same_components(connected_components(_to(m, gpu_device), **kw), want)


def _reported_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # the mode's own notice ("... is a prototype feature ...") is no report of a synchronisation
    return out, [w for w in seen if "called a synchronizing" in str(w.message)]


def test_host_synchronisations(gpu_device):
    """connected_components synchronises once (the read of the count and status), clean_map at most twice (that, and the kept rows), as torch's
    synchronisation debug mode reports them; with the declared reads taken out ("error" mode around ops.voxel_components) nothing else does."""
    from pagnerf_amd import clean_map, connected_components, ops
    m, kw, want = _reference("five_ids_0_26_same")
    on_device = _to(m, gpu_device)
    connected_components(on_device, **kw)                                                  # warm up: allocator, library load
    got, syncs = _reported_syncs(lambda: connected_components(on_device, **kw))
    _same_components(got, want)
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    for mode in ("keep", "largest", "split"):
        clean_map(on_device, min_voxels=3, mode=mode)
        _, syncs = _reported_syncs(lambda: clean_map(on_device, min_voxels=3, mode=mode))
        assert 1 <= len(syncs) <= 2, (mode, [str(w.message) for w in syncs])
    component = torch.empty(m["instances"].numel(), dtype=torch.int64, device=gpu_device)
    count_status = torch.empty(2, dtype=torch.int64, device=gpu_device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.voxel_components(on_device["voxels"], on_device["instances"], 26, True, (0,), component, count_status)       # the launches alone: no synchronisation
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert count_status.tolist() == [want["components"], 0] and torch.equal(component.cpu(), want["component"])


# ----------------------------------------------------------------------------------------------- the command lines
def test_the_fuse_command_cleans_and_splits_on_the_device(gpu_device, tmp_path):
    import csv
    import pickle
    from pagnerf_amd import clean_map_reference, fuse_map, map_export, save_map
    from test_map_components_host import _cloud_of_the_clean_case
    src = save_map(_cloud_of_the_clean_case(), tmp_path / "nerf_pc.pkl")
    args = ["fuse", src, "--voxel-size", str(2.0 / 64), "--min-component", "2", "--split", "split", "--out", str(tmp_path / "c.pkl"), "--table", str(tmp_path / "c.csv")]
    assert map_export.main(args + ["--device", str(gpu_device)]) == 0
    back = pickle.load(open(tmp_path / "c.pkl", "rb"))
    want = clean_map_reference(fuse_map(_cloud_of_the_clean_case(), 2.0 / 64, device="cpu"), min_voxels=2, mode="split")
    assert not back[0]["component"].is_cuda and back[0]["name"] == "nerf_pc_fused"
    C.assert_same(back[0], want, ("instances", "count", "agreement", "voxels", "component"))
    rows = list(csv.reader(open(tmp_path / "c.csv", newline="")))
    assert rows[0][:3] == ["id", "instance", "voxels"] and [r[:3] for r in rows[1:]] == [["1", "5", "40"], ["2", "6", "12"]]


def test_save_map_of_the_train_command_cleans_the_fused_map(gpu_device, tmp_path, monkeypatch):
    """train.save_map with min_component / split (--map-min-component / --map-split) on a stand-in trainer: the cleaned map of the fused map that the
    call without them writes, and the per-component table beside it."""
    import csv
    import pickle
    import types
    from pagnerf_amd import clean_map_reference, map_export, train
    from test_gpu_map_export import _scene
    pipe, base = _scene(gpu_device, 3)
    leaves = [types.SimpleNamespace(key="base_rays", field=f, src=getattr(base, f)) for f in ("origins", "dirs")]
    dataset = types.SimpleNamespace(_leaves=leaves, _rays_range={"base_rays": (0.0, 3.0)}, num_imgs=3)
    trainer = types.SimpleNamespace(pipeline=pipe, render_batch=1000)
    export = map_export.generate_pc_map_from_views
    th = dict(min_density=0.0, min_alpha=0.5, depth_range=(0.0, 3.0))
    monkeypatch.setattr(map_export, "generate_pc_map_from_views", lambda *a, **kw: export(*a, **dict(kw, **th)))
    fused = pickle.load(open(train.save_map(trainer, dataset, str(tmp_path / "map.pkl"), voxel_size=2.0 / 16), "rb"))
    assert "component" not in fused[0] and fused[0]["count"].numel() > 0
    back = pickle.load(open(train.save_map(trainer, dataset, str(tmp_path / "clean.pkl"), voxel_size=2.0 / 16, min_component=2, split="split"), "rb"))
    want = clean_map_reference(fused[0], min_voxels=2, mode="split")
    C.assert_same(back[0], want, ("instances", "count", "agreement", "voxels", "component"))
    rows = list(csv.reader(open(tmp_path / "clean.instances.csv", newline="")))
    assert rows[0][:3] == ["id", "instance", "voxels"] and len(rows) == 1 + int(want["component"].max())
