"""GPU checks of the fused voxel map (pagnerf_amd/map_export.py on csrc/voxelmap.hip) against the tensor-op definitions fuse_points_reference /
label_table_reference on the same inputs: bit for bit on exactly representable clouds (every fp32 sum of a run is exact in any order), integer
outputs equal and means within the derived bound on random fp32 clouds, invariance under chunking and repetition, the capacity guard, and the
views export fused end to end."""
import numpy as np
import pytest
import torch

import voxel_map_cases as C

pytestmark = pytest.mark.gpu

_REFERENCES = {}


def _reference(name):
    """The definition's result of an exact case, computed once and shared."""
    from pagnerf_amd import fuse_points_reference
    if name not in _REFERENCES:
        cloud, kw = C.exact_case(name)
        _REFERENCES[name] = (cloud, kw, fuse_points_reference(cloud["points"], cloud["ids"], cloud["color"], cloud["voxel_size"], **kw))
    return _REFERENCES[name]


def _fuse(cloud, dev, chunks=None, **kw):
    from pagnerf_amd import VoxelMap
    vm = VoxelMap(cloud["voxel_size"], device=dev, **kw)
    K = cloud["ids"].numel()
    edges = [0, K] if chunks is None else chunks
    for s, e in zip(edges[:-1], edges[1:]):
        vm.add(cloud["points"][s:e].to(dev), cloud["ids"][s:e].to(dev), cloud["color"][s:e].to(dev) if cloud["color"] is not None else None)
    return vm.finish()


@pytest.mark.parametrize("name", C.EXACT_CASES)
def test_exact_cases_equal_the_definition_bit_for_bit(gpu_device, name):
    cloud, kw, want = _reference(name)
    got = _fuse(cloud, gpu_device, **kw)
    assert got["points"].is_cuda and got["voxel_size"] == want["voxel_size"] and torch.equal(got["origin"].cpu(), want["origin"])
    assert want["count"].numel() > 0 and (cloud["color"] is None) == ("color" not in got)
    C.assert_same(got, want, C.FUSED_KEYS, name)
    if name == "one_voxel_65536":
        assert got["count"].tolist() == [65536]
    if name.startswith("straddle"):
        assert int(want["count"].sum()) == int(name[8:])


def test_a_chunk_of_dropped_rows_changes_nothing(gpu_device):
    from pagnerf_amd import VoxelMap
    dev = gpu_device
    cloud, kw, want = _reference("ties_300")
    bad = C.dropped_rows(500, 21)
    vm = VoxelMap(cloud["voxel_size"], device=dev)
    vm.add(*[t.to(dev) for t in bad])
    vm.add(cloud["points"].to(dev), cloud["ids"].to(dev), cloud["color"].to(dev))
    vm.add(*[t[:70].to(dev) for t in bad])
    C.assert_same(vm.finish(), want, C.FUSED_KEYS)
    only = VoxelMap(cloud["voxel_size"], device=dev).add(*[t.to(dev) for t in bad]).finish()     # nothing but dropped rows: an empty map
    assert only["points"].shape == (0, 3) and only["color"].shape == (0, 3) and only["count"].numel() == 0
    nothing = VoxelMap(cloud["voxel_size"], device=dev).add(torch.zeros(0, 3, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)).finish()
    assert nothing["points"].shape == (0, 3) and "color" not in nothing and nothing["voxels"].shape == (0, 3) and nothing["instances"].dtype == torch.int64


def test_keys_equal_the_tensor_op_form(gpu_device):
    from pagnerf_amd import map_export, ops
    rs = np.random.RandomState(8)
    p = torch.from_numpy(np.concatenate([rs.uniform(-1.2, 1.2, (3000, 3)).astype(np.float32), C.dropped_rows(300, 9)[0].numpy(),
                                         (rs.randint(-40, 41, (700, 3)) / 32.0).astype(np.float32)]))         # faces, limits' faces, below the origin
    for v, origin, limits in ((2.0 / 16, (-1.0, -1.0, -1.0), None), (0.0937, (-0.31, -1.07, -0.5), None), (2.0 / 16, (-1.0, -1.0, -1.0), [[-0.5, -1.0, -0.25], [0.5, 0.75, 1.0]]),
                              (1.0e-6, (-1.0, -1.0, -1.0), None)):
        got = ops.voxel_keys(p.to(gpu_device), origin, v, limits)
        want = map_export._reference_keys(p, v, origin, limits)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), (v, origin)
        assert int((want == map_export.DROPPED_KEY).sum()) > 300
    assert int((want != map_export.DROPPED_KEY).sum()) > 0 and int(want[want != map_export.DROPPED_KEY].max()) >> 42 > 1 << 19        # indices near 2^21


# ----------------------------------------------------------------------------------------------- the table
def _table_cases():
    return {"one_instance": [37], "two_hundred": [1 + i % 30 for i in range(200)], "across_blocks": [300, 1, 255, 256, 257, 1, 1, 600]}


@pytest.mark.parametrize("color", [True, False])
@pytest.mark.parametrize("name", sorted(_table_cases()))
def test_exact_tables_equal_the_definition(gpu_device, name, color):
    from pagnerf_amd import instance_table, label_table_reference
    m = C.exact_table_map(_table_cases()[name], 31, color=color)
    on_device = {k: (v.to(gpu_device) if torch.is_tensor(v) else v) for k, v in m.items()}
    for ignore in ((0,), (), (-6, 3, 12345)):
        want = label_table_reference(m, ignore=ignore)
        got = instance_table(on_device, ignore=ignore)
        assert got["ids"].is_cuda
        C.assert_same(got, want, C.TABLE_KEYS, (name, ignore))
        C.assert_same(instance_table(m, ignore=ignore, device=gpu_device), want, C.TABLE_KEYS, (name, ignore))       # a CPU map: the table comes back to the CPU
    assert label_table_reference(m, ignore=())["ids"].numel() == len(_table_cases()[name])


def test_one_label_owning_100000_voxels(gpu_device):
    """One point per voxel, so the voxel means are the points themselves; multiples of 1/128 keep the 100 000-term sums exact (100 000 * 128 < 2^24)."""
    from pagnerf_amd import instance_table, label_table_reference
    rs = np.random.RandomState(41)
    n = 100000
    flat = rs.permutation(128 ** 3)[:n]                                                    # n distinct voxels of the 128^3 lattice, two positions per axis in each
    steps = np.stack([flat // (128 * 128), flat // 128 % 128, flat % 128], 1) * 2 + rs.randint(0, 2, (n, 3))
    pts = torch.from_numpy((steps / 128.0 - 1.0).astype(np.float32))
    assert n * 128 <= 1 << 24 and float(pts.abs().max()) <= 1.0
    cloud = dict(points=pts, ids=torch.full((n,), 7, dtype=torch.int64), color=torch.from_numpy((rs.randint(0, 129, (n, 3)) / 128.0).astype(np.float32)),
                 voxel_size=2.0 / 128)
    fused = _fuse(cloud, gpu_device)
    assert fused["count"].numel() == n and bool((fused["count"] == 1).all()) and bool((fused["agreement"] == 1.0).all())
    order = torch.argsort((fused["voxels"].long().cpu() * torch.tensor([128 * 128, 128, 1])).sum(1))
    assert torch.equal(order, torch.arange(n))                                             # ascending key order
    assert torch.equal(fused["points"].cpu().sort(0).values, pts.sort(0).values)
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in fused.items()}
    for ignore in ((0,), (7,)):
        C.assert_same(instance_table(fused, ignore=ignore), label_table_reference(cpu, ignore=ignore), C.TABLE_KEYS, ignore)
    assert instance_table(fused)["voxels"].tolist() == [n] and instance_table(fused, ignore=(7,))["ids"].numel() == 0


# ----------------------------------------------------------------------------------------------- random fp32 inputs
def test_random_cloud_integers_equal_means_within_the_derived_bound(gpu_device):
    from pagnerf_amd import fuse_points_reference, instance_table, label_table_reference, map_export
    cloud = C.random_cloud()
    want = fuse_points_reference(cloud["points"], cloud["ids"], cloud["color"], cloud["voxel_size"])
    got = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in _fuse(cloud, gpu_device).items()}
    V = want["count"].numel()
    assert 1800 < V < 2300 and int(want["count"].max()) > 15
    C.assert_same(got, want, ("instances", "count", "voxels"))
    assert torch.equal(got["agreement"], want["agreement"])                                # a quotient of two integers below 2^24
    keys = map_export._reference_keys(cloud["points"], cloud["voxel_size"], C.ORIGIN, None)
    ukeys, inv = torch.unique(keys, return_inverse=True)
    assert ukeys.numel() == V
    for k in ("points", "color"):
        mean, bound = C.run_mean_bound(cloud[k], inv, V)
        err = (got[k].double() - mean).abs()
        print("%s: largest error / bound %.3f" % (k, float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), k
    # the table of the device's own map: integers equal, means within the bound of the label's voxel rows
    table = {k: v.cpu() for k, v in instance_table(got, ignore=(), device=gpu_device).items()}
    ref = label_table_reference(got, ignore=())
    C.assert_same(table, ref, ("ids", "voxels", "observations", "bbox_min", "bbox_max", "volume"))
    ulab, linv = torch.unique(got["instances"], return_inverse=True)
    for k, src in (("centroid", "points"), ("color", "color")):
        mean, bound = C.run_mean_bound(got[src], linv, ulab.numel())
        assert bool(((table[k].double() - mean).abs() <= bound).all()), k


# ----------------------------------------------------------------------------------------------- invariance
def test_chunking_and_repetition_do_not_change_a_bit(gpu_device):
    cloud = C.random_cloud()
    K = cloud["ids"].numel()
    whole = _fuse(cloud, gpu_device)
    again = _fuse(cloud, gpu_device)
    parts = _fuse(cloud, gpu_device, chunks=[0, 1, 64, 64, 5000, 5257, 12001, K])          # seven uneven chunks, the third one empty
    C.assert_same(again, whole, C.FUSED_KEYS, "repetition")
    C.assert_same(parts, whole, C.FUSED_KEYS, "chunking")
    from pagnerf_amd import instance_table
    C.assert_same(instance_table(parts), instance_table(whole), C.TABLE_KEYS)
    C.assert_same(instance_table(whole), instance_table(again), C.TABLE_KEYS)


# ----------------------------------------------------------------------------------------------- capacity
def test_capacity_guard(gpu_device):
    from pagnerf_amd import VoxelMap, map_export, ops
    dev = gpu_device
    cloud, kw, want = _reference("ties_300")
    V = want["count"].numel()
    assert V == 300
    with pytest.raises(RuntimeError, match="capacity >= %d" % V):
        _fuse(cloud, dev, capacity=V - 1)
    C.assert_same(_fuse(cloud, dev, capacity=V), want, C.FUSED_KEYS)
    # guard rows behind buffers of V - 1 rows: the counter reports all V voxels, nothing at or past the capacity is written
    cap, guard = V - 1, 64
    pts, ids, col = cloud["points"].to(dev), cloud["ids"].to(dev), cloud["color"].to(dev)
    rows = map_export.rows_by_key_and_id(ops.voxel_keys(pts, C.ORIGIN, cloud["voxel_size"]), ids, pts, col)
    bufs = dict(points=torch.full((cap + guard, 3), -7.0, device=dev), color=torch.full((cap + guard, 3), -7.0, device=dev),
                instances=torch.full((cap + guard,), -7, dtype=torch.int64, device=dev), count=torch.full((cap + guard,), -7, dtype=torch.int32, device=dev),
                agreement=torch.full((cap + guard,), -7.0, device=dev), voxels=torch.full((cap + guard, 3), -7, dtype=torch.int32, device=dev))
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.voxel_fuse(*rows, 1, bufs["points"][:cap], bufs["color"][:cap], bufs["instances"][:cap], bufs["count"][:cap], bufs["agreement"][:cap],
                   bufs["voxels"][:cap], counter)
    assert int(counter.item()) == V
    for k, b in bufs.items():
        assert torch.equal(b[:cap].cpu(), want[k][:cap]), k
        assert bool((b[cap:] == -7).all()), k
    # the table's guard: 5 labels into 3 rows
    from pagnerf_amd import instance_table
    m = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in C.exact_table_map([3, 1, 7, 2, 30], 5).items()}
    with pytest.raises(RuntimeError, match="capacity >= 5"):
        instance_table(m, ignore=(), capacity=3)
    assert instance_table(m, ignore=(), capacity=5)["ids"].tolist() == [-6, -3, 0, 3, 6]


def test_one_row_per_voxel_across_the_scan_chunks(gpu_device):
    """65537 sorted rows of distinct keys are 257 blocks of kept rows, one block more than the scan takes per pass: voxel k lands at row 3 + k
    behind a counter that starts at 3, every value as it went in (one row per voxel: the mean is the row)."""
    from pagnerf_amd import ops
    dev = gpu_device
    n, start = 65537, 3
    k = torch.arange(n, dtype=torch.int64, device=dev)
    vox = torch.stack((k >> 12, k >> 6 & 63, k & 63), 1)
    keys = vox[:, 0] << 42 | vox[:, 1] << 21 | vox[:, 2]
    ids = k % 1000 - 3
    pts = vox.float() + torch.tensor([0.5, 0.25, 0.75], device=dev)
    col = (k % 256).float()[:, None] / 256 + torch.tensor([0.0, 0.25, 0.5], device=dev)
    cap = start + n
    out = dict(points=torch.full((cap, 3), -7.0, device=dev), color=torch.full((cap, 3), -7.0, device=dev),
               instances=torch.full((cap,), -7, dtype=torch.int64, device=dev), count=torch.full((cap,), -7, dtype=torch.int32, device=dev),
               agreement=torch.full((cap,), -7.0, device=dev), voxels=torch.full((cap, 3), -7, dtype=torch.int32, device=dev))
    counter = torch.full((1,), start, dtype=torch.int64, device=dev)
    ops.voxel_fuse(keys, ids, pts, col, 1, out["points"], out["color"], out["instances"], out["count"], out["agreement"], out["voxels"], counter)
    assert int(counter.item()) == cap
    want = dict(points=pts, color=col, instances=ids, count=torch.ones(n, dtype=torch.int32, device=dev), agreement=torch.ones(n, device=dev),
                voxels=vox.int())
    for name, b in out.items():
        assert torch.equal(b[start:], want[name]), name
        assert bool((b[:start] == -7).all()), name


# ----------------------------------------------------------------------------------------------- end to end
def test_views_export_fused_end_to_end(gpu_device):
    import pagnerf_amd
    from pagnerf_amd import fuse_map, fuse_points_reference, generate_pc_map_from_views, instance_table, map_export
    from test_gpu_map_export import _scene
    pipe, base = _scene(gpu_device, 3)
    cams = [0, 1, 2]
    stacked = pagnerf_amd.Rays(base.origins.repeat(3, 1), base.dirs.repeat(3, 1))
    with torch.no_grad():
        rb = pagnerf_amd.batch_render(pipe, stacked, channels=["depth", "density", "rgb", "inst_embedding"], render_batch=1000, cam_ids=cams)
    hit = rb.hit & (rb.alpha[:, 0] > 0)                                                    # thresholds from the buffers' own quantiles, as the export's test
    q = lambda t, p: float(torch.quantile(t[hit].float(), p))                            # noqa: E731
    min_alpha = min(q(rb.alpha[:, 0], 0.3), float(rb.alpha[hit].max()) * (1 - 1e-6))
    th = dict(min_density=q(rb.density[:, 0], 0.5), min_alpha=min_alpha, depth_range=(q(rb.depth[:, 0], 0.2), q(rb.depth[:, 0], 0.8)))
    data = generate_pc_map_from_views(pipe, base, cam_ids=cams, render_batch=1000, **th)
    cloud = data[0]
    K = cloud["points"].shape[0]
    assert K > 200
    v = 2.0 / 16
    fused = fuse_map(data, v, device=gpu_device)
    want = fuse_points_reference(cloud["points"], cloud["inst_embedding"], cloud["color"], v)
    V = want["count"].numel()
    keys = map_export._reference_keys(cloud["points"], v, C.ORIGIN, None)
    inside = keys != map_export.DROPPED_KEY                                                # points outside the lattice's cube are no part of the map
    assert 0 < V < K and not fused["points"].is_cuda and fused["name"] == "nerf_pc_fused" and int(fused["count"].sum()) == int(inside.sum()) > 200
    C.assert_same(fused, want, ("instances", "count", "agreement", "voxels"))
    inv = torch.unique(keys[inside], return_inverse=True)[1]
    for k in ("points", "color"):                                                          # arbitrary fp32 rows: the means to the derived bound
        mean, bound = C.run_mean_bound(cloud[k][inside], inv, V)
        assert bool(((fused[k].double() - mean).abs() <= bound).all()), k
    table = instance_table(fused, ignore=(), device=gpu_device)
    assert not table["ids"].is_cuda and int(table["voxels"].sum()) == V and int(table["observations"].sum()) == int(inside.sum())
    assert torch.equal(table["ids"], torch.unique(fused["instances"]))


def test_save_map_of_the_train_command_writes_the_fused_map_and_the_table(gpu_device, tmp_path, monkeypatch):
    """train.save_map (--save-map PATH [--map-voxel-size V --map-min-votes N]) on a stand-in trainer: without a voxel size the raw cloud as before, with
    one the fused map and PATH's .instances.csv beside it."""
    import csv
    import pickle
    import types
    from pagnerf_amd import fuse_points_reference, label_table_reference, map_export, train
    from test_gpu_map_export import _scene
    pipe, base = _scene(gpu_device, 3)
    leaves = [types.SimpleNamespace(key="base_rays", field=f, src=getattr(base, f)) for f in ("origins", "dirs")]
    dataset = types.SimpleNamespace(_leaves=leaves, _rays_range={"base_rays": (0.0, 3.0)}, num_imgs=3)
    trainer = types.SimpleNamespace(pipeline=pipe, render_batch=1000)
    export = map_export.generate_pc_map_from_views
    th = dict(min_density=0.0, min_alpha=0.5, depth_range=(0.0, 3.0))                      # the defaults are tuned to BUP20's scale
    monkeypatch.setattr(map_export, "generate_pc_map_from_views", lambda *a, **kw: export(*a, **dict(kw, **th)))
    raw = pickle.load(open(train.save_map(trainer, dataset, str(tmp_path / "raw.pkl")), "rb"))
    assert raw[0]["points"].shape[0] > 0 and "count" not in raw[0] and not (tmp_path / "raw.instances.csv").exists()
    back = pickle.load(open(train.save_map(trainer, dataset, str(tmp_path / "map.pkl"), voxel_size=2.0 / 16, min_votes=2), "rb"))
    want = fuse_points_reference(raw[0]["points"], raw[0]["inst_embedding"], raw[0]["color"], 2.0 / 16, min_votes=2)
    assert len(back) == 1 and back[0]["name"] == "nerf_pc" and 0 < back[0]["count"].numel() < raw[0]["points"].shape[0]
    C.assert_same(back[0], want, ("instances", "count", "agreement", "voxels"))
    rows = list(csv.reader(open(tmp_path / "map.instances.csv", newline="")))
    assert rows[0][:3] == ["id", "voxels", "observations"] and [int(r[0]) for r in rows[1:]] == label_table_reference(want)["ids"].tolist()
