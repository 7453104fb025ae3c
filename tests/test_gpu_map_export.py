"""GPU checks of the map export (pagnerf_amd/map_export.py on csrc/map.hip): the reference's results in g14_map.npz (kept count, ids and order
exact, colours bit-equal, points within the tolerance test_rays_to_3d_points_vs_oracle uses for the same transform, dense cases exact), chunking
invariance, the capacity guard, instance widths and strides, ids input, a mean-shift labeller, the torch form of utils/render_map.py:107-120 on the
device, and the two exports end to end on a small BAPipeline."""
import numpy as np
import pytest
import torch

import test_map_export_host as H
from conftest import golden

pytestmark = pytest.mark.gpu

POINT_TOL = dict(rtol=1e-5, atol=1e-6)


def _pipeline(view, dev, nef=None, tracer=None):
    import pagnerf_amd
    return pagnerf_amd.BAPipeline(nef, torch.from_numpy(np.asarray(view)), tracer=tracer).to(dev)


def _buffers(d, dev, lo=0, hi=None):
    import pagnerf_amd
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(dev)              # noqa: E731
    return pagnerf_amd.RenderBuffer(**{k: t(d[k]) for k in ("depth", "alpha", "hit", "density", "rgb", "inst_embedding")})


def _rays(bo, bd, dev):
    import pagnerf_amd
    return pagnerf_amd.Rays(torch.from_numpy(bo).to(dev), torch.from_numpy(bd).to(dev))


def _append(pipe, base, d, cams, chunks, dev, capacity=None, **kw):
    """map_points_from_buffers over consecutive chunks of the given sizes (cycled) -> the accumulator."""
    from pagnerf_amd import MapAccumulator, map_points_from_buffers
    N = d["depth"].shape[0]
    out = MapAccumulator(N if capacity is None else capacity, dev)
    s, i = 0, 0
    while s < N:
        e = min(N, s + chunks[i % len(chunks)])
        map_points_from_buffers(pipe, base, _buffers(d, dev, s, e), cams, ray0=s, out=out, **kw)
        s, i = e, i + 1
    return out


def _torch_form(pipe, base, rb, cams, min_density=40.0, min_alpha=0.9, depth_range=(0.6, 0.8)):
    """utils/render_map.py:107-120 as tensor ops on the device."""
    import pagnerf_amd
    C = len(cams)
    stacked = pagnerf_amd.Rays(base.origins.repeat(C, 1), base.dirs.repeat(C, 1))
    points = pipe.rays_to_3d_points(stacked, rb.depth, cams)
    inst = torch.argmax(rb.inst_embedding, dim=-1)
    m = rb.density[:, 0] > min_density
    m = torch.logical_and(m, rb.alpha[:, 0] > min_alpha)
    m = torch.logical_and(m, rb.hit)
    m = torch.logical_and(m, rb.depth[:, 0] < depth_range[1])
    m = torch.logical_and(m, rb.depth[:, 0] > depth_range[0])
    return points[m], inst[m], rb.rgb[m]


@pytest.mark.parametrize("name", sorted(H.VIEWS_CASES))
def test_views_cases_equal_the_reference(gpu_device, name):
    g = golden("g14_map.npz")
    c = H.VIEWS_CASES[name]
    d = H.views_inputs(name)
    pipe = _pipeline(d["view"], gpu_device)
    base = _rays(g[name + "/base_origins"], g[name + "/base_dirs"], gpu_device)
    cams = list(range(c["cams"]))
    out = _append(pipe, base, d, cams, [H.RENDER_BATCH], gpu_device, **H.THRESHOLDS)       # the reference's chunks
    pts, col, ids = out.finish()
    kept = g[name + "/kept"]
    assert pts.shape[0] == kept.size
    assert np.array_equal(ids.cpu().numpy(), g[name + "/inst_embedding"])
    assert torch.equal(col, torch.from_numpy(d["rgb"][kept]).to(gpu_device)) and col.cpu().numpy().tobytes() == g[name + "/color"].tobytes()
    np.testing.assert_allclose(pts.cpu().numpy(), g[name + "/points"], **POINT_TOL)


class _SeededNef:
    """The maker's nef stand-in on the device: seeded density / instance rows in call order; records the queried samples."""

    def __init__(self, name, dev):
        c = H.DENSE_CASES[name]
        self.I, self.device = c["I"], dev
        self.rs_density, self.rs_inst = np.random.RandomState(c["seed"]), np.random.RandomState(c["seed"] + 100)
        self.queried = []

    def __call__(self, coords, ray_d, channels):
        n = coords.shape[0]
        assert coords.shape[1:] == (1, 3) and ray_d is None
        if channels == "density":
            self.queried.append(coords[:, 0].clone())
            return torch.from_numpy(H.dense_density(self.rs_density, n)).to(self.device).reshape(n, 1, 1)
        assert channels == "inst_embedding"
        return torch.from_numpy(H.dense_inst(self.rs_inst, n, self.I)).to(self.device)


@pytest.mark.parametrize("batch", [20000, 777])
@pytest.mark.parametrize("name", sorted(H.DENSE_CASES))
def test_dense_cases_equal_the_reference(gpu_device, name, batch):
    from pagnerf_amd import generate_pc_map, get_dense_occupied_points
    g = golden("g14_map.npz")
    c = H.DENSE_CASES[name]
    noise = torch.from_numpy(g[name + "/noise"])
    limits = torch.tensor(c["limits"]) if c["limits"] is not None else None
    nef = _SeededNef(name, gpu_device)
    occ = get_dense_occupied_points(nef, c["level"], c["min_density"], limits, noise=noise, render_batch=batch)
    assert occ.is_cuda and occ.shape == g[name + "/occupied"].shape and occ.cpu().numpy().tobytes() == g[name + "/occupied"].tobytes()
    lattice = H.np_lattice(c["level"], c["limits"])
    res = np.float32(2.0 ** c["level"])
    want = (lattice + (g[name + "/noise"] / res * np.float32(2.0) - np.float32(1.0))).astype(np.float32)      # the shift of about -1, as written
    assert torch.cat(nef.queried).cpu().numpy().tobytes() == want.tobytes()
    data = generate_pc_map(_SeededNef(name, gpu_device), c["level"], min_density=c["min_density"], limits=limits, noise=noise, render_batch=batch)
    assert len(data) == 1 and data[0]["name"] == "nerf_pc" and not data[0]["points"].is_cuda
    assert data[0]["points"].numpy().tobytes() == g[name + "/points"].tobytes() and data[0]["points"].shape == g[name + "/points"].shape
    assert data[0]["instances"].dtype == torch.int64 and np.array_equal(data[0]["instances"].numpy(), g[name + "/instances"])


def test_chunking_does_not_change_the_result(gpu_device):
    name = "chunk_inside_image"
    g = golden("g14_map.npz")
    d = H.views_inputs(name)
    pipe = _pipeline(d["view"], gpu_device)
    base = _rays(g[name + "/base_origins"], g[name + "/base_dirs"], gpu_device)
    cams = [0, 1, 2]
    whole = _append(pipe, base, d, cams, [d["depth"].shape[0]], gpu_device, **H.THRESHOLDS).finish()
    assert whole[0].shape[0] == g[name + "/kept"].size
    rpc = base.origins.shape[0]
    for chunks in ([1000], [20000], [64], [63], [1, 63, 64, 1000, rpc - 1128 + 500, 20000]):      # the last list has a chunk across the border of images 0 and 1
        if chunks in ([64], [63]):
            sub = {k: (v[:3000] if k != "view" else v) for k, v in d.items()}             # small chunks on the first 3000 rays
            a = _append(pipe, base, sub, cams, chunks, gpu_device, **H.THRESHOLDS).finish()
            b = _append(pipe, base, sub, cams, [3000], gpu_device, **H.THRESHOLDS).finish()
        else:
            a, b = _append(pipe, base, d, cams, chunks, gpu_device, **H.THRESHOLDS).finish(), whole
        for x, y in zip(a, b):
            assert torch.equal(x, y), chunks
    ones = {k: (v[7000:7200] if k != "view" else v) for k, v in d.items()}                # chunks of one ray, starting inside image 0
    from pagnerf_amd import MapAccumulator, map_points_from_buffers
    acc = MapAccumulator(200, gpu_device)
    for i in range(200):
        map_points_from_buffers(pipe, base, _buffers(ones, gpu_device, i, i + 1), cams, ray0=7000 + i, out=acc, **H.THRESHOLDS)
    lo = int((g[name + "/kept"] < 7000).sum())
    hi = int((g[name + "/kept"] < 7200).sum())
    for x, y in zip(acc.finish(), whole):
        assert torch.equal(x, y[lo:hi])


def test_capacity_guard(gpu_device):
    from pagnerf_amd import MapAccumulator, map_points_from_buffers
    name = "ties_and_nan"
    g = golden("g14_map.npz")
    d = H.views_inputs(name)
    pipe = _pipeline(d["view"], gpu_device)
    base = _rays(g[name + "/base_origins"], g[name + "/base_dirs"], gpu_device)
    full = _append(pipe, base, d, [0, 1, 2], [1000], gpu_device, **H.THRESHOLDS).finish()
    K, cap, guard = full[0].shape[0], 100, 64
    assert K > cap
    acc = MapAccumulator(cap + guard, gpu_device)
    acc.points.fill_(-7.0), acc.color.fill_(-7.0), acc.ids.fill_(-7)
    small = MapAccumulator.__new__(MapAccumulator)                                        # the first `cap` rows of the guarded buffers
    small.capacity, small.points, small.color, small.ids, small.count = cap, acc.points[:cap], acc.color[:cap], acc.ids[:cap], acc.count
    for s in range(0, d["depth"].shape[0], 1000):
        map_points_from_buffers(pipe, base, _buffers(d, gpu_device, s, s + 1000), [0, 1, 2], ray0=s, out=small, **H.THRESHOLDS)
    assert int(acc.count.item()) == K                                                    # the counter reports the full count
    for got, want in zip((acc.points, acc.color, acc.ids), full):
        assert torch.equal(got[:cap], want[:cap])
        assert bool((got[cap:] == -7).all())                                             # nothing written at or past the capacity
    with pytest.raises(RuntimeError, match="capacity"):
        small.finish()


@pytest.mark.parametrize("I", [1, 3, 6, 200, 201, 1024])
def test_instance_widths_strides_and_ids_input(gpu_device, I):
    from pagnerf_amd import MapAccumulator, ops
    dev = gpu_device
    rs = np.random.RandomState(I)
    n = 1500
    inst = (np.round(rs.rand(n, I) * 16) / 16).astype(np.float32)
    inst[rs.rand(n) < 0.1, rs.randint(0, I)] = np.nan
    want = torch.from_numpy(H.np_argmax(inst)).to(dev)
    value = torch.from_numpy(rs.rand(n).astype(np.float32)).to(dev)
    pts = torch.from_numpy(rs.rand(n, 3).astype(np.float32)).to(dev)
    t = torch.from_numpy(inst).to(dev)
    assert torch.equal(torch.argmax(t, dim=-1), want)                                    # the restatement is torch's rule
    wide = torch.full((n, I + 5), 9.0, device=dev)                                       # a non-contiguous row stride (and an unaligned one)
    wide[:, 1:I + 1] = t
    for rows in (t, wide[:, 1:I + 1]):
        for thr in (0.7, -1.0, 2.0):                                                     # some, all, none kept
            acc = MapAccumulator(n, dev, color=False)
            ops.map_select(pts, acc.points, acc.count, value=value, threshold=thr, inst=rows, ids_out=acc.ids)
            p, _, ids = acc.finish()
            m = value > thr
            assert torch.equal(p, pts[m]) and torch.equal(ids, want[m])
        acc = MapAccumulator(n, dev, color=False)                                        # the `argmax != 0` predicate
        ops.map_select(pts, acc.points, acc.count, inst=rows, ids_out=acc.ids)
        p, _, ids = acc.finish()
        assert torch.equal(p, pts[want != 0]) and torch.equal(ids, want[want != 0])
    acc = MapAccumulator(n, dev, color=False)                                            # ids in place of inst
    given = want * 3 - 6
    ops.map_select(pts, acc.points, acc.count, ids=given, ids_out=acc.ids)
    p, _, ids = acc.finish()
    assert torch.equal(p, pts[given != 0]) and torch.equal(ids, given[given != 0])


def test_append_behind_a_counter_across_the_scan_chunks(gpu_device):
    """65537 rows are 257 blocks: the one-workgroup scan takes 256 block counts per pass, so its second pass starts from the carry of the first
    with a single block.  Rows at wave, block and pass borders are kept, about half of the others; the counter starts at 5."""
    from pagnerf_amd import ops
    dev = gpu_device
    n, start, guard = 65537, 5, 64
    i = np.arange(n, dtype=np.int64)
    keep = ((i * 2654435761 % (1 << 32)) >> 16 & 1).astype(bool)
    keep[[63, 64, 255, 256, 65279, 65280, 65535, 65536]] = True
    K = int(keep.sum())
    assert n // 3 < K < 2 * n // 3
    mask = torch.from_numpy(keep).to(dev)
    pts = torch.from_numpy(np.stack([i, i + 0.5, -i], 1).astype(np.float32)).to(dev)
    given = torch.from_numpy(i * 3 + 1).to(dev)
    value = mask.float()
    want_p, want_i = pts[mask], given[mask]
    for cap in (start + K, start + K - 1):
        points = torch.full((cap + guard, 3), -7.0, device=dev)
        ids = torch.full((cap + guard,), -7, dtype=torch.int64, device=dev)
        count = torch.full((1,), start, dtype=torch.int64, device=dev)
        ops.map_select(pts, points[:cap], count, value=value, threshold=0.5, ids=given, ids_out=ids[:cap])
        assert int(count.item()) == start + mask.sum().item()                             # the full count, whatever the capacity
        assert torch.equal(points[start:cap], want_p[:cap - start]) and torch.equal(ids[start:cap], want_i[:cap - start])
        for b in (points, ids):
            assert bool((b[:start] == -7).all()) and bool((b[cap:] == -7).all())         # nothing before the counter's start or past the capacity


def test_everything_and_nothing_kept_and_the_torch_form(gpu_device):
    name = "six_channels"
    g = golden("g14_map.npz")
    d = H.views_inputs(name)
    pipe = _pipeline(d["view"], gpu_device)
    base = _rays(g[name + "/base_origins"], g[name + "/base_dirs"], gpu_device)
    rb = _buffers(d, gpu_device)
    N = d["depth"].shape[0]
    for th in (H.THRESHOLDS, dict(min_density=1e9, min_alpha=0.9, depth_range=(0.6, 0.8)), dict(min_density=-1.0, min_alpha=-1.0, depth_range=(-1.0, 9.0))):
        allhit = th["min_density"] < 0
        dd = dict(d, hit=np.ones(N, bool)) if allhit else d
        rb = _buffers(dd, gpu_device)
        pts, col, ids = _append(pipe, base, dd, [0, 1], [700], gpu_device, **th).finish()
        wp, wi, wc = _torch_form(pipe, base, rb, [0, 1], **th)
        assert pts.shape[0] == (N if allhit else wp.shape[0]) and (th["min_density"] < 1e8 or pts.shape[0] == 0)
        assert torch.equal(ids, wi) and torch.equal(col, wc)
        np.testing.assert_allclose(pts.cpu().numpy(), wp.cpu().numpy(), **POINT_TOL)
    ids_in = torch.from_numpy(np.random.RandomState(3).randint(-5, 1 << 40, N)).to(gpu_device)      # precomputed ids in place of inst
    out = _append(pipe, base, d, [0, 1], [700], gpu_device, labels=lambda x: ids_in[:x.shape[0]], **H.THRESHOLDS)
    kept = torch.from_numpy(g[name + "/kept"]).to(gpu_device)
    sel = torch.cat([kept[kept < 700], kept[(kept >= 700) & (kept < 1400)] - 700, kept[kept >= 1400] - 1400])
    assert torch.equal(out.finish()[2], ids_in[sel])


def test_meanshift_labels(gpu_device):
    from pagnerf_amd import MeanShift
    dev = gpu_device
    torch.manual_seed(5)
    centres = torch.nn.functional.normalize(torch.randn(5, 16), dim=-1)
    lab = torch.randint(0, 5, (2, 400))
    X = (centres[lab] + 0.05 * torch.randn(2, 400, 16)).to(dev)
    ms = MeanShift()
    ms.train_clustering(X, lab.to(dev))
    assert ms.fitted
    name = "six_channels"
    g = golden("g14_map.npz")
    d = H.views_inputs(name)
    N = d["depth"].shape[0]
    emb = (centres[torch.randint(0, 5, (N,))] + 0.05 * torch.randn(N, 16)).numpy().astype(np.float32)
    d = dict(d, inst_embedding=emb)
    pipe = _pipeline(d["view"], dev)
    base = _rays(g[name + "/base_origins"], g[name + "/base_dirs"], dev)
    out = _append(pipe, base, d, [0, 1], [600], dev, labels=ms.predict_clusters, **H.THRESHOLDS).finish()
    want = ms.predict_clusters(torch.from_numpy(emb).to(dev))[torch.from_numpy(g[name + "/kept"]).to(dev)]
    assert torch.equal(out[2], want) and want.unique().numel() > 1


# ----------------------------------------------------------------------------------------------- end to end
def _scene(dev, cams, h=32, w=48):
    import pagnerf_amd
    import test_gpu_parity as T
    nef, tracer, _, _, _ = T._make_scene(dev, "bf16", N=8, S=32)
    tracer.raymarch_type, tracer.num_steps, tracer.ray_max_travel = "voxel", 2, 0.8      # the voxel march: deterministic
    view = H.view_matrices(np.random.RandomState(77), cams)
    view[:, :3, 3] = np.array([0.0, 0.0, -1.1], np.float32)                               # cameras 1.1 from the origin, looking at it
    pipe = pagnerf_amd.BAPipeline(nef, torch.from_numpy(view), tracer=tracer, near=0.0, far=3.0).to(dev)
    bo, bd = H.base_rays_np(h, w)
    return pipe, _rays(bo, bd, dev)


def test_views_export_end_to_end(gpu_device):
    import pagnerf_amd
    from pagnerf_amd import generate_pc_map_from_views
    pipe, base = _scene(gpu_device, 3)
    cams = [0, 1, 2]
    chans = ["depth", "density", "rgb", "inst_embedding"]
    stacked = pagnerf_amd.Rays(base.origins.repeat(3, 1), base.dirs.repeat(3, 1))
    with torch.no_grad():
        rb = pagnerf_amd.batch_render(pipe, stacked, channels=chans, render_batch=1000, cam_ids=cams)
    # thresholds from the rendered buffers' own quantiles (the reference's defaults are tuned to BUP20's scale)
    hit = rb.hit & (rb.alpha[:, 0] > 0)
    assert hit.float().mean() > 0.3
    q = lambda t, p: float(torch.quantile(t[hit].float(), p))                            # noqa: E731
    min_alpha = min(q(rb.alpha[:, 0], 0.3), float(rb.alpha[hit].max()) * (1 - 1e-6))     # saturated alphas: the threshold stays below the maximum
    th = dict(min_density=q(rb.density[:, 0], 0.5), min_alpha=min_alpha, depth_range=(q(rb.depth[:, 0], 0.2), q(rb.depth[:, 0], 0.8)))
    wp, wi, wc = _torch_form(pipe, base, rb, cams, **th)
    share = wp.shape[0] / rb.depth.shape[0]
    assert 0.05 < share < 0.5, share
    data = generate_pc_map_from_views(pipe, base, cam_ids=cams, render_batch=1000, **th)
    assert len(data) == 1 and data[0]["name"] == "nerf_pc" and not data[0]["points"].is_cuda
    assert data[0]["inst_embedding"].dtype == torch.int64 and torch.equal(data[0]["inst_embedding"], wi.cpu())
    assert torch.equal(data[0]["color"], wc.cpu())
    np.testing.assert_allclose(data[0]["points"].numpy(), wp.cpu().numpy(), **POINT_TOL)


def test_dense_export_end_to_end(gpu_device):
    from pagnerf_amd import generate_pc_map
    pipe, _ = _scene(gpu_device, 2)
    nef = pipe.nef
    level = 4
    lattice = torch.from_numpy(H.np_lattice(level, None)).to(gpu_device)
    noise = torch.rand(lattice.shape[0], 3, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        samples = lattice + (noise.to(gpu_device) / 2.0 ** level * 2.0 - 1.0)
        density = nef(coords=samples[:, None], ray_d=None, channels="density")[:, 0, 0]
        thr = float(torch.quantile(density.float(), 0.6))
        occ = lattice[density > thr]
        inst = nef(coords=occ[:, None], ray_d=None, channels="inst_embedding").float().reshape(occ.shape[0], -1)
        lab = torch.argmax(inst, dim=-1)
    keep = lab != int(torch.mode(lab).values)                                            # the torch form of :160-165 with the commonest label as "0"
    data = generate_pc_map(nef, level, min_density=thr, noise=noise, render_batch=1500,
                           labels=lambda x: torch.where(torch.argmax(x.float(), -1) == int(torch.mode(lab).values), 0, torch.argmax(x.float(), -1) + 1))
    assert 0 < occ.shape[0] < lattice.shape[0]
    assert torch.equal(data[0]["points"], occ[keep].cpu()) and torch.equal(data[0]["instances"], (lab[keep] + 1).cpu())
    data = generate_pc_map(nef, level, min_density=thr, noise=noise, render_batch=1500)  # the plain argmax labels
    assert torch.equal(data[0]["points"], occ[lab != 0].cpu()) and torch.equal(data[0]["instances"], lab[lab != 0].cpu())


def test_views_export_memory_does_not_grow_with_the_cameras(gpu_device):
    from pagnerf_amd import render_points_at_depth
    peaks = {}
    for cams in (3, 6):
        pipe, base = _scene(gpu_device, cams, h=64, w=96)
        th = dict(min_density=0.0, min_alpha=0.5, depth_range=(0.0, 3.0))
        render_points_at_depth(pipe, base, render_batch=4000, **th)                      # warm up: workspaces, streams
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = render_points_at_depth(pipe, base, render_batch=4000, **th)
        torch.cuda.synchronize()
        peaks[cams] = torch.cuda.max_memory_allocated() - before
        del out, pipe
    rows = 6 * 64 * 96 * 32                                                              # 6 cameras' worth of output rows: 12 + 12 + 8 bytes each
    assert peaks[6] - peaks[3] <= rows + (2 << 20), peaks                                  # + the allocator's 2 MiB block rounding
