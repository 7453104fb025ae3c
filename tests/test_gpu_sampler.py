"""The ray-sampling kernel (csrc/sample.hip, pag_sample_batch / pag_sample_advance) against the definition in pagnerf_amd/dataset.py: the indices bit
for bit, every copy width and dtype of the gather, the uint8 -> f32 conversion, source offsets past 2^32, graph replay, a sync-free BatchSampler epoch and
the analytic scene trained from images.  The definition itself: tests/test_sampler_host.py."""
import os
import sys

import pytest
import torch

from conftest import REPO

SIZES = (1, 2, 3, 4, 5, 7, 16, 17, 255, 256, 257, 1000, 4097, 921600)      # the bijection list of tests/test_sampler_host.py

pytestmark = pytest.mark.gpu


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("seed,draw", [(0, 0), (7, 3), (-5, (1 << 32) + 9)])
def test_indices_are_the_definition(gpu_device, seed, draw):
    """ray_idx == sample_indices for every size of the bijection list, k = min(n, 300) (two workgroups, the second partly empty), a repeated view."""
    import pagnerf_amd
    from pagnerf_amd.dataset import sample_indices
    views = [2, 0, 2]
    for n in SIZES:
        k = min(n, 300)
        ds = pagnerf_amd.DeviceMultiviewDataset({"imgs": torch.zeros(3, n, 1, dtype=torch.uint8)}, gpu_device).seed(seed, draw)
        out = ds.sample(views, k, ray_idx=True)
        want = sample_indices(n, k, seed, draw, views)
        assert _eq(out["ray_idx"], want), n
        assert out["cam_id"].tolist() == views and out["cam_idx"].dtype == torch.int32 and out["cam_idx"].tolist() == [v for v in views for _ in range(k)]
        if n == 921600:
            ds.advance()
            assert _eq(ds.sample(views, 4096, ray_idx=True)["ray_idx"], sample_indices(n, 4096, seed, draw + 1, views))         # the best.yaml shape


def _modes(V, n, gen):
    """Rows of 1, 2, 3, 4, 6, 7, 12 and 16 bytes, 12 arrays in all (rays and base_rays count two each)."""
    import pagnerf_amd
    r = lambda *s: torch.rand(*s, generator=gen)
    i = lambda hi, dt, *s: torch.randint(0, hi, s, generator=gen).to(dt)
    return {"imgs": r(V, n, 4),                                       # f32 x 4: 16 bytes
            "semantics": i(6, torch.int64, V, n, 1),                  # 8
            "instance": i(200, torch.int64, V, n, 2),                 # 16
            "sem_conf": r(V, n, 1),                                   # 4
            "normals": r(V, n, 3),                                    # 12
            "u1": i(256, torch.uint8, V, n, 1), "u3": i(256, torch.uint8, V, n, 3), "u7": i(256, torch.uint8, V, n, 7),      # 1, 3, 7
            "h1": i(30000, torch.int16, V, n, 1), "h3": i(30000, torch.int16, V, n, 3),                                    # 2, 6
            "base_rays": pagnerf_amd.Rays(r(n, 3), r(n, 3), dist_min=0.5, dist_max=4.0)}                                   # shared, 12


@pytest.fixture(scope="module")
def gather_case(gpu_device):
    import pagnerf_amd
    V, n, k = 4, 1000, 300
    data = _modes(V, n, torch.Generator().manual_seed(3))
    ds = pagnerf_amd.DeviceMultiviewDataset(data, gpu_device).seed(21, 4)
    assert len(ds._leaves) == 12
    views = [3, 1, 3]
    return ds, data, views, k, ds.sample(views, k, ray_idx=True)


def test_gather_is_bit_exact(gather_case):
    """Every mode == mode[views][:, idx], one launch for the twelve arrays, and == the tensor-op form on the same device and on the CPU."""
    import pagnerf_amd
    from pagnerf_amd import ops
    from pagnerf_amd.dataset import sample_indices
    ds, data, views, k, out = gather_case
    idx = sample_indices(ds.num_pixels, k, 21, 4, views)
    assert _eq(out["ray_idx"], idx)
    widths = set()
    for key, src in data.items():
        if key == "base_rays":
            for f in ("origins", "dirs"):
                assert _eq(getattr(out[key], f), getattr(src, f)[idx])
            assert (out[key].dist_min, out[key].dist_max) == (0.5, 4.0)
        else:
            assert _eq(out[key], src[torch.tensor(views)[:, None], idx]), key
    for l in ds._leaves:
        widths.add(ops.sample_copy_width(l.src.data_ptr(), ds._leaf_out(out, l).data_ptr(), l.row_bytes))
    assert widths == {16, 8, 4, 2, 1}                                  # every copy width ran
    ds.use_kernel = False
    form = ds.sample(views, k, ray_idx=True)
    ds.use_kernel = True
    cpu = pagnerf_amd.DeviceMultiviewDataset(data, "cpu").seed(21, 4).sample(views, k, ray_idx=True)
    for other in (form, cpu):
        assert set(other) == set(out)
        for key, v in out.items():
            for a, b in ([(v.origins, other[key].origins), (v.dirs, other[key].dirs)] if key == "base_rays" else [(v, other[key])]):
                assert torch.equal(a.cpu().long() if key == "cam_id" else a.cpu(), b.cpu().long() if key == "cam_id" else b.cpu()), key


def test_slot_slices_and_out_buffers(gather_case):
    ds, data, views, k, out = gather_case
    parts = [ds.sample(views, k, slots=s, ray_idx=True) for s in ((0, 1), (1, 255), (256, 44))]
    for key in ("imgs", "u7", "h3", "semantics", "ray_idx"):
        assert _eq(torch.cat([p[key] for p in parts], 1), out[key]), key
    assert _eq(torch.cat([p["base_rays"].dirs for p in parts], 1), out["base_rays"].dirs)
    assert parts[1]["cam_idx"].tolist() == [v for v in views for _ in range(255)]
    buf = ds.empty_batch(3, k, ray_idx=True)
    ptrs = {key: (v.origins if key == "base_rays" else v).data_ptr() for key, v in buf.items()}
    assert ds.sample(views, k, out=buf) is buf
    for key, v in out.items():
        if key == "base_rays":
            assert _eq(buf[key].origins, v.origins) and _eq(buf[key].dirs, v.dirs)
        else:
            assert _eq(buf[key], v), key
        assert (buf[key].origins if key == "base_rays" else buf[key]).data_ptr() == ptrs[key]
    with pytest.raises(ValueError):
        ds.sample(views, k - 1, out=buf)
    with pytest.raises(IndexError):
        ds.sample([4], 8)


def test_bool_mask_and_odd_byte_offset(gpu_device):
    """A bool mode, and a uint8 x 4 mode whose storage starts at an odd address: the kernel must fall back to single bytes there."""
    import pagnerf_amd
    from pagnerf_amd import ops
    from pagnerf_amd.dataset import sample_indices
    V, n, k = 3, 257, 200
    gen = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (V * n * 4 + 1,), generator=gen).to(torch.uint8).to(gpu_device)
    odd = raw[1:].view(V, n, 4)
    mask = (torch.rand(V, n, 1, generator=gen) > 0.5)
    ds = pagnerf_amd.DeviceMultiviewDataset({"imgs": odd, "masks": mask}, gpu_device).seed(2, 9)
    assert ds._leaves[0].src.data_ptr() == raw.data_ptr() + 1 and ds._leaves[0].src.data_ptr() % 2 == 1          # held in place, not copied
    out = ds.sample([0, 2, 1], k, ray_idx=True)
    assert ops.sample_copy_width(ds._leaves[0].src.data_ptr(), out["imgs"].data_ptr(), 4) == 1
    idx = sample_indices(n, k, 2, 9, [0, 2, 1])
    assert _eq(out["ray_idx"], idx)
    assert _eq(out["imgs"], odd.cpu()[torch.tensor([0, 2, 1])[:, None], idx])
    assert out["masks"].dtype == torch.bool and _eq(out["masks"], mask[torch.tensor([0, 2, 1])[:, None], idx])


@pytest.mark.parametrize("C", [3, 4, 8])
def test_uint8_storage_returns_x_over_255(gpu_device, C):
    """store_uint8: the batch is x.float() / 255 exactly - IEEE division, what torch computes on the CPU (a device's `x / 255` may multiply by the
    rounded reciprocal instead, which differs in the last bit for some of the 256 values).  C = 3: single bytes; 4, 8: uchar4 -> float4."""
    import pagnerf_amd
    V, n, k = 2, 300, 300
    u = torch.randint(0, 256, (V, n, C), generator=torch.Generator().manual_seed(C), dtype=torch.uint8)
    u[0, :256, 0] = torch.arange(256, dtype=torch.uint8)                # every value occurs
    img = u.float() / 255
    ds = pagnerf_amd.DeviceMultiviewDataset({"imgs": img}, gpu_device, store_uint8=("imgs",)).seed(1, 1)
    assert ds._leaves[0].src.dtype == torch.uint8 and _eq(ds._leaves[0].src, u)
    out = ds.sample([0, 1], k, ray_idx=True)
    idx = out["ray_idx"].cpu()
    assert sorted(idx[0].tolist()) == list(range(n))
    want = u[torch.arange(V)[:, None], idx].float() / 255
    assert out["imgs"].dtype == torch.float32 and _eq(out["imgs"], want)
    ds.use_kernel = False
    assert torch.equal(ds.sample([0, 1], k)["imgs"], out["imgs"])              # the tensor-op form on the device
    with pytest.raises(ValueError):
        pagnerf_amd.DeviceMultiviewDataset({"imgs": (img + 1e-4).to(gpu_device)}, gpu_device, store_uint8=("imgs",))


def test_source_offsets_past_4_gib(gpu_device):
    """V = 3 views of n = 2^29 + 3 uint8 x 4 pixels (6.4 GB, never initialised): known rows are written only where the definition says the kernel will
    read, and the last view's rows all lie past byte 2^32."""
    import pagnerf_amd
    from pagnerf_amd.dataset import sample_indices
    V, n, k = 3, (1 << 29) + 3, 64
    views = [2, 0, 2, 1]
    big = torch.empty(V, n, 4, dtype=torch.uint8, device=gpu_device)
    ds = pagnerf_amd.DeviceMultiviewDataset({"imgs": big}, gpu_device).seed(13, 1 << 33)
    assert ds._leaves[0].src.data_ptr() == big.data_ptr()
    idx = sample_indices(n, k, 13, 1 << 33, views)                      # CPU [4, 64]
    offsets = (torch.tensor(views)[:, None] * n + idx) * 4
    assert int(offsets[0].min()) >= 1 << 32 and int(offsets[2].min()) >= 1 << 32 and int(offsets.max()) + 4 <= V * n * 4
    assert int(offsets[3].max()) >= 1 << 31                             # and past what a signed 32-bit offset reaches, in the middle view
    rows = torch.randint(0, 256, (len(views), k, 4), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    rows[2] = rows[0]                                                   # the repeated view reads the same pixels
    rows_dev = rows.to(gpu_device)
    for b, v in enumerate(views):                                       # 256 four-byte copies: no indexing kernel over a 6.4 G-element tensor
        for j, pix in enumerate(idx[b].tolist()):
            big[v, pix].copy_(rows_dev[b, j])
    out = ds.sample(views, k, ray_idx=True)
    assert _eq(out["ray_idx"], idx) and _eq(out["imgs"], rows)


def test_graph_replay_draws_afresh(gpu_device):
    """sample + advance captured once on one stream, replayed three times: replay r is the eager batch of draw0 + r (the state lives on the device)."""
    import pagnerf_amd
    data = _modes(3, 500, torch.Generator().manual_seed(8))
    ds = pagnerf_amd.DeviceMultiviewDataset(data, gpu_device)
    seed, draw0, k = 17, (1 << 32) - 2, 128
    views = torch.tensor([1, 1, 2, 0], dtype=torch.int32, device=gpu_device)
    buf = ds.empty_batch(4, k, ray_idx=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # warm-up off the capture, as torch asks
        ds.sample(views, k, out=buf)
        ds.advance()
    torch.cuda.current_stream().wait_stream(side)
    ds.seed(seed, draw0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ds.sample(views, k, out=buf)
        ds.advance()
    replays = []
    for _ in range(3):
        graph.replay()
        replays.append({key: (v.dirs.clone() if key == "base_rays" else v.clone()) for key, v in buf.items()})
    torch.cuda.synchronize()
    assert ds.state.tolist() == [seed, draw0 + 3]
    eager = pagnerf_amd.DeviceMultiviewDataset(data, gpu_device)
    for r, got in enumerate(replays):
        want = eager.seed(seed, draw0 + r).sample(views, k, ray_idx=True)
        for key, v in got.items():
            assert _eq(v, want[key].dirs if key == "base_rays" else want[key]), (r, key)
    assert not torch.equal(replays[0]["ray_idx"], replays[1]["ray_idx"])
    # the host mirror saw one advance (the capture); the tensor-op form reads the device state, so it follows the replays all the same
    assert ds.draw == draw0 + 1
    ds.use_kernel = False
    assert _eq(ds.sample(views, k, ray_idx=True)["ray_idx"], eager.seed(seed, draw0 + 3).sample(views, k, ray_idx=True)["ray_idx"])


def test_view_outside_the_dataset_in_a_device_tensor(gpu_device):
    """Views handed over as a device tensor cannot be checked on the host: both forms give zero rows and ray_idx -1 for them, and read nothing."""
    import pagnerf_amd
    data = _modes(3, 300, torch.Generator().manual_seed(2))
    ds = pagnerf_amd.DeviceMultiviewDataset(data, gpu_device).seed(3, 1)
    views = torch.tensor([1, 3, -1, 2], dtype=torch.int32, device=gpu_device)
    out = ds.sample(views, 100, ray_idx=True)
    good = ds.sample([1, 2], 100, ray_idx=True)
    ds.use_kernel = False
    form = ds.sample(views, 100, ray_idx=True)
    for key in ("imgs", "semantics", "u7", "h3", "ray_idx"):
        assert _eq(out[key][[0, 3]], good[key]) and _eq(out[key], form[key]), key
        assert bool((out[key][[1, 2]] == (-1 if key == "ray_idx" else 0)).all()), key
    assert _eq(out["base_rays"].dirs, form["base_rays"].dirs) and float(out["base_rays"].dirs[[1, 2]].abs().sum()) == 0.0
    assert out["cam_id"].tolist() == form["cam_id"].tolist() == [1, 3, -1, 2] and _eq(out["cam_idx"], form["cam_idx"])


def test_batch_sampler_epoch_without_host_sync(gpu_device):
    """V = 5, batches of 2, n = 64, k = 16: an epoch under torch.cuda.set_sync_debug_mode("error") (any wait for the device raises), then equal to the
    CPU form's batches."""
    import pagnerf_amd
    gen = torch.Generator().manual_seed(4)
    data = {"imgs": torch.rand(5, 8, 8, 3, generator=gen), "semantics": torch.randint(0, 6, (5, 64, 1), generator=gen),
            "rays": pagnerf_amd.Rays(torch.rand(5, 64, 3, generator=gen), torch.rand(5, 64, 3, generator=gen))}
    ds = pagnerf_amd.DeviceMultiviewDataset(data, gpu_device)
    sampler = pagnerf_amd.BatchSampler(ds, batch_size=2, num_samples=16, seed=9, ray_idx=True)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = list(sampler)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    want = list(pagnerf_amd.BatchSampler(pagnerf_amd.DeviceMultiviewDataset(data, "cpu"), batch_size=2, num_samples=16, seed=9, ray_idx=True))
    assert len(got) == len(want) == len(sampler) == 3 and [g["imgs"].shape for g in got] == [(2, 16, 3), (2, 16, 3), (1, 16, 3)]
    for g, w in zip(got, want):
        assert set(g) == set(w) and g["cam_id"].tolist() == w["cam_id"].tolist()
        for key in ("imgs", "semantics", "ray_idx", "cam_idx"):
            assert _eq(g[key], w[key]), key
        assert _eq(g["rays"].origins, w["rays"].origins) and _eq(g["rays"].dirs, w["rays"].dirs)
    assert ds.draw == 3 and ds.state.tolist() == [9, 3]


def test_sample_rays_transform_on_device_tensors(gpu_device):
    import pagnerf_amd
    from pagnerf_amd.dataset import sample_indices
    gen = torch.Generator().manual_seed(6)
    imgs, o, d = torch.rand(3, 100, 4, generator=gen), torch.rand(3, 100, 3, generator=gen), torch.rand(3, 100, 3, generator=gen)
    batch = {"imgs": imgs.to(gpu_device), "rays": pagnerf_amd.Rays(o.to(gpu_device), d.to(gpu_device)), "filenames": ["a", "b", "c"]}
    out = pagnerf_amd.SampleRays(30, seed=2)(batch)
    assert list(out) == ["imgs", "rays"] and out["imgs"].is_cuda
    idx = sample_indices(100, 10, 2, 0, [0, 1, 2])
    assert _eq(out["imgs"], imgs[torch.arange(3)[:, None], idx]) and _eq(out["rays"].dirs, d[torch.arange(3)[:, None], idx])
    one = pagnerf_amd.SampleRays(7, seed=2)({"imgs": batch["imgs"][1], "rays": batch["rays"][1]})
    assert _eq(one["imgs"], imgs[1][sample_indices(100, 7, 2, 0, 0)]) and one["rays"].origins.shape == (7, 3)


def _scene(gpu_device):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import train_synthetic as TS
    ds = TS.scene_images(8, 32, 32, gpu_device)
    assert (ds.num_imgs, ds.num_pixels) == (8, 1024) and ds.modes == ["imgs", "semantics", "instance", "rays"]
    return TS, ds


def test_analytic_scene_batches_carry_their_ground_truth(gpu_device):
    """scripts/train_synthetic.py --from-images 8 32x32: every ray of every batch of an epoch comes with the colour and labels the closed form gives for
    THAT ray (the gather keeps the modes aligned), each view's pixels are distinct, and an epoch deals every view once."""
    import pagnerf_amd
    TS, ds = _scene(gpu_device)
    seen = []
    for batch in pagnerf_amd.BatchSampler(ds, batch_size=4, num_samples=256, seed=123, drop_last=True, ray_idx=True):
        rays, gt = TS.batch_to_step(batch)
        assert rays.origins.shape == (1024, 3) and (rays.dist_min, rays.dist_max) == (0.0, 1.9)
        rgb, sem, inst = TS.scene_truth(rays.origins.cpu(), rays.dirs.cpu())
        assert torch.allclose(gt["rgb"].cpu(), rgb, rtol=0, atol=1e-6)          # sin() of a vectorised loop may differ in the last bit with the row's position
        assert torch.equal(gt["sem"].cpu(), sem) and torch.equal(gt["inst"].cpu(), inst)
        assert all(len(set(row)) == 256 for row in batch["ray_idx"].tolist())
        seen += batch["cam_id"].tolist()
    assert sorted(seen) == list(range(8))


def test_analytic_scene_trains_from_images(gpu_device):
    """scripts/train_synthetic.py --from-images 8 32x32: 20 steps of the script's train step fed by BatchSampler; the loss is finite and lower at the end
    than at the start.  The run keeps the trainer's schedule under configs/bup20/best.yaml (sem_epoch_start = inst_epoch_start = 601,
    pc_nerf/trainer.py:400-432): the 20 steps are epochs 0 - 9, which render and supervise rgb alone (L1 x 10), so the loss is the same quantity at
    both ends: measured on an MI355X 3.8186 at step 1, 2.0482 at step 20 (1.6975 at step 40; fp32 3.8187 / 2.0470).  This departs from the script's
    default step on purpose, and the all-terms step is exercised by the next test.
    With all three terms from the first step (--panoptic-epoch-start 0, what the script's default path does) the step overshoots before it learns,
    with either input: measured on an MI355X at 1024 rays x 48 samples, loss of step 1 / 10 / 15 / 20 / 30 / 40 = 5695 / 9379 / 31634 / 13529 / 4705 /
    4800 from images and 5686 / 9884 / 25753 / 12842 / 5620 / 5019 on fresh random rays (instance NLL x 1000, grid learning rate 0.1)."""
    import types
    TS, ds = _scene(gpu_device)
    a = types.SimpleNamespace(rays=1024, samples=48, grid="permuto", batch_images=4, graphs="off", panoptic_epoch_start=601)
    _, _, losses = TS.train_from_images("bf16", a, gpu_device, ds, steps=20)
    losses = losses.float().cpu()
    print("losses", [round(float(x), 4) for x in losses])
    assert losses.shape == (20,) and bool(torch.isfinite(losses).all())
    assert float(losses[0]) < 100.0                                     # rgb L1 x 10 alone: no x 1000 instance term in it
    assert float(losses[-1]) < float(losses[0])


def test_analytic_scene_all_terms_from_the_sampler(gpu_device):
    """The same 20 steps with every term from the first step (--panoptic-epoch-start 0): the sampler's semantics and instance modes supervise the step.
    The first loss carries the instance term - 1000 x NLL of a 200-way head near its uniform start, ln 200 = 5.3 - and every loss is finite.  That it
    is NOT below the start after 20 steps is the overshoot recorded in the test above; it is so on fresh random rays too."""
    import types
    TS, ds = _scene(gpu_device)
    a = types.SimpleNamespace(rays=1024, samples=48, grid="permuto", batch_images=4, graphs="off", panoptic_epoch_start=0)
    _, _, losses = TS.train_from_images("bf16", a, gpu_device, ds, steps=20)
    losses = losses.float().cpu()
    print("losses", [round(float(x), 1) for x in losses])
    assert losses.shape == (20,) and bool(torch.isfinite(losses).all())
    assert 0.5 * 5298.0 < float(losses[0]) < 2.0 * 5298.0
