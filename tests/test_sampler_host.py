"""The device-resident dataset's sampling definition on the CPU (pagnerf_amd/dataset.py): the keyed permutation (bijection, slot independence,
determinism, sensitivity, uniformity), epoch_views, the gather and collation against the reference's SampleRays output in tests/golden/g18_sample_rays.npz
(made by tests/golden/make_golden_sample_rays.py from datasets/transforms/ray_sampler.py), BatchSampler / SampleRays on CPU tensors, and the C ABI's
argument refusals.  The kernel itself: tests/test_gpu_sampler.py."""
import ctypes
import math

import pytest
import torch

from conftest import golden

SIZES = (1, 2, 3, 4, 5, 7, 16, 17, 255, 256, 257, 1000, 4097, 921600)


@pytest.mark.parametrize("n", SIZES)
def test_full_draw_is_a_permutation(n):
    from pagnerf_amd.dataset import sample_indices
    p = sample_indices(n, n, seed=3, draw=5, view=1)
    assert p.dtype == torch.int64 and p.shape == (n,)
    assert torch.equal(torch.sort(p).values, torch.arange(n))
    q = sample_indices(n, n + 7, seed=3, draw=5, view=1)                     # randperm(n)[:k] with k > n: n rows
    assert torch.equal(p, q)


def test_slot_independence_and_determinism():
    from pagnerf_amd.dataset import sample_indices
    for n, k, a in ((1000, 100, 37), (4097, 300, 1), (17, 17, 16), (921600, 4096, 1365)):
        whole = sample_indices(n, k, 9, 2, 4)
        assert torch.equal(whole, sample_indices(n, k, 9, 2, 4))
        assert torch.equal(torch.cat([sample_indices(n, k, 9, 2, 4, 0, a), sample_indices(n, k, 9, 2, 4, a, k - a)]), whole)
        assert torch.equal(sample_indices(n, k // 2 + 1, 9, 2, 4), whole[:k // 2 + 1])          # k does not enter slot j
        assert torch.equal(sample_indices(n, n, 9, 2, 4, 5, 3), whole[5:8])
        assert len(set(whole.tolist())) == k
    assert sample_indices(5, 3, 0, 0, 0, 3, 0).shape == (0,)


def test_keys_and_batched_form_agree_with_the_scalar_definition():
    """round_keys() in Python ints is what csrc/sample.hip computes per thread; the tensor form over lists of draws / views gives the same rows."""
    from pagnerf_amd import dataset as D
    for seed, draw, view in ((0, 0, 0), (3, 5, 1), (-1, (1 << 40) + 9, 77), ((1 << 63) + 5, -2, 2 ** 31 - 1)):
        rk = D._round_keys_t(seed, draw, view, D.DOMAIN_RAYS, None)
        assert [int(r) for r in rk] == D.round_keys(seed, draw, view) and len(rk) == D.ROUNDS == 6
    assert D.fmix32(1) == 0x514E28B7 and D.fmix32(0) == 0                          # murmur3's finaliser
    assert [D.half_bits(n) for n in (1, 2, 4, 5, 16, 17, 256, 257, 921600, 1 << 30)] == [1, 1, 1, 2, 2, 3, 4, 5, 10, 15]
    rows = D.sample_indices(1000, 50, 4, [7, 8, 1 << 33], [2, 0, 2])
    for b, (d, v) in enumerate(((7, 2), (8, 0), (1 << 33, 2))):
        assert torch.equal(rows[b], D.sample_indices(1000, 50, 4, d, v))
    assert D.sample_indices(1000, 50, 4, 7, []).shape == (0, 50)


def test_every_key_word_changes_the_draw():
    from pagnerf_amd.dataset import sample_indices
    n = 1000
    base = sample_indices(n, n, 7, 11, 3)
    for other in (sample_indices(n, n, 7, 12, 3), sample_indices(n, n, 7, 11, 4), sample_indices(n, n, 8, 11, 3),
                  sample_indices(n, n, 7, 11 + (1 << 32), 3), sample_indices(n, n, 7 + (1 << 32), 11, 3), sample_indices(n, n, -7, 11, 3)):
        assert int((other != base).sum()) > n // 2


def test_arguments_are_checked():
    from pagnerf_amd.dataset import sample_indices, epoch_views
    for bad in (dict(n=0, k=1), dict(n=(1 << 30) + 1, k=1), dict(n=5, k=0), dict(n=5, k=3, slot_begin=2, slot_count=2), dict(n=5, k=9, slot_begin=0, slot_count=6),
                dict(n=5, k=3, slot_begin=-1, slot_count=1)):
        with pytest.raises(ValueError):
            sample_indices(seed=0, draw=0, view=0, **bad)
    assert sample_indices(1 << 30, 4, 0, 0, 0).max() < (1 << 30)
    with pytest.raises(ValueError):
        epoch_views(5, 0, 0, 0)


@pytest.mark.parametrize("n,k,T", [(1000, 100, 2000), (300, 64, 3000), (7, 7, 4000)])
def test_uniformity(n, k, T):
    """Over T draws: the inclusion count of each pixel against T k / n - a chi-square whose variance under sampling WITHOUT replacement is smaller by the
    finite-population factor (1 - k / n), by which it is divided - and the slot-0 value against T / n.  Both below dof + 6 sqrt(2 dof), dof = n - 1: the
    six-sigma tail of the chi-square distribution.  With k = n every pixel is included in every draw: the statistic is 0 / 0 there, and the condition is
    that every count is exactly T."""
    from pagnerf_amd.dataset import sample_indices
    p = sample_indices(n, k, seed=11, draw=torch.arange(T), view=2)            # [T, k]: row d is draw d
    assert torch.equal(p[T // 2], sample_indices(n, k, seed=11, draw=T // 2, view=2))
    inc = torch.bincount(p.reshape(-1), minlength=n).double()
    first = torch.bincount(p[:, 0], minlength=n).double()
    bound = (n - 1) + 6.0 * math.sqrt(2.0 * (n - 1))
    chi_first = float(((first - T / n) ** 2 / (T / n)).sum())
    if k == n:
        assert bool((inc == T).all())
        chi_inc = 0.0
    else:
        chi_inc = float(((inc - T * k / n) ** 2 / (T * k / n)).sum()) / (1.0 - k / n)
    print("n %d k %d T %d: inclusion %.1f, slot 0 %.1f, bound %.1f" % (n, k, T, chi_inc, chi_first, bound))
    assert chi_inc < bound and chi_first < bound


def test_epoch_views():
    from pagnerf_amd.dataset import epoch_views
    for V, bs in ((5, 2), (6, 6), (7, 3), (1, 4), (100, 6)):
        b = epoch_views(V, bs, seed=1, epoch=0)
        assert [len(x) for x in b] == [bs] * (V // bs) + ([V % bs] if V % bs else [])           # DataLoader(batch_size, drop_last=False)
        assert sorted(torch.cat(b).tolist()) == list(range(V)) and all(x.dtype == torch.int64 for x in b)
        d = epoch_views(V, bs, seed=1, epoch=0, drop_last=True)
        assert [len(x) for x in d] == [bs] * (V // bs) and all(torch.equal(x, y) for x, y in zip(d, b))
    e0, e1, s1 = (torch.cat(epoch_views(100, 6, seed=s, epoch=e)) for s, e in ((1, 0), (1, 1), (2, 0)))
    assert int((e0 != e1).sum()) > 50 and int((e0 != s1).sum()) > 50
    from pagnerf_amd.dataset import sample_indices
    assert not torch.equal(e0, sample_indices(100, 100, 1, 0, 0))                                # its own key domain


def _dataset_from(g, tag, device="cpu"):
    import pagnerf_amd
    data = {}
    for key in g[tag + "_in_keys"].tolist():
        if key == "rays":
            o, d = (torch.from_numpy(g["%s_in_rays.%s" % (tag, f)]) for f in ("origins", "dirs"))
            if tag == "single":
                o, d = o[None], d[None]
            data[key] = pagnerf_amd.Rays(o, d, dist_min=0.25, dist_max=3.0)
        elif "%s_in_%s" % (tag, key) in g.files:
            t = torch.from_numpy(g["%s_in_%s" % (tag, key)])
            data[key] = t[None] if tag == "single" else t
        else:
            data[key] = "excluded"                       # cameras / cameras_ts / filenames: never touched
    return pagnerf_amd.DeviceMultiviewDataset(data, device), data


@pytest.mark.parametrize("tag", ["single", "batch"])
def test_gather_reproduces_the_reference_sample_rays(tag):
    """The reference's SampleRays output (both modes), from the pixel indices it chose (imgs channel 0): keys, shapes, dtypes and every value."""
    g = golden("g18_sample_rays.npz")
    ds, data = _dataset_from(g, tag)
    V = 1 if tag == "single" else int(g["meta"][3])
    k = int(g["meta"][2]) if tag == "single" else int(g["meta"][4]) // V
    assert ds.num_imgs == V and ds.num_pixels == int(g["meta"][1])
    out_keys = g[tag + "_out_keys"].tolist()
    assert ds.modes == out_keys and not set(ds.modes) & {"cameras", "cameras_ts", "filenames"}
    idx = torch.from_numpy(g[tag + "_out_imgs"][..., 0]).long().reshape(V, k)
    out = ds.gather(list(range(V)), idx, ray_idx=True)
    assert set(out) == set(out_keys) | {"cam_id", "cam_idx", "ray_idx"}
    for key in out_keys:
        fields = [("rays.origins", out[key].origins), ("rays.dirs", out[key].dirs)] if key == "rays" else [(key, out[key])]
        for name, got in fields:
            want = torch.from_numpy(g["%s_out_%s" % (tag, name)])
            got = got[0] if tag == "single" else got
            assert got.dtype == want.dtype and got.shape == want.shape and got.is_contiguous(), name
            assert torch.equal(got, want), name
    assert (out["rays"].dist_min, out["rays"].dist_max) == (0.25, 3.0)
    assert out["cam_id"].tolist() == list(range(V)) and out["cam_idx"].tolist() == [v for v in range(V) for _ in range(k)]
    assert torch.equal(out["ray_idx"], idx)


def _toy(V=5, n=64, seed=0):
    import pagnerf_amd
    gen = torch.Generator().manual_seed(seed)
    pix = torch.arange(V * n, dtype=torch.float32).reshape(V, n, 1)
    return {"imgs": torch.cat([pix, torch.rand(V, n, 3, generator=gen)], -1).reshape(V, 8, n // 8, 4),           # [V, H, W, C]
            "semantics": torch.randint(0, 6, (V, n, 1), generator=gen),
            "rays": pagnerf_amd.Rays(torch.rand(V, n, 3, generator=gen), torch.rand(V, n, 3, generator=gen), dist_min=0.1, dist_max=2.0),
            "base_rays": pagnerf_amd.Rays(torch.zeros(8, n // 8, 3), torch.rand(8, n // 8, 3, generator=gen)),
            "cameras": {"a": 1}, "filenames": ["x"] * V}


def test_sample_is_the_definition_on_cpu_tensors():
    import pagnerf_amd
    from pagnerf_amd.dataset import sample_indices
    data = _toy()
    ds = pagnerf_amd.DeviceMultiviewDataset(data, "cpu").seed(4, draw=2)
    assert (ds.num_imgs, ds.num_pixels, ds.modes) == (5, 64, ["imgs", "semantics", "rays", "base_rays"]) and len(ds) == 5
    out = ds.sample([3, 0, 3], 16, ray_idx=True)
    for b, v in enumerate((3, 0, 3)):
        idx = sample_indices(64, 16, 4, 2, v)
        assert torch.equal(out["ray_idx"][b], idx)
        assert torch.equal(out["imgs"][b], data["imgs"].reshape(5, 64, 4)[v, idx]) and torch.equal(out["imgs"][b, :, 0], (v * 64 + idx).float())
        assert torch.equal(out["rays"].dirs[b], data["rays"].dirs[v, idx])
        assert torch.equal(out["base_rays"].dirs[b], data["base_rays"].dirs.reshape(64, 3)[idx])
    assert torch.equal(out["ray_idx"][0], out["ray_idx"][2]) and not torch.equal(out["ray_idx"][0], out["ray_idx"][1])    # the view is part of the key
    assert out["cam_id"].tolist() == [3, 0, 3] and out["cam_idx"].dtype == torch.int32 and out["cam_idx"].tolist() == [3] * 16 + [0] * 16 + [3] * 16
    assert "ray_idx" not in ds.sample([1], 16)
    # slices of the slots concatenate to the batch; more samples than pixels = every pixel; out= buffers are filled in place
    parts = [ds.sample([3, 0, 3], 16, slots=s, ray_idx=True) for s in ((0, 5), (5, 11))]
    assert torch.equal(torch.cat([p["imgs"] for p in parts], 1), out["imgs"]) and torch.equal(torch.cat([p["ray_idx"] for p in parts], 1), out["ray_idx"])
    assert ds.sample([2], 1000)["imgs"].shape == (1, 64, 4)
    buf = ds.empty_batch(3, 16, ray_idx=True)
    assert ds.sample([3, 0, 3], 16, out=buf) is buf and torch.equal(buf["imgs"], out["imgs"]) and torch.equal(buf["rays"].origins, out["rays"].origins)
    assert torch.equal(buf["ray_idx"], out["ray_idx"]) and buf["cam_id"].tolist() == [3, 0, 3]
    ds.advance()
    assert ds.draw == 3 and ds.state.tolist() == [4, 3]
    assert torch.equal(ds.sample([1], 16, ray_idx=True)["ray_idx"][0], sample_indices(64, 16, 4, 3, 1))
    with pytest.raises(IndexError):
        ds.sample([5], 4)
    with pytest.raises(ValueError):
        pagnerf_amd.DeviceMultiviewDataset({"imgs": torch.zeros(2, 6, 3), "semantics": torch.zeros(2, 7, 1)}, "cpu")


def test_batch_sampler_on_cpu_tensors():
    import pagnerf_amd
    from pagnerf_amd.dataset import epoch_views, sample_indices
    ds = pagnerf_amd.DeviceMultiviewDataset(_toy(), "cpu")
    bs = pagnerf_amd.BatchSampler(ds, batch_size=2, num_samples=16, seed=6, ray_idx=True)
    assert len(bs) == 3 and len(pagnerf_amd.BatchSampler(ds, 2, 16, drop_last=True)) == 2 and len(pagnerf_amd.BatchSampler(ds, 5, 16)) == 1
    bs = pagnerf_amd.BatchSampler(ds, batch_size=2, num_samples=16, seed=6, ray_idx=True)
    draw = 0
    for epoch in range(2):
        batches = list(bs)
        views = epoch_views(5, 2, 6, epoch)
        assert [b["imgs"].shape[0] for b in batches] == [2, 2, 1]
        for b, v in zip(batches, views):
            assert b["cam_id"].tolist() == v.tolist()
            assert torch.equal(b["ray_idx"], torch.stack([sample_indices(64, 16, 6, draw, int(w)) for w in v]))
            draw += 1
    assert ds.draw == 6
    bs.set_epoch(0)
    assert [b["cam_id"].tolist() for b in bs] == [v.tolist() for v in epoch_views(5, 2, 6, 0)]


def test_store_uint8_takes_exact_images_only():
    import pagnerf_amd
    u = torch.randint(0, 256, (2, 9, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    u[0, 0] = torch.tensor([0, 255, 1])
    img = u.float() / 255
    ds = pagnerf_amd.DeviceMultiviewDataset({"imgs": img}, "cpu", store_uint8=("imgs",))
    assert ds._leaves[0].src.dtype == torch.uint8 and ds.nbytes == 2 * 9 * 3
    out = ds.sample([1, 0], 9, ray_idx=True)
    assert out["imgs"].dtype == torch.float32 and torch.equal(out["imgs"], img[torch.tensor([[1], [0]]), out["ray_idx"]])
    bad = img.clone()
    bad[1, 4, 2] += 1e-4
    with pytest.raises(ValueError):
        pagnerf_amd.DeviceMultiviewDataset({"imgs": bad}, "cpu", store_uint8=("imgs",))
    with pytest.raises(ValueError):
        pagnerf_amd.DeviceMultiviewDataset({"imgs": img * 1.5}, "cpu", store_uint8=("imgs",))
    with pytest.raises(ValueError):
        pagnerf_amd.DeviceMultiviewDataset({"imgs": img.half()}, "cpu", store_uint8=("imgs",))


def test_sample_rays_transform_on_cpu_tensors():
    """The reference's transform name, both modes: rows of every mode at one draw's pixels, the excluded keys dropped, a new draw per call."""
    import pagnerf_amd
    from pagnerf_amd.dataset import sample_indices
    data = _toy()
    item = {"imgs": data["imgs"].reshape(5, 64, 4)[2], "semantics": data["semantics"][2], "rays": data["rays"][2], "cameras": None, "filenames": "x"}
    tf = pagnerf_amd.SampleRays(10, seed=3)
    a, b = tf(item), tf(item)
    assert list(a) == ["imgs", "semantics", "rays"] and a["imgs"].shape == (10, 4) and a["rays"].origins.shape == (10, 3)
    idx = sample_indices(64, 10, 3, 0, 0)
    assert torch.equal(a["imgs"], item["imgs"][idx]) and torch.equal(a["rays"].dirs, item["rays"].dirs[idx]) and torch.equal(a["semantics"], item["semantics"][idx])
    assert torch.equal(b["imgs"], item["imgs"][sample_indices(64, 10, 3, 1, 0)])
    batch = {"imgs": data["imgs"].reshape(5, 64, 4)[:3], "rays": data["rays"][:3], "base_rays": data["base_rays"].reshape(64, 3)}
    out = pagnerf_amd.SampleRays(30, seed=3)(batch)
    assert out["imgs"].shape == (3, 10, 4) and out["base_rays"].dirs.shape == (3, 10, 3)
    for v in range(3):
        idx = sample_indices(64, 10, 3, 0, v)
        assert torch.equal(out["imgs"][v], batch["imgs"][v, idx]) and torch.equal(out["base_rays"].dirs[v], batch["base_rays"].dirs[idx])
    with pytest.raises(NotImplementedError):
        pagnerf_amd.SampleRays(4)({"rays": data["rays"].reshape(5, 8, 8, 3), "imgs": data["imgs"]})


def test_public_names():
    import pagnerf_amd
    for n in ("DeviceMultiviewDataset", "BatchSampler", "SampleRays", "sample_indices", "epoch_views"):
        assert getattr(pagnerf_amd, n) is getattr(pagnerf_amd.dataset, n)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib
    return _lib.load()


def test_sample_entry_points_validate_without_gpu(lib):
    """pag_sample_batch / pag_sample_advance refuse NULL pointers, n outside [1, 2^30], k <= 0, more than 12 modes, row_bytes <= 0, slots outside
    [0, min(k, n)) and a conversion that does not fit row_bytes before any launch; an empty batch is a no-op."""
    from pagnerf_amd import _lib as L
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)

    def modes(*rows):
        arr = (L.SampleMode * max(1, len(rows)))()
        for a, (src, dst, row_bytes, per_view, convert) in zip(arr, rows):
            a.src, a.dst, a.row_bytes, a.per_view, a.convert = src, dst, row_bytes, per_view, convert
        return arr

    ok = modes((p, p, 4, 1, 0))
    call = lambda state=p, views=p, B=2, V=3, n=100, k=10, begin=0, count=10, m=ok, nm=1, ridx=None, cidx=None: \
        lib.pag_sample_batch(state, views, B, V, n, k, begin, count, m, nm, ridx, cidx, None)
    assert call(B=0) == 0 and call(count=0) == 0 and call(B=0, state=None, views=None, m=None, nm=0) == 0                     # nothing to do
    assert call(state=None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert call(views=None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert call(m=None) == -1 and b"NULL" in lib.pag_last_error_string()
    assert call(m=modes((None, p, 4, 1, 0))) == -1 and b"NULL" in lib.pag_last_error_string()
    assert call(m=modes((p, None, 4, 1, 0))) == -1 and b"NULL" in lib.pag_last_error_string()
    for n in (0, -1, (1 << 30) + 1):
        assert call(n=n) == -1 and b"2^30" in lib.pag_last_error_string()
    for k in (0, -3):
        assert call(k=k) == -1 and b"k " in lib.pag_last_error_string()
    assert call(m=(L.SampleMode * 13)(), nm=13) == -1 and b"n_modes" in lib.pag_last_error_string()
    for rb in (0, -4):
        assert call(m=modes((p, p, rb, 1, 0))) == -1 and b"row_bytes" in lib.pag_last_error_string()
    for begin, count, n, k in ((5, 6, 100, 10), (0, 11, 100, 10), (0, 8, 7, 10), (-1, 2, 100, 10), (0, -1, 100, 10)):
        assert call(begin=begin, count=count, n=n, k=k) == -1 and b"slots" in lib.pag_last_error_string()
    assert call(m=modes((p, p, 6, 1, 1))) == -1 and b"multiple of 4" in lib.pag_last_error_string()                            # uint8 -> f32 rows are 4 C bytes
    assert call(m=modes((p, p, 4, 1, 2))) == -1 and b"conversion" in lib.pag_last_error_string()
    assert call(B=70000) == -1 and call(V=0) == -1
    assert lib.pag_sample_advance(None, None) == -1 and b"NULL" in lib.pag_last_error_string()


def test_copy_width_is_the_widest_aligned_one(lib):
    """16 / 8 / 4 / 2 / 1 bytes: the widest that divides the row and both base addresses; 4 or 1 source bytes per step for the conversion."""
    from pagnerf_amd import _lib as L
    w = lambda src, dst, rb, conv=L.SAMPLE_COPY: lib.pag_sample_copy_width(src, dst, rb, conv)
    base = 1 << 20
    assert [w(base, base, rb) for rb in (1, 2, 3, 4, 6, 7, 8, 12, 16, 24, 32, 48)] == [1, 2, 1, 4, 2, 1, 8, 4, 16, 8, 16, 16]
    assert w(base + 1, base, 16) == 1 and w(base, base + 2, 16) == 2 and w(base + 4, base, 16) == 4 and w(base + 8, base + 16, 32) == 8
    assert w(base, base, 0) == 0 and w(base, base, 4, 7) == 0
    assert w(base, base, 16, L.SAMPLE_U8_TO_F32) == 4 and w(base, base, 12, L.SAMPLE_U8_TO_F32) == 1 and w(base + 1, base, 16, L.SAMPLE_U8_TO_F32) == 1
    assert w(base, base + 4, 16, L.SAMPLE_U8_TO_F32) == 1 and w(base, base, 6, L.SAMPLE_U8_TO_F32) == 0
