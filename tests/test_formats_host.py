"""The NeRF-standard loader on the CPU (pagnerf_amd/formats.py): the definition's fixed points, the ray geometry against pinhole algebra written here,
consistency with the pose pipeline's algebra, the loader end to end on folders written into a temp dir, and the C ABI's argument refusals.
The kernels themselves: tests/test_gpu_formats.py."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import formats_scene as S


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """The three-JSON folder with labels, and its CPU load (left unchanged by the tests that share it)."""
    from pagnerf_amd import formats
    root = str(tmp_path_factory.mktemp("three"))
    truth = S.write_folder(root, "three")
    return root, truth, formats.load_nerf_standard(root, "train", mip=1, device="cpu")


# ----------------------------------------------------------------------------------------------------------------------------- the definition
def test_definition_fixed_points():
    from pagnerf_amd.formats import prepare_labels_reference, prepare_views_reference
    src = S.source(2, 6, 10, 3, seed=1)
    imgs, masks = prepare_views_reference(src, 0, "white")
    assert imgs.dtype == torch.float32 and imgs.shape == (2, 6, 10, 3) and masks.dtype == torch.bool and masks.shape == (2, 6, 10, 1)
    assert torch.equal(imgs, torch.from_numpy(src.numpy().astype(np.float32) / np.float32(255))) and bool(masks.all())          # u8 / 255 exactly
    for mip in (1, 2):                                                                                                          # a constant block gives its value
        const = torch.full((1, 8, 12, 3), 77, dtype=torch.uint8)
        out = prepare_views_reference(const, mip, "black")[0]
        assert out.shape == (1, 8 >> mip, 12 >> mip, 3) and torch.equal(out, torch.full_like(out, float(np.float32(77) / np.float32(255))))
    px = torch.tensor([[[[200, 100, 50, 0], [200, 100, 50, 255], [9, 9, 9, 128], [9, 9, 9, 127]]]], dtype=torch.uint8)          # [1,1,4,4]
    white, mw = prepare_views_reference(px, 0, "white")
    black, mb = prepare_views_reference(px, 0, "black")
    assert torch.equal(white[0, 0, 0], torch.ones(3)) and torch.equal(black[0, 0, 0], torch.zeros(3))                           # a = 0
    opaque = torch.from_numpy(np.array([200, 100, 50], dtype=np.float32) / np.float32(255))
    assert torch.equal(white[0, 0, 1], opaque) and torch.equal(black[0, 0, 1], opaque)                                          # a = 1
    assert mw.reshape(-1).tolist() == mb.reshape(-1).tolist() == [False, True, True, False]                                     # 128/255 > 0.5 >= 127/255
    a = np.float32(128) / np.float32(255)
    assert float(white[0, 0, 2, 0]) == float(np.float32(np.float32(np.float32(9) / np.float32(255)) * a) + np.float32(np.float32(1) - a))
    lab = torch.arange(2 * 4 * 8, dtype=torch.uint8).reshape(2, 4, 8)
    assert torch.equal(prepare_labels_reference(lab, 1), lab[:, ::2, ::2].long()[..., None]) and prepare_labels_reference(lab, 2).shape == (2, 1, 2, 1)
    assert torch.equal(prepare_labels_reference(lab, 1).float()[:, :, :, 0],
                       torch.nn.functional.interpolate(lab[:, None].float(), scale_factor=0.5, mode="nearest")[:, 0])
    for bad in (torch.zeros(1, 6, 10, 4, dtype=torch.uint8), torch.zeros(1, 8, 10, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="divisible"):
            prepare_views_reference(bad, 2, "white")
    with pytest.raises(ValueError, match="divisible"):
        prepare_labels_reference(torch.zeros(1, 5, 4, dtype=torch.uint8), 1)
    with pytest.raises(ValueError):
        prepare_views_reference(torch.zeros(1, 4, 4, 2, dtype=torch.uint8), 0, "white")


def test_block_mean_matches_float64_mean():
    """The single division of the integer block sum is the float64 mean of the u / 255 values, rounded once."""
    from pagnerf_amd.formats import prepare_views_reference
    src = S.source(2, 8, 12, 3, seed=2)
    for mip in (1, 2):
        f = 1 << mip
        exact = (src.double().reshape(2, 8 // f, f, 12 // f, f, 3).sum((2, 4)) / (255.0 * f * f)).float()
        assert torch.equal(prepare_views_reference(src, mip, "white")[0], exact)


# --------------------------------------------------------------------------------------------------------------------------------- geometry
def test_rays_hit_the_projected_point():
    """Three poses (two of them not axis-aligned), non-zero cx / cy: a world point that plain pinhole algebra projects onto the centre of pixel
    (row j, col i) lies on that pixel's ray, in front of the camera.  The expected values use nothing of the package's ray code."""
    from pagnerf_amd.formats import rays_reference, standard_cameras
    w, h, angle, cx, cy = 8, 6, 0.8, 4.6, 2.7
    R = np.concatenate([np.eye(3)[None], S.rotations(2, seed=5)])
    t = np.array([[0.0, 0.0, 0.0], [0.3, -0.7, 1.1], [-1.2, 0.4, 0.2]])
    frames = []
    for r, tt in zip(R, t):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = r, tt
        frames.append(dict(transform_matrix=T.tolist()))
    meta = dict(camera_angle_x=angle, cx=cx, cy=cy, aabb_scale=1.0, frames=frames)
    for basis, Bm in ((None, np.eye(3)), ("default", np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]]))):          # x' = x, y' = z, z' = -y
        fx, fy, x0, y0, c2w, views = standard_cameras(meta, w, h, 0, **({} if basis else dict(world_basis=None)))
        focal = 0.5 * w / math.tan(0.5 * angle)
        assert fx == fy == focal
        rays = rays_reference(c2w, w, h, fx, fy, x0, y0)
        assert rays.origins.shape == rays.dirs.shape == (3, h, w, 3) and (rays.dist_min, rays.dist_max) == (0.0, 6.0)
        for v in range(3):
            Rw, tw = Bm @ R[v], Bm @ t[v]
            assert np.allclose(c2w[v].numpy(), np.concatenate([Rw, tw[:, None]], 1), atol=1e-7)
            assert np.allclose(views[v].numpy() @ np.concatenate([np.concatenate([Rw, tw[:, None]], 1), [[0, 0, 0, 1.0]]]), np.eye(4), atol=1e-6)
            for j, i, depth in ((0, 0, 1.0), (2, 5, 2.5), (5, 7, 0.7), (3, 4, 4.0)):
                # pinhole: u = cx + f Xc / (-Zc), v = cy - f Yc / (-Zc) for a camera that looks down -z with y up; pixel centre (i + 0.5, j + 0.5)
                Xc = np.array([(i + 0.5 - cx) * depth / focal, -(j + 0.5 - cy) * depth / focal, -depth])
                X = Rw @ Xc + tw
                o, d = rays.origins[v, j, i].double().numpy(), rays.dirs[v, j, i].double().numpy()
                assert np.array_equal(rays.origins[v, j, i].numpy(), c2w[v, :, 3].numpy())
                assert np.linalg.norm(np.cross(d, X - o)) <= 1e-5 * np.linalg.norm(X - o) and d @ (X - o) > 0
                assert abs(np.linalg.norm(d) - 1) <= S.RAY_TOL


def test_odd_sizes_centre_pixel_looks_down_minus_z():
    from pagnerf_amd.formats import rays_reference, standard_cameras
    meta = dict(camera_angle_x=1.0, frames=[dict(transform_matrix=np.eye(4).tolist())])
    fx, fy, x0, y0, c2w, views = standard_cameras(meta, 5, 3, 0, world_basis=None)
    assert (x0, y0) == (0.0, 0.0) and torch.equal(views[0], torch.eye(4))
    rays = rays_reference(c2w, 5, 3, fx, fy, x0, y0)
    assert torch.equal(rays.dirs[0, 1, 2], torch.tensor([0.0, 0.0, -1.0])) and torch.equal(rays.origins[0], torch.zeros(3, 5, 3))
    assert rays.dirs[0, 1, 3, 0] > 0 and rays.dirs[0, 0, 2, 1] > 0           # +x to the right, +y up (image rows go down)


def test_intrinsics_keys():
    from pagnerf_amd.formats import standard_cameras
    fr = [dict(transform_matrix=np.eye(4).tolist())]
    fx, fy, x0, y0, _, _ = standard_cameras(dict(x_fov=60.0, y_fov=40.0, camera_angle_x=0.1, fl_x=7.0, frames=fr), 10, 8, 1)
    assert fx == 5.0 / math.tan(math.radians(30.0)) and fy == 4.0 / math.tan(math.radians(20.0))                   # degrees win over everything
    fx, fy, _, _, _, _ = standard_cameras(dict(camera_angle_x=0.7, camera_angle_y=0.5, fl_x=7.0, frames=fr), 10, 8, 0)
    assert fx == 5.0 / math.tan(0.35) and fy == 4.0 / math.tan(0.25)
    fx, fy, x0, y0, _, _ = standard_cameras(dict(fl_x=30.0, cx=11.0, cy=9.0, frames=fr), 5, 3, 2)                   # focal lengths only without an angle
    assert (fx, fy, x0, y0) == (7.5, 7.5, 11.0 / 4 - 2, 9.0 / 4 - 1)
    with pytest.raises(ValueError, match="x_fov"):
        standard_cameras(dict(frames=fr), 4, 4, 0)
    T = np.eye(4)
    T[:3, 3] = [1.0, 2.0, 3.0]
    _, _, _, _, c2w, _ = standard_cameras(dict(camera_angle_x=1.0, scale=0.5, aabb_scale=2.0, offset=[0.5, 0.0, -1.0], frames=[dict(transform_matrix=T.tolist())]),
                                          4, 4, 0, world_basis=None)
    assert c2w[0, :, 3].tolist() == [0.75, 0.5, -0.25]                                                               # t / aabb_scale * scale + offset
    _, _, _, _, c2w, _ = standard_cameras(dict(camera_angle_x=1.0, aabb_scale=1.0, frames=[dict(transform_matrix=T.tolist())]), 4, 4, 0)
    assert c2w[0, :, 3].tolist() == [1.0, 3.0, -2.0]                                                                 # the default basis: x' = x, y' = z, z' = -y


@pytest.mark.parametrize("B,H0,W0,mip", S.SHAPES + S.WIDE_SHAPES)
def test_fp32_rays_meet_the_kernel_bound(B, H0, W0, mip):
    """The bound the kernel is held to on these inputs (tests/test_gpu_formats.py) is reachable in fp32: the tensor-op form meets it on the CPU."""
    from pagnerf_amd.formats import rays_reference
    h, w = H0 >> mip, W0 >> mip
    c2w = S.camera_to_world(B, seed=H0)
    exact = rays_reference(c2w.double(), w, h, **S.INTRINSICS)
    got = rays_reference(c2w, w, h, **S.INTRINSICS)
    assert got.dirs.dtype == torch.float32 and torch.equal(got.origins, c2w[:, None, None, :, 3].expand(B, h, w, 3))
    assert float((got.dirs.double() - exact.dirs).abs().max()) <= S.RAY_TOL
    assert float((torch.linalg.norm(got.dirs.double(), dim=-1) - 1).abs().max()) <= S.RAY_TOL


# ----------------------------------------------------------------------------------------------------------------------------------- loader
def test_loader_three_json_layout(folder):
    from pagnerf_amd.formats import prepare_labels_reference, prepare_views_reference, rays_reference, standard_cameras
    root, truth, ds = folder
    tr = truth["train"]
    L = S.leaves(ds)
    assert ds.num_imgs == 5 and ds.image_shape == (6, 10) and ds.num_pixels == 60 and ds.filenames == ["r_%d" % i for i in range(5)]
    assert set(ds.modes) == {"imgs", "masks", "rays", "base_rays", "semantics", "instance"} and ds.scale == 0.5
    assert ds.semantic_info == dict(num_classes=5, num_instances=16, things_ids=[2, 3, 4], stuff_ids=[0, 1])
    imgs, masks = prepare_views_reference(torch.from_numpy(tr["images"]), 1, "white")
    assert torch.equal(L[("imgs", None)], imgs.reshape(5, 60, 3)) and torch.equal(L[("masks", None)], masks.reshape(5, 60, 1)) and bool(masks.all())
    for mode in ("semantics", "instance"):
        assert L[(mode, None)].dtype == torch.int64 and torch.equal(L[(mode, None)], prepare_labels_reference(torch.from_numpy(tr[mode]), 1).reshape(5, 60, 1))
    fx, fy, x0, y0, c2w, views = standard_cameras(tr["meta"], 10, 6, 1)
    rays = rays_reference(c2w, 10, 6, fx, fy, x0, y0)
    assert torch.equal(L[("rays", "origins")], rays.origins.reshape(5, 60, 3)) and torch.equal(L[("rays", "dirs")], rays.dirs.reshape(5, 60, 3))
    assert torch.equal(ds.view_matrices, views) and ds._rays_range == dict(rays=(0.0, 6.0), base_rays=(0.0, 6.0))
    assert x0 == (20 / 2 + 0.6) / 2 - 5 and y0 == (12 / 2 - 0.3) / 2 - 3
    from pagnerf_amd import formats
    val = formats.load_nerf_standard(root, "val", mip=0, device="cpu", bg_color="black")
    assert val.num_imgs == 2 and val.image_shape == (12, 20)
    assert torch.equal(S.leaves(val)[("imgs", None)], prepare_views_reference(torch.from_numpy(truth["val"]["images"]), 0, "black")[0].reshape(2, 240, 3))
    with pytest.raises(RuntimeError, match="unsupported"):
        formats.load_nerf_standard(root, "extra", device="cpu")
    with pytest.raises(ValueError, match="divisible"):
        formats.load_nerf_standard(root, "train", mip=3, device="cpu")


def test_rays_agree_with_the_pose_pipeline(folder):
    """base_rays pushed through view_matrices by BAPipeline's algebra, (R^T (o - t), R^T d), are the stored world rays."""
    _, _, ds = folder
    L = S.leaves(ds)
    R, t = ds.view_matrices[:, :3, :3].double(), ds.view_matrices[:, :3, 3].double()
    o = torch.matmul(L[("base_rays", "origins")].double()[None] - t[:, None, :], R)                      # row-vector form of R^T (o - t)
    d = torch.matmul(L[("base_rays", "dirs")].double()[None].expand(5, -1, -1), R)
    assert float((o - L[("rays", "origins")].double()).abs().max()) <= 2e-6
    assert float((d - L[("rays", "dirs")].double()).abs().max()) <= 2e-6


def test_loader_one_json_layout_missing_file_and_no_labels(tmp_path):
    from pagnerf_amd import formats
    truth = S.write_folder(str(tmp_path), "one", n=4, labels=False, missing=(2,), seed=3)
    ds = formats.load_nerf_standard(str(tmp_path), device="cpu")
    assert ds.num_imgs == 3 and ds.filenames == ["0000", "0001", "0003"] and ds.image_shape == (12, 20)
    assert set(ds.modes) == {"imgs", "masks", "rays", "base_rays"} and not hasattr(ds, "semantic_info")
    assert torch.equal(S.leaves(ds)[("imgs", None)], formats.prepare_views_reference(torch.from_numpy(truth["train"]["images"]), 0, "white")[0].reshape(3, 240, 3))
    kept = [f for i, f in enumerate(truth["train"]["meta"]["frames"]) if i != 2]
    assert torch.equal(ds.view_matrices, formats.standard_cameras(dict(truth["train"]["meta"], frames=kept), 20, 12, 0)[5])
    with pytest.raises(RuntimeError, match="unsupported"):
        formats.load_nerf_standard(str(tmp_path), "val", device="cpu")                                  # one JSON: train only
    with open(tmp_path / "second.json", "w") as f:
        json.dump({}, f)
    with pytest.raises(RuntimeError, match="number of splits"):
        formats.load_nerf_standard(str(tmp_path), device="cpu")


def test_partial_labels_are_refused(tmp_path):
    from pagnerf_amd import formats
    S.write_folder(str(tmp_path), "one", n=3, partial=True)
    with pytest.raises(ValueError, match="semantic_path"):
        formats.load_nerf_standard(str(tmp_path), device="cpu")


def test_workers_and_chunks_do_not_change_the_dataset(folder):
    from pagnerf_amd import formats
    root, _, ds = folder
    want = S.leaves(ds)
    view_bytes = 12 * 20 * (3 + 2)
    for kw in (dict(num_workers=3), dict(chunk_bytes=2 * view_bytes), dict(chunk_bytes=1, num_workers=2)):           # 1, 3 and 5 chunks
        got = S.leaves(formats.load_nerf_standard(root, "train", mip=1, device="cpu", **kw))
        assert got.keys() == want.keys()
        for key in want:
            assert torch.equal(got[key], want[key]), (kw, key)


def test_decoders_agree(folder):
    """decode_image (PIL where it imports) and visualize.read_png return the same arrays for what write_png writes."""
    from pagnerf_amd import formats, visualize
    root, truth, _ = folder
    for name, want in (("train/r_0.png", truth["train"]["images"][0]), ("train/sem_0.png", truth["train"]["semantics"][0])):
        a, b = formats.decode_image(os.path.join(root, name)), visualize.read_png(os.path.join(root, name))
        assert a.dtype == np.uint8 and np.array_equal(a, b) and np.array_equal(a, want)


def test_command_line_writes_what_the_trainer_reads(folder, tmp_path):
    from pagnerf_amd import formats
    from pagnerf_amd.dataset import BatchSampler
    from pagnerf_amd.train import load_npz_dataset
    root, _, ds = folder
    out = str(tmp_path / "train.npz")
    assert formats.main([root, "--split", "train", "--mip", "1", "--bg-color", "white", "--out", out, "--device", "cpu"]) == 0
    back = load_npz_dataset(out, "cpu")
    want, got = S.leaves(ds), S.leaves(back)
    assert got.keys() == want.keys()
    for key in want:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    assert back.semantic_info == ds.semantic_info and torch.equal(back.view_matrices, ds.view_matrices) and back.image_shape == ds.image_shape
    assert back.filenames == ds.filenames and back.scale == ds.scale and back._rays_range == ds._rays_range
    batches = list(BatchSampler(back, batch_size=2, num_samples=16, seed=4))
    assert len(batches) == 3 and batches[0]["imgs"].shape == (2, 16, 3) and batches[0]["rays"].dirs.shape == (2, 16, 3)
    assert batches[0]["semantics"].dtype == torch.int64 and batches[0]["masks"].dtype == torch.bool and batches[2]["imgs"].shape == (1, 16, 3)


def test_train_accepts_a_folder(folder):
    """train.load_dataset: a folder goes through the loader with the YAML namespace's mip / bg_color / dataset_num_workers; the keys are known."""
    from pagnerf_amd import config, train
    root, _, ds = folder
    got = train.load_dataset(root, "train", dict(mip=1, bg_color="white", dataset_num_workers=2), torch.device("cpu"))
    for key, want in S.leaves(ds).items():
        assert torch.equal(S.leaves(got)[key], want)
    assert train.load_dataset(root, "val", {}, torch.device("cpu")).image_shape == (12, 20)
    assert {"mip", "bg_color", "dataset_num_workers"} <= config.known_keys()


# ---------------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_prepare_entry_points_validate_without_gpu(lib):
    """pag_prepare_views / pag_prepare_labels refuse NULL pointers, C0 other than 3 / 4, sizes 2^mip does not divide, mip outside [0, 8], views outside
    the destination and an unknown background before any launch; an empty chunk and a call without outputs are no-ops."""
    from pagnerf_amd import _lib as L
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    err = lib.pag_last_error_string

    def views(src=p, B=2, H0=8, W0=12, C0=4, mip=1, bg=1, c2w=p, fx=5.0, fy=5.0, off=0, V=2, imgs=p, masks=p, origins=p, dirs=p):
        return lib.pag_prepare_views(src, B, H0, W0, C0, mip, bg, c2w, fx, fy, 0.0, 0.0, off, V, imgs, masks, origins, dirs, None)

    assert views(B=0) == 0 and views(imgs=None, masks=None, origins=None, dirs=None, src=None, c2w=None) == 0                  # nothing to do
    assert views(src=None) == -1 and b"NULL src" in err()
    assert views(c2w=None) == -1 and b"NULL c2w" in err()
    for C0 in (0, 1, 2, 5):
        assert views(C0=C0) == -1 and b"C0" in err()
    for mip in (-1, 9):
        assert views(mip=mip) == -1 and b"mip" in err()
    for H0, W0, mip in ((9, 12, 1), (8, 10, 2), (8, 12, 3)):
        assert views(H0=H0, W0=W0, mip=mip) == -1 and b"divisible" in err()
    assert views(H0=0) == -1 and views(W0=-4) == -1 and views(B=-1) == -1 and views(B=70000, V=70000) == -1
    for off, V in ((1, 2), (-1, 2), (0, 1), (0, 0)):
        assert views(off=off, V=V) == -1 and b"outside" in err()
    assert views(bg=2) == -1 and b"background" in err()
    assert views(fx=0.0) == -1 and b"focal" in err()
    assert views(fy=float("nan")) == -1 and b"focal" in err()

    def planes(*rows):
        arr = (L.LabelPlane * max(1, len(rows)))()
        for a, (src, dst) in zip(arr, rows):
            a.src, a.dst = src, dst
        return arr

    def labels(pl=planes((p, p)), n=1, B=2, H0=8, W0=12, mip=1, off=0, V=2):
        return lib.pag_prepare_labels(pl, n, B, H0, W0, mip, off, V, None)

    assert labels(B=0) == 0 and labels(pl=None, n=0) == 0
    assert labels(pl=None) == -1 and b"NULL planes" in err()
    assert labels(pl=planes((None, p))) == -1 and b"NULL src" in err()
    assert labels(pl=planes((p, None))) == -1 and b"NULL src" in err()
    assert labels(pl=(L.LabelPlane * 9)(), n=9) == -1 and b"n_planes" in err()
    assert labels(n=-1) == -1 and labels(mip=9) == -1 and labels(H0=7) == -1 and b"divisible" in err()
    assert labels(off=1) == -1 and b"outside" in err()
    assert L.PREPARE_MAX_PLANES == 8 and ctypes.sizeof(L.LabelPlane) == 16


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from pagnerf_amd import ops
    src = torch.zeros(1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.prepare_views(src, 0, "white", imgs=torch.zeros(1, 4, 4, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.prepare_labels([(src[..., 0].contiguous(), torch.zeros(1, 4, 4, 1, dtype=torch.int64))], 0)
