"""pag_prepare_views / pag_prepare_labels (csrc/prepare.hip) against the definition in pagnerf_amd/formats.py at the smallest shapes that can go wrong,
the write discipline of a chunk inside a larger destination, the loader on the device, and a short PanopticTrainer run on a loaded folder."""
import os

import pytest
import torch

import formats_scene as S

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def run_kernel(src, mip, bg, c2w, V=None, off=0, **want):
    """The four outputs (or those named in want) for src as views [off, off + B) of V-view destinations pre-filled with the sentinel."""
    from pagnerf_amd import ops
    dev = src.device
    B, H0, W0, _ = src.shape
    V = B if V is None else V
    h, w = H0 >> mip, W0 >> mip
    out = dict(imgs=torch.full((V, h, w, 3), SENTINEL, device=dev), masks=torch.full((V, h, w, 1), 7, dtype=torch.uint8, device=dev),
               origins=torch.full((V, h, w, 3), SENTINEL, device=dev), dirs=torch.full((V, h, w, 3), SENTINEL, device=dev))
    asked = {k: v for k, v in out.items() if not want or want.get(k)}
    ops.prepare_views(src, mip, bg, off, c2w=c2w, intrinsics=tuple(S.INTRINSICS[k] for k in ("fx", "fy", "x0", "y0")), **asked)
    return out


@pytest.mark.parametrize("bg", ("white", "black"))
@pytest.mark.parametrize("C0", (3, 4))
@pytest.mark.parametrize("B,H0,W0,mip", S.SHAPES + S.WIDE_SHAPES)
def test_kernels_match_the_definition(gpu_device, B, H0, W0, mip, C0, bg):
    from pagnerf_amd import formats, ops
    h, w = H0 >> mip, W0 >> mip
    src = S.source(B, H0, W0, C0, seed=H0 + C0).to(gpu_device)
    c2w_host = S.camera_to_world(B, seed=H0)
    c2w = c2w_host.to(gpu_device)
    got = run_kernel(src, mip, bg, c2w)
    imgs, masks = formats.prepare_views_reference(src, mip, bg)                       # the definition on the same device tensors
    assert torch.equal(got["imgs"], imgs)
    assert torch.equal(got["masks"], masks.to(torch.uint8))
    if C0 == 4:
        assert 0 < int(masks.sum()) < masks.numel()                                    # both sides of the threshold
        assert bool((imgs == (1.0 if bg == "white" else 0.0)).any())                     # a block of alpha 0 is the background
    assert torch.equal(got["origins"], c2w[:, None, None, :, 3].expand(B, h, w, 3))
    exact = formats.rays_reference(c2w_host.double(), w, h, **S.INTRINSICS)           # float64 on the CPU
    dirs = got["dirs"].cpu().double()
    err, norm = float((dirs - exact.dirs).abs().max()), float((torch.linalg.norm(dirs, dim=-1) - 1).abs().max())
    print("dirs max abs error %.3g, | |dir| - 1 | %.3g" % (err, norm))
    assert err <= S.RAY_TOL and norm <= S.RAY_TOL
    # the label planes of the chunk: two in one launch, int64
    g = torch.Generator().manual_seed(W0)
    planes = [torch.randint(0, 256, (B, H0, W0), dtype=torch.uint8, generator=g).to(gpu_device) for _ in range(2)]
    dst = [torch.full((B, h, w, 1), -3, dtype=torch.int64, device=gpu_device) for _ in planes]
    ops.prepare_labels(list(zip(planes, dst)), mip)
    for p, d in zip(planes, dst):
        assert torch.equal(d, formats.prepare_labels_reference(p, mip))
    torch.cuda.synchronize()


def test_unaligned_source_leaves_the_vector_paths(gpu_device):
    """An RGBA chunk that starts at an odd byte, or one or two words past a 16-byte boundary (a view into a larger staging buffer), gives the same bits as
    the aligned one: the entry point picks the byte path, the narrower loads, or - at 16 bytes - the widest ones again."""
    from pagnerf_amd import formats
    for B, H0, W0, mip in ((2, 12, 20, 2), (2, 8, 32, 1)):                               # f = 4: 16-byte loads when aligned; f = 2: 8-byte
        src = S.source(B, H0, W0, 4, seed=9).to(gpu_device)
        flat = torch.zeros(src.numel() + 16, dtype=torch.uint8, device=gpu_device)
        want = formats.prepare_views_reference(src, mip, "white")[0]
        for shift in (1, 4, 8, 16):
            flat[shift:shift + src.numel()] = src.reshape(-1)
            got = run_kernel(flat[shift:shift + src.numel()].view(B, H0, W0, 4), mip, "white", None, imgs=True)
            assert torch.equal(got["imgs"], want), (W0, shift)
    torch.cuda.synchronize()


def test_destinations_need_no_more_than_their_own_alignment(gpu_device):
    """ONE destination starting 4 bytes (the masks: 1 byte) past a 16-byte boundary - a view into a larger buffer: every output has the bits of the
    aligned call, and the bytes around each destination stay."""
    from pagnerf_amd import ops
    B, H0, W0, mip = 2, 8, 32, 1
    h, w = H0 >> mip, W0 >> mip
    src = S.source(B, H0, W0, 4, seed=5).to(gpu_device)
    c2w = S.camera_to_world(B, seed=6).to(gpu_device)
    want = run_kernel(src, mip, "black", c2w)
    kinds = dict(imgs=(3, torch.float32, SENTINEL), masks=(1, torch.uint8, 7), origins=(3, torch.float32, SENTINEL), dirs=(3, torch.float32, SENTINEL))
    for shifted in kinds:
        flat, views = {}, {}
        for key, (C, dtype, fill) in kinds.items():
            off, count = (1 if key == shifted else 0), B * h * w * C
            flat[key] = torch.full((count + 8,), fill, dtype=dtype, device=gpu_device)
            views[key] = flat[key][off:off + count].view(B, h, w, C)
        assert views[shifted].data_ptr() % (4 if shifted == "masks" else 16) != 0 and views[shifted].is_contiguous()
        ops.prepare_views(src, mip, "black", 0, c2w=c2w, intrinsics=tuple(S.INTRINSICS[k] for k in ("fx", "fy", "x0", "y0")), **views)
        for key, (C, dtype, fill) in kinds.items():
            off, count = (1 if key == shifted else 0), B * h * w * C
            assert torch.equal(views[key], want[key]), (shifted, key)
            assert bool((flat[key][:off] == fill).all()) and bool((flat[key][off + count:] == fill).all()), (shifted, key)
    torch.cuda.synchronize()


@pytest.mark.parametrize("H0,W0", ((10, 14), (8, 24)))                                    # odd and even output widths
def test_chunk_writes_only_its_own_views(gpu_device, H0, W0):
    """2 views into the middle of a 5-view destination: views 0, 1 and 4 keep the sentinel in every output; asking for the image alone, or for the rays
    alone, leaves the other buffers as they were."""
    from pagnerf_amd import formats
    B, mip, V, off = 2, 1, 5, 2
    h, w = H0 // 2, W0 // 2
    src = S.source(B, H0, W0, 4, seed=3).to(gpu_device)
    c2w = S.camera_to_world(V, seed=4).to(gpu_device)
    got = run_kernel(src, mip, "white", c2w, V=V, off=off)
    imgs, masks = formats.prepare_views_reference(src, mip, "white")
    assert torch.equal(got["imgs"][off:off + B], imgs) and torch.equal(got["masks"][off:off + B], masks.to(torch.uint8))
    assert torch.equal(got["origins"][off:off + B], c2w[off:off + B, None, None, :, 3].expand(B, h, w, 3))               # the DESTINATION view's camera
    exact = formats.rays_reference(c2w[off:off + B].cpu().double(), w, h, **S.INTRINSICS)
    assert float((got["dirs"][off:off + B].cpu().double() - exact.dirs).abs().max()) <= S.RAY_TOL
    for v in (0, 1, 4):
        for key in ("imgs", "origins", "dirs"):
            assert bool((got[key][v] == SENTINEL).all()), (key, v)
        assert bool((got["masks"][v] == 7).all())
    only = run_kernel(src, mip, "white", c2w, V=V, off=off, imgs=True)
    assert torch.equal(only["imgs"], got["imgs"]) and bool((only["masks"] == 7).all())
    assert bool((only["origins"] == SENTINEL).all()) and bool((only["dirs"] == SENTINEL).all())
    only = run_kernel(src, mip, "white", c2w, V=V, off=off, origins=True, dirs=True)
    assert torch.equal(only["origins"], got["origins"]) and torch.equal(only["dirs"], got["dirs"])
    assert bool((only["imgs"] == SENTINEL).all()) and bool((only["masks"] == 7).all())
    torch.cuda.synchronize()


def test_loader_on_the_device(gpu_device, tmp_path):
    """The folder loaded on the GPU in five chunks equals the CPU load: images, masks and labels bit for bit, rays within the kernel's bound."""
    from pagnerf_amd import formats
    S.write_folder(str(tmp_path), "three")
    cpu = S.leaves(formats.load_nerf_standard(str(tmp_path), "train", mip=1, device="cpu"))
    for kw in (dict(chunk_bytes=1, num_workers=2), dict(), dict(use_kernel=False, chunk_bytes=3 * 12 * 20 * 5)):
        ds = formats.load_nerf_standard(str(tmp_path), "train", mip=1, device=gpu_device, **kw)
        torch.cuda.synchronize()
        got = S.leaves(ds)
        assert got.keys() == cpu.keys() and ds.device == gpu_device
        for key, want in cpu.items():
            assert got[key].dtype == want.dtype and got[key].shape == want.shape
            if key[0] in ("rays", "base_rays"):
                assert float((got[key].cpu().double() - want.double()).abs().max()) <= S.RAY_TOL, (kw, key)
            else:
                assert torch.equal(got[key].cpu(), want), (kw, key)
        batch = ds.sample([0, 3], 16)
        assert batch["imgs"].shape == (2, 16, 3) and batch["masks"].dtype == torch.bool and batch["semantics"].dtype == torch.int64
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def scene_folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("scene"))
    S.write_trainer_scene(root)
    return root


@pytest.mark.parametrize("with_labels", (False, True))
def test_trainer_runs_on_a_loaded_folder(gpu_device, tmp_path, scene_folder, with_labels):
    """Three epochs of the tiniest PanopticTrainer configuration on the loaded folder: rgb only on the stored world rays, and with labels and pose
    optimisation on base_rays / view_matrices."""
    import math
    from pagnerf_amd import config, formats
    ds = formats.load_nerf_standard(scene_folder, "train", device=gpu_device, chunk_bytes=2 * 32 * 32 * 5)
    val = formats.load_nerf_standard(scene_folder, "val", device=gpu_device)
    assert ds.num_imgs == 4 and val.num_imgs == 2 and ds.image_shape == (32, 32) and ds.semantic_info["things_ids"] == S.SCENE_THINGS
    cfg = dict(S.TRAINER_CFG, log_dir=str(tmp_path), epochs=3)
    if not with_labels:
        cfg.update(optimize_extrinsics=False, optimize_val_extrinsics=False, sem_epoch_start=100, inst_epoch_start=100)
    torch.manual_seed(11)
    pipe, tr = config.build_from_config(cfg, ds, val, device=gpu_device)
    with torch.no_grad():                                   # densities astride the prune threshold, tables that differ
        pipe.nef.decoder_density.lout.bias[0] = 2.96
        for g in (pipe.nef.grid, pipe.nef.delta_grid):
            g.tables.normal_(0.0, 1e-2)
    for _ in range(3):
        tr.run_epoch()
    torch.cuda.synchronize()
    assert tr.epoch == 3 and tr.log_dict and all(math.isfinite(float(v)) for v in tr.log_dict.values())


def test_train_command_line_takes_a_folder(gpu_device, tmp_path, scene_folder):
    """python -m pagnerf_amd.train --dataset FOLDER (its entry point, in this process): one epoch, the folder's own val split found, a checkpoint written."""
    import yaml
    from pagnerf_amd import train
    with open(tmp_path / "scene.yaml", "w") as f:
        yaml.safe_dump(dict(trainer=dict(S.TRAINER_CFG, mip=0, dataset_num_workers=2)), f)
    log_dir = tmp_path / "run"
    assert train.main(["--config", str(tmp_path / "scene.yaml"), "--dataset", scene_folder, "--log-dir", str(log_dir), "--set", "epochs=1",
                       "--set", "val_extrinsics_every=0"]) == 0
    assert os.path.getsize(log_dir / "model.pth") > 0
