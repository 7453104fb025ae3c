"""csrc/bup20.hip against the definitions in pagnerf_amd/bup20.py at the smallest shapes that can go wrong: pag_coco_keys + pag_coco_labels, pag_bup20_pred_stats
+ pag_bup20_prepare, each writing a chunk into the middle of a larger sentinel-filled destination; the loader on the device against its tensor-op run;
and a short PanopticTrainer run through train.main on a synthetic BUP20 folder."""
import os

import numpy as np
import pytest
import torch

import bup20_scene as S
import formats_scene as F

pytestmark = pytest.mark.gpu

SENTINEL = -7
CASES = [(H0, W0, mip) for H0, W0, mips in S.SHAPES for mip in mips]


def label_frames(H0, W0):
    sets = S.annotation_sets(H0, W0)
    return [sets[k] for k in ("five", "outside", "on_boundary", "two_parts", "rle", "restart")] + [None, []]


@pytest.mark.parametrize("H0,W0,mip", CASES)
def test_labels_match_the_definition(gpu_device, H0, W0, mip):
    """Eight frames in one chunk - the five polygons, one wholly outside, a vertex on a pixel boundary, a two-part annotation with an empty one, RLE in both
    forms, the full-cover restart, a frame without labels and one without annotations - as views 1..8 of ten."""
    from pagnerf_amd import bup20, ops
    frames = label_frames(H0, W0)
    B, V, off, max_label = len(frames), len(frames) + 2, 1, 2
    h, w = H0 >> mip, W0 >> mip
    tables = bup20.coco_tables(frames, H0, W0)
    assert 0 < tables["max_part_keys"] <= bup20.COCO_MAX_PART_KEYS and len(tables["cand"]) >= 1
    dev = ops.coco_upload(tables, gpu_device)
    sem = torch.full((V, h, w, 1), SENTINEL, dtype=torch.int64, device=gpu_device)
    inst = torch.full((V, h, w, 1), SENTINEL, dtype=torch.int64, device=gpu_device)
    ops.coco_keys(dev, H0, W0)
    ops.coco_labels(dev, H0, W0, mip, max_label, off, semantics=sem, instance=inst)
    torch.cuda.synchronize()
    # the keys of every polygon part are the definition's, sorted
    count, begin, keys = (dev.tensors[k].cpu().numpy() for k in ("part_key_count", "part_key_begin", "keys"))
    part = 0
    for anns in frames:
        for _, seg in anns or []:
            for p in bup20.segmentation_parts(seg, H0, W0):
                assert np.array_equal(keys[begin[part]:begin[part] + count[part]], bup20.part_keys(p, H0, W0)), part
                part += 1
    for b, anns in enumerate(frames):
        want_sem, want_inst = bup20.coco_labels_reference(anns, H0, W0, mip, max_label)
        assert torch.equal(sem[off + b].cpu(), want_sem), b
        assert torch.equal(inst[off + b].cpu(), want_inst), b
    for v in (0, V - 1):
        assert bool((sem[v] == SENTINEL).all()) and bool((inst[v] == SENTINEL).all())
    assert bool((sem[off + 6] == -1).all()) and bool((sem[off + 7] == 0).all()) and int(sem[off + 5].max()) == 2 and int(inst[off + 5].max()) == 6
    # one destination alone
    only = torch.full((V, h, w, 1), SENTINEL, dtype=torch.int64, device=gpu_device)
    dev = ops.coco_upload(tables, gpu_device)
    ops.coco_keys(dev, H0, W0)
    ops.coco_labels(dev, H0, W0, mip, max_label, off, instance=only)
    assert torch.equal(only, inst)
    torch.cuda.synchronize()


def test_a_part_beyond_the_sort_cap_is_refused(gpu_device):
    """A zigzag of 2200 vertices: its key bound passes PAG_COCO_MAX_PART_KEYS, both entry points refuse the tables with PAG_ERR_ARG before any launch, and the
    loader's fallback writes the definition's planes for that frame and the kernels' for the others."""
    from pagnerf_amd import bup20, ops
    H0, W0, mip = S.H0, S.W0, 1
    zigzag = [c for i in range(2200) for c in (5 + 9 * (i % 2), 3 + 0.008 * i)]
    frames = [[(1, [zigzag]), (1, [S.RECTANGLE])], S.annotation_sets(H0, W0)["five"], None]
    tables = bup20.coco_tables(frames, H0, W0)
    assert tables["max_part_keys"] > bup20.COCO_MAX_PART_KEYS
    dev = ops.coco_upload(tables, gpu_device)
    sem = torch.full((4, H0 >> mip, W0 >> mip, 1), SENTINEL, dtype=torch.int64, device=gpu_device)
    inst = sem.clone()
    with pytest.raises(RuntimeError, match=r"pag_coco_keys failed \(-1\)"):
        ops.coco_keys(dev, H0, W0)
    with pytest.raises(RuntimeError, match=r"pag_coco_labels failed \(-1\)"):
        ops.coco_labels(dev, H0, W0, mip, 1, 1, semantics=sem, instance=inst)
    torch.cuda.synchronize()
    assert bool((sem == SENTINEL).all()) and bool((inst == SENTINEL).all())
    bup20._labels_on_device(ops, frames, H0, W0, mip, 1, 1, sem, inst)
    torch.cuda.synchronize()
    for b, anns in enumerate(frames):
        want_sem, want_inst = bup20.coco_labels_reference(anns, H0, W0, mip, 1)
        assert torch.equal(sem[1 + b].cpu(), want_sem) and torch.equal(inst[1 + b].cpu(), want_inst), b
    assert int(sem[1].sum()) > 0 and bool((sem[0] == SENTINEL).all())


def prepare_on_device(ops, dev_in, mip, bg, max_depth, V, off, n_ids, only=None):
    img, raw, sem, inst, conf = dev_in
    B, H0, W0, _ = img.shape
    h, w, d = H0 >> mip, W0 >> mip, img.device
    counts = ops.bup20_pred_stats(inst, raw, max_depth, n_ids) if max_depth > 0 else None
    out = dict(imgs=torch.full((V, h, w, 3), float(SENTINEL), device=d), masks=torch.full((V, h, w, 1), 7, dtype=torch.uint8, device=d),
               depths=torch.full((V, h, w, 1), float(SENTINEL), device=d), semantics_pred=torch.full((V, h, w, 1), SENTINEL, dtype=torch.int64, device=d),
               instance_pred=torch.full((V, h, w, 1), SENTINEL, dtype=torch.int64, device=d), sem_conf_out=torch.full((V, h, w, 1), float(SENTINEL), device=d),
               inst_conf_out=torch.full((V, h, w, 1), float(SENTINEL), device=d))
    asked = {k: v for k, v in out.items() if only is None or k in only}
    ops.bup20_prepare(img, mip, bg, off, depth_raw=raw, sem=sem, inst=inst, sem_conf=conf, inst_conf=conf * 0.5, counts=counts, **asked)
    return out, counts


@pytest.mark.parametrize("max_depth", (1.4, -1.0))
@pytest.mark.parametrize("H0,W0,mip", CASES)
def test_preparation_matches_the_definition(gpu_device, H0, W0, mip, max_depth):
    """Two frames as views 1..2 of four: the counts and every output bit for bit the definition evaluated on the same device tensors; ids at and one pixel
    above 2 valid == total, an absent id, depth 0, raw depths about the threshold, the maximum id; max_depth <= 0 filters nothing."""
    from pagnerf_amd import bup20, ops
    B, V, off, n_ids = 2, 4, 1, 7
    host = S.frame_inputs(B, H0, W0, 3 if mip != 1 else 4, seed=H0 + mip)
    dev_in = tuple(t.to(gpu_device) for t in host)
    img, raw, sem, inst, conf = dev_in
    assert int(inst.max()) == n_ids - 1
    got, counts = prepare_on_device(ops, dev_in, mip, "white" if H0 != 24 else "black", max_depth, V, off, n_ids)
    torch.cuda.synchronize()
    want_counts = None
    if max_depth > 0:
        want_counts = bup20.pred_stats_reference(inst, raw, max_depth, n_ids)
        assert torch.equal(counts, want_counts) and torch.equal(counts.cpu(), bup20.pred_stats_reference(host[3], host[1], max_depth, n_ids))
        assert counts[0, 1].tolist() == [4, 2] and counts[0, 2].tolist() == [3, 2] and counts[0, 4].tolist() == [0, 0]
    want = bup20.prepare_frames_reference(img, mip, "white" if H0 != 24 else "black", raw, sem, inst, conf, conf * 0.5, want_counts)
    for key, name in (("imgs", "imgs"), ("depths", "depths"), ("semantics_pred", "semantics_pred"), ("instance_pred", "instance_pred"),
                      ("sem_conf_out", "sem_conf"), ("inst_conf_out", "inst_conf")):
        assert got[key].dtype == want[name].dtype and torch.equal(got[key][off:off + B], want[name]), key
        for v in (0, V - 1):
            assert bool((got[key][v] == SENTINEL).all()), key
    assert torch.equal(got["masks"][off:off + B], want["masks"].to(torch.uint8)) and bool((got["masks"][0] == 7).all())
    assert got["instance_pred"].dtype == torch.int64
    kept = got["instance_pred"][off]
    assert bool((kept == 2).any()) and bool((kept == n_ids - 1).any()) and bool((kept == 1).any()) == (max_depth <= 0)
    if max_depth > 0 and mip <= 1:                                              # at mip 2 the taps miss row 0, where id 1 lives
        assert bool((got["sem_conf_out"][off:off + B] != bup20.prepare_frames_reference(img, mip, sem_conf=conf)["sem_conf"]).any())      # a flipped pixel
    # the CPU definition gives the same bits as the device's
    cpu = bup20.prepare_frames_reference(host[0], mip, "white" if H0 != 24 else "black", host[1], host[2], host[3], host[4], host[4] * 0.5,
                                         want_counts.cpu() if want_counts is not None else None)
    for name in want:
        assert torch.equal(cpu[name], want[name].cpu()), name
    # NULL destinations: the image alone, the labels alone
    only, _ = prepare_on_device(ops, dev_in, mip, "white" if H0 != 24 else "black", max_depth, V, off, n_ids, only=("imgs",))
    assert torch.equal(only["imgs"], got["imgs"]) and all(bool((only[k] == (7 if k == "masks" else SENTINEL)).all()) for k in only if k != "imgs")
    only, _ = prepare_on_device(ops, dev_in, mip, "white" if H0 != 24 else "black", max_depth, V, off, n_ids, only=("semantics_pred", "inst_conf_out"))
    assert torch.equal(only["semantics_pred"], got["semantics_pred"]) and torch.equal(only["inst_conf_out"], got["inst_conf_out"])
    assert bool((only["imgs"] == SENTINEL).all()) and bool((only["instance_pred"] == SENTINEL).all())
    torch.cuda.synchronize()


def test_pred_stats_beyond_the_lds_histogram(gpu_device):
    """3000 ids: the counts go straight to memory; the maximum id is counted."""
    from pagnerf_amd import bup20, ops
    g = torch.Generator().manual_seed(5)
    inst = torch.randint(0, 3000, (2, 66, 130), generator=g).to(torch.int32)
    inst[0, 0, 0] = 2999
    raw = torch.randint(-32768, 32768, (2, 66, 130), generator=g).to(torch.int16)
    for n_ids in (3000, 2048, 2049):
        ids = inst.clamp(max=n_ids - 1).to(gpu_device)
        got = ops.bup20_pred_stats(ids, raw.to(gpu_device), 1.4, n_ids)
        assert torch.equal(got.cpu(), bup20.pred_stats_reference(ids.cpu(), raw, 1.4, n_ids)) and int(got[0, n_ids - 1, 0]) >= 1
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("bup20") / "BUP_20")
    os.makedirs(root)
    return root, S.write_tree(root)


MODES = ["imgs", "depths", "semantics", "instance", "sem_conf", "inst_conf", "preds_mask2former"]


@pytest.mark.parametrize("max_depth", (1.4, -1))
@pytest.mark.parametrize("pose_src", ("odom", "metashape"))
@pytest.mark.parametrize("split", ("train", "val"))
def test_loader_on_the_device(gpu_device, tree, split, pose_src, max_depth):
    """load_bup20 on the device equals its own tensor-op run on the same folder: every mode bit for bit, ray directions to RAY_TOL; in one chunk and in
    one chunk per frame with decode threads."""
    from pagnerf_amd import bup20
    root, _ = tree
    kw = dict(mip=1, load_modes=MODES, pose_src=pose_src, max_depth=max_depth, seq_num_frames=S.SEQ_NUM_FRAMES, device=gpu_device)
    want = S.leaves(bup20.load_bup20(root, split, use_kernel=False, **kw))
    for extra in (dict(), dict(chunk_bytes=1, num_workers=2)):
        ds = bup20.load_bup20(root, split, **kw, **extra)
        torch.cuda.synchronize()
        got = S.leaves(ds)
        assert got.keys() == want.keys() and ds.device == gpu_device
        for key, t in want.items():
            assert got[key].dtype == t.dtype and got[key].shape == t.shape
            if key == ("rays", "dirs"):
                assert float((got[key].double() - t.double()).abs().max()) <= F.RAY_TOL, key
            else:
                assert torch.equal(got[key], t), key
        if split == "val":
            assert int(got[("instance", None)][2].max()) >= 5 and bool((got[("instance", None)][0] == -1).all())
        batch = ds.sample([0, 1], 16)
        assert batch["imgs"].shape == (2, 16, 3) and batch["semantics_pred"].dtype == torch.int64 and batch["sem_conf"].dtype == torch.float32
    torch.cuda.synchronize()


def test_train_command_line_takes_a_bup20_folder(gpu_device, tree, tmp_path):
    """python -m pagnerf_amd.train --dataset FOLDER (its entry point, in this process) with a cut-down best.yaml: epochs 0 and 1 on the folder's train
    window, validated on its val window, a checkpoint and a metrics row written."""
    import yaml
    from pagnerf_amd import train
    root, _ = tree
    cfg = dict(F.TRAINER_CFG, mip=0, dataset_num_workers=2, multiview_dataset_format="bup20", load_modes=MODES, class_labels=["bg", "pepper"],
               dataset_center_idx=0, pose_src="odom", max_depth=1.4, model_rescaling="largest", scale=1.0, offset=[0.0, 0.0, 0.0],
               seq_num_frames=S.SEQ_NUM_FRAMES, anchor_frame_idxs=[0])
    with open(tmp_path / "bup20.yaml", "w") as f:
        yaml.safe_dump(dict(trainer=cfg), f)
    log_dir = tmp_path / "run"
    assert train.main(["--config", str(tmp_path / "bup20.yaml"), "--dataset", root, "--log-dir", str(log_dir), "--set", "epochs=1",
                       "--set", "val_extrinsics_every=0"]) == 0
    assert os.path.getsize(log_dir / "model.pth") > 0
    with open(log_dir / "metrics.csv") as f:
        rows = [line for line in f.read().splitlines() if line]
    assert len(rows) >= 2
