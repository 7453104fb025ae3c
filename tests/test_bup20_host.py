"""pagnerf_amd/bup20.py on the host: the coverage rule against geometry, the label combination, the pure functions of the loader, the tensor-op forms of the
frame preparation, and the CPU load of a synthetic folder."""
import os

import numpy as np
import pytest
import torch

import bup20_scene as S


# ------------------------------------------------------------------------------------------------------------------------------- coverage rule
@pytest.mark.parametrize("name", sorted(S.POLYGONS))
def test_coverage_rule_against_even_odd(name):
    """polygon_mask_reference agrees with the float64 even-odd rule at the pixel centre on every pixel whose centre is more than 0.5 px from the boundary;
    the excluded band holds at most a quarter of the pixels.  Measured with this restatement: 25 / 240 / 140 / 409 / 4 covered pixels, at most 19 % of
    the pixels within a full pixel of the boundary, every disagreement within 0.10 px of it (0 / 3 / 6 / 3 / 0 pixels)."""
    from pagnerf_amd import bup20
    poly = S.POLYGONS[name]
    got = bup20.polygon_mask_reference(poly, S.H0, S.W0)
    inside, dist = S.even_odd(poly, S.H0, S.W0)
    far = dist > 0.5
    wrong = got != inside
    print("%s: area %d, %.1f %% within 0.5 px, %.1f %% within 1 px, %d disagreements, the farthest %.3f px from the boundary"
          % (name, got.sum(), 100 * (~far).mean(), 100 * (dist <= 1.0).mean(), wrong.sum(), dist[wrong].max() if wrong.any() else 0.0))
    assert (~far).mean() <= 0.25
    assert not (wrong & far).any()
    assert int(got.sum()) == S.AREAS[name]


def test_rectangle_is_the_block():
    from pagnerf_amd import bup20
    want = np.zeros((10, 10), dtype=bool)
    want[2:7, 2:7] = True
    assert np.array_equal(bup20.polygon_mask_reference(S.RECTANGLE, 10, 10), want)
    assert np.array_equal(bup20.polygon_mask_reference([S.RECTANGLE], 10, 10), want)
    assert not bup20.polygon_mask_reference([], 10, 10).any()


def test_rle_round_trips_and_key_carry():
    from pagnerf_amd import bup20
    for poly in S.POLYGONS.values():
        mask = bup20.polygon_mask_reference(poly, S.H0, S.W0)
        for seg in bup20.mask_rle(mask):
            assert np.array_equal(bup20.keys_mask(bup20.rle_keys(seg, S.H0, S.W0), S.H0, S.W0), mask)
    assert bup20.rle_counts(dict(size=[3, 2], counts="12")) == [1, 2]
    # a negative difference in the compressed string: runs 5, 1, 5, 1, 1 -> differences from the fourth run on
    mask = np.zeros((13, 1), dtype=bool)
    mask[5:6] = mask[11:12] = True
    listed, packed = bup20.mask_rle(mask)
    assert listed["counts"] == [5, 1, 5, 1, 1] and bup20.rle_counts(packed) == listed["counts"]
    with pytest.raises(ValueError):
        bup20.rle_keys(dict(size=[4, 4], counts=[20]), 4, 4)
    # a key at Y = h carries into the next column: it toggles pixel (x + 1, 0)
    h, w = 4, 3
    m = bup20.keys_mask(np.array([1 * h + 2, 1 * h + h]), h, w)               # column 1 from row 2 to its end
    assert m[2:, 1].all() and m.sum() == 2
    m = bup20.keys_mask(np.array([1 * h + 2, 2 * h + 1]), h, w)               # open across the column end: rows 2.. of column 1 and row 0 of column 2
    assert m[2:, 1].all() and m[0, 2] and m.sum() == 3
    # a polygon that reaches below the image closes its columns with keys at Y = h, and stays inside the image
    keys = bup20.polygon_keys_reference([1, 1, 3, 1, 3, 9, 1, 9], h, w)
    assert (keys % h == 0).sum() >= 2 and h * 2 in keys.tolist()
    assert np.array_equal(bup20.keys_mask(keys, h, w), np.array([[0, 0, 0], [0, 1, 1], [0, 1, 1], [0, 1, 1]], dtype=bool))


def test_label_combination():
    from pagnerf_amd import bup20
    h, w = S.H0, S.W0
    cover = lambda poly: bup20.polygon_mask_reference(poly, h, w)
    sets = S.annotation_sets(h, w)
    # two overlapping parts are an OR, an empty segmentation keeps its index and covers nothing, instance = last index + 1
    sem, inst = bup20.coco_labels_reference(sets["two_parts"], h, w, 0, 1)
    both = cover(S.RECTANGLE) | cover(S.TRIANGLE)
    small = cover([1, 1, 6, 1, 6, 6])
    assert (cover(S.RECTANGLE) & cover(S.TRIANGLE)).any()
    assert np.array_equal(sem[..., 0].numpy(), (both | small).astype(np.int64))
    assert np.array_equal(inst[..., 0].numpy(), np.where(small, 3, np.where(both, 1, 0)))
    assert sem.dtype == torch.int64 and sem.shape == (h, w, 1)
    # overlapping annotations add up and clip at max_label
    anns = [(1, [S.TRIANGLE]), (2, [S.STAR]), (2, [S.QUAD])]
    total = cover(S.TRIANGLE) * 1 + cover(S.STAR) * 2 + cover(S.QUAD) * 2
    assert total.max() == 5
    for max_label in (2, 3, 9):
        sem, _ = bup20.coco_labels_reference(anns, h, w, 0, max_label)
        assert np.array_equal(sem[..., 0].numpy(), np.minimum(total, max_label))
    # the sum starts again at an annotation that covers every pixel - a polygon or an RLE - and goes on after it
    sem, inst = bup20.coco_labels_reference(sets["restart"], h, w, 0, 5)            # star, full RLE, triangle, full polygon, rectangle, star
    assert np.array_equal(sem[..., 0].numpy(), 1 + cover(S.RECTANGLE) * 1 + cover(S.STAR) * 1)
    assert np.array_equal(inst[..., 0].numpy(), np.where(cover(S.STAR), 6, np.where(cover(S.RECTANGLE), 5, 4)))
    sem, inst = bup20.coco_labels_reference(sets["restart"][:3], h, w, 0, 5)
    assert np.array_equal(sem[..., 0].numpy(), 1 + cover(S.TRIANGLE) * 1) and cover(S.STAR).any()
    assert np.array_equal(inst[..., 0].numpy(), np.where(cover(S.TRIANGLE), 3, 2))
    # the nearest shrink and the frame without labels
    full = bup20.coco_labels_reference(sets["five"], h, w, 0, 1)
    for mip in (1, 2):
        f = 1 << mip
        for a, b in zip(bup20.coco_labels_reference(sets["five"], h, w, mip, 1), full):
            assert torch.equal(a, b[::f, ::f])
    sem, inst = bup20.coco_labels_reference(None, h, w, 1, 1)
    assert sem.shape == (h // 2, w // 2, 1) and (sem == -1).all() and (inst == -1).all()


def test_coco_tables():
    """The tables of the kernels: offsets, the key bound that covers every part's true count, RLE keys in place, candidates for the counting pass."""
    from pagnerf_amd import bup20
    h, w = S.H0, S.W0
    sets = S.annotation_sets(h, w)
    frames = [None, sets["five"], sets["restart"], [], sets["two_parts"]]
    t = bup20.coco_tables(frames, h, w)
    assert t["frame_labelled"].tolist() == [0, 1, 1, 1, 1] and t["frame_ann_begin"].tolist() == [0, 0, 5, 11, 11, 14]
    assert t["ann_cover"].tolist().count(h * w) == 1 and t["cand"].tolist() == [2, 5 + 3]         # the quad's vertex box contains the image too
    assert all(a.dtype == np.int32 for k, a in t.items() if k != "max_part_keys")
    part = 0
    for anns in frames:
        for label, seg in anns or []:
            for kind, data in bup20.segmentation_parts(seg, h, w):
                room = t["part_key_begin"][part + 1] - t["part_key_begin"][part]
                keys = bup20.part_keys((kind, data), h, w)
                assert len(keys) <= room <= (t["max_part_keys"] if kind == "poly" else room)
                if kind == "keys":
                    assert t["part_key_count"][part] == len(keys)
                    assert np.array_equal(t["keys"][t["part_key_begin"][part]:t["part_key_begin"][part + 1]], keys)
                else:
                    v0, v1 = t["part_vert_begin"][part:part + 2]
                    assert t["point_begin"][v1] - t["point_begin"][v0] == len(bup20.edge_points(bup20.round_vertices(data))[0])
                part += 1
    assert part == len(t["part_key_count"])
    zigzag = [c for i in range(2200) for c in (5 + (i % 2), 3 + 0.001 * i)]
    assert bup20.coco_tables([[(1, [zigzag])]], h, w)["max_part_keys"] > bup20.COCO_MAX_PART_KEYS


# ----------------------------------------------------------------------------------------------------------------------------- pure host functions
def test_window():
    from pagnerf_amd import bup20
    assert bup20.window_deltas(40, "train") == list(range(-41, 42, 2)) and bup20.window_deltas(40, "val") == list(range(-40, 41, 2))
    assert bup20.window_deltas(5, "train") == [-5, -3, -1, 1, 3, 5] and bup20.window_deltas(4, "val") == [-4, -2, 0, 2, 4]
    with pytest.raises(ValueError):
        bup20.window_deltas(4, "test")
    seq = ["s/%03d.png" % i for i in range(100)]
    # n = 40: positions 41 .. 59 survive the edge rule
    kept = bup20.keep_eval_frames([seq[i] for i in (0, 40, 41, 50, 59, 60, 99)], lambda p: seq, 40)
    assert kept == [seq[41], seq[50], seq[59]]
    got = bup20.window_paths(seq[50], seq, "train", 40)
    assert got == [seq[50 - d] for d in range(41, -42, -2)] and len(got) == 42
    got = bup20.window_paths(seq[50], seq, "val", 40, train_paths=[seq[52], seq[53]], eval_paths=[seq[50]])
    assert got == [seq[50 - d] for d in range(40, -41, -2) if 50 - d != 52] and seq[50] in got
    # clamped repeats survive: centre 41 of a 70-frame sequence at n = 40 reaches below 0 and above 69
    short = seq[:70]
    got = bup20.window_paths(short[41], short, "train", 40)
    assert got[0] == short[0] and got[-6:] == [short[69]] * 6 and got.count(short[0]) == 1 and len(got) == 42
    # n = 4 on 14 frames: the windows of the synthetic folder
    seq = ["s/%02d.png" % i for i in range(14)]
    kept = bup20.keep_eval_frames([seq[i] for i in S.EVAL_POS], lambda p: seq, 4)
    assert kept == [seq[6], seq[9]]
    train = [seq[i] for i in S.TRAIN_POS]
    for split in ("train", "val"):
        for c in (6, 9):
            assert bup20.window_paths(seq[c], seq, split, 4, train, kept) == [seq[i] for i in S.window_positions(split, c)]
    assert S.window_positions("train", 6) == [1, 3, 5, 11] and S.window_positions("val", 9) == [5, 9, 11, 13]
    assert S.window_positions("train", 9) == [4, 8, 10, 12, 13]


def test_paths_classes_and_modes(tmp_path):
    from pagnerf_amd import bup20
    assert bup20.dataset_rel_path("/data/sets/BUP_20/20200924/row3/1.png") == os.path.join("BUP_20", "20200924", "row3", "1.png")
    assert bup20.dataset_rel_path("a/b/c/d.png") == "d.png"
    with pytest.raises(ValueError):
        bup20.dataset_rel_path("a/b/c")
    cats = {7: dict(name="pepper_red", supercategory="pepper"), 3: dict(name="bg", supercategory="none"), 9: dict(name="leaf", supercategory="plant"),
            4: dict(name="pepper", supercategory="bg")}
    assert dict(bup20.class_map(cats, ["bg", "pepper"])) == {7: 1, 3: 0, 4: 0}                      # the supercategory wins over the name
    info = bup20.semantic_info([])
    assert info["num_classes"] == 2 and info["stuff_ids"] == [0] and info["things_ids"] == [1] and info["num_instances"] == 200
    assert bup20.semantic_info(["bg", "crop", "weed"])["things_ids"] == [1, 2]
    modes = ["imgs", "depths", "semantics", "instance", "sem_conf", "inst_conf", "preds_mask2former"]
    assert bup20.filter_load_modes(modes, "train") == ("preds_mask2former", ["semantics", "instance", "sem_conf", "inst_conf"])
    assert bup20.filter_load_modes(modes, "val") == ("preds_mask2former", modes[:-1])
    assert bup20.filter_load_modes([], "val") == ("instance_preds", ["imgs", "depths", "semantic", "instance"])
    with pytest.raises(ValueError):
        bup20.filter_load_modes(["imgs", "semantics"], "train")
    with pytest.raises(FileNotFoundError):
        bup20.dataset_files(str(tmp_path))
    assert not bup20.is_bup20_folder(str(tmp_path))
    for name in ("CKA_sweet_pepper_2020_summer.json", "CKA_sweet_pepper_2020_summer.yaml"):
        (tmp_path / name).write_text("{}")
    assert bup20.is_bup20_folder(str(tmp_path))
    assert [os.path.basename(p) for p in bup20.dataset_files(str(tmp_path))] == ["CKA_sweet_pepper_2020_summer.json", "CKA_sweet_pepper_2020_summer.yaml"]
    (tmp_path / "BUP_20.json").write_text("{}")
    assert [os.path.basename(p) for p in bup20.dataset_files(str(tmp_path))] == ["BUP_20.json", "CKA_sweet_pepper_2020_summer.yaml"]
    assert sorted(os.listdir(tmp_path)) == ["BUP_20.json", "CKA_sweet_pepper_2020_summer.json", "CKA_sweet_pepper_2020_summer.yaml"]        # nothing copied


def test_poses_and_odometry(tmp_path):
    from pagnerf_amd import bup20
    scene = S.write_tree(str(tmp_path))
    ts, seq = scene["ts"], scene["seq"]
    for src in ("odom", "rgbd", "metashape"):
        odom = bup20.read_odometry(seq, src)
        assert sorted(odom) == sorted(ts)
        for t in ts:
            assert np.abs(odom[t] - scene["odom"][t]).max() < 1e-12, src
    with pytest.raises(ValueError):
        bup20.read_odometry(seq, "gps")
    params = bup20.read_params(os.path.join(seq, "params.yaml"))
    assert np.array_equal(params["extrinsics"], scene["E"]) and np.array_equal(params["intrinsics"], scene["K"])
    names, scale, offset = [ts[i] for i in (2, 4, 6, 8, 10)], 0.7, [0.1, -0.2, -1.4]
    poses = bup20.frame_poses(scene["odom"], names, ts[6], scene["E"])
    assert np.abs(poses[2] - np.eye(4)).max() < 1e-12                                                # the centre frame is the identity
    c2w, views = bup20.bup20_cameras(bup20.scale_and_shift(bup20.cv_to_gl(poses), scale, offset))
    want_c2w, want_views = S.expected_cameras(scene["odom"], names, ts[6], scene["E"], scale, offset)
    assert c2w.dtype == torch.float32 and c2w.shape == (5, 3, 4) and views.shape == (5, 4, 4)
    assert np.abs(c2w.double().numpy() - want_c2w).max() < 2e-7 and np.abs(views.double().numpy() - want_views).max() < 2e-7
    fx, fy, x0, y0 = bup20.bup20_intrinsics(scene["K"], 1, S.H0 // 2, S.W0 // 2)
    assert (fx, fy) == (41.3 / 2, 39.9 / 2) and abs(x0 - 0.35) < 1e-12 and abs(y0 + 0.2) < 1e-12


def test_ply_and_rescaling(tmp_path):
    from pagnerf_amd import bup20
    rs = np.random.RandomState(1)
    v = rs.uniform(-1, 1, (50, 3)) * np.array([3.0, 1.5, 0.8]) + np.array([0.5, -0.25, 1.0])
    v32 = v.astype(np.float32).astype(np.float64)
    bounds = np.stack([v32.min(0), v32.max(0)], 1)
    for binary in (False, True):
        path = str(tmp_path / ("mesh_%d.ply" % binary))
        S.write_ply(path, v, binary)
        assert np.array_equal(bup20.ply_vertex_bounds(path), bounds)
    lengths, centers = bounds[:, 1] - bounds[:, 0], bounds.sum(1) / 2
    scale, offset = bup20.scale_from_bounds(bounds, "largest")
    assert scale == 0.98 * 2 / lengths[0] and np.allclose(offset, -centers * scale, rtol=0, atol=1e-15)
    scale, offset = bup20.scale_from_bounds(bounds, "snap_to_bottom")
    assert scale == 2 / lengths[0] and offset[:2] == list(-centers[:2] * scale) and offset[2] == -bounds[2, 0] * scale - 1
    with pytest.raises(NotImplementedError):
        bup20.scale_from_bounds(bounds, "tight")
    root = tmp_path / "set" / "BUP_20"
    root.mkdir(parents=True)
    assert bup20.load_scale_and_offset(str(root)) == (1.0, [0.0, 0.0, -1.4])
    S.write_ply(str(tmp_path / "set" / "mesh.ply"), v, True)
    assert bup20.load_scale_and_offset(str(root), "largest") == bup20.scale_from_bounds(bounds, "largest")


def test_prediction_decoders(tmp_path):
    from pagnerf_amd import bup20
    rs = np.random.RandomState(2)
    h, w = 6, 8
    S.write_predictions(str(tmp_path), "f", np.random.RandomState(2), h, w)
    sem, imap, conf = S.predictions(rs, h, w)
    image = str(tmp_path / "f.png")
    for name in S.PREDS:
        s, m, c = bup20.read_prediction(image, name)
        assert s.dtype == np.int32 and m.dtype == np.int32 and c.dtype == np.float32 and s.shape == m.shape == c.shape == (h, w)
        assert np.array_equal(s, sem) and np.array_equal(m, imap), name
    logit = torch.from_numpy(conf.copy())
    logit[torch.from_numpy(imap == 0)] *= -1
    assert np.array_equal(bup20.read_prediction(image, "preds_mask2former")[2], torch.sigmoid(logit).numpy())
    c = bup20.read_prediction(image, "preds_maskrcnn")[2]
    assert np.array_equal(c[imap > 0], conf.clip(0.55, 0.99)[imap > 0]) and (c[imap == 0] == np.float32(0.9)).all()
    assert (bup20.read_prediction(image, "preds_deeplab")[2] == 1).all()
    assert np.array_equal(bup20.read_prediction(image, "preds_pan_unet")[2], conf.clip(0, 1))
    one = bup20.decode_maskrcnn(dict(masks=torch.full((1, 1, h, w), 0.7)))                      # a single mask keeps its axis
    assert (one[1] == 1).all() and one[2].shape == (h, w)
    with pytest.raises(NotImplementedError):
        bup20.read_prediction(image, "instance_preds")


# ------------------------------------------------------------------------------------------------------------------------- tensor-op forms, loading
@pytest.mark.parametrize("f", (2, 4))
@pytest.mark.parametrize("C", (1, 3))
def test_bilinear_definition_is_interpolate(f, C):
    from pagnerf_amd import bup20
    g = torch.Generator().manual_seed(f + C)
    for x in (torch.rand(2, 6 * f, 10 * f, C, generator=g), torch.randint(0, 256, (2, 6 * f, 10 * f, C), generator=g).float() / 255):
        want = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2).contiguous(), (6, 10), mode="bilinear").permute(0, 2, 3, 1)
        assert torch.equal(bup20.bilinear_shrink_reference(x, f), want)
        want = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), (6, 10), mode="bilinear").permute(0, 2, 3, 1)          # channels-last input
        assert torch.equal(bup20.bilinear_shrink_reference(x, f), want)
    assert torch.equal(bup20.bilinear_shrink_reference(x, 1), x)


def test_keep_rule_is_the_float_quotient():
    from pagnerf_amd import bup20
    total, valid = torch.meshgrid(torch.arange(1, 65), torch.arange(0, 65), indexing="ij")
    ok = valid <= total
    counts = torch.stack([total[ok], valid[ok]], -1).to(torch.int32)
    assert torch.equal(bup20.keep_ids(counts), counts[:, 1].float() / counts[:, 0].float() > 0.5)
    big = torch.tensor([[(1 << 24) - 1, 1 << 23], [(1 << 24) - 2, (1 << 23) - 1], [(1 << 24) - 2, 1 << 23]], dtype=torch.int32)
    assert torch.equal(bup20.keep_ids(big), big[:, 1].float() / big[:, 0].float() > 0.5)


def test_prepare_definition():
    from pagnerf_amd import bup20
    B, h, w = 2, 8, 12
    img, raw, sem, inst, conf = S.frame_inputs(B, h, w)
    counts = bup20.pred_stats_reference(inst, raw, 1.4, 7)
    assert counts[0, 1].tolist() == [4, 2] and counts[0, 2].tolist() == [3, 2] and counts[0, 4].tolist() == [0, 0] and int(counts[0, 6, 0]) >= 1
    assert int(counts[..., 0].sum()) == B * h * w
    d = bup20.depth_metres(raw)
    assert float(d[0, 1, 4]) == np.float32(65535) * np.float32(0.001) and float(d[0, 1, 3]) == 0.0
    valid = ((d > 0) & (d <= torch.tensor(1.4)))[0, 1, :6].tolist()
    assert valid[0] and not valid[2] and valid[3:] == [False, False, False]
    keep = bup20.keep_ids(counts)
    assert not bool(keep[0, 1]) and bool(keep[0, 2])
    for mip in (0, 1):
        f = 1 << mip
        got = bup20.prepare_frames_reference(img, mip, "white", raw, sem, inst, conf, conf, counts)
        inst2 = torch.where(torch.gather(keep, 1, inst.reshape(B, -1).long()).reshape(inst.shape), inst, torch.zeros_like(inst))
        assert (inst2 != 1).all() and (inst2 == 2).any()
        assert torch.equal(got["instance_pred"][..., 0], inst2[:, ::f, ::f].long()) and got["instance_pred"].dtype == torch.int64
        assert torch.equal(got["semantics_pred"][..., 0], (sem * (inst2 != 0))[:, ::f, ::f].long())
        flipped = (inst != 0) & (inst2 == 0)
        c = torch.where(flipped, torch.ones_like(conf), conf)
        want = torch.nn.functional.interpolate(c[:, None], (h // f, w // f), mode="bilinear")[:, 0] if mip else c
        assert torch.equal(got["sem_conf"][..., 0], want) and torch.equal(got["inst_conf"], got["sem_conf"])
        x = img.float().div(255).permute(0, 3, 1, 2)
        want = torch.nn.functional.interpolate(x, (h // f, w // f), mode="bilinear").permute(0, 2, 3, 1) if mip else x.permute(0, 2, 3, 1)
        assert torch.equal(got["imgs"], want) and got["masks"].all() and got["masks"].dtype == torch.bool
        plain = bup20.prepare_frames_reference(img, mip, "white", None, sem, inst, conf, None, None)
        assert torch.equal(plain["instance_pred"][..., 0], inst[:, ::f, ::f].long()) and torch.equal(plain["semantics_pred"][..., 0], sem[:, ::f, ::f].long())
        assert "depths" not in plain and "inst_conf" not in plain
    rgba = torch.cat([img, torch.randint(0, 256, (B, h, w, 1), dtype=torch.uint8)], -1)
    rgba[:, :2, :2, 3] = 0
    got = bup20.prepare_frames_reference(rgba, 1, "white")
    assert bool((got["imgs"][:, 0, 0] == 1).all()) and not bool(got["masks"][:, 0, 0].any()) and 0 < int(got["masks"].sum()) < got["masks"].numel()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("bup20") / "BUP_20")
    os.makedirs(root)
    return root, S.write_tree(root)


ALL_MODES = ["imgs", "depths", "semantics", "instance", "sem_conf", "inst_conf"]


@pytest.mark.parametrize("preds", S.PREDS)
def test_load_on_the_cpu(tree, preds):
    """Both splits of the synthetic folder on the CPU: the window, the modes the filter leaves, labels on the centre frame only, cameras and attributes."""
    from pagnerf_amd import bup20
    import formats_scene as F
    root, scene = tree
    ts = scene["ts"]
    for split, idx, center in (("train", 0, 6), ("val", 0, 6), ("val", 1, 9)):
        ds = bup20.load_bup20(root, split, mip=1, load_modes=ALL_MODES + [preds], dataset_center_idx=idx, max_depth=1.4, seq_num_frames=S.SEQ_NUM_FRAMES,
                              device="cpu", num_workers=2 if idx else 0, chunk_bytes=1 if idx else 64 << 20)
        pos = S.window_positions(split, center)
        got = S.leaves(ds)
        assert ds.filenames == [ts[p] + ".png" for p in pos] and ds.num_imgs == len(pos) and ds.image_shape == (S.H0 // 2, S.W0 // 2)
        want_modes = {"imgs", "masks", "rays", "base_rays", "semantics", "semantics_pred", "instance", "instance_pred", "sem_conf", "inst_conf"}
        assert {k for k, _ in got} == (want_modes | {"depths"} if split == "val" else want_modes)
        assert ds.semantic_info == dict(num_classes=2, num_instances=200, things_ids=[1], stuff_ids=[0])
        assert ds._rays_range == dict(rays=(0.0, 2.0), base_rays=(0.0, 2.0)) and ds.scale == 1.0
        for v, p in enumerate(pos):
            if split == "val" and p == center:
                sem, inst = bup20.coco_labels_reference(scene["anns"][p], S.H0, S.W0, 1, 1)
                assert torch.equal(got[("semantics", None)][v], sem) and torch.equal(got[("instance", None)][v], inst) and int(inst.max()) >= 5
            else:
                assert (got[("semantics", None)][v] == -1).all() and (got[("instance", None)][v] == -1).all()
        img = torch.from_numpy(np.stack([scene["images"][ts[p]] for p in pos]))
        raw = torch.from_numpy(np.stack([scene["depths"][ts[p]] for p in pos]).view(np.int16))
        pr = [bup20.read_prediction(os.path.join(scene["seq"], ts[p] + ".png"), preds) for p in pos]
        sem, inst, conf = (torch.from_numpy(np.stack([q[i] for q in pr])) for i in range(3))
        counts = bup20.pred_stats_reference(inst, raw, 1.4, int(inst.max()) + 1)
        want = bup20.prepare_frames_reference(img, 1, "white", raw, sem, inst, conf, conf, counts)
        for key in ("imgs", "masks", "semantics_pred", "instance_pred", "sem_conf", "inst_conf") + (("depths",) if split == "val" else ()):
            assert torch.equal(got[(key, None)], want[key]), key
        names = [ts[p] for p in pos]
        c2w, views = S.expected_cameras(scene["odom"], names, ts[center], scene["E"], 1.0, [0.0, 0.0, -1.4])
        assert np.abs(ds.view_matrices.double().numpy() - views).max() < 2e-7
        assert np.abs(got[("rays", "origins")][:, 0, 0].double().numpy() - c2w[:, :, 3]).max() < 2e-7
        fx, fy, x0, y0 = bup20.bup20_intrinsics(scene["K"], 1, S.H0 // 2, S.W0 // 2)
        assert ds.intrinsics == dict(fx=fx, fy=fy, x0=x0, y0=y0)
        from pagnerf_amd.formats import rays_reference
        exact = rays_reference(torch.from_numpy(c2w), S.W0 // 2, S.H0 // 2, fx, fy, x0, y0)
        assert float((got[("rays", "dirs")].double() - exact.dirs).abs().max()) <= F.RAY_TOL


def test_load_options(tree, tmp_path):
    from pagnerf_amd import bup20
    import formats_scene as F
    root, scene = tree
    kw = dict(load_modes=["imgs", "semantics", "instance", "preds_deeplab"], seq_num_frames=S.SEQ_NUM_FRAMES, device="cpu")
    for name, value in (("add_noise_to_train_poses", True), ("dataset_mode", "all_frames_window")):
        with pytest.raises(NotImplementedError, match=name):
            bup20.load_bup20(root, "train", **dict(kw, **{name: value}))
    with pytest.raises(IndexError):
        bup20.load_bup20(root, "val", dataset_center_idx=2, **kw)
    with pytest.raises(ValueError):
        bup20.load_bup20(root, "test", **kw)
    # no depth filter without max_depth, metashape poses, an explicit scale and offset, the CKA names
    other = str(tmp_path / "BUP_20")
    os.makedirs(other)
    S.write_tree(other, cka_names=True)
    a = bup20.load_bup20(root, "val", pose_src="metashape", scale=0.5, offset=[0.0, 0.1, 0.2], **kw)
    b = bup20.load_bup20(other, "val", pose_src="odom", scale=0.5, offset=[0.0, 0.1, 0.2], **kw)
    assert a.scale == 0.5 and {k for k, _ in S.leaves(a)} == {"imgs", "masks", "rays", "base_rays", "semantics", "semantics_pred", "instance", "instance_pred"}
    for key, t in S.leaves(a).items():
        other_t = S.leaves(b)[key]
        assert torch.equal(t, other_t) if t.dtype != torch.float32 else float((t - other_t).abs().max()) < 1e-5, key
    pr = bup20.read_prediction(os.path.join(scene["seq"], scene["ts"][6] + ".png"), "preds_deeplab")
    assert torch.equal(S.leaves(a)[("instance_pred", None)][2, ..., 0], torch.from_numpy(pr[1]).long())
    # the command line writes the .npz that train.load_npz_dataset reads
    from pagnerf_amd import train
    out = str(tmp_path / "val.npz")
    assert bup20.main([root, "--split", "val", "--mip", "1", "--load-modes", "imgs", "semantics", "instance", "preds_deeplab", "--seq-num-frames", "4",
                       "--device", "cpu", "--out", out]) == 0
    ds = train.load_npz_dataset(out, "cpu")
    assert ds.num_imgs == 5 and ds.image_shape == (S.H0 // 2, S.W0 // 2) and ds.semantic_info["things_ids"] == [1]


def test_train_dispatch(tree, tmp_path, monkeypatch):
    """train.load_dataset sends a BUP20 folder, or any folder under a bup20 YAML, to load_bup20 with the namespace's options; other paths go where they went."""
    from pagnerf_amd import bup20, formats, train
    root, _ = tree
    calls = []
    monkeypatch.setattr(bup20, "load_bup20", lambda *a, **k: calls.append(("bup20", a, k)) or "B")
    monkeypatch.setattr(formats, "load_nerf_standard", lambda *a, **k: calls.append(("standard", a, k)) or "S")
    cfg = dict(mip=1, load_modes=["imgs", "preds_deeplab"], class_labels=["bg", "pepper"], dataset_center_idx=1, pose_src="metashape", max_depth=1.4,
               model_rescaling="largest", dataset_num_workers=3)
    assert train.load_dataset(root, "val", cfg, "cpu") == "B"
    kind, a, k = calls.pop()
    assert kind == "bup20" and a == (root, "val") and k["mip"] == 1 and k["load_modes"] == cfg["load_modes"] and k["class_labels"] == cfg["class_labels"]
    assert k["dataset_center_idx"] == 1 and k["pose_src"] == "metashape" and k["max_depth"] == 1.4 and k["model_rescaling"] == "largest"
    assert k["scale"] is None and k["offset"] is None and k["num_workers"] == 3 and k["device"] == "cpu"
    plain = str(tmp_path / "plain")
    os.makedirs(plain)
    assert train.load_dataset(plain, "train", dict(cfg), "cpu") == "S" and calls.pop()[0] == "standard"
    for name in bup20.FORMAT_NAMES:
        assert train.load_dataset(plain, "train", dict(cfg, multiview_dataset_format=name), "cpu") == "B" and calls.pop()[0] == "bup20"
    assert train.load_dataset(plain, "train", dict(cfg, multiview_dataset_format="standard"), "cpu") == "S"
    with open(os.path.join(plain, "transforms.json"), "w") as f:                                 # a NeRF-standard folder stays one under a shipped YAML
        f.write("{}")
    assert train.load_dataset(plain, "train", dict(cfg, multiview_dataset_format="bup20"), "cpu") == "S" and calls.pop()[0] == "standard"
    os.remove(os.path.join(plain, "transforms.json"))
    assert train.is_bup20(root, {}) and train.is_bup20(plain, dict(multiview_dataset_format="BUP_20")) and not train.is_bup20(plain, {})
