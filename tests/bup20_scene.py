"""What tests/test_bup20_host.py and tests/test_gpu_bup20.py share: the polygons of the coverage tests, a float64 even-odd rule, an independent float64
statement of the camera chain, seeded kernel inputs, and a synthetic BUP20-shaped folder written with PIL and pagnerf_amd.visualize.write_png."""
import bz2
import json
import math
import os
import pickle

import numpy as np
import torch

H0, W0 = 24, 32
SEQ_NUM_FRAMES = 4
SEQ_LEN = 14
EVAL_POS, TRAIN_POS = (2, 6, 9, 12), (7,)          # positions in the sequence: eval 2 and 12 are too close to the ends for n = 4
PREDS = ("preds_mask2former", "preds_maskrcnn", "preds_deeplab", "preds_pan_unet")
CLASS_LABELS = ["bg", "pepper"]

RECTANGLE = [2, 2, 7, 2, 7, 7, 2, 7]
TRIANGLE = [3.3, 2.1, 28.7, 5.5, 12.2, 21.9]
STAR = [c for i in range(10) for c in (16 + (11 if i % 2 == 0 else 4.5) * math.cos(2 * math.pi * i / 10), 12 + (11 if i % 2 == 0 else 4.5) * math.sin(2 * math.pi * i / 10))]
QUAD = [-5.5, -3.2, 20.1, 4.4, 36.6, 30.3, 10, 18.2]
SLIVER = [4, 4, 28, 4.3, 28, 4.6]
POLYGONS = dict(rectangle=RECTANGLE, triangle=TRIANGLE, star=STAR, quad=QUAD, sliver=SLIVER)
AREAS = dict(rectangle=25, triangle=240, star=140, quad=409, sliver=4)          # at 24 x 32


def even_odd(poly, h, w):
    """-> (inside bool [h,w], distance float64 [h,w]): the float64 even-odd rule at the pixel centres (x + 0.5, y + 0.5) and their distance to the
    polygon's boundary."""
    p = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    inside = np.zeros((h, w), dtype=bool)
    dist = np.full((h, w), np.inf)
    for (x0, y0), (x1, y1) in zip(p, q):
        if y0 != y1:
            crosses = ((y0 <= ys) != (y1 <= ys)) & (xs < x0 + (ys - y0) * (x1 - x0) / (y1 - y0))
            inside ^= crosses
        dx, dy = x1 - x0, y1 - y0
        L2 = dx * dx + dy * dy
        t = np.clip(((xs - x0) * dx + (ys - y0) * dy) / L2, 0, 1) if L2 > 0 else np.zeros_like(xs)
        dist = np.minimum(dist, np.hypot(xs - (x0 + t * dx), ys - (y0 + t * dy)))
    return inside, dist


def full_cover(h, w):
    """A polygon whose vertex box contains the h x w image: it covers every pixel."""
    return [-1, -1, w + 1, -1, w + 1, h + 1, -1, h + 1]


def annotation_sets(h, w):
    """{name: [(label, segmentation)]} at h x w: the label cases of the GPU test (the polygons are placed for 24 x 32 and clip at smaller sizes)."""
    from pagnerf_amd import bup20
    sx, sy = w / 32.0, h / 24.0
    scale = lambda poly: [c * (sx if i % 2 == 0 else sy) for i, c in enumerate(poly)]
    blob = np.zeros((h, w), dtype=bool)
    blob[h // 3:h // 3 + 3, 1:w - 2] = True
    blob[0, 0] = blob[h - 1, w - 1] = True
    rle_list, rle_string = bup20.mask_rle(blob)
    return dict(
        five=[(1, [scale(TRIANGLE)]), (1, [scale(STAR)]), (0, [scale(QUAD)]), (1, [scale(SLIVER)]), (1, [scale(RECTANGLE)])],
        outside=[(1, [[w + 3, 2, w + 9, 2, w + 6, 8]]), (1, [[-9, -9, -2, -9, -2, -2]])],
        on_boundary=[(1, [[2.0, 3.0, w - 4.5, 3.5, w / 2.0, h - 2.5]]), (1, [[0, 0, 5, 0, 5, 5, 0, 5]])],
        two_parts=[(1, [scale(RECTANGLE), scale(TRIANGLE)]), (1, []), (1, [[1, 1, 6, 1, 6, 6]])],
        rle=[(1, rle_list), (1, [scale(STAR)]), (1, rle_string)],
        restart=[(1, [scale(STAR)]), (1, bup20.mask_rle(np.ones((h, w), dtype=bool))[1]), (1, [scale(TRIANGLE)]), (1, [full_cover(h, w)]),
                 (1, [scale(RECTANGLE)]), (1, [scale(STAR)])],
    )


# ------------------------------------------------------------------------------------------------------------------------------------- cameras
def quat_matrix(q):
    """(qx, qy, qz, qw) -> rotation float64 [3,3], the textbook formula on the normalised quaternion."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def rigid_inverse(T):
    return rigid(T[:3, :3].T, -T[:3, :3].T @ T[:3, 3])


def expected_cameras(odom, names, center, E, scale, offset):
    """The camera chain written out for rigid transforms in float64, nothing of the package: odom {name: 4x4} -> (c2w [V,3,4], view [V,4,4])."""
    c2w, views = [], []
    for n in names:
        frame = rigid_inverse(E) @ rigid_inverse(odom[n]) @ odom[center] @ E
        R = frame[:3, :3] * np.array([1.0, -1.0, -1.0])[None, :]            # OpenCV -> GL: the y and z columns change sign
        t = frame[:3, 3] * scale + np.asarray(offset, dtype=np.float64)
        view = rigid(R * np.array([-1.0, -1.0, 1.0])[None, :], t)          # the world's x and y axes change sign
        views.append(view)
        c2w.append(rigid_inverse(view)[:3])
    return np.stack(c2w), np.stack(views)


# --------------------------------------------------------------------------------------------------------------------------------------- folder
def timestamps(n=SEQ_LEN):
    return ["16009%08d" % (1000 * i + 17) for i in range(n)]


def scene_odometry(n=SEQ_LEN, seed=3):
    """n rigid transforms as (t [3], q [4] not normalised): a camera that drifts along x and turns a little."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        q = np.array([0.02 * math.sin(i), 0.03 * math.cos(2 * i), 0.01 * i, 1.0]) * (1.0 + 0.1 * rs.rand())
        out.append((np.array([0.05 * i, 0.01 * math.sin(i), 0.4 + 0.005 * i]) + 0.002 * rs.standard_normal(3), q))
    return out


def write_ply(path, vertices, binary):
    v = np.asarray(vertices, dtype=np.float32)
    header = "ply\nformat %s 1.0\ncomment test\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n" \
             "element face 1\nproperty list uchar int vertex_indices\nend_header\n" % ("binary_little_endian" if binary else "ascii", len(v))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        if binary:
            rows = np.zeros(len(v), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1")])
            rows["x"], rows["y"], rows["z"], rows["red"] = v[:, 0], v[:, 1], v[:, 2], 200
            f.write(rows.tobytes())
            f.write(bytes([3]) + np.array([0, 1, 2], dtype="<i4").tobytes())
        else:
            for x, y, z in v:
                f.write(("%r %r %r 200\n" % (float(x), float(y), float(z))).encode("ascii"))
            f.write(b"3 0 1 2\n")


def predictions(rs, h, w):
    """A detector's output for one frame: semantics, instance ids 0..3 as blocks, a confidence / logit plane."""
    imap = np.zeros((h, w), dtype=np.int64)
    imap[2:h // 2, 2:w // 3] = 1
    imap[h // 2:h - 2, w // 3:w // 2 + 3] = 2
    imap[3:h - 3, w - 8:w - 1] = 3
    sem = (imap > 0).astype(np.int64)
    return sem, imap, rs.uniform(0.05, 3.0, (h, w)).astype(np.float32)


def write_predictions(folder, stem, rs, h, w):
    sem, imap, conf = predictions(rs, h, w)
    for name in PREDS:
        os.makedirs(os.path.join(folder, name), exist_ok=True)
    with open(os.path.join(folder, "preds_mask2former", stem + ".pkl"), "wb") as f:
        pickle.dump((torch.from_numpy(sem), torch.from_numpy(imap), torch.from_numpy(conf)), f)
    masks = torch.zeros(3, 1, h, w)
    for i in range(3):
        masks[i, 0] = torch.from_numpy((imap == i + 1) * conf.clip(0.55, 0.99) + (imap != i + 1) * (imap > 0) * 0.2)
    with open(os.path.join(folder, "preds_maskrcnn", stem + ".pkl"), "wb") as f:
        pickle.dump(dict(masks=masks), f)
    with open(os.path.join(folder, "preds_deeplab", stem + ".pkl"), "wb") as f:
        pickle.dump(dict(panoptic=torch.from_numpy(np.stack([sem, imap])[None])), f)
    with bz2.open(os.path.join(folder, "preds_pan_unet", stem + ".pkl.bz2"), "wb") as f:
        pickle.dump(dict(sem_seg=dict(preds=sem, confidence=torch.from_numpy(conf.clip(0, 1))[None]), instances=dict(imap=imap)), f)


def write_tree(root, cka_names=False, seed=0):
    """The synthetic dataset under `root` -> dict(ts, seq folder, odom {ts: 4x4}, E, K, images {ts: uint8 [H0,W0,3]}, depths {ts: uint16 [H0,W0]},
    anns {position: [(label, segmentation)]} of the eval frames)."""
    from PIL import Image
    from pagnerf_amd.visualize import write_png
    import yaml
    rs = np.random.RandomState(seed)
    ts = timestamps()
    seq = os.path.join(root, "20200924", "row3")
    os.makedirs(os.path.join(seq, "depth"), exist_ok=True)
    images, depths = {}, {}
    for i, t in enumerate(ts):
        images[t] = rs.randint(0, 256, (H0, W0, 3)).astype(np.uint8)
        write_png(os.path.join(seq, t + ".png"), images[t])
        d = rs.randint(300, 2600, (H0, W0)).astype(np.uint16)
        d[:2, :5] = 0
        d[2, :3] = (1399, 1400, 1401)
        depths[t] = d
        Image.fromarray(d).save(os.path.join(seq, "depth", t + ".png"))
        write_predictions(seq, t, rs, H0, W0)
    with open(os.path.join(seq, "notes.txt"), "w") as f:           # another suffix: not part of the sequence
        f.write("x")
    raw = scene_odometry()
    odom = {t: rigid(quat_matrix(q), tr) for t, (tr, q) in zip(ts, raw)}
    for name in ("odometry.csv", "rgbd_odom.csv"):
        with open(os.path.join(seq, name), "w") as f:
            f.write("#timestamp,tx,ty,tz,qx,qy,qz,qw\n")
            for t, (tr, q) in zip(ts, raw):
                f.write(",".join([t] + [repr(float(v)) for v in list(tr) + list(q)]) + "\n")
    meta = np.stack([odom[t] for t in ts])
    meta[:, :3, 3] /= 0.03
    np.savez(os.path.join(seq, "metashape_cameras.npz"), meta, np.array(ts))
    E = rigid(quat_matrix([0.5, -0.5, 0.5, -0.45]), [0.02, -0.01, 0.1])
    K = np.array([[41.3, 0.0, W0 / 2 + 0.7], [0.0, 39.9, H0 / 2 - 0.4], [0.0, 0.0, 1.0]])
    with open(os.path.join(seq, "params.yaml"), "w") as f:
        yaml.safe_dump(dict(intrinsics=K.tolist(), extrinsics=E.tolist()), f)

    sets = annotation_sets(H0, W0)
    anns = {6: sets["five"] + sets["rle"][:1], 9: sets["restart"], 2: sets["two_parts"], 12: sets["outside"]}
    cats = [dict(id=7, name="pepper_red", supercategory="pepper"), dict(id=3, name="bg", supercategory="none"), dict(id=9, name="leaf", supercategory="plant")]
    doc = dict(images=[], annotations=[], categories=cats)
    ids = {}
    for pos in sorted(set(EVAL_POS + TRAIN_POS)):
        ids[pos] = 100 + pos
        doc["images"].append(dict(id=ids[pos], path="/data/BUP_20/20200924/row3/%s.png" % ts[pos], height=H0, width=W0))
        for label, seg in anns.get(pos, []):
            doc["annotations"].append(dict(id=len(doc["annotations"]), image_id=ids[pos], category_id=7 if label else 3, segmentation=seg, iscrowd=0))
            if len(doc["annotations"]) % 3 == 0:                  # a category outside class_labels: skipped, and takes no instance index
                doc["annotations"].append(dict(id=len(doc["annotations"]), image_id=ids[pos], category_id=9, segmentation=[RECTANGLE], iscrowd=0))
    name = "CKA_sweet_pepper_2020_summer" if cka_names else "BUP_20"
    with open(os.path.join(root, name + ".json"), "w") as f:
        json.dump(doc, f)
    with open(os.path.join(root, name + ".yaml"), "w") as f:
        yaml.safe_dump(dict(image_sets=dict(train=[ids[p] for p in TRAIN_POS], valid=[], eval=[ids[p] for p in EVAL_POS])), f)
    return dict(ts=ts, seq=seq, odom=odom, E=E, K=K, images=images, depths=depths, anns=anns)


def window_positions(split, center):
    """The sequence positions of the window about position `center` for n = 4, written out by hand from the rule."""
    deltas = (5, 3, 1, -1, -3, -5) if split == "train" else (4, 2, 0, -2, -4)
    pos = [min(SEQ_LEN - 1, max(0, center - d)) for d in deltas]
    drop = set(TRAIN_POS) | ({6, 9} if split == "train" else set())
    return [p for p in pos if p not in drop]


# ---------------------------------------------------------------------------------------------------------------------------- kernel inputs
# (H0, W0, mips): fewer pixels than a wave, the folder's size, several workgroups with a ragged tail
SHAPES = ((10, 14, (0, 1)), (24, 32, (0, 1, 2)), (66, 130, (0, 1)))


def frame_inputs(B, h, w, C0=3, seed=0, max_id=6):
    """Seeded chunk inputs: img uint8 [B,h,w,C0], depth int16 bit patterns, sem / inst int32, conf float32, with the depth filter's edge cases in view 0:
    id 1 exactly at 2 valid == total, id 2 one pixel above it (for max_depth 1.4), id 4 absent, depth 0, raw 1399 / 1400 / 1401, the maximum id."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, h, w, C0), dtype=torch.uint8, generator=g)
    depth = torch.randint(200, 1390, (B, h, w), generator=g).to(torch.int32)           # valid for max_depth 1.4: the other ids are kept
    inst = torch.randint(0, max_id + 1, (B, h, w), generator=g).to(torch.int32)
    inst[inst == 4] = 0
    inst[inst == 1] = 5
    inst[inst == 2] = 5
    inst[:, 0, :8] = torch.tensor([1, 1, 1, 1, 2, 2, 2, max_id], dtype=torch.int32)
    depth[:, 0, :8] = torch.tensor([900, 900, 0, 5000, 900, 900, 5000, 900], dtype=torch.int32)        # id 1: 2 of 4 valid; id 2: 2 of 3 (max_depth 1.4)
    depth[:, 1, :6] = torch.tensor([1399, 1400, 1401, 0, 65535, 40000], dtype=torch.int32)             # about the threshold; words above 2^15
    sem = (inst > 0).to(torch.int32) + (inst > 3).to(torch.int32)
    conf = torch.rand(B, h, w, generator=g)
    raw = torch.where(depth >= 32768, depth - 65536, depth).to(torch.int16)
    return img, raw, sem, inst, conf


def leaves(ds):
    """{(mode, field): tensor [V,h,w,C] (a shared mode: [h,w,C])} of a DeviceMultiviewDataset."""
    h, w = ds.image_shape
    return {(l.key, l.field): l.src.reshape((ds.num_imgs, h, w, -1) if l.per_view else (h, w, -1)) for l in ds._leaves}
