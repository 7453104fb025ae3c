#!/usr/bin/env python3
"""Generate g13_panoptic.npz from the REFERENCE's utils/metrics/panoptic_quality_func.py and utils/outlier_rejection.py (imported unmodified from the
reference checkout) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_panoptic.py

PQ: _prepocess_image, _panoptic_quality_update and _panoptic_quality_compute, with the PanopticQuality class's state accumulation restated over the
updates (the class itself needs torchmetrics.metric.Metric, which is not installed).  Per case the fixture holds things / stuff (sorted, and the set
iteration order they were used in), each update's preds and target, the accumulated iou_sum / tp / fp / fn and the nine compute() values.

Cleanup: pc_nerf/trainer.py:750-772 restated on int64 [K, H, W] masks - the flat 3x3 opening written out per mask (kornia is not installed: erosion
with outside pixels inside the mask, dilation with outside pixels outside), the reference's mask_center_of_mass_outlier_rejection, the < min_area
removal and the argmax relabel.  An outlier case is only kept when no mask pixel's distance lies within 1e-4 relative of its threshold; otherwise the
next seed is tried.  The maker checks that the numpy restatement of tests/test_panoptic_eval_host.py reproduces every case.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PAGNERF_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import test_panoptic_eval_host as H                                 # noqa: E402

MARGIN = 1e-4


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod


def reference_modules():
    # utils/outlier_rejection.py imports kaolin and wisp at module level for functions not used here
    for name in ("kaolin", "kaolin.render"):
        _stub(name)
    _stub("kaolin.render.camera", Camera=object)
    _stub("wisp")
    _stub("wisp.core", Rays=object)
    from utils.metrics import panoptic_quality_func as F
    from utils import outlier_rejection as O
    return F, O


def reference_pq(F, things, stuff, updates, allow_unknown=True):
    void = F._get_void_color(things, stuff)
    cid = F._get_category_id_to_continous_id(things, stuff)
    n = len(things) + len(stuff)
    st = [torch.zeros(n, dtype=torch.double)] + [torch.zeros(n, dtype=torch.int) for _ in range(3)]
    for p, t in updates:
        fp = F._prepocess_image(things, stuff, torch.from_numpy(p.copy()), void, allow_unknown)
        ft = F._prepocess_image(things, stuff, torch.from_numpy(t.copy()), void, True)
        for i, v in enumerate(F._panoptic_quality_update(fp, ft, cid, void)):
            st[i] += v
    res = F._panoptic_quality_compute(things, stuff, *st)
    comp = np.array([float(res[g][k]) for g in ("all", "things", "stuff") for k in ("pq", "rq", "sq")])
    return [s.numpy() for s in st], comp


def _open_masks(masks):
    """Flat 3x3 opening of [K, H, W] masks: erosion = min over the in-image 3x3 neighbourhood, dilation = max over it."""
    K, Hh, Ww = masks.shape
    p = torch.nn.functional.pad(masks, (1, 1, 1, 1), value=2)                   # masks are 0 / 1: 2 is "inside", -1 "outside"
    er = torch.stack([p[:, dy:dy + Hh, dx:dx + Ww] for dy in range(3) for dx in range(3)]).min(0).values
    p = torch.nn.functional.pad(er, (1, 1, 1, 1), value=-1)
    return torch.stack([p[:, dy:dy + Hh, dx:dx + Ww] for dy in range(3) for dx in range(3)]).max(0).values


def reference_clean(O, ids, num_openings, outlier, min_area, std_threshold):
    instances = torch.from_numpy(ids)
    inst_type = instances.dtype
    mask_ids = instances.unique()
    if mask_ids.shape[0] <= 1:
        return ids.copy(), True
    masks = (instances == mask_ids[1:][:, None, None]).type(inst_type)
    for _ in range(num_openings):
        masks = _open_masks(masks).type(inst_type)
    margin_ok = True
    if outlier:
        # margin check in the reference's float32 arithmetic
        cy, cx, gy, gx = O.center_of_mass(masks)
        d = torch.sqrt((gy - cy[:, None, None]) ** 2 + (gx - cx[:, None, None]) ** 2)
        nd = d.clone()
        nd[~masks.bool()] = torch.nan
        mean = torch.nanmean(nd, dim=(-1, -2), keepdim=True)
        std = torch.sqrt(torch.nanmean((nd - mean) ** 2, dim=(-1, -2), keepdim=True))
        thr = mean + std_threshold * std
        close = (torch.abs(d - thr) <= MARGIN * thr) & masks.bool()
        margin_ok = not bool(close.any())
        masks = O.mask_center_of_mass_outlier_rejection(masks, std_threshold=std_threshold)
    small = masks.sum(dim=[1, 2]) < min_area
    masks[small] = torch.zeros_like(masks[0])
    stack = torch.cat(((masks.sum(dim=0) == 0).type(inst_type)[None], masks))
    return mask_ids[torch.argmax(stack, dim=0)].numpy(), margin_ok


def pq_cases():
    cases = []
    dp = np.array([[[[6, 0, 6, 6], [0, 0, 6, 0], [0, 0, 6, 0], [0, 7, 6, 1], [0, 7, 7, 7]],
                    [[0, 0, 0, 0], [0, 0, 0, 9], [0, 0, 0, 9], [0, 0, 0, 0], [0, 0, 0, 0]]]], np.int64)
    dt = np.array([[[[6, 0, 6, 0], [0, 0, 6, 0], [0, 0, 6, 1], [0, 7, 1, 1], [0, 7, 7, 7]],
                    [[0, 1, 0, 1], [1, 1, 0, 1], [1, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]]]], np.int64)
    cases.append(("docstring", {0, 1}, {6, 7}, [(dp, dt)]))

    rs = np.random.RandomState(11)
    p, t = H.synth_panoptic(rs, 1, 96, 128, {1, 2, 3}, {4, 5}, 12, extra_cats=(6,))
    t[0, 0][rs.rand(96, 128) < 0.05] = -1                            # unlabelled
    t[0, 0][:8, :16] = -1
    p[0, 0][rs.rand(96, 128) < 0.02] = 9                             # unknown pred category
    p[0, 0][40:56, 60:80] = 6                                        # the void colour's own category id
    cases.append(("mixed", {1, 2, 3}, {4, 5}, [(p, t)]))

    rs = np.random.RandomState(12)
    p, t = H.synth_panoptic(rs, 2, 96, 128, {1, 2}, {3}, 4)
    for a in (p, t):
        a[0, 1] = np.where(a[0, 1] % 2 == 0, 0, 3)                   # image 0 ids {0, 3}
        a[1, 1] = np.where(a[1, 1] % 2 == 0, 0, 2)                   # image 1 ids {0, 2}: 2 + 3 collides with image 0's 3
    cases.append(("batch2_collision", {1, 2}, {3}, [(p, t)]))

    # IoU exactly 0.5 (not matched) and a void fraction exactly 0.5 (not skipped)
    t = np.zeros((1, 2, 4, 8), np.int64)
    p = np.zeros((1, 2, 4, 8), np.int64)
    t[0, 0] = 2
    p[0, 0] = 2
    t[0, 0, :, :2] = 1; t[0, 1, :, :2] = 1                          # target thing: 8 px
    p[0, 0, :, 1:3] = 1; p[0, 1, :, 1:3] = 5                         # pred thing: 8 px, 4 shared -> IoU 4 / 12
    p[0, 0, 0:2, 0] = 1; p[0, 1, 0:2, 0] = 5                         # ... 6 shared, union 12 -> IoU exactly 0.5
    t[0, 0, :, 4:6] = 1; t[0, 1, :, 4:6] = 7                         # second target: 8 px, half predicted void
    p[0, 0, :, 4] = 3                                                # category 3 is unknown -> void colour: void fraction 4 / 8
    p[0, 0, :, 5] = 2                                                # the rest of it predicted as stuff: unmatched, counted as fn
    t[0, 0, :, 7] = 3                                                # target void under half of a pred thing: void fraction 4 / 8
    p[0, 0, :, 6:8] = 1; p[0, 1, :, 6:8] = 9                         # ... unmatched, counted as fp
    cases.append(("half_iou_half_void", {1}, {2}, [(p, t)]))

    rs = np.random.RandomState(13)
    t = np.zeros((1, 2, 64, 64), np.int64)
    t[0, 0] = 1
    t[0, 1] = np.arange(64 * 64).reshape(64, 64)
    p = t.copy()
    sel = rs.rand(64, 64) < 0.3
    p[0, 1][sel] = rs.randint(0, 64 * 64, size=int(sel.sum()))       # merged and split one-pixel segments
    cases.append(("segment_per_pixel", {1}, {2}, [(p, t)]))

    rs = np.random.RandomState(14)
    p, t = H.synth_panoptic(rs, 1, 96, 128, {1, 2}, {3}, 6)
    cases.append(("unseen_category", {1, 2}, {3, 8}, [(p, t)]))      # stuff 8 appears nowhere: left out of the means

    rs = np.random.RandomState(15)
    p, t = H.synth_panoptic(rs, 1, 96, 128, {1, 2}, {3}, 6)
    p[0, 0][p[0, 0] == 3] = 1
    t[0, 0][t[0, 0] == 3] = 2
    cases.append(("no_detections", {1, 2}, {3}, [(p, t)]))           # no stuff pixel anywhere: the stuff group is nan

    rs = np.random.RandomState(16)
    p, t = H.synth_panoptic(rs, 1, 96, 128, {8, 1, 3}, {20, 5}, 10)
    cases.append(("set_order", {8, 1, 3}, {20, 5}, [(p, t)]))

    rs = np.random.RandomState(17)
    ups = [H.synth_panoptic(rs, 1, 96, 128, {1, 2, 3}, {4}, 9, flip=f) for f in (0.02, 0.05, 0.1)]
    cases.append(("three_updates", {1, 2, 3}, {4}, ups))
    return cases


def clean_cases():
    """(name, seed, generator, args) -> ids image; args = (num_openings, outlier_rejection, min_area, std_threshold)."""
    def gen_bg5(rs):
        return H.synth_ids(rs, 96, 128, [5, 7, 9, 12, 30, 31], cell=16, noise=0.03)

    def gen_neg(rs):
        return H.synth_ids(rs, 96, 128, [-7, -2, 0, 4, 11], cell=12, noise=0.02)

    def gen_single(rs):
        return np.full((96, 128), 42, np.int64)

    def gen_small(rs):
        img = np.zeros((96, 128), np.int64)
        img[10:22, 10:22] = 3                                        # 144 px -> 144 after opening
        img[40:49, 40:52] = 4                                        # 108 px
        img[40:49, 52] = 4                                           # a 1-px spur: opened away
        img[60:70, 60:70] = 5                                        # 100 px: exactly min_area
        img[80:83, 5:45] = 6                                         # 3 x 40: survives the opening (120 px)
        img[85:87, 5:80] = 7                                         # 2 px thick: opened away
        img[5:15, 100:109] = 8                                       # 90 px: too small
        return img

    def gen_border(rs):
        img = H.synth_ids(rs, 96, 128, [1, 2, 3, 4, 5, 6, 7], cell=24, noise=0.0)
        img[0, :] = 9
        img[:, -1] = 10
        img[-2:, :20] = 11
        return img

    def gen_outlier(rs):
        img = np.zeros((96, 128), np.int64)
        for k in range(1, 6):
            y, x = rs.randint(10, 80), rs.randint(10, 110)
            img[y - 6:y + 6, x - 8:x + 8] = k
            yy, xx = rs.randint(0, 93), rs.randint(0, 125)
            img[yy:yy + 3, xx:xx + 3] = k                            # a far fragment of the same id
        return img

    return [("bg_not_zero", 500, gen_bg5, (1, False, 100, 2.0)),
            ("negative_ids_outlier", 510, gen_neg, (1, True, 100, 2.0)),
            ("single_id", 520, gen_single, (1, True, 100, 2.0)),
            ("small_masks", 530, gen_small, (1, False, 100, 2.0)),
            ("border", 540, gen_border, (1, False, 100, 2.0)),
            ("border_outlier", 550, gen_border, (1, True, 100, 2.0)),
            ("outlier_on", 560, gen_outlier, (1, True, 20, 2.0)),
            ("outlier_off", 560, gen_outlier, (1, False, 20, 2.0)),
            ("no_opening_outlier", 570, gen_outlier, (0, True, 20, 1.5)),
            ("three_openings", 530, gen_small, (3, False, 100, 2.0))]


def main():
    F, O = reference_modules()
    out = {}
    names = []
    for name, things, stuff, updates in pq_cases():
        st, comp = reference_pq(F, things, stuff, updates)
        for i, (p, t) in enumerate(updates):
            out["%s/preds%d" % (name, i)] = p.astype(np.int32)
            out["%s/target%d" % (name, i)] = t.astype(np.int32)
        out[name + "/n_updates"] = np.int64(len(updates))
        out[name + "/things"] = np.array(sorted(things), np.int64)
        out[name + "/stuff"] = np.array(sorted(stuff), np.int64)
        out[name + "/things_order"] = np.array(list(things), np.int64)
        for k, v in zip(("iou_sum", "tp", "fp", "fn"), st):
            out[name + "/" + k] = v
        out[name + "/compute"] = comp
        mine = H.restated_states(things, stuff, updates)
        assert mine[0].tobytes() == st[0].tobytes() and all(np.array_equal(a, b) for a, b in zip(mine[1:], st[1:])), name
        names.append(name)
        print("pq %-20s pq %s tp %s fp %s fn %s" % (name, comp[0], st[1].tolist(), st[2].tolist(), st[3].tolist()))
    out["pq_names"] = np.array(names)

    cnames = []
    for name, seed, gen, args in clean_cases():
        for s in range(seed, seed + 50):
            ids = gen(np.random.RandomState(s))
            ref, ok = reference_clean(O, ids, *args)
            if ok:
                break
        else:
            raise RuntimeError("no seed without a near-threshold pixel for " + name)
        mine = H.np_clean(ids, num_openings=args[0], outlier_rejection=args[1], min_area=args[2], std_threshold=args[3])
        assert np.array_equal(mine, ref), name
        out[name + "/ids"] = ids.astype(np.int32) if ids.min() >= -2**31 and ids.max() < 2**31 else ids
        out[name + "/cleaned"] = ref.astype(out[name + "/ids"].dtype)
        out[name + "/args"] = np.array(args, np.float64)
        cnames.append(name)
        print("clean %-20s seed %d ids %s -> %s" % (name, s, np.unique(ids).tolist(), np.unique(ref).tolist()))
    out["clean_names"] = np.array(cnames)
    path = os.path.join(HERE, "g13_panoptic.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
