"""The BUP20 loader (pagnerf_amd/bup20.py) on the GPU at the dataset's size: 41 frames of 720 x 1280 (the val window at seq_num_frames = 40) of a synthetic
folder written here from a seed.

    python3 scripts/bench_bup20.py [--frames-h 720] [--frames-w 1280] [--reps 5] [--workers 16] [--out FILE]

Three things, each named for what it is:
  load      the whole load_bup20 call (host clock around a call that ends in a device synchronise): kernel path and use_kernel=False, alternating, with
            best.yaml's modes (imgs, semantics, instance, preds_mask2former; max_depth 1.4; mip 0).  It contains the host decode.
  launches  the two label launches (pag_coco_keys + pag_coco_labels, with the counting pass) of the centre frame's annotations and the two preparation
            launches (pag_bup20_pred_stats + pag_bup20_prepare) of the 41 frames against their tensor-op forms on the same device tensors, alternating,
            device-event times after warm-up, at mip 0 and 2; the results are compared before timing.  Event times include launch latency.
  decode    the host decode alone, one thread: one RGB PNG, one 16-bit depth PNG, one pickled mask2former prediction.
The parent commit has no loader to compare with, and no speed is claimed beyond what this prints.  Needs a GPU: there is no fallback."""
import argparse
import json
import math
import os
import pickle
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

N = 40                      # seq_num_frames
SEQ_LEN = 2 * N + 3         # the centre at N + 1 is N + 1 frames from both ends
MODES = ["imgs", "semantics", "instance", "preds_mask2former"]


def annotations(h, w, count=24):
    """`count` pepper-sized polygons of 24 vertices, one two-part, one polygon around the whole image (the counting pass) and one RLE."""
    from pagnerf_amd import bup20
    rs = np.random.RandomState(1)
    out = []
    for i in range(count):
        cx, cy, r = rs.uniform(0.1, 0.9) * w, rs.uniform(0.1, 0.9) * h, rs.uniform(0.03, 0.12) * h
        ring = lambda cx, cy, r: [c for k in range(24) for c in (cx + r * (1 + 0.2 * math.sin(3 * k)) * math.cos(2 * math.pi * k / 24),
                                                                  cy + r * (1 + 0.2 * math.sin(3 * k)) * math.sin(2 * math.pi * k / 24))]
        out.append((1, [ring(cx, cy, r)] + ([ring(cx + r, cy + r, r / 2)] if i == 3 else [])))
    out.append((0, [[-2, -2, w + 2, -2, w + 2, h + 2, -2, h + 2]]))
    blob = np.zeros((h, w), dtype=bool)
    blob[h // 4:h // 2, w // 3:w // 2] = True
    out.append((1, bup20.mask_rle(blob)[1]))
    return out


def write_folder(root, h, w):
    """The window's 41 frames with their content (a smooth picture with noise, depth about the 1.4 m threshold, a mask2former pickle of twelve instances),
    the other frames of the sequence as empty files of the right name (they are listed, never decoded)."""
    import yaml
    from PIL import Image
    from pagnerf_amd.visualize import write_png
    rs = np.random.RandomState(0)
    ts = ["16009%08d" % (1000 * i + 17) for i in range(SEQ_LEN)]
    seq = os.path.join(root, "20200924", "row3")
    os.makedirs(os.path.join(seq, "depth"))
    os.makedirs(os.path.join(seq, "preds_mask2former"))
    yy, xx = np.mgrid[0:h, 0:w]
    centre = N + 1
    for i, t in enumerate(ts):
        if (i - centre) % 2:
            open(os.path.join(seq, t + ".png"), "wb").close()
            continue
        pic = np.stack([(xx + 3 * i) % 256, (yy * 255 // h), (xx ^ yy) & 255], -1) + rs.randint(-6, 7, (h, w, 3))
        write_png(os.path.join(seq, t + ".png"), pic.clip(0, 255).astype(np.uint8))
        depth = (900 + 700 * np.sin(xx / 97.0 + i) * np.cos(yy / 61.0) + rs.randint(-20, 21, (h, w))).clip(0, 65535).astype(np.uint16)
        Image.fromarray(depth).save(os.path.join(seq, "depth", t + ".png"))
        imap = np.zeros((h, w), dtype=np.int32)
        for k in range(12):
            cx, cy, r = rs.uniform(0.1, 0.9) * w, rs.uniform(0.1, 0.9) * h, rs.uniform(0.04, 0.1) * h
            imap[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = k + 1
        with open(os.path.join(seq, "preds_mask2former", t + ".pkl"), "wb") as f:
            pickle.dump((torch.from_numpy((imap > 0).astype(np.int32)), torch.from_numpy(imap), torch.from_numpy(rs.standard_normal((h, w)).astype(np.float32) + 2)), f)
    with open(os.path.join(seq, "odometry.csv"), "w") as f:
        f.write("#timestamp,tx,ty,tz,qx,qy,qz,qw\n")
        for i, t in enumerate(ts):
            f.write("%s,%r,%r,%r,%r,%r,%r,1.0\n" % (t, 0.01 * i, 0.002 * math.sin(i), 0.4, 0.01 * math.sin(i), 0.01 * math.cos(i), 0.002 * i))
    with open(os.path.join(seq, "params.yaml"), "w") as f:
        yaml.safe_dump(dict(intrinsics=[[900.0, 0.0, w / 2.0], [0.0, 900.0, h / 2.0], [0.0, 0.0, 1.0]], extrinsics=np.eye(4).tolist()), f)
    anns = annotations(h, w)
    doc = dict(images=[dict(id=1, path="/data/BUP_20/20200924/row3/%s.png" % ts[centre], height=h, width=w)],
               annotations=[dict(id=i, image_id=1, category_id=1 if label else 2, segmentation=seg, iscrowd=0) for i, (label, seg) in enumerate(anns)],
               categories=[dict(id=1, name="pepper", supercategory="pepper"), dict(id=2, name="bg", supercategory="bg")])
    with open(os.path.join(root, "BUP_20.json"), "w") as f:
        json.dump(doc, f)
    with open(os.path.join(root, "BUP_20.yaml"), "w") as f:
        yaml.safe_dump(dict(image_sets=dict(train=[], valid=[], eval=[1])), f)
    return seq, ts, anns


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stat(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-h", type=int, default=720)
    ap.add_argument("--frames-w", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bup20.py needs a GPU (no fallback)")
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import bup20, ops
    dev = torch.device("cuda:0")
    h, w = a.frames_h, a.frames_w
    out = dict(frames=N + 1, size=[h, w], reps=a.reps, workers=a.workers, device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "BUP_20")
        os.makedirs(root)
        t0 = time.perf_counter()
        seq, ts, anns = write_folder(root, h, w)
        print(json.dumps(dict(folder_written_s=time.perf_counter() - t0)), flush=True)

        # ---- the whole load
        kw = dict(mip=0, load_modes=MODES, max_depth=1.4, seq_num_frames=N, device=dev, num_workers=a.workers)
        loads = {"kernel": [], "tensor_ops": []}
        for it in range(1 + a.reps):
            for name, use_kernel in (("kernel", True), ("tensor_ops", False)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ds = bup20.load_bup20(root, "val", use_kernel=use_kernel, **kw)
                torch.cuda.synchronize()
                if it:
                    loads[name].append((time.perf_counter() - t0) * 1e3)
                assert ds.num_imgs == N + 1
                del ds
        out["load"] = dict(what="load_bup20, split val, mip 0, %s, max_depth 1.4, %d decode threads; host clock to a device synchronise" % (MODES, a.workers),
                           **{k: stat(v) for k, v in loads.items()})
        print(json.dumps(out["load"]), flush=True)

        # ---- the launches against their tensor-op forms, on the frames the loader would stage
        paths = [os.path.join(seq, ts[N + 1 + d] + ".png") for d in range(-N, N + 1, 2)]
        img = torch.from_numpy(np.stack([bup20.decode_rgb(p) for p in paths])).to(dev)
        raw = torch.from_numpy(np.stack([bup20.decode_depth(os.path.join(seq, "depth", os.path.basename(p))) for p in paths]).view(np.int16)).to(dev)
        preds = [bup20.read_prediction(p, "preds_mask2former") for p in paths]
        sem, inst, conf = (torch.from_numpy(np.stack([q[i] for q in preds])).to(dev) for i in range(3))
        n_ids, V = int(inst.max()) + 1, len(paths)
        tables = bup20.coco_tables([anns], h, w)
        out["labels_tables"] = dict(annotations=len(anns), polygon_vertices=int(len(tables["verts"])), boundary_points=int(tables["point_begin"][-1]),
                                    key_slots=int(len(tables["keys"])), max_part_keys=tables["max_part_keys"], counting_candidates=int(len(tables["cand"])))
        out["launches"] = []
        for mip in (0, 2):
            hh, ww = h >> mip, w >> mip
            dst = dict(imgs=torch.empty(V, hh, ww, 3, device=dev), masks=torch.empty(V, hh, ww, 1, dtype=torch.bool, device=dev),
                       semantics_pred=torch.empty(V, hh, ww, 1, dtype=torch.int64, device=dev), instance_pred=torch.empty(V, hh, ww, 1, dtype=torch.int64, device=dev),
                       sem_conf_out=torch.empty(V, hh, ww, 1, device=dev), inst_conf_out=torch.empty(V, hh, ww, 1, device=dev))
            gt = [torch.empty(1, hh, ww, 1, dtype=torch.int64, device=dev) for _ in range(2)]

            def prep_kernel():
                counts = ops.bup20_pred_stats(inst, raw, 1.4, n_ids)
                ops.bup20_prepare(img, mip, "white", 0, depth_raw=raw, sem=sem, inst=inst, sem_conf=conf, inst_conf=conf, counts=counts, **dst)

            def prep_tensor():
                counts = bup20.pred_stats_reference(inst, raw, 1.4, n_ids)
                return bup20.prepare_frames_reference(img, mip, "white", None, sem, inst, conf, conf, counts)

            def labels_kernel():                    # the upload of the tables is part of the route: they are built per chunk
                t = ops.coco_upload(tables, dev)
                ops.coco_keys(t, h, w)
                ops.coco_labels(t, h, w, mip, 1, 0, semantics=gt[0], instance=gt[1])

            def labels_tensor():                    # the definition is NumPy on the host; its planes are uploaded
                s, i = bup20.coco_labels_reference(anns, h, w, mip, 1)
                return s.to(dev), i.to(dev)

            prep_kernel()
            want = prep_tensor()
            labels_kernel()
            ws, wi = labels_tensor()
            torch.cuda.synchronize()
            same = dict({k: bool(torch.equal(dst[k + "_out" if k.endswith("conf") else k], v)) for k, v in want.items()},
                        semantics=bool(torch.equal(gt[0][0], ws)), instance=bool(torch.equal(gt[1][0], wi)))
            del want
            times = dict(prepare_kernel=[], prepare_tensor_ops=[], labels_kernel=[], labels_host_definition=[])
            for it in range(2 + a.reps):
                for name, fn in (("prepare_kernel", prep_kernel), ("prepare_tensor_ops", prep_tensor), ("labels_kernel", labels_kernel),
                                 ("labels_host_definition", labels_tensor)):
                    t = event_ms(fn)
                    if it >= 2:
                        times[name].append(t)
            case = dict(case="%d x %d x %d, mip %d" % (V, h, w, mip), same_results=same, **{k: stat(v) for k, v in times.items()})
            out["launches"].append(case)
            print(json.dumps(case), flush=True)

        # ---- the host decode alone
        p = paths[0]
        dec = {}
        for name, fn in (("rgb_png", lambda: bup20.decode_rgb(p)), ("depth_png", lambda: bup20.decode_depth(os.path.join(seq, "depth", os.path.basename(p)))),
                         ("mask2former_pickle", lambda: bup20.read_prediction(p, "preds_mask2former"))):
            fn()
            v = []
            for _ in range(5):
                t0 = time.perf_counter()
                fn()
                v.append((time.perf_counter() - t0) * 1e3)
            dec[name] = stat(v)
        out["decode"] = dict(what="one %d x %d frame, one thread" % (h, w), **dec)
        print(json.dumps(out["decode"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1))
    print(json.dumps(dict(bench_bup20="done")))


if __name__ == "__main__":
    main()
