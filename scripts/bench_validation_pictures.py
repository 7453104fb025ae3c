#!/usr/bin/env python3
"""The validation pictures of one 720 x 1280 image (pagnerf_amd.visualize, csrc/visualize.hip), and what they cost validate().

    python scripts/bench_validation_pictures.py [--blocks 5] [--iters 20] [--compare-tree DIR] [--json profiles/validation_pictures.json]

All inputs present: f32 rgb / depth / ground truth, six int64 label images (6 classes, 40 instance ids on 80-pixel blocks), two confidences.
  render_ms / reference_ms   ValidationPictures.render (two launches, 15 pictures) against validation_pictures_reference, the tensor-op form, on the
                             same GPU: --blocks alternating blocks of --iters calls each, HIP events around a block, per call; the median over
                             the blocks and their spread (max - min) are reported, and the pictures of the two are compared (they must be equal)
  copy_ms                    the stack [15,H,W,3] to a pinned host buffer, host clock around copy + synchronise
  png_ms_per_picture         write_png of each of the 15 pictures (level 3, one thread), host clock; with the file sizes
  validate_ms_per_image      PanopticTrainer.validate on the scene of tests/test_gpu_trainer.py (2 views of 32 x 32, a toy size: it measures validate()'s
                             overheads, which is what the switch must not add to) with val_pictures off and on, in child processes that alternate;
                             --compare-tree DIR adds blocks of another checkout of this repository (built, e.g. the commit before) with the switch off.
                             A block is the median of --iters validate() calls after 2 warm-ups; spread = max - min over a variant's blocks.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def validate_block(tree, pictures, iters):
    """Child process: per-image validate() times [ms] of one block in checkout `tree`."""
    sys.path.insert(0, os.path.join(tree, "tests"))
    sys.path.insert(0, tree)
    import torch
    import test_gpu_trainer as T
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        extra = dict(val_pictures=True, num_val_frames_to_save=1) if pictures else {}
        pipe, tr = T.make_trainer(dev, tmp, use_graphs=False, **extra)
        n = (tr.val_dataset if tr.val_dataset is not None else tr.dataset).num_imgs
        times = []
        for i in range(iters + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.validate(0)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / n)
        written = len(os.listdir(os.path.join(tmp, "val", "epoch_0"))) if pictures else 0
    print(json.dumps({"ms_per_image": statistics.median(times[2:]), "files": written}), flush=True)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def inputs(dev, H, W):
    import torch
    g = torch.Generator(device=dev).manual_seed(0)
    blocks = torch.randint(0, 41, (H // 80, W // 80), device=dev, generator=g).repeat_interleave(80, 0).repeat_interleave(80, 1)
    noise = lambda p, hi: torch.where(torch.rand(H, W, device=dev, generator=g) < p, torch.randint(0, hi, (H, W), device=dev, generator=g), blocks)
    sem = lambda: (noise(0.02, 41) % 6)
    f = lambda *s: torch.rand(*s, device=dev, generator=g)
    return dict(rgb=f(H, W, 3), depth=0.2 + 5.0 * f(H, W, 1), gts=f(H, W, 3), semantics=sem(), instances=noise(0.001, 41), inst_conf=f(H, W), sem_gt=sem(),
                inst_gt=noise(0.0, 41), sem_pred=sem(), inst_pred=noise(0.01, 41), inst_conf_pred=f(H, W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--compare-tree", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--validate-block", nargs=2, metavar=("TREE", "PICTURES"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.validate_block:
        return validate_block(a.validate_block[0], a.validate_block[1] == "1", a.iters)
    sys.path.insert(0, ROOT)
    import torch
    import pagnerf_amd
    from pagnerf_amd import visualize as V
    dev = torch.device("cuda:0")
    H, W = 720, 1280
    d = inputs(dev, H, W)
    keys = ("semantics", "instances", "inst_conf", "sem_gt", "inst_gt", "sem_pred", "inst_pred", "inst_conf_pred")
    rb = pagnerf_amd.RenderBuffer(rgb=d["rgb"], depth=d["depth"])
    vp = V.ValidationPictures()
    kernel = lambda: vp.render(rb, d["gts"], **{k: d[k] for k in keys})
    reference = lambda: V.validation_pictures_reference(rb, d["gts"], **{k: d[k] for k in keys})
    got, want = kernel(), reference()
    assert list(got) == list(want) == list(V.PICTURES) and all(torch.equal(got[n], want[n]) for n in want), "pictures differ from the tensor-op form"
    out = {"image": [H, W], "pictures": len(got), "blocks": a.blocks, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "boxes_present": int((V.instance_boxes(d["instances"])[:, 0] <= V.instance_boxes(d["instances"])[:, 2]).sum())}

    def block(fn, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / n
    for fn in (kernel, reference):
        block(fn, 3)
    ker, ref = [], []
    for _ in range(a.blocks):
        ker.append(block(kernel, a.iters))
        ref.append(block(reference, max(2, a.iters // 5)))
    out["render_ms"], out["reference_ms"] = spread(ker), spread(ref)
    out["bytes_written_mb"] = round(vp.stack.numel() / 1e6, 2)

    host = torch.empty(vp.stack.shape, dtype=torch.uint8).pin_memory()
    copies = []
    for _ in range(a.iters + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(vp.stack, non_blocking=True)
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    out["copy_ms"] = spread(copies[2:])
    arrays = host.numpy()
    with tempfile.TemporaryDirectory() as tmp:
        png = {}
        for i, name in enumerate(got):
            path = os.path.join(tmp, name + ".png")
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                V.write_png(path, arrays[i])
                ts.append((time.perf_counter() - t0) * 1e3)
            png[name] = {"ms": round(statistics.median(ts), 2), "kb": os.path.getsize(path) // 1024}
    out["png_ms_per_picture"] = png
    out["png_ms_all_pictures_one_thread"] = round(sum(p["ms"] for p in png.values()), 1)

    variants = [("off", ROOT, "0"), ("on", ROOT, "1")] + ([("compare_tree_off", os.path.abspath(a.compare_tree), "0")] if a.compare_tree else [])
    blocks = {name: [] for name, _, _ in variants}
    for _ in range(a.blocks):
        for name, tree, pictures in variants:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--validate-block", tree, pictures], capture_output=True,
                               text=True, timeout=600, env=dict(os.environ, PAG_GRAPHS="0"))
            if r.returncode != 0:
                raise RuntimeError("validate block %s failed:\n%s" % (name, r.stderr[-3000:]))
            blocks[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out["validate_ms_per_image"] = {name: dict(spread([b["ms_per_image"] for b in bs]), files=bs[0]["files"]) for name, bs in blocks.items()}
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
