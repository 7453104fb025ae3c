#!/usr/bin/env python3
"""Device panoptic evaluation (pagnerf_amd.metrics, csrc/panoptic.hip) of one 720 x 1280 validation image.

    python scripts/bench_panoptic_eval.py [--iters 20] [--json out.json]

Inputs are synthetic: 6 classes on 40-pixel blocks, 200 predicted instance ids (1 % single-pixel noise) and 100 ground-truth ids.  Timed with HIP
events, median of --iters after 3 warm-ups: clean_instances with one opening and outlier rejection (the label path of best.yaml), one
PanopticQuality.update (allow_unknown_preds_category=True, as the trainer calls it) and one MulticlassIoU.update, each alone and the three in a
row.  Peak memory is the rise of torch's allocator peak over the three calls.

Budget (arithmetic, not measured): <= 1 ms per image for the three together.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def blocky(rs, H, W, cell, values):
    h, w = -(-H // cell), -(-W // cell)
    return np.kron(rs.choice(values, size=(h, w)), np.ones((cell, cell), dtype=np.int64))[:H, :W]


def inputs(dev, H=720, W=1280, seed=0):
    rs = np.random.RandomState(seed)
    sem_t = blocky(rs, H, W, 40, np.arange(6))
    inst_t = blocky(rs, H, W, 40, np.arange(100))
    sem_p = sem_t.copy()
    flip = blocky(rs, H, W, 40, [0, 0, 0, 1]).astype(bool)
    sem_p[flip] = rs.randint(0, 6, size=int(flip.sum()))
    inst_p = blocky(rs, H, W, 40, np.arange(200))
    m = rs.rand(H, W) < 0.01
    inst_p[m] = rs.randint(0, 200, size=int(m.sum()))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return d(sem_p), d(inst_p), d(np.stack((sem_t, inst_t))[None])


def timed(fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from pagnerf_amd.metrics import MulticlassIoU, PanopticQuality, clean_instances
    dev = torch.device("cuda:0")
    sem_p, inst_p, target = inputs(dev)
    pq = PanopticQuality({1, 2, 3, 4}, {0, 5}, allow_unknown_preds_category=True).to("cuda")
    iou = MulticlassIoU(6).to("cuda")
    cleaned = clean_instances(inst_p, num_openings=1, outlier_rejection=True)
    preds = torch.stack((sem_p, cleaned))[None]

    def all_three():
        c = clean_instances(inst_p, num_openings=1, outlier_rejection=True)
        pq.update(torch.stack((sem_p, c))[None], target)
        iou.update(sem_p, target[0, 0])

    out = {"image": [720, 1280], "classes": 6, "pred_ids": 200, "gt_ids": 100, "iters": a.iters, "budget_ms": 1.0,
           "device": torch.cuda.get_device_name(0)}
    for name, fn in (("clean_instances_ms", lambda: clean_instances(inst_p, num_openings=1, outlier_rejection=True)),
                     ("pq_update_ms", lambda: pq.update(preds, target)),
                     ("iou_update_ms", lambda: iou.update(sem_p, target[0, 0])),
                     ("all_three_ms", all_three)):
        med, best = timed(fn, a.iters)
        out[name] = round(med, 4)
        out[name.replace("_ms", "_min_ms")] = round(best, 4)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    all_three()
    torch.cuda.synchronize()
    out["peak_extra_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
    out["within_budget"] = out["all_three_ms"] <= 1.0
    pq.reset()
    pq.update(preds, target)
    res = pq.compute()
    out["pq_all"] = float(res["all"]["pq"])
    out["tp"] = int(pq.true_positives.sum())
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
