#!/usr/bin/env python3
"""The validation row of one 720 x 1280 image on the device (pagnerf_amd.metrics: MaskMeanAveragePrecision, PeakSignalNoiseRatio,
ValidationMetrics).

    python scripts/bench_validation_metrics.py [--iters 20] [--json profiles/validation_metrics.json]

Inputs are those of scripts/bench_panoptic_eval.py (6 classes, 200 predicted and 100 ground-truth instance ids on 40-pixel blocks) plus a
[720, 1280, 200] f32 instance channel and a [720, 1280, 6] semantic channel whose argmax are the predicted label images.  Timed with HIP events,
median of --iters after 3 warm-ups:
  map_update_ms       MaskMeanAveragePrecision.update(cleaned, target, pred_raw=instances, empty_detection_if_single_id=True)
  psnr_update_ms      PeakSignalNoiseRatio.update on the [..., :3] view of a four-channel target
  evaluator_ms        ValidationMetrics.update with labelled=(True, True), one opening and outlier rejection (the label path of best.yaml)
  three_in_a_row_ms   clean_instances, PanopticQuality.update and MulticlassIoU.update as bench_panoptic_eval.py times them, in the same run
  mask_stack_ms       the tensor-op form of the intersections: the distinct ids, one [K, H*W] f32 mask stack per side and one matmul
with the peak memory of the mAP update beside that of the mask-stack form, and the evaluator's time split by entry point (events around each call)
and by the two torch reductions over the instance channel.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_panoptic_eval import inputs, timed      # noqa: E402


def peak_extra_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from pagnerf_amd import RenderBuffer, ops
    from pagnerf_amd.metrics import (MaskMeanAveragePrecision, MulticlassIoU, PanopticQuality, PeakSignalNoiseRatio, ValidationMetrics,
                                     clean_instances)
    dev = torch.device("cuda:0")
    H, W = 720, 1280
    sem_p, inst_p, target = inputs(dev)
    sem_t, inst_t = target[0, 0].contiguous(), target[0, 1].contiguous()
    g = torch.Generator(device=dev).manual_seed(0)
    emb = 0.5 * torch.rand(H, W, 200, device=dev, generator=g)
    emb.scatter_(2, inst_p[..., None], 1.0)
    sem = 0.5 * torch.rand(H, W, 6, device=dev, generator=g)
    sem.scatter_(2, sem_p[..., None], 1.0)
    rb = RenderBuffer(rgb=torch.rand(H, W, 3, device=dev, generator=g), semantics=sem, inst_embedding=emb)
    gts = torch.rand(H, W, 4, device=dev, generator=g)
    assert torch.equal(emb.argmax(-1), inst_p) and torch.equal(sem.argmax(-1), sem_p)

    things, stuff = {1, 2, 3, 4}, {0, 5}
    cleaned = clean_instances(inst_p, num_openings=1, outlier_rejection=True)
    mp, psnr = MaskMeanAveragePrecision().to(dev), PeakSignalNoiseRatio().to(dev)
    ev = ValidationMetrics(6, things, stuff, inst_num_dilations=1, inst_outlier_rejection=True).to(dev)
    pq = PanopticQuality(things, stuff, allow_unknown_preds_category=True).to(dev)
    iou = MulticlassIoU(6).to(dev)

    def map_update():
        mp.update(cleaned, inst_t, pred_raw=inst_p, empty_detection_if_single_id=True)

    def evaluator():
        ev.update(rb, gts, sem_t, inst_t, labelled=(True, True))

    def three_in_a_row():
        c = clean_instances(inst_p, num_openings=1, outlier_rejection=True)
        pq.update(torch.stack((sem_p, c))[None], target)
        iou.update(sem_p, sem_t)

    def mask_stack():
        ids_d, ids_g = inst_p.unique()[1:], inst_t.unique()[1:]
        md = (cleaned.reshape(-1) == ids_d[:, None]).float()
        mg = (inst_t.reshape(-1) == ids_g[:, None]).float()
        return md @ mg.t(), md.sum(1), mg.sum(1)

    out = {"image": [H, W], "classes": 6, "pred_ids": 200, "gt_ids": 100, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for name, fn in (("map_update_ms", map_update), ("psnr_update_ms", lambda: psnr.update(rb.rgb[..., :3], gts[..., :3])),
                     ("evaluator_ms", evaluator), ("three_in_a_row_ms", three_in_a_row), ("mask_stack_ms", mask_stack),
                     ("argmax_and_max_ms", lambda: (torch.argmax(emb, dim=-1), torch.max(emb, dim=-1)[0]))):
        med, best = timed(fn, a.iters)
        out[name] = round(med, 4)
        out[name.replace("_ms", "_min_ms")] = round(best, 4)
    out["map_update_peak_extra_mb"] = peak_extra_mb(map_update)
    out["mask_stack_peak_extra_mb"] = peak_extra_mb(mask_stack)
    out["evaluator_peak_extra_mb"] = peak_extra_mb(evaluator)
    ops.profile_start(only={"pag_mask_ap_update", "pag_panoptic_clean", "pag_panoptic_pq_update", "pag_confusion_matrix"})
    for _ in range(a.iters):
        evaluator()
    out["evaluator_entry_points_ms"] = {k: round(statistics.median(v), 4) for k, v in ops.profile_stop().items()}
    # Both forms of the intersections on a prediction that follows the target (the timed ids are independent of it, so nothing matches there): half
    # of the target's blocks keep their id, half get id + 100, 1 % of the pixels are noise.  A pair with IoU >= 0.5 is the only such pair of its
    # detection and of its ground truth (disjoint masks; an exact 0.5 from two sides aside), so the greedy matching at 0.5 matches exactly those pairs.
    g2 = torch.Generator(device=dev).manual_seed(1)
    moved = torch.rand(H // 40, W // 40, device=dev, generator=g2) < 0.5
    pred2 = inst_t + 100 * moved.repeat_interleave(40, 0).repeat_interleave(40, 1)
    noise = torch.rand(H, W, device=dev, generator=g2) < 0.01
    pred2 = torch.where(noise, torch.randint(0, 200, (H, W), device=dev, generator=g2), pred2)
    ids_d, ids_g = pred2.unique()[1:101], inst_t.unique()[1:]
    md, mg = (pred2.reshape(-1) == ids_d[:, None]).float(), (inst_t.reshape(-1) == ids_g[:, None]).float()
    inter = md @ mg.t()
    union = md.sum(1)[:, None] + mg.sum(1)[None] - inter
    one = MaskMeanAveragePrecision().to(dev)
    one.update(pred2, inst_t)
    out["check_stack_pairs_iou_ge_0.5"] = int((inter / union >= 0.5).sum())
    out["check_matched_at_0.5"] = int(((one.slots[:100] >> 1) & 1).sum())
    out["check"] = {k: round(v, 6) for k, v in one.compute_fp64().items()}
    assert out["check_stack_pairs_iou_ge_0.5"] == out["check_matched_at_0.5"] > 0, out
    out["val"] = {k: round(v, 6) for k, v in ev.compute().items()}
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
