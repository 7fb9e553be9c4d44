"""Time of the head's training objective on the GPU -- targets, the three losses and their backward to the nine head maps -- for the
ScanNet head on the G18 scenes (tests/head_loss_restated.py; 40x40x16 / 20x20x8 / 10x10x4 levels, 18 classes, thresholds 27 / 18)
and for the ARKit head on the G19 scenes (tests/head_loss_arkit_restated.py; the same levels, 17 classes, boxes with yaw,
RotatedIoU3DLoss; `--head arkit`), at 1, 12 and 60 ground-truth boxes per scene and batch 1 and 4, two routes alternated in one
process:

  hip    NerfDetHeadConvs.loss_by_feat on csrc/assign.hip + backward (six launches and a few element-wise operations per batch)
  dense  the same objective in the reference's form as ATen operations on the GPU (tests/head_loss_restated.dense_form_loss: per
         scene points x boxes tensors, boolean indexing, three host reads) + backward -- the reference itself needs mmdet / mmcv;
         the ARKit head's with the rotated IoU of tests/rotated_iou_restated.py in place of mmcv's diff_iou_rotated_3d

HIP events around each call (the device drained inside), medians over the repeats after warm-up.  One JSON line per (route, boxes,
batch); `--json PATH` also writes them as one JSON list.  `--only hip --reps 3` is what the kernel trace runs.

    python tools/head_loss_timing.py [--head scannet|arkit|both] [--reps 30] [--only hip] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import head_loss_arkit_restated as A  # noqa: E402
import head_loss_restated as R  # noqa: E402
from mvsdet_amd.head import NerfDetHeadConvs  # noqa: E402

KIND = {1: "one", 12: "twelve", 60: "sixty"}


def time_calls(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", choices=["hip", "dense"], default=None)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--head", choices=["scannet", "arkit", "both"], default="scannet")
    args = ap.parse_args()
    rows = []
    for which in (("scannet", "arkit") if args.head == "both" else (args.head,)):
        rows += time_head(which, args)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


def time_head(which, args):
    dev = torch.device("cuda:0")
    M = A if which == "arkit" else R   # scenes, ground-truth triplets and the dense form of the head
    head = NerfDetHeadConvs(n_classes=17, n_reg_outs=7, arkit_head=True) if which == "arkit" else NerfDetHeadConvs()
    rows = []
    for n_boxes in (1, 12, 60):
        for B in (1, 4):
            c, r, k, v, origins, gts = M.batch([KIND[n_boxes]] * B, [2700 + n_boxes + 5 * i for i in range(B)])
            maps = [t.to(dev).requires_grad_(True) for t in c + r + k]
            v = v.to(dev)
            gts_dev = [g.to(dev) for g in gts]
            trip = [M.gt_triplet(g) for g in gts]
            metas = R.metas_for(origins)
            seen = {}

            def total(losses):
                return losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]

            def hip():
                for m in maps:
                    m.grad = None
                t = total(head.loss_by_feat(maps[:3], maps[3:6], maps[6:], v, gts_dev, metas))
                t.backward()
                seen["hip"] = t.detach()

            def dense():
                for m in maps:
                    m.grad = None
                t = total(M.dense_form_loss(maps[:3], maps[3:6], maps[6:], v, trip, origins))
                t.backward()
                seen["dense"] = t.detach()

            timed = {}
            for rep in range(2):   # alternated: both routes warm up, then both are measured
                for route, fn in (("hip", hip), ("dense", dense)):
                    if args.only and route != args.only:
                        continue
                    ms = time_calls(fn, args.reps if rep else 3, 2)
                    timed[route] = ms
            for route, ms in timed.items():
                row = dict(head=which, route=route, boxes=n_boxes, batch=B, total_loss=round(float(seen[route]), 6), reps=args.reps,
                           ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


if __name__ == "__main__":
    main()
