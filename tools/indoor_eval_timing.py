"""Time of the indoor metrics on a validation-set-sized synthetic set: 312 scenes, 18 labels, detections from ops.head_predict on the
random head maps of the G15 generator (tests/golden/make_goldens_g15.py; nms_pre 1000, score_thr .01, iou_thr .25; `--maps` distinct
scenes, reused in turn), ground truth = 0-9 jittered copies of a scene's own detections under their labels.

  hip    IndoorEvaluator: one update per scene (the HeadPrediction route, no host synchronisation) and compute(), HIP events around
         the updates and around compute (its one read-back included)
  numpy  tests/indoor_eval_restated.indoor_eval on the host (float64 geometry in Python loops), wall clock, one process; the core
         count of the machine is reported beside it

Prints one JSON line per route; `--json PATH` also writes them as one JSON list.

    python tools/indoor_eval_timing.py [--scenes 312] [--maps 8] [--reps 5] [--host-scenes 312] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import indoor_eval_restated as R  # noqa: E402
import make_goldens_g15 as g15  # noqa: E402
from mvsdet_amd import ops  # noqa: E402
from mvsdet_amd.evaluation import IndoorEvaluator  # noqa: E402

THR = (0.25, 0.5)


def make_set(dev, n_scenes, n_maps, seed=2100):
    """Per scene a HeadPrediction of one scene and the tuple of head.pad_ground_truth, on the device; the same as host scenes of
    the restatement (bottom-centred rows)."""
    g = np.random.default_rng(seed)
    preds = []
    for m in range(n_maps):
        c, r, k, v, origins = g15.batch_inputs(["random"], [seed + m])
        c, r, k = [t.to(dev) for t in c], [t.to(dev) for t in r], [t.to(dev) for t in k]
        preds.append(ops.head_predict(c, r, k, v.to(dev), origins, 1000, 0.01, 0.25))
    torch.cuda.synchronize()
    device_set, host_set = [], []
    for s in range(n_scenes):
        p = preds[s % n_maps]
        n = int(p.counts[0])
        boxes = p.boxes[0, :n].cpu().numpy()
        labels = p.labels[0, :n].cpu().numpy()
        ng = min(int(g.integers(0, 10)), n)
        src = g.choice(n, ng, replace=False) if ng else np.zeros(0, np.int64)
        gb = boxes[src].copy()
        gb[:, :3] += g.normal(0, 0.1, (ng, 3)).astype(np.float32)
        gb[:, 3:6] *= g.uniform(0.8, 1.25, (ng, 3)).astype(np.float32)
        gl = labels[src].astype(np.int64)
        gt = (torch.from_numpy(gb).to(dev).reshape(1, ng, 6), torch.zeros((1, ng), device=dev),
              torch.from_numpy(gl).to(dev).reshape(1, ng), torch.tensor([ng], dtype=torch.int32, device=dev))
        device_set.append((p, gt))
        bottom = lambda b: np.concatenate([b[:, :2], (b[:, 2] + b[:, 5] * np.float32(-0.5))[:, None], b[:, 3:6],  # noqa: E731
                                           np.zeros((len(b), 1), np.float32)], 1).astype(np.float32)
        host_set.append(dict(boxes=bottom(boxes), scores=p.scores[0, :n].cpu().numpy(), labels=labels, gt_boxes=bottom(gb),
                             gt_labels=gl))
    return device_set, host_set


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=312)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-scenes", type=int, default=312, help="scenes the NumPy restatement is timed on (it is slow)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    device_set, host_set = make_set(dev, args.scenes, args.maps)
    n_det = sum(len(s["scores"]) for s in host_set)
    n_gt = sum(len(s["gt_labels"]) for s in host_set)
    nmax = max(int(p.boxes.shape[1]) for p, _ in device_set)
    ev = IndoorEvaluator(18, THR, capacity=min(nmax * args.scenes, 1 << 20), gt_capacity=max(n_gt, 1), device=dev)
    upd, cmp_, ret = [], [], None
    for rep in range(args.reps + 1):           # the first repeat warms up
        ev.reset()
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        for p, gt in device_set:
            ev.update(p, gt)
        e[1].record()
        ret = ev.compute()
        e[2].record()
        e[2].synchronize()
        if rep:
            upd.append(e[0].elapsed_time(e[1]))
            cmp_.append(e[1].elapsed_time(e[2]))
    rows = [dict(route="hip", scenes=args.scenes, detections=n_det, padded_rows=nmax * args.scenes, gt_boxes=n_gt, reps=args.reps,
                 update_ms_median=round(statistics.median(upd), 3), compute_ms_median=round(statistics.median(cmp_), 3),
                 total_ms_median=round(statistics.median([a + b for a, b in zip(upd, cmp_)]), 3),
                 total_ms_min=round(min(a + b for a, b in zip(upd, cmp_)), 3), mAP_25=ret["mAP_0.25"], mAR_25=ret["mAR_0.25"])]
    print(json.dumps(rows[0]), flush=True)
    if args.host_scenes > 0:
        sub = host_set[:args.host_scenes]
        t0 = time.perf_counter()
        want = R.indoor_eval(sub, THR, {i: str(i) for i in range(18)})
        dt = time.perf_counter() - t0
        row = dict(route="numpy", scenes=len(sub), detections=sum(len(s["scores"]) for s in sub), seconds=round(dt, 3),
                   host_cores=os.cpu_count(), cores_usable=len(os.sched_getaffinity(0)), threads_used=1, mAP_25=want["mAP_0.25"],
                   mAR_25=want["mAR_0.25"])
        if len(sub) == len(host_set):
            row["max_abs_difference_to_hip"] = max(abs(ret[k] - want[k]) for k in want if not np.isnan(want[k]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
