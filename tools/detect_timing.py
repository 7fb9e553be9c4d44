"""Per-scene time of the ScanNet head's post-processing on the GPU, on planted-object and random head maps (the G15 generators,
tests/golden/make_goldens_g15.py; 40x40x16 / 20x20x8 / 10x10x4 levels, 18 classes, nms_pre 1000, score_thr .01, iou_thr .25):

  hip   NerfDetHeadConvs.predict_by_feat on csrc/detect.hip (four launches, the one count read-back included)
  aten  the same predict written as ATen operations and the greedy Python loop of aligned_3d_nms (our restatement of
        nerfdet_head.py:301-420, 564-628), on the GPU

HIP events around each call, a device synchronise inside it; warm-up calls first.  Prints one JSON line per (route, input) with the
median, min and max over the repeats; `--json PATH` also writes them as one JSON list.

    python tools/detect_timing.py [--reps 30] [--aten-reps 5] [--only hip] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_goldens_g15 as g15  # noqa: E402
from mvsdet_amd.head import NerfDetHeadConvs  # noqa: E402

CFG = types.SimpleNamespace(nms_pre=1000, score_thr=0.01, iou_thr=0.25)


def aten_predict(center_preds, bbox_preds, cls_preds, valid_pred, origin, cfg):
    """One scene as ATen ops: upsampled valid mask, scores, per-level top-k, decode, score filter, greedy NMS loop, conversion."""
    boxes, scores = [], []
    for lvl, (c, r, k) in enumerate(zip(center_preds, bbox_preds, cls_preds)):
        size = c.shape[-3:]
        vm = torch.nn.functional.interpolate(valid_pred, size=size, mode="trilinear").round().bool()[0]
        n = torch.tensor(size)
        vs = torch.tensor(g15.VOXEL) * (2 ** lvl)
        grid = torch.stack(torch.meshgrid([torch.arange(s) for s in size], indexing="ij"))
        pts = (grid * vs.view(3, 1, 1, 1) + (origin - n / 2. * vs).view(3, 1, 1, 1)).reshape(3, -1).t().to(c.device)
        sc = (k[0].sigmoid() * c[0].sigmoid() * vm).reshape(k.shape[1], -1).t()
        reg = r[0].reshape(6, -1).t()
        if sc.shape[0] > cfg.nms_pre > 0:
            ids = sc.max(1).values.topk(cfg.nms_pre).indices
            sc, reg, pts = sc[ids], reg[ids], pts[ids]
        boxes.append(torch.stack([pts[:, 0] - reg[:, 0], pts[:, 1] - reg[:, 2], pts[:, 2] - reg[:, 4],
                                  pts[:, 0] + reg[:, 1], pts[:, 1] + reg[:, 3], pts[:, 2] + reg[:, 5]], -1))
        scores.append(sc)
    b, s = torch.cat(boxes), torch.cat(scores)
    s, lab = s.max(1)
    keep = s > cfg.score_thr
    b, s, lab = b[keep], s[keep], lab[keep]
    lo, hi = b[:, :3], b[:, 3:]
    area = (hi - lo).prod(1)
    order = torch.argsort(s)
    picks = []
    zero = b.new_zeros(1)
    while order.shape[0]:
        i, rest = order[-1], order[:-1]
        picks.append(i)
        ext = torch.max(zero, torch.min(hi[i], hi[rest]) - torch.max(lo[i], lo[rest]))
        inter = ext[:, 0] * ext[:, 1] * ext[:, 2]
        iou = inter / (area[i] + area[rest] - inter) * (lab[i] == lab[rest]).float()
        order = rest[torch.nonzero(iou <= cfg.iou_thr).flatten()]
    ids = b.new_tensor(picks, dtype=torch.long)
    b = b[ids]
    return torch.cat([(b[:, :3] + b[:, 3:]) / 2., b[:, 3:] - b[:, :3]], 1), s[ids], lab[ids]


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
    ap.add_argument("--aten-reps", type=int, default=5)
    ap.add_argument("--only", choices=["hip", "aten"], default=None)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    head = NerfDetHeadConvs(test_cfg=CFG)
    rows = []
    for kind, seed in (("planted", 1507), ("random", 1517)):
        c, r, k, v, origins = g15.batch_inputs([kind], [seed])
        c, r, k, v = [t.to(dev) for t in c], [t.to(dev) for t in r], [t.to(dev) for t in k], v.to(dev)
        metas = [{"lidar2img": {"origin": origins[0].numpy()}}]
        kept = {}

        def hip():
            kept["hip"] = len(head.predict_by_feat(c, r, k, v, metas)[0])

        def aten():
            kept["aten"] = len(aten_predict(c, r, k, v, origins[0], CFG)[1])
            torch.cuda.synchronize()

        for route, fn, reps, warm in (("hip", hip, args.reps, 5), ("aten", aten, args.aten_reps, 1)):
            if args.only and route != args.only:
                continue
            ms = time_calls(fn, reps, warm)
            row = dict(route=route, input=kind, kept=kept[route], reps=reps, ms_median=round(statistics.median(ms), 4),
                       ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
