"""Per-scene time of the ARKit head's post-processing on the GPU (csrc/detect.hip's rotated route), on planted rotated objects and
random head maps: the G16 generators (tests/golden/make_goldens_g16.py; 40x40x16 / 20x20x8 / 10x10x4 levels, 17 classes, 7
regression channels, nms_pre 1000, score_thr .01, iou_thr .25) at the fixture's seeds, and a denser random map (`dense`: class
logits 2.5 higher, some 17 x 1000 (point, class) pairs above score_thr).

NerfDetHeadConvs(arkit_head=True).predict_by_feat: seven launches and the one count read-back.  HIP events around each call, a
device synchronise inside it; warm-up calls first.  Prints one JSON line per input with the (point, class) pairs above score_thr,
the kept boxes and the median, min and max over the repeats; `--json PATH` also writes them as one JSON list.

    python tools/detect_arkit_timing.py [--reps 30] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(ROOT))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "tests", "golden"))

import make_goldens_g16 as g16  # noqa: E402
from detect_timing import time_calls  # noqa: E402
from mvsdet_amd import ops  # noqa: E402
from mvsdet_amd.head import NerfDetHeadConvs  # noqa: E402

CFG = types.SimpleNamespace(nms_pre=1000, score_thr=0.01, iou_thr=0.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    head = NerfDetHeadConvs(17, 3, 128, 7, arkit_head=True, test_cfg=CFG)
    rows = []
    for name, kind, seed, shift in (("planted", "planted", 1600, 0.0), ("random", "random", 1743, 0.0),
                                    ("dense", "random", 1743, 2.5)):
        c, r, k, v, origins = g16.batch_inputs([kind], [seed])
        c, r, k, v = [t.to(dev) for t in c], [t.to(dev) for t in r], [(t + shift).to(dev) for t in k], v.to(dev)
        metas = [{"lidar2img": {"origin": origins[0].numpy()}}]
        pairs = 0
        for lvl, size in enumerate(g16.LEVELS):
            vm = torch.nn.Upsample(size=size, mode="trilinear")(v).round().bool()[0]
            s = (k[lvl][0].sigmoid() * c[lvl][0].sigmoid() * vm).reshape(17, -1)
            if s.shape[1] > CFG.nms_pre:
                s = s[:, s.max(0).values.topk(CFG.nms_pre).indices]
            pairs += int((s > CFG.score_thr).sum())
        kept = {}

        def hip():
            kept["n"] = len(head.predict_by_feat(c, r, k, v, metas)[0])

        ms = time_calls(hip, args.reps, 5)
        row = dict(route="hip", input=name, pairs_above_score_thr=pairs, kept=kept["n"], reps=args.reps,
                   ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
    # the standalone nms3d on one class of 2 400 random boxes at a constant density (4 m x 4 m per 64 boxes)
    g = torch.Generator().manual_seed(0)
    n = 2400
    spread = 4.0 * (n / 64) ** 0.5
    b = torch.cat([torch.rand(n, 2, generator=g) * spread, torch.rand(n, 1, generator=g), 0.2 + torch.rand(n, 3, generator=g),
                   8 * torch.rand(n, 1, generator=g) - 4], 1).to(dev)
    s = torch.rand(n, generator=g).to(dev)
    kept = {}

    def nms():
        kept["n"] = len(ops.nms3d(b, s, 0.25))

    ms = time_calls(nms, args.reps, 5)
    row = dict(route="nms3d", input=f"{n} boxes", kept=kept["n"], reps=args.reps, ms_median=round(statistics.median(ms), 4),
               ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))
    print(json.dumps(row), flush=True)
    rows.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
