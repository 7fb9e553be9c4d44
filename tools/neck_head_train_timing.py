"""One training step (forward + backward) of the 3-D neck and the detection head at the shipped shape (1,256,40,40,16), on the two
routes of `autograd_route` ("aten": the framework's layers / MIOpen; "hip": our kernels), alternated in one process and timed with
device events after warm-up.

    python tools/neck_head_train_timing.py [--steps 10] [--warmup 3] [--routes aten,hip] [--json out.json]

For the per-layer breakdown run one route alone under the kernel tracer:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/neck_head_train_timing.py --routes hip --steps 3 --warmup 1
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mvsdet_amd.head import NerfDetHeadConvs  # noqa: E402
from mvsdet_amd.neck import IndoorImVoxelNeck  # noqa: E402


def build(route, dev):
    torch.manual_seed(0)
    neck = IndoorImVoxelNeck(256, 128, [1, 1, 1]).train().to(dev)
    head = NerfDetHeadConvs(18, 3, 128, 6).train().to(dev)
    head.init_weights()
    neck.autograd_route = head.autograd_route = route
    return neck, head


def step(neck, head, x, rs):
    centers, regs, clss = head(neck(x))
    loss = sum((t * r).sum() for ts, rr in zip(zip(centers, regs, clss), rs) for t, r in zip(ts, rr))
    loss.backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--routes", default="aten,hip")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    routes = a.routes.split(",")
    g = torch.Generator().manual_seed(1)
    x = (torch.rand((1, 256, 40, 40, 16), generator=g) * (torch.rand((1, 1, 40, 40, 16), generator=g) > 0.6)).to(dev)
    x.requires_grad_(True)
    models = {r: build(r, dev) for r in routes}
    rs = [[torch.randn((1, c, 40 >> i, 40 >> i, 16 >> i), generator=g).to(dev) for c in (1, 6, 18)] for i in range(3)]
    for _ in range(a.warmup):
        for r in routes:
            step(*models[r], x, rs)
    torch.cuda.synchronize()
    times = {r: [] for r in routes}
    for _ in range(a.steps):
        for r in routes:            # alternated: the routes see the same clocks and the same neighbours
            for p in list(models[r][0].parameters()) + list(models[r][1].parameters()) + [x]:
                p.grad = None
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            step(*models[r], x, rs)
            t1.record()
            t1.synchronize()
            times[r].append(t0.elapsed_time(t1))
    res = {r: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for r, v in times.items()}
    if "aten" in res and "hip" in res:
        res["speedup"] = res["aten"]["median_ms"] / res["hip"]["median_ms"]
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
