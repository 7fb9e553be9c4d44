"""A training step of level 0 of the 2-D feature pyramid at the scene shapes of tools/fpn_timing.py (40 / 80 / 100 views of 256 x 60x80,
512 x 30x40, 1024 x 15x20, 2048 x 8x10): forward + backward of sum(out * R) with all four stages and all ten parameters requiring
grad, on the HIP autograd route (`FPNLevel0(autograd_route="hip")`: csrc/fpn.hip forward, csrc/fpn_bwd.hip backward) and on the torch
route (five F.conv2d and three F.interpolate under ATen's autograd: ATen / MIOpen fp32, the yardstick, not code of this package).

One process, one GPU, HIP events around `--steps` steps, the two routes alternating within every round after a warm-up of both;
median and minimum of the rounds.  Reported besides: device kernels per route (torch.profiler), and the weight-gradient kernel of the
3x3 convolution alone with its share of the 2.5 PFLOP/s bf16 matrix peak -- three bf16 products per multiply-add,
3 x 2 x N H W x 256 x 2304 operations.  The routes' gradients are checked against each other first.  Without a device the run fails.
The text goes to --out (default profiles/fpn_train_timing.txt) and to stdout.

    python tools/fpn_train_timing.py [--out FILE] [--views 40,80,100] [--rounds N] [--steps N]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvsdet_amd import ops  # noqa: E402
from mvsdet_amd.fpn import FPNLevel0  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpn_train_timing.txt"))
ap.add_argument("--views", default="40,80,100")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
args = ap.parse_args()

assert torch.cuda.is_available(), "fpn_train_timing needs a ROCm device: a CPU run gives no time"
dev = torch.device("cuda:0")
CH, COUT, SIZES = (256, 512, 1024, 2048), 256, ((60, 80), (30, 40), (15, 20), (8, 10))
BF16_PEAK = 2.5e15

gen = torch.Generator().manual_seed(17)
sd = {}
for i, c in enumerate(CH):
    sd[f"neck.lateral_convs.{i}.conv.weight"] = torch.randn(COUT, c, 1, 1, generator=gen) / c ** 0.5
    sd[f"neck.lateral_convs.{i}.conv.bias"] = torch.randn(COUT, generator=gen) * 0.1
sd["neck.fpn_convs.0.conv.weight"] = torch.randn(COUT, COUT, 3, 3, generator=gen) / (9 * COUT) ** 0.5
sd["neck.fpn_convs.0.conv.bias"] = torch.randn(COUT, generator=gen) * 0.1
hip = FPNLevel0.from_state_dict(sd, route="hip", autograd_route="hip").to(dev)
ref = FPNLevel0.from_state_dict(sd, route="torch").to(dev)

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def step(module, stages, r):
    """One training step's worth of the pyramid: forward, backward of sum(out * r) into .grad of the stages and the parameters."""
    for t in stages + list(module.parameters()):
        t.grad = None
    (module(stages) * r).sum().backward()


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(str(getattr(e, "device_type", "")).endswith("CUDA") for e in prof.events())
    except Exception as exc:   # a build without device tracing: report that, time anyway
        return f"not counted ({type(exc).__name__})"


for n_views in [int(v) for v in args.views.split(",")]:
    stages = [torch.randn(n_views, c, h, w, generator=gen).to(dev).requires_grad_(True) for c, (h, w) in zip(CH, SIZES)]
    r = torch.randn(n_views, COUT, 60, 80, generator=gen).to(dev)
    l0 = torch.randn(n_views, COUT, 60, 80, generator=gen).to(dev)
    say(f"=== {n_views} views: stages " + ", ".join(f"{c} x {h}x{w}" for c, (h, w) in zip(CH, SIZES)))
    # the two routes against each other: every gradient within 1e-4 of the largest gradient of its tensor
    step(ref, stages, r)
    want = [s.grad.clone() for s in stages] + [p.grad.clone() for p in ref.parameters()]
    step(hip, stages, r)
    got = [s.grad.clone() for s in stages] + [p.grad.clone() for p in hip.parameters()]
    worst = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(got, want))
    say(f"    HIP against torch, 4 stage and 10 parameter gradients: largest difference {worst:.3g} of the tensor's largest gradient")
    assert worst <= 1e-4, "the two routes disagree"
    del want, got
    routes = (
        ("HIP forward + backward", lambda: step(hip, stages, r)),
        ("torch forward + backward", lambda: step(ref, stages, r)),
        ("3x3 weight gradient alone", lambda: ops.fpn.weight_grad(r, l0, 9)),
        ("lateral 0 weight gradient alone", lambda: ops.fpn.weight_grad(r, stages[0].detach(), 1)),
    )
    for _, fn in routes:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in routes}
    for _ in range(args.rounds):                       # the routes alternate within a round
        for name, fn in routes:
            ms[name].append(timed(fn, args.steps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, fn in routes:
        say(f"    {name:34s} median {med[name]:7.3f} ms   min {min(ms[name]):7.3f} ms   max {max(ms[name]):7.3f} ms   "
            f"device kernels {count_kernels(fn)}")
    say(f"    HIP / torch, forward + backward: {med['HIP forward + backward'] / med['torch forward + backward']:.3f}")
    ops3 = 3 * 2 * n_views * 60 * 80 * COUT * 9 * COUT
    t3 = med["3x3 weight gradient alone"] * 1e-3
    say(f"    3x3 weight gradient (kernel and its split sum): {ops3 / 1e9:.0f} G bf16 operations (three products per multiply-add) in "
        f"{t3 * 1e3:.3f} ms = {ops3 / t3 / 1e12:.0f} TFLOP/s = {100 * ops3 / t3 / BF16_PEAK:.1f} % of the 2.5 PFLOP/s bf16 matrix peak "
        f"(fp32-equivalent {ops3 / 3 / t3 / 1e12:.0f} TFLOP/s)")
    del stages, r, l0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
