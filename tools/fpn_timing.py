"""Level 0 of the 2-D feature pyramid at the scene shapes: one scene of 40 views (backbone stages 256 x 60x80, 512 x 30x40, 1024 x 15x20,
2048 x 8x10) and the test pipelines' 80 and 100 views.  Timed in one process on one GPU, HIP events around `--steps` calls, the routes
alternating within every round, after a warm-up of every route at every shape; median and minimum of the rounds:

  * FPNLevel0 on csrc/fpn.hip with the packed output (what `forward_scene_from_stages` runs: the bf16 pieces of the weights are cut
    on every call) and without it, and its five kernels alone on pieces cut beforehand (what keeping the pieces would run);
  * the torch level-0-only chain (five F.conv2d, three F.interpolate) followed by `ops.pack_features`;
  * the torch full four-output FPN (what the reference's `self.neck(x)` runs before `[0]` drops three outputs) followed by
    `ops.pack_features`;
  * `ops.pack_features` alone, and the 3x3 kernel alone.

The torch routes are ATen / MIOpen code, not code of this package: they are the yardstick.  Reported: the ratios of the HIP route
with the packed output to the two torch routes, device kernels per route (torch.profiler), and the 3x3 kernel's share of the bf16
matrix peak: its three bf16 products per multiply-add, 3 x 2 x N H W x 256 x 2304 operations, over its time and 2.5 PFLOP/s.
The routes are checked against each other first.  The text goes to --out (default profiles/fpn_timing.txt) and to stdout.

    python tools/fpn_timing.py [--out FILE] [--views 40,80,100] [--rounds N] [--steps N]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvsdet_amd import ops  # noqa: E402
from mvsdet_amd.fpn import FPNLevel0  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpn_timing.txt"))
ap.add_argument("--views", default="40,80,100")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()

assert torch.cuda.is_available(), "fpn_timing needs a ROCm device: a CPU run gives no time"
dev = torch.device("cuda:0")
CH, COUT, SIZES = (256, 512, 1024, 2048), 256, ((60, 80), (30, 40), (15, 20), (8, 10))
BF16_PEAK = 2.5e15

gen = torch.Generator().manual_seed(17)
sd = {}
for i, c in enumerate(CH):
    sd[f"neck.lateral_convs.{i}.conv.weight"] = torch.randn(COUT, c, 1, 1, generator=gen) / c ** 0.5
    sd[f"neck.lateral_convs.{i}.conv.bias"] = torch.randn(COUT, generator=gen) * 0.1
    sd[f"neck.fpn_convs.{i}.conv.weight"] = torch.randn(COUT, COUT, 3, 3, generator=gen) / (9 * COUT) ** 0.5
    sd[f"neck.fpn_convs.{i}.conv.bias"] = torch.randn(COUT, generator=gen) * 0.1
fpn = FPNLevel0.from_state_dict(sd).to(dev).requires_grad_(False)
pieces = [ops.gemm_split_weight(w.detach().reshape(COUT, -1)) for w in fpn.lateral_weights]
pieces3 = ops.gemm_split_weight(ops.fpn.conv3x3_matrix(fpn.out_weight))
upper = [(sd[f"neck.fpn_convs.{i}.conv.weight"].to(dev), sd[f"neck.fpn_convs.{i}.conv.bias"].to(dev)) for i in (1, 2, 3)]

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def torch_full(stages):
    """The stock module's forward: every lateral, the top-down sums, all four 3x3 output convolutions."""
    lat = [F.conv2d(s, fpn.lateral_weights[i], fpn.lateral_biases[i]) for i, s in enumerate(stages)]
    for i in range(3, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
    outs = [F.conv2d(lat[0], fpn.out_weight, fpn.out_bias, padding=1)]
    outs += [F.conv2d(lat[i], w, b, padding=1) for i, (w, b) in zip((1, 2, 3), upper)]
    return outs


def kernels_only(stages, packed):
    """FPNLevel0.forward_hip on pieces cut beforehand: the four lateral launches and the 3x3 launch."""
    top = None
    for i in range(3, -1, -1):
        top = ops.fpn.lateral(stages[i], pieces[i], fpn.lateral_biases[i], top)
    return ops.fpn.conv3x3(top, pieces3, fpn.out_bias, True, packed)


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


with torch.no_grad():
    for n_views in [int(v) for v in args.views.split(",")]:
        stages = [torch.randn(n_views, c, h, w, generator=gen).to(dev) for c, (h, w) in zip(CH, SIZES)]
        l0 = torch.randn(n_views, COUT, 60, 80, generator=gen).to(dev)
        routes = (
            ("HIP, packed output", lambda: fpn(stages, packed=True)),
            ("HIP, no packed output", lambda: fpn(stages)),
            ("HIP kernels alone, packed output", lambda: kernels_only(stages, True)),
            ("torch level 0 only + pack_features", lambda: ops.pack_features(fpn.forward_torch(stages))),
            ("torch four-output FPN + pack_features", lambda: ops.pack_features(torch_full(stages)[0])),
            ("pack_features alone", lambda: ops.pack_features(l0)),
            ("3x3 kernel alone, both outputs", lambda: ops.fpn.conv3x3(l0, pieces3, fpn.out_bias, True, True)),
        )
        say(f"=== {n_views} views: stages " + ", ".join(f"{c} x {h}x{w}" for c, (h, w) in zip(CH, SIZES)))
        a, pa = fpn(stages, packed=True)
        b = fpn.forward_torch(stages)
        diff, size = float((a - b).abs().max()), float(b.abs().max())
        say(f"    HIP against torch level 0: largest difference {diff:.3g} of {size:.3g}; packed output == pack_features(feature): "
            f"{torch.equal(pa, ops.pack_features(a))}; torch four-output [0] == torch level 0: {torch.equal(torch_full(stages)[0], b)}")
        assert diff <= 1e-4 * size, "the two routes disagree"
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
            say(f"    {name:42s} median {med[name]:7.3f} ms   min {min(ms[name]):7.3f} ms   device kernels {count_kernels(fn)}")
        hip = med["HIP, packed output"]
        say(f"    HIP with packed output / torch level 0 + pack:     {hip / med['torch level 0 only + pack_features']:.3f}")
        say(f"    HIP with packed output / torch four-output + pack: {hip / med['torch four-output FPN + pack_features']:.3f}")
        ops3 = 3 * 2 * n_views * 60 * 80 * COUT * 9 * COUT
        t3 = med["3x3 kernel alone, both outputs"] * 1e-3
        say(f"    3x3 kernel: {ops3 / 1e9:.0f} G bf16 operations (three products per multiply-add) in {t3 * 1e3:.3f} ms = "
            f"{ops3 / t3 / 1e12:.0f} TFLOP/s = {100 * ops3 / t3 / BF16_PEAK:.1f} % of the 2.5 PFLOP/s bf16 matrix peak "
            f"(fp32-equivalent {ops3 / 3 / t3 / 1e12:.0f} TFLOP/s)")
        del stages, l0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
