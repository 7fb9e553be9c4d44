"""The ResNet-50 stages at the scene shapes: 40 views of 240x320 and the test pipelines' 80 and 100 views.  Timed in one process on one
GPU, HIP events around `--steps` calls, the routes alternating within every round, after a warm-up of every route at every shape;
median and min - max of the rounds:

  * ResNetStages on csrc/resnet.hip (route "hip": the stem on torch's layers, 52 launches behind it; the folded, split weights are
    kept on the module) and on torch's layers (route "torch": ATen / MIOpen fp32, what a caller runs today -- the yardstick);
  * the stem alone, and each of layer1..layer4 alone on the HIP route;
  * each layer KIND alone by level: the 1x1 of stride 1 and 2 and the 3x3 of stride 1 and 2 at C2..C5 (the level a layer WRITES; a
    stride-2 layer of layerK reads the level below), every launch of that kind and level in one pass, with its multiply-adds, TFLOP/s
    in bf16 operations (three products per multiply-add) and the share of the 2.5 PFLOP/s bf16 matrix peak.

The routes are checked against each other first.  The text goes to --out (default profiles/resnet_timing.txt) and to stdout.

    python tools/resnet_timing.py [--out FILE] [--views 40,80,100] [--rounds N] [--steps N]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvsdet_amd import ops  # noqa: E402
from mvsdet_amd import resnet as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_timing.txt"))
ap.add_argument("--views", default="40,80,100")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()

assert torch.cuda.is_available(), "resnet_timing needs a ROCm device: a CPU run gives no time"
dev = torch.device("cuda:0")
PLANES, DEPTHS, STRIDES, HW = (64, 128, 256, 512), (3, 4, 6, 3), (1, 2, 2, 2), (240, 320)
BF16_PEAK = 2.5e15

gen = torch.Generator().manual_seed(23)
sd = {}


def conv(name, cout, cin, k):
    sd[name + ".weight"] = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (k * k * cin)) ** 0.5


def bn(name, c, gain=1.0):
    sd[name + ".weight"] = (0.5 + torch.rand(c, generator=gen)) * gain
    sd[name + ".bias"] = torch.randn(c, generator=gen) * 0.1
    sd[name + ".running_mean"] = torch.randn(c, generator=gen) * 0.1
    sd[name + ".running_var"] = 0.5 + 1.5 * torch.rand(c, generator=gen)


conv("conv1", 64, 3, 7)
bn("bn1", 64)
c = 64
for li, (p, d) in enumerate(zip(PLANES, DEPTHS)):
    for bi in range(d):
        b = f"layer{li + 1}.{bi}"
        conv(b + ".conv1", p, c, 1), bn(b + ".bn1", p)
        conv(b + ".conv2", p, p, 3), bn(b + ".bn2", p)
        conv(b + ".conv3", 4 * p, p, 1), bn(b + ".bn3", 4 * p, 0.5)
        if bi == 0:
            conv(b + ".downsample.0", 4 * p, c, 1), bn(b + ".downsample.1", 4 * p, 0.5)
        c = 4 * p
net = M.ResNetStages.from_state_dict(sd, prefix="", strides=STRIDES).to(dev).requires_grad_(False)

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def with_route(route, img):
    net.route = route
    return net(img)


def record_launches(stem):
    """One pass of the HIP route with every launch noted: {(kind, level): [closure, ...]}, {(kind, level): multiply-adds} and the
    input of every layer."""
    groups, macs, inputs = {}, {}, []
    real1, real3 = ops.resnet.conv1x1, ops.resnet.conv3x3
    level = [0]

    def note(kind, k, x, cout, stride, call):
        key = (f"{kind} stride {stride}", level[0])
        groups.setdefault(key, []).append(call)
        n, cin, h, w = x.shape
        macs[key] = macs.get(key, 0) + n * ops.resnet.out_size(h, stride) * ops.resnet.out_size(w, stride) * cout * cin * k * k

    def conv1x1(x, wsplit, shift, cout, stride=1, residual=None, relu=True):
        note("1x1", 1, x, cout, stride, lambda: real1(x, wsplit, shift, cout, stride, residual, relu))
        return real1(x, wsplit, shift, cout, stride, residual, relu)

    def conv3x3(x, wsplit, shift, cout, stride=1, relu=True):
        note("3x3", 3, x, cout, stride, lambda: real3(x, wsplit, shift, cout, stride, relu))
        return real3(x, wsplit, shift, cout, stride, relu)

    ops.resnet.conv1x1, ops.resnet.conv3x3 = conv1x1, conv3x3
    try:
        s = stem
        for li, blocks in enumerate(net.layers):
            level[0] = li + 2
            inputs.append(s)
            for b in blocks:
                s = M._block_hip(s, b)
    finally:
        ops.resnet.conv1x1, ops.resnet.conv3x3 = real1, real3
    return groups, macs, inputs


def layer_alone(li, s):
    for b in net.layers[li]:
        s = M._block_hip(s, b)
    return s


with torch.no_grad():
    for n_views in [int(v) for v in args.views.split(",")]:
        img = torch.randn(n_views, 3, *HW, generator=gen).to(dev)
        say(f"=== {n_views} views of {HW[0]}x{HW[1]}: ResNet-50, C2..C5 = " +
            ", ".join(f"{4 * p} x {tuple(t.shape[2:])[0]}x{tuple(t.shape[2:])[1]}" for p, t in zip(PLANES, with_route('hip', img))))
        a, b = with_route("hip", img), with_route("torch", img)
        for i, (x, y) in enumerate(zip(a, b)):
            diff, size = float((x - y).abs().max()), float(y.abs().max())
            say(f"    C{i + 2}: HIP against torch: largest difference {diff:.3g} of {size:.3g}")
            assert diff <= 1e-3 * size, "the two routes disagree"
        del a, b
        stem = net.stem(img)
        groups, macs, inputs = record_launches(stem)
        assert sum(len(v) for v in groups.values()) == 52
        routes = [("HIP route (stem on torch + 52 launches)", lambda: with_route("hip", img)),
                  ("torch route (ATen / MIOpen fp32)", lambda: with_route("torch", img)),
                  ("stem alone (torch, both routes)", lambda: net.stem(img))]
        routes += [(f"layer{li + 1} alone, HIP", (lambda li=li: layer_alone(li, inputs[li]))) for li in range(4)]
        kinds = sorted(groups)
        routes += [(f"{kind} -> C{lvl}: {len(groups[(kind, lvl)])} launches", (lambda k=(kind, lvl): [f() for f in groups[k]]))
                   for kind, lvl in kinds]
        for _, fn in routes:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in routes}
        for _ in range(args.rounds):                       # the routes alternate within a round
            for name, fn in routes:
                ms[name].append(timed(fn, args.steps))
        med = {name: statistics.median(v) for name, v in ms.items()}
        for (name, _), key in zip(routes, [None] * 7 + kinds):
            text = f"    {name:44s} median {med[name]:8.3f} ms   min {min(ms[name]):8.3f}   max {max(ms[name]):8.3f}"
            if key is not None:
                flop = 3 * 2 * macs[key]
                t = med[name] * 1e-3
                text += (f"   {macs[key] / 1e9:7.2f} GMAC  {flop / t / 1e12:6.0f} TFLOP/s bf16 = {100 * flop / t / BF16_PEAK:5.1f} % of peak"
                         f" (fp32-equivalent {2 * macs[key] / t / 1e12:5.0f} TFLOP/s)")
            say(text)
        hip, tor = routes[0][0], routes[1][0]
        spread = max(max(ms[hip]) - min(ms[hip]), max(ms[tor]) - min(ms[tor]))
        say(f"    HIP route / torch route: {med[hip] / med[tor]:.3f}   (torch - HIP = {med[tor] - med[hip]:.3f} ms; the larger min - max "
            f"spread of the two rows is {spread:.3f} ms)")
        layers = sum(med[f"layer{li + 1} alone, HIP"] for li in range(4))
        say(f"    layers 1-4 on HIP: {layers:.3f} ms for {sum(macs.values()) / 1e9:.1f} GMAC = "
            f"{100 * 6 * sum(macs.values()) / (layers * 1e-3) / BF16_PEAK:.1f} % of the bf16 matrix peak")
        del img, stem, groups, inputs, routes
        torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
