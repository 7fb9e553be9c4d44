"""A training step of the ResNet-50 stages at the scene shapes (40 / 80 / 100 views of 240x320) after `freeze_(1)` -- the shipped
configs' frozen_stages=1, norm_eval=True, BatchNorm requires_grad=False: layers 2-4 train -- forward + backward of sum_k sum(C_k * R_k),
on the HIP autograd route (`ResNetStages(autograd_route="hip")`: csrc/resnet.hip forward, csrc/resnet_bwd.hip backward) and on the torch
route (F.conv2d under ATen's autograd: ATen / MIOpen fp32, the yardstick, not code of this package).

One process, one GPU, HIP events around `--steps` steps, the two routes alternating within every round after a warm-up of both;
median with min - max of the rounds.  Reported besides: device kernels and host synchronisations of one step per route
(torch.profiler), and each new kernel kind alone at every shipped shape it runs at (layers 2-4), all launches of a kind in one pass,
through its C entry alone (weights cut, outputs and workspaces allocated outside the timed call), with its multiply-adds and its
share of the 2.5 PFLOP/s bf16 matrix peak (three bf16 products per multiply-add).  The routes'
gradients are checked against each other first.  Without a device the run fails.  The text goes to --out (default
profiles/resnet_train_timing.txt) and to stdout.

    python tools/resnet_train_timing.py [--out FILE] [--views 40,80,100] [--rounds N] [--steps N]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvsdet_amd import _lib, ops  # noqa: E402
from mvsdet_amd import resnet as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_train_timing.txt"))
ap.add_argument("--views", default="40,80,100")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "resnet_train_timing needs a ROCm device: a CPU run gives no time"
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
hip = M.ResNetStages.from_state_dict(sd, prefix="", strides=STRIDES, route="hip", autograd_route="hip").to(dev).freeze_(1)
ref = M.ResNetStages.from_state_dict(sd, prefix="", strides=STRIDES, route="torch").to(dev).freeze_(1)

lines = []
bytes_moved = [0]   # of the elementwise gate launches of one step


def say(text):
    print(text, flush=True)
    lines.append(text)


def trained(module):
    return [p for p in module.parameters() if p.requires_grad]


def step(module, img, rs):
    """One training step's worth of the backbone: forward, backward of sum_k sum(C_k * R_k) into .grad of the trained weights."""
    for p in trained(module):
        p.grad = None
    sum((c * r).sum() for c, r in zip(module(img), rs)).backward()


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def count_events(fn):
    """(device kernels, host synchronisations and device-to-host copies) of one call."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        events = prof.events()
        kernels = sum(str(getattr(e, "device_type", "")).endswith("CUDA") for e in events)
        syncs = sum(("ynchronize" in e.name or "DtoH" in e.name or "_local_scalar_dense" in e.name) for e in events) - 1   # ours, above
        return kernels, syncs
    except ImportError as exc:   # a torch without its profiler: report that, time anyway; any other failure is an error
        return f"not counted ({type(exc).__name__})", "not counted"


def record_backward(img, rs):
    """One HIP step with every gradient launch noted: {kind: [closure, ...]} and {kind: multiply-adds}."""
    groups, macs = {}, {}
    R = ops.resnet
    lib = _lib.load()

    def stream():
        return _lib.current_stream(dev)
    real = {n: getattr(R, n) for n in ("conv1x1_input_grad", "conv3x3_input_grad", "weight_grad", "relu_gate")}

    def note(kind, n_macs, call):
        groups.setdefault(kind, []).append(call)
        macs[kind] = macs.get(kind, 0) + n_macs

    # Every closure calls the C entry ALONE: the weight pieces are cut, the outputs and the workspaces allocated here, once, outside
    # the timed call.  What a step pays besides (the cuts, the allocations, the products that scale the rows of dW) is in the step's
    # row and in "everything else of the backward" below.
    def conv1x1_input_grad(g, weight, scale, gate=None, residual=None, spread=1):
        n, k, h, w = g.shape
        c = int(weight.shape[1])
        g, wq, out = g.contiguous(), ops.gemm_split_weight(R.transposed_matrix(weight, scale)), torch.empty((n, c, h, w), device=dev)
        res, gt = (None if residual is None else residual.contiguous()), (None if gate is None else gate.contiguous())
        note("1x1 input gradient", n * h * w * k * c, lambda: _lib.check(lib.mvsdet_resnet_conv1x1_dx_bf16x3(
            _lib.ptr(g), _lib.ptr(wq), _lib.ptr(res), _lib.ptr(gt), _lib.ptr(out), n, c, k, h, w, int(spread), stream()), "dx1x1"))
        return real["conv1x1_input_grad"](g, weight, scale, gate, residual, spread)

    def conv3x3_input_grad(g, weight, scale, size, stride=1, gate=None):
        n, k, ho, wo = g.shape
        c, h, w = int(weight.shape[1]), int(size[0]), int(size[1])
        mats = [R.flipped_matrix(weight, scale)] if stride == 1 else R.class_matrices(weight, scale)
        g, wq, out = g.contiguous(), torch.cat([ops.gemm_split_weight(m) for m in mats]), torch.empty((n, c, h, w), device=dev)
        gt = None if gate is None else gate.contiguous()
        # the real multiply-adds: every output pixel's nine taps (9 Ho Wo = about 2.25 H W at stride 2)
        note(f"3x3 input gradient, stride {stride}", n * ho * wo * 9 * k * c, lambda: _lib.check(lib.mvsdet_resnet_conv3x3_dx_bf16x3(
            _lib.ptr(g), _lib.ptr(wq), _lib.ptr(gt), _lib.ptr(out), n, c, k, h, w, int(stride), stream()), "dx3x3"))
        return real["conv3x3_input_grad"](g, weight, scale, size, stride, gate)

    def weight_grad(gy, x, taps, stride=1):
        n, k, ho, wo = gy.shape
        c, h, w = int(x.shape[1]), int(x.shape[2]), int(x.shape[3])
        kind = f"weight gradient, {taps} tap{'s' if taps > 1 else ''}, stride {stride}" + (" (4.21's kernel)" if stride == 1 else "")
        sizes, entry = ((lib.mvsdet_fpn_dw_workspace_bytes, lib.mvsdet_fpn_dw_bf16x3) if stride == 1 else
                        (lib.mvsdet_resnet_dw_s2_workspace_bytes, lib.mvsdet_resnet_dw_s2_bf16x3))
        nbytes = sizes(taps, n, c, k, h, w)
        gy, x = gy.contiguous(), x.contiguous()
        dw, ws = torch.empty((k, c, 3 if taps == 9 else 1, 3 if taps == 9 else 1), device=dev), torch.empty(nbytes // 4, device=dev)
        note(kind, n * ho * wo * taps * k * c, lambda: _lib.check(entry(_lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(ws), nbytes, taps, n, c, k,
                                                                        h, w, stream()), "dw"))
        return real["weight_grad"](gy, x, taps, stride)

    def relu_gate(g, y):
        g, y = g.contiguous(), y.contiguous()
        out = torch.empty_like(g)
        note("relu gate (elementwise)", 0, lambda: _lib.check(lib.mvsdet_resnet_relu_gate_f32(_lib.ptr(g), _lib.ptr(y), _lib.ptr(out), g.numel(),
                                                                                             stream()), "gate"))
        bytes_moved[0] += 12 * g.numel()
        return real["relu_gate"](g, y)

    wrapped = dict(conv1x1_input_grad=conv1x1_input_grad, conv3x3_input_grad=conv3x3_input_grad, weight_grad=weight_grad, relu_gate=relu_gate)
    for n, f in wrapped.items():
        setattr(R, n, f)
    try:
        step(hip, img, rs)
    finally:
        for n, f in real.items():
            setattr(R, n, f)
    return groups, macs


for n_views in [int(v) for v in args.views.split(",")]:
    img = torch.randn(n_views, 3, *HW, generator=gen).to(dev)
    with torch.no_grad():
        shapes = [tuple(t.shape) for t in hip(img)]
    rs = [torch.randn(*s, generator=gen).to(dev) for s in shapes]
    say(f"=== {n_views} views of {HW[0]}x{HW[1]}: ResNet-50 after freeze_(1), {len(trained(hip))} trained weights, C2..C5 = " +
        ", ".join(f"{s[1]} x {s[2]}x{s[3]}" for s in shapes))
    # The two routes against each other, as a sanity check only.  Their forwards differ in the last bits, so a few pre-activations near
    # zero fall on different sides of the ReLU ("flips", counted below at the stage outputs); a flipped gate moves one pixel's whole
    # contribution, which on the 8x10 maps of layer 4 is a visible part of one entry.  Hence the L2 norm per tensor here; the exact
    # comparison, with the gates imposed, is tests/test_gpu_resnet_grad.py's.
    step(ref, img, rs)
    want = [p.grad.clone() for p in trained(ref)]
    step(hip, img, rs)
    got = [p.grad.clone() for p in trained(hip)]
    with torch.no_grad():
        flips = [int(((x > 0) != (y > 0)).sum()) for x, y in zip(hip(img), ref(img))]
    worst = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(got, want))
    worst2 = max(float((a - b).norm()) / float(b.norm()) for a, b in zip(got, want))
    say(f"    HIP against torch, {len(got)} weight gradients: largest |difference| {worst:.3g} of the tensor's largest gradient, largest L2 "
        f"difference {worst2:.3g} of the tensor's L2 norm; ReLU flips between the routes' forwards at C2..C5: {flips}")
    assert worst2 <= 2e-2, "the two routes disagree"
    del want, got
    bytes_moved[0] = 0
    groups, macs = record_backward(img, rs)
    kinds = sorted(groups)
    routes = [("HIP forward + backward", lambda: step(hip, img, rs)), ("torch forward + backward", lambda: step(ref, img, rs)),
              ("HIP forward alone (no_grad)", lambda: _no_grad(hip, img)), ("torch forward alone (no_grad)", lambda: _no_grad(ref, img))]

    def _no_grad(module, x):
        with torch.no_grad():
            return module(x)

    routes += [(f"{kind}: {len(groups[kind])} calls", (lambda k=kind: [f() for f in groups[k]])) for kind in kinds]
    for _, fn in routes:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in routes}
    for _ in range(args.rounds):                       # the routes alternate within a round
        for name, fn in routes:
            ms[name].append(timed(fn, args.steps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    for (name, fn), key in zip(routes, [None] * 4 + kinds):
        text = f"    {name:58s} median {med[name]:8.3f} ms   min {min(ms[name]):8.3f}   max {max(ms[name]):8.3f}"
        if key is None:
            kernels, syncs = count_events(fn)
            text += f"   device kernels {kernels}, host synchronisations {syncs}"
        elif macs[key]:
            flop, t = 3 * 2 * macs[key], med[name] * 1e-3
            text += f"   {macs[key] / 1e9:8.2f} GMAC  {flop / t / 1e12:6.0f} TFLOP/s bf16 = {100 * flop / t / BF16_PEAK:5.1f} % of peak"
        else:
            text += f"   {bytes_moved[0] / 1e9:8.2f} GB read + written = {bytes_moved[0] / (med[name] * 1e-3) / 1e12:5.2f} TB/s"
        say(text)
    h, t = routes[0][0], routes[1][0]
    spread = max(max(ms[h]) - min(ms[h]), max(ms[t]) - min(ms[t]))
    say(f"    HIP / torch, forward + backward: {med[h] / med[t]:.3f}   (torch - HIP = {med[t] - med[h]:.3f} ms; the larger min - max spread "
        f"of the two rows is {spread:.3f} ms; ratio of the minima {min(ms[h]) / min(ms[t]):.3f}, of the maxima {max(ms[h]) / max(ms[t]):.3f})")
    bwd = med[h] - med[routes[2][0]]
    alone = sum(med[name] for name, _ in routes[4:])
    say(f"    backward alone (step - forward alone): HIP {bwd:.3f} ms, torch {med[t] - med[routes[3][0]]:.3f} ms")
    say(f"    the HIP backward's gradient kernels alone sum to {alone:.3f} ms; everything else of the backward (the per-call cuts of the "
        f"transposed weights, allocations, the products that scale the rows of dW, autograd's sums, launch gaps): {bwd - alone:.3f} ms")
    del img, rs, groups, routes
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
