"""The NVS branch's Gaussian head at the training shape (N = 40 views of 256 channels on 60x80 maps, 6 chosen, cropped to 59x80, one
surface of 84 floats, images 240x320): forward + backward under autograd of `functional.gaussian_head` on csrc/gshead.hip beside the
torch route of MVSDetHotPath.novel_views (fancy index, crop, transposing reshape, cat, ReLU, nn.Linear; with use_rgb_gaussian also
the caller's F.interpolate and transpose), on the same GPU, with and without the rgb columns.  Both end in the same linear loss and
both fill the (N,C,Hf,Wf) feature gradient.  HIP events, the two routes alternating within every round; median and minimum of the
rounds.  Also counted, for one step of each: device kernels (torch.profiler) and host synchronisations (torch's sync debug mode).  The
two are checked against each other first.  The text goes to --out (default profiles/gshead_timing.txt) and to stdout.

    python tools/gshead_timing.py [--out FILE] [--rounds N] [--steps N] [--rgb both|with|without]
"""
import argparse
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvsdet_amd import functional as F_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gshead_timing.txt"))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--rgb", choices=["both", "with", "without"], default="both", help="which of the two layer widths to run (a kernel trace wants one)")
args = ap.parse_args()

dev = torch.device("cuda:0")
N, V, C, Hf, Wf, h, w, S, M = 40, 6, 256, 60, 80, 59, 80, 1, 84
R = h * w
gen = torch.Generator().manual_seed(29)
feature0 = (1.4 * torch.randn(N, C, Hf, Wf, generator=gen)).to(dev)
depth0 = (1.0 + 2.0 * torch.rand(N, 1, h, w, generator=gen)).to(dev)
images = torch.rand(N, 3, 4 * Hf, 4 * Wf, generator=gen).to(dev)
ids = torch.tensor([3, 9, 17, 22, 30, 38])
ids_dev = ids.to(dev)
LOSS_W = torch.randn(V, R, S, M // S, generator=gen).to(dev)
layers = {}
for rgb in (False, True):
    torch.manual_seed(5)
    layers[rgb] = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(C + (4 if rgb else 1), M)).to(dev)


def leaves_of(rgb):
    feature, depth = feature0.detach().requires_grad_(True), depth0.detach().requires_grad_(True)
    for p in layers[rgb].parameters():
        p.grad = None
    return feature, depth


def finish(raw, feature, depth, rgb):
    (raw * LOSS_W).sum().backward()
    return raw.detach(), [feature.grad, depth.grad, layers[rgb][1].weight.grad, layers[rgb][1].bias.grad]


def hip(rgb):
    feature, depth = leaves_of(rgb)
    lin = layers[rgb][1]
    raw = F_.gaussian_head(feature, depth, lin.weight, lin.bias, ids_dev, h, w, S, denorm_images=images if rgb else None)
    return finish(raw, feature, depth, rgb)


def torch_route(rgb):
    feature, depth = leaves_of(rgb)
    rows = [feature[ids_dev][:, :, :h, :w].reshape(V, C, R).transpose(1, 2), depth[ids_dev].reshape(V, R, 1)]   # hotpath.novel_views
    if rgb:                                                                                                    # mvsdet.py:319-333
        new_rgb = torch.nn.functional.interpolate(images[ids_dev], scale_factor=0.25, mode="bilinear")[:, :, :h, :w]
        rows.append(new_rgb.reshape(V, 3, -1).transpose(2, 1))
    raw = layers[rgb](torch.cat(rows, dim=-1))
    return finish(raw.reshape(V, R, S, M // S), feature, depth, rgb)


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        return len(names), names
    except Exception as exc:   # a build without device tracing: report that, time anyway
        return None, [f"not counted: {type(exc).__name__}: {exc}"]


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return sum("synchroniz" in str(x.message) for x in seen)


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


say(f"{N} views of {C} channels on {Hf}x{Wf}, {V} chosen, cropped to {h}x{w}: {V * R} rows; {S} surface(s), M = {M}; images {4 * Hf}x{4 * Wf}")
say(f"the row matrix the torch route writes and reads: {V * R * (C + 4) * 4 / 1e6:.1f} MB with rgb")
for rgb in [r for r in (False, True) if args.rgb in ("both", "with" if r else "without")]:
    say(f"--- {'with' if rgb else 'without'} the rgb columns (K = {C + (4 if rgb else 1)})")
    routes = (("functional.gaussian_head forward + backward (HIP)", lambda: hip(rgb)), ("the torch route forward + backward", lambda: torch_route(rgb)))
    (oa, ga), (ob, gb) = routes[0][1](), routes[1][1]()
    say(f"    raw: HIP against the torch route, largest difference {float((oa - ob).abs().max()):.3g} of {float(ob.abs().max()):.3g}")
    for n, a, b in zip(("feature", "depth_coding", "weight", "bias"), ga, gb):
        say(f"    d {n}: largest difference {float((a - b).abs().max()):.3g} of {float(b.abs().max()):.3g}")
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()), "the two disagree"
    for _, fn in routes:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in routes}
    for _ in range(args.rounds):                       # the two alternate within a round
        for name, fn in routes:
            ms[name].append(timed(fn, args.steps))
    for name, fn in routes:
        syncs = count_syncs(fn)
        n_kernels, names = count_kernels(fn)
        say(f"{name}: median {statistics.median(ms[name]):.3f} ms, min {min(ms[name]):.3f} ms per step over {args.rounds} rounds of {args.steps}; "
            f"{syncs} host synchronisation(s); {n_kernels if n_kernels is not None else '?'} device kernels (the loss's and autograd's own included)")
        ours = [n for n in names if "gshead" in n]
        if ours:
            say(f"    of these the head's own: {len(ours)}")
            for n in ours:
                say(f"        {n[:150]}")
        elif n_kernels is None:
            say(f"    {names[0]}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
