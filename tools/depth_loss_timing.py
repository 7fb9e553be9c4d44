"""loss_depth of one scene at the reference-true shape (40 views, ground truth 239x320, the 59x80 crop of a 60x80 depth expectation):
forward + backward of ops.depth.depth_loss beside the reference's own ATen sequence (mvsdet.py:902-913: F.interpolate, `> 0`, two
boolean-mask gathers, abs, mean, and autograd's backward of them) on the same GPU.  HIP events, median and minimum of 7 rounds of 50
steps.  Also counted, for one step of each: device kernels (torch.profiler) and host synchronisations (torch's sync debug mode,
which warns on every blocking call).  The two are checked against each other first.  The text goes to --out
(default profiles/depth_loss_timing.txt) and to stdout.

    python tools/depth_loss_timing.py [--out FILE]
"""
import argparse
import os
import statistics
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvsdet_amd import functional as F_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_loss_timing.txt"))
args = ap.parse_args()

dev = torch.device("cuda:0")
N, Hg, Wg, h, w = 40, 239, 320, 59, 80
gen = torch.Generator(device=dev)
gen.manual_seed(24)
yy, xx = torch.meshgrid(torch.linspace(0, 1, Hg, device=dev), torch.linspace(0, 1, Wg, device=dev), indexing="ij")
gt = (3.5 + 2.0 * torch.sin(3 * xx + torch.arange(N, device=dev).view(N, 1, 1) * 0.3) * torch.cos(2 * yy)).contiguous()
gt[torch.rand(N, Hg, Wg, device=dev, generator=gen) > 0.9] = 0.0        # isolated holes
gt[:, 40:90, 100:180] = 0.0                                            # a blob
full = F.interpolate(gt.unsqueeze(1), size=(60, 80), mode="bilinear").squeeze(1) + 0.3 * torch.randn(N, 60, 80, device=dev, generator=gen)


def hip():
    leaf = full.detach().requires_grad_(True)
    loss = F_.depth_loss_func_new([leaf[:, :h, :w].unsqueeze(1)], [gt])["loss_depth"]
    loss.backward()
    return loss.detach(), leaf.grad


def aten():
    leaf = full.detach().requires_grad_(True)
    cur_est = leaf[:, :h, :w].unsqueeze(1).squeeze(1)
    cur_gt = F.interpolate(gt.unsqueeze(1), size=(h, w), mode="bilinear").squeeze(1)
    tmp_mask = cur_gt > 0
    loss = 0. + torch.mean(torch.abs(cur_est[tmp_mask] - cur_gt[tmp_mask]))
    loss.backward()
    return loss.detach(), leaf.grad


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
    print(text)
    lines.append(text)


(la, ga), (lb, gb) = hip(), aten()
say(f"loss_depth, one scene, {N} views, gt {Hg}x{Wg} -> {h}x{w} (crop of 60x80): HIP {float(la)!r}  ATen {float(lb)!r}; "
    f"gradients differ at {int((ga != gb).sum())} of {ga.numel()} elements")
assert torch.allclose(la, lb, rtol=1e-5, atol=0) and int(((ga != 0) != (gb != 0)).sum()) == 0, "the two disagree"
for name, fn in (("ops.depth.depth_loss forward + backward (HIP)", hip), ("the reference's ATen sequence forward + backward", aten)):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 50)
    syncs = count_syncs(fn)
    n_kernels, names = count_kernels(fn)
    say(f"{name}: median {statistics.median(ms):.4f} ms, min {min(ms):.4f} ms per step; {syncs} host synchronisation(s); "
        f"{n_kernels if n_kernels is not None else '?'} device kernels (autograd's own included)")
    for n in names:
        say(f"    {n[:150]}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
