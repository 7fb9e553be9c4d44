"""loss_pc of one scene at the reference-true shape (40 views, 10 chosen, 240x320 images, the 59x80 crop of a 60x80 depth expectation):
forward + backward under autograd of functional.warp_img + functional.photometric_loss on csrc/photoloss.hip beside the project's own
ATen restatement of the reference's sequence (functional._warp_img_host / _photometric_loss_host: torch.inverse, the gathers, about
sixty small launches, and autograd's backward of them) on the same GPU.  Both include the one F.interpolate of the images.  HIP
events, median and minimum of 7 rounds of 50 steps.  Also counted, for one step of each: device kernels (torch.profiler) and host
synchronisations (torch's sync debug mode, which warns on every blocking call).  The two are checked against each other first.
The text goes to --out (default profiles/photo_loss_timing.txt) and to stdout.

    python tools/photo_loss_timing.py [--out FILE]
"""
import argparse
import math
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_loss_timing.txt"))
args = ap.parse_args()

dev = torch.device("cuda:0")
N, B, Hi, Wi, h, w = 40, 10, 240, 320, 59, 80
gen = torch.Generator(device=dev)
gen.manual_seed(25)
yy, xx = torch.meshgrid(torch.linspace(0, 1, Hi, device=dev), torch.linspace(0, 1, Wi, device=dev), indexing="ij")
phase = torch.arange(N, device=dev).view(N, 1, 1, 1) * 0.05 + torch.arange(3, device=dev).view(1, 3, 1, 1)
images = (0.5 + 0.3 * torch.sin(9 * xx + phase) * torch.cos(7 * yy + phase) + 0.05 * torch.rand(N, 3, Hi, Wi, device=dev, generator=gen)).contiguous()
w2c = torch.eye(4).repeat(N, 1, 1)
for i in range(N):                                   # a camera path: a few degrees and centimetres between neighbours
    a = 0.03 * i
    w2c[i, :3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]) @ \
        torch.tensor([[1, 0, 0], [0, math.cos(0.01 * i), -math.sin(0.01 * i)], [0, math.sin(0.01 * i), math.cos(0.01 * i)]])
    w2c[i, :3, 3] = torch.tensor([0.05 * i, 0.01 * (i % 3), 0.02 * (i % 5)])
w2c = w2c.to(dev)
K = torch.tensor([[68.0, 0, 39.8, 0], [0, 68.0, 29.3, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device=dev)
nbr = torch.stack([(torch.arange(N) + 1) % N, (torch.arange(N) + 2) % N], dim=1).to(dev)
full = (2.5 + 0.5 * torch.sin(3 * xx[:60 * 4:4, :80 * 4:4] + torch.arange(N, device=dev).view(N, 1, 1) * 0.2)).unsqueeze(1).contiguous()
ref_id = torch.randperm(N, generator=torch.Generator().manual_seed(25))[:B].to(dev)


def hip():
    leaf = full.detach().requires_grad_(True)
    warped, mask, chosen = F_.warp_img(images, nbr, w2c, K, leaf[:, :, :h, :w], ref_id=ref_id)
    loss = F_.photometric_loss([warped], [mask], [chosen])["loss_pc"]
    loss.backward()
    return loss.detach(), leaf.grad


def aten():
    leaf = full.detach().requires_grad_(True)
    small = F.interpolate(images, scale_factor=0.25, mode="bilinear")[:, :, :h, :w].permute(0, 2, 3, 1)
    warped, mask, chosen = F_._warp_img_host(small, nbr, w2c, K, leaf[:, :, :h, :w], ref_id)
    loss = F_._photometric_loss_host([warped], [mask], [chosen])["loss_pc"]
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
gmax = float(gb.abs().max())
say(f"loss_pc, one scene, {N} views, {B} chosen, images {Hi}x{Wi} -> {h}x{w} (crop of 60x80): HIP {float(la)!r}  ATen {float(lb)!r}; "
    f"gradients differ by at most {float((ga - gb).abs().max()) / gmax:.2e} of the largest magnitude {gmax:.3g}; "
    f"{int((ga != 0).sum())} / {int((gb != 0).sum())} non-zero elements")
assert torch.allclose(la, lb, rtol=1e-5, atol=0) and float((ga - gb).abs().max()) <= 1e-3 * gmax, "the two disagree"
for name, fn in (("functional.warp_img + photometric_loss forward + backward (HIP)", hip),
                 ("the ATen restatement of the reference's sequence forward + backward", aten)):
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
