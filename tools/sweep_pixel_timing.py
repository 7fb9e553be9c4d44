"""The fused per-pixel sweep (ops.plane_sweep_variance_pixel: homo_warping's depth_values (B,D,H,W) form) at the reference-true
shape -- 40 views, 2 neighbours, 256 channels, 12 hypotheses, 60x80 maps -- with a smooth and a rough depth map, beside two
things on the same GPU in the same run: the plane operator on the plane depths the smooth map is built around, and the
reference's op sequence as ATen operations (K grid_samples plus the variance statements of mvsdet.py:439-467).  Forward, and
forward + backward of sum(var * R).  HIP events, median and minimum of 7 rounds.  The three are checked against each other first."""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvsdet_amd import ops, synthetic  # noqa: E402
from mvsdet_amd.hotpath import MVSDetHotPath  # noqa: E402

dev = torch.device("cuda:0")
N, K, C, D, hw = 40, 2, 256, 12, (60, 80)
H, W = hw
hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D, topk=3)
geo = hp.prepare_scene(synthetic.make_img_meta(N, hw, seed=5), dev)
nbr, proj, planes = geo.neighbor_ids, geo.proj_rel, geo.depth_values
feat = synthetic.make_features(N, C, hw, seed=5).to(dev)
g = torch.Generator(device=dev)
g.manual_seed(5)
interval = 4.8 / D
ys, xs = torch.meshgrid(torch.arange(H, device=dev) / H, torch.arange(W, device=dev) / W, indexing="ij")
low = torch.sin(6.2832 * xs) * torch.cos(6.2832 * ys)
DEPTHS = {
    "broadcast": planes[:, :, None, None].expand(N, D, H, W).contiguous(),
    "smooth": (planes[:, :, None, None] + 0.35 * interval * low + 0.05 * interval * (2 * torch.rand(N, D, H, W, device=dev, generator=g) - 1)
               ).clamp_min(0.2).contiguous(),
    "rough": 0.2 + 4.8 * torch.rand(N, D, H, W, device=dev, generator=g),
}
R = torch.rand(N, C, D, H, W, device=dev, generator=g)


def aten_warp(src, pj, depth):
    """module.py:105-146 with a 4-D depth, on the device."""
    with torch.no_grad():
        rot, trans = pj[:, :3, :3], pj[:, :3, 3:4]
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
        xyz = torch.stack((xx.reshape(-1), yy.reshape(-1), torch.ones(H * W, device=dev)))[None].repeat(N, 1, 1)
        pts = torch.matmul(rot, xyz).unsqueeze(2).repeat(1, 1, D, 1) * depth.view(N, 1, D, H * W) + trans.view(N, 3, 1, 1)
        xy = pts[:, :2] / pts[:, 2:3]
        grid = torch.stack((xy[:, 0] / ((W - 1) / 2) - 1, xy[:, 1] / ((H - 1) / 2) - 1), dim=3)
    return F.grid_sample(src, grid.view(N, D * H, W, 2), mode="bilinear", padding_mode="zeros", align_corners=False).view(N, C, D, H, W)


def aten_variance(f, depth):
    ref = f.unsqueeze(2).repeat(1, 1, D, 1, 1)
    vsum, vsq = ref, ref ** 2
    for j in range(K):
        w = aten_warp(f[nbr[:, j]], proj[:, j], depth)
        vsum = vsum + w
        vsq = vsq + w ** 2
    return vsq / (K + 1) - (vsum / (K + 1)) ** 2


def timed(name, fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    print(f"{name}: median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms", flush=True)
    return min(ms)


def fwd_bwd(op, f, depth):
    f.grad = None
    (op(f, depth) * R).sum().backward()


pixel = lambda f, depth: ops.plane_sweep_variance_pixel(f, nbr, proj, depth)
plane = lambda f, depth: ops.plane_sweep_variance(f, nbr, proj, planes)
# the three against each other: bits on the broadcast depth, the forward bar against ATen on the others
assert torch.equal(pixel(feat, DEPTHS["broadcast"]), plane(feat, None)), "pixel and plane operators disagree on a broadcast depth"
for name in ("smooth", "rough"):
    a, b = pixel(feat, DEPTHS[name]), aten_variance(feat, DEPTHS[name])
    ok = torch.isfinite(b)
    print(f"{name}: max |fused - ATen| = {float((a - b)[ok].abs().max()):.3e} over {int(ok.sum())} finite elements of {b.numel()}", flush=True)
    del a, b, ok
# algorithmic bytes of the forward: the plane form's (volume out, K + 1 source maps in) + the depth reads of every slab
S = (C + 31) // 32
fwd_bytes = N * C * D * H * W * 4 + (K + 1) * N * C * H * W * 4 + N * S * D * H * W * 4
atomic_bytes = N * C * D * H * W * K * 4 * 4
def taps_inside(depth):
    """fraction of the 4 K taps per (pixel, hypothesis) that lie inside the source maps (the others add nothing)"""
    tot = 0.0
    for j in range(K):
        pj = proj[:, j]
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
        xyz = torch.stack((xx.reshape(-1), yy.reshape(-1), torch.ones(H * W, device=dev)))[None].repeat(N, 1, 1)
        pts = torch.matmul(pj[:, :3, :3], xyz).unsqueeze(2) * depth.view(N, 1, D, H * W) + pj[:, :3, 3:4].view(N, 3, 1, 1)
        ix = (pts[:, 0] / pts[:, 2]) * W / (W - 1) - 0.5
        iy = (pts[:, 1] / pts[:, 2]) * H / (H - 1) - 0.5
        x0, y0 = ix.floor(), iy.floor()
        inx = ((x0 >= 0) & (x0 <= W - 1)).float() + ((x0 >= -1) & (x0 <= W - 2)).float()
        iny = ((y0 >= 0) & (y0 <= H - 1)).float() + ((y0 >= -1) & (y0 <= H - 2)).float()
        tot += float((inx * iny).mean()) / 4
    return tot / K


print(f"shape N={N} K={K} C={C} D={D} {H}x{W}: forward {fwd_bytes / 1e9:.3f} GB algorithmic, backward {atomic_bytes / 1e9:.2f} GB of float adds "
      f"(floor {atomic_bytes / 1.3e12 * 1e3:.1f} ms at 1.3 TB/s)", flush=True)
leaf = feat.clone().requires_grad_(True)
# forward + backward of sum(var * R) goes through autograd: besides the operators' own launches it contains torch's elementwise
# passes over the (N,C,D,H,W) volume (the product with R and its backward); the backward operators are also timed alone
with torch.no_grad():
    timed("plane operator, backward operator alone (pack + geometry + kernel + unpack)",
          lambda: ops.plane_sweep_variance_backward(feat, nbr, proj, planes, R), 10)
with torch.no_grad():
    t = timed("plane operator, forward (plane depths)", lambda: plane(feat, None), 20)
timed("plane operator, forward + backward", lambda: fwd_bwd(plane, leaf, None), 10)
for name in ("broadcast", "smooth", "rough"):
    depth = DEPTHS[name]
    with torch.no_grad():
        t = timed(f"pixel operator, forward, {name} depth", lambda: pixel(feat, depth), 20)
    print(f"    = {fwd_bytes / t / 1e9:.2f} TB/s of algorithmic bytes ({fwd_bytes / t / 1e9 / 8.0 * 100:.0f} % of 8 TB/s HBM)")
    timed(f"pixel operator, forward + backward, {name} depth", lambda: fwd_bwd(pixel, leaf, depth), 5)
    with torch.no_grad():
        tb = timed(f"pixel operator, backward operator alone (pack + memset + kernel + unpack), {name} depth",
                   lambda: ops.plane_sweep_variance_pixel_backward(feat, nbr, proj, depth, R), 5)
    frac = taps_inside(depth)
    print(f"    taps inside the source maps: {100 * frac:.1f} % -> {atomic_bytes * frac / 1e9:.2f} GB added, {atomic_bytes * frac / tb / 1e9:.2f} TB/s "
          f"over the whole operator (bound 1.3 TB/s: {atomic_bytes * frac / 1.3e12 * 1e3:.1f} ms)")
    print(f"    = {atomic_bytes / tb / 1e9:.2f} TB/s if every tap were added ({atomic_bytes / 1e9:.2f} GB; taps outside the source maps are "
          f"not: the 1.3 TB/s bound is on the bytes actually added)")
    if name != "broadcast":
        with torch.no_grad():
            timed(f"ATen sequence, forward, {name} depth", lambda: aten_variance(feat, depth), 3)
        timed(f"ATen sequence, forward + backward, {name} depth", lambda: fwd_bwd(lambda f, d: aten_variance(f, d), leaf, depth), 2)
