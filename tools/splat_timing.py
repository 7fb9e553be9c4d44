"""The NVS branch's render at the training shape (2 target views, 6 source views of 59x80 pixels = 28 320 Gaussians, 239x320 images,
25 harmonics per channel): forward + backward under autograd of functional.render_cuda on csrc/splat.hip beside a dense ATen form of
the same formulas on the same GPU -- the restated preprocess (tests/splat_restated.py) on the device, then per tile every Gaussian of
the tile's list at every pixel of the tile: alpha as an (entries, 256) matrix, T by a cumulative product, the early stop as a mask.
HIP events, median and minimum of the rounds.  Also counted, for one step of each: device kernels (torch.profiler) and host
synchronisations (torch's sync debug mode).  The two are checked against each other first.  The text goes to --out (default
profiles/splat_timing.txt) and to stdout.

    python tools/splat_timing.py [--out FILE] [--rounds N]

--depth: instead, the rendered depth at the same shape: forward + backward of the fused colour + depth call
(ops.splat.rasterize_depth) against the two-pass route the colour rasteriser alone offers -- `rasterize` for the colour, then, as
render_depth_cuda does, every Gaussian's depth built by torch operations from the means and rendered as three equal precomputed colour
channels (`rasterize(use_sh=False)`, one view at a time: the value differs per view), averaged.  Both in one process, alternating
round by round, device events; kernels and host synchronisations of one step of each.  Default --out profiles/splat_depth_timing.txt.
"""
import argparse
import math
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import splat_restated as R  # noqa: E402
from mvsdet_amd import functional as F_  # noqa: E402
from mvsdet_amd.ops import splat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--depth", action="store_true", help="time the fused colour + depth call against the two-pass route")
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "splat_depth_timing.txt" if args.depth else "splat_timing.txt")

dev = torch.device("cuda:0")
V, SRC, h, w, H, W, D = 2, 6, 59, 80, 239, 320, 25
gen = torch.Generator().manual_seed(26)


def pose(i):
    a, b = 0.06 * i - 0.2, 0.02 * i
    m = torch.eye(4)
    m[:3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]) @ \
        torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    m[:3, 3] = torch.tensor([0.15 * i - 0.5, 0.03 * (i % 3), 0.05 * (i % 2)])
    return m


K = torch.tensor([[0.9, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]])
# one Gaussian per source pixel, at the pixel's depth, about a pixel's footprint wide
yy, xx = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij")
means, covs = [], []
for i in range(SRC):
    c2w = pose(i + 1)
    depth = 2.2 + 0.7 * torch.sin(5 * xx + i) * torch.cos(4 * yy) + 0.05 * torch.rand(h, w, generator=gen)
    rays = torch.stack([(xx - 0.5) / 0.9, (yy - 0.5) / 1.2, torch.ones_like(xx)], -1) * depth[..., None]
    means.append((rays.reshape(-1, 3) @ c2w[:3, :3].T + c2w[:3, 3]))
    sigma = (depth.reshape(-1) * 0.6 / (w * 0.9))[:, None, None]
    L = torch.eye(3) + 0.3 * torch.randn(h * w, 3, 3, generator=gen)
    covs.append((L @ L.transpose(1, 2)) * sigma * sigma)
means, covs = torch.cat(means).to(dev), torch.cat(covs).to(dev)
G = means.shape[0]
sh = 0.2 * torch.randn(G, 3, D, generator=gen)
sh[:, :, 0] = 0.8 * torch.randn(G, 3, generator=gen)
sh, opac = sh.to(dev), torch.rand(G, generator=gen).mul(0.9).add(0.05).to(dev)
ext = torch.stack([pose(0), pose(4.5)]).to(dev)
intr = K.expand(V, 3, 3).contiguous().to(dev)
near, far = torch.full((V,), 0.5, device=dev), torch.full((V,), 15.0, device=dev)
bg = torch.zeros(V, 3, device=dev)
weight = torch.randn(V, 3, H, W, generator=gen).to(dev)
LEAVES = (means, covs, sh, opac)


def hip():
    leaves = [t.detach().requires_grad_(True) for t in LEAVES]
    image = F_.render_cuda(ext, intr, near, far, (H, W), bg, *[t[None].expand(V, *t.shape) for t in leaves])
    (image * weight).sum().backward()
    return image.detach(), [t.grad for t in leaves]


def aten():
    leaves = [t.detach().requires_grad_(True) for t in LEAVES]
    cams = splat.splat_cameras(ext, intr, near, far, True)
    tiles_x, tiles_y = -(-W // R.TILE), -(-H // R.TILE)
    ys, xs = torch.meshgrid(torch.arange(R.TILE, device=dev), torch.arange(R.TILE, device=dev), indexing="ij")
    views = []
    for v in range(V):
        p = R.preprocess(*leaves, cams[v], H, W)
        order = torch.sort(torch.where(p["ok"], p["depth"].detach(), torch.full_like(p["depth"], float("inf"))), stable=True).indices
        order = order[:int(p["ok"].sum())]
        rect = p["rect"][order]
        image = torch.zeros(3, tiles_y * R.TILE, tiles_x * R.TILE, device=dev)
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                idx = order[(rect[:, 0] <= tx) & (tx < rect[:, 1]) & (rect[:, 2] <= ty) & (ty < rect[:, 3])]
                X, Y = (xs + tx * R.TILE).reshape(1, -1).float(), (ys + ty * R.TILE).reshape(1, -1).float()
                dx, dy = p["px"][idx, None] - X, p["py"][idx, None] - Y
                con = p["conic"][idx]
                power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
                raw = leaves[3][idx, None] * torch.exp(power)
                alpha = raw + (torch.clamp(raw, max=R.ALPHA_CAP) - raw).detach()
                alpha = torch.where((power > 0) | (alpha < R.ALPHA_MIN), torch.zeros_like(alpha), alpha)
                Tn = torch.cumprod(1.0 - alpha, 0)
                T = torch.cat([torch.ones_like(Tn[:1]), Tn[:-1]])
                wgt = torch.where(Tn < R.T_STOP, torch.zeros_like(alpha), alpha * T)
                T_final = torch.where(Tn < R.T_STOP, torch.ones_like(Tn), Tn).amin(0) if idx.numel() else torch.ones(R.TILE * R.TILE, device=dev)
                tile = p["colour"][idx].T @ wgt + T_final[None] * bg[v][:, None]
                image[:, ty * R.TILE:(ty + 1) * R.TILE, tx * R.TILE:(tx + 1) * R.TILE] = tile.view(3, R.TILE, R.TILE)
        views.append(image[:, :H, :W])
    image = torch.stack(views)
    (image * weight).sum().backward()
    return image.detach(), [t.grad for t in leaves]


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


def write_out():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def depth_timing(mode="depth", steps=20):
    keys = splat.default_max_keys(G)
    cams = splat.splat_cameras(ext, intr, near, far, True)
    w2c_z = torch.linalg.inv(ext)[:, 2]                       # (V,4): the row that gives camera-space z; fixed cameras, built once
    wdepth = torch.randn(V, H, W, generator=gen).to(dev)
    black = torch.zeros(1, 3, device=dev)

    def fused():
        leaves = [t.detach().requires_grad_(True) for t in LEAVES]
        image, depth, _, _ = splat.rasterize_depth(*leaves, cams, near, far, bg, H, W, keys, True, mode)
        ((image * weight).sum() + (depth * wdepth).sum()).backward()
        return image.detach(), depth.detach(), [t.grad for t in leaves]

    def two_pass():
        leaves = [t.detach().requires_grad_(True) for t in LEAVES]
        image = splat.rasterize(*leaves, cams, bg, H, W, keys, True)[0]
        value = leaves[0] @ w2c_z[:, :3].T + w2c_z[:, 3]       # (G,V)
        depth = torch.stack([splat.rasterize(leaves[0], leaves[1], value[:, v, None, None].expand(G, 3, 1), leaves[3], cams[v:v + 1], black,
                                             H, W, keys, False)[0][0].mean(0) for v in range(V)])
        ((image * weight).sum() + (depth * wdepth).sum()).backward()
        return image.detach(), depth.detach(), [t.grad for t in leaves]

    def alone():
        leaves = [t.detach().requires_grad_(True) for t in (means, covs, opac)]
        depth = splat.depth_only(*leaves, cams, near, far, H, W, keys, mode)[0]
        (depth * wdepth).sum().backward()
        return depth.detach()

    (ia, da, ga), (ib, db, gb) = fused(), two_pass()
    say(f"rendered depth, mode {mode}: {V} views of {G} Gaussians, {H}x{W}, {D} harmonics, forward + backward of sum(image w) + sum(depth w')")
    say(f"fused against two passes: image bits equal {bool(torch.equal(ia, ib))}; depth largest difference {float((da - db).abs().max()):.3g} "
        f"of {float(db.abs().max()):.3g} (the value is z_s / s in the kernel and a matrix product in torch; one blend against the mean of three)")
    for n, a, b in zip(("means", "covariances", "harmonics", "opacities"), ga, gb):
        say(f"    d {n}: largest difference {float((a - b).abs().max()):.3g} of {float(b.abs().max()):.3g}")
    assert float((da - db).abs().max()) <= 1e-4 * float(db.abs().max()), "the two disagree"
    routes = (("fused colour + depth (rasterize_depth)", fused), ("two passes (rasterize + rasterize(use_sh=False) per view)", two_pass),
              ("depth alone (depth_only)", alone))
    for _, fn in routes:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in routes}
    for _ in range(args.rounds):                               # alternating: one round of each after the other
        for name, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
    for name, fn in routes:
        syncs = count_syncs(fn)
        n_kernels, _ = count_kernels(fn)
        say(f"{name}: median {statistics.median(ms[name]):.3f} ms, min {min(ms[name]):.3f} ms per step over {args.rounds} rounds of {steps}; "
            f"{syncs} host synchronisation(s); {n_kernels if n_kernels is not None else '?'} device kernels (autograd's own included)")
    a, b = statistics.median(ms[routes[0][0]]), statistics.median(ms[routes[1][0]])
    say(f"fused / two passes = {a / b:.3f} (medians)")
    write_out()


if args.depth:
    depth_timing()
    sys.exit(0)

(ia, ga), (ib, gb) = hip(), aten()
cams = splat.splat_cameras(ext, intr, near, far, True)
_, ws = splat.rasterize(*LEAVES, cams, bg, H, W, splat.default_max_keys(G), True)
st = splat.status(ws, V)
say(f"{V} views of {G} Gaussians ({SRC} source views of {h}x{w}), {H}x{W}, {D} harmonics: keys per view {[s['needed'] for s in st]} of "
    f"{st[0]['capacity']} = {[round(s['needed'] / G, 3) for s in st]} per Gaussian")
close = (ia - ib).abs() <= 1e-4 * ib.abs() + 1e-5
say(f"HIP against the dense ATen form: {float((~close).float().mean()):.2e} of the pixel values apart by more than 1e-4 |x| + 1e-5 "
    f"(a pixel's decision may fall the other way in float32); largest difference {float((ia - ib).abs().max()):.3g}")
for n, a, b in zip(("means", "covariances", "harmonics", "opacities"), ga, gb):
    say(f"    d {n}: largest difference {float((a - b).abs().max()):.3g} of {float(b.abs().max()):.3g}")
assert float((~close).float().mean()) < 1e-3, "the two disagree"
for name, fn, steps in (("functional.render_cuda forward + backward (HIP)", hip, 20), ("the dense ATen form forward + backward", aten, 1)):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    syncs = count_syncs(fn)
    n_kernels, names = count_kernels(fn)
    say(f"{name}: median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms per step; {syncs} host synchronisation(s); "
        f"{n_kernels if n_kernels is not None else '?'} device kernels (autograd's own included)")
    if n_kernels is not None and n_kernels <= 60:
        for n in names:
            say(f"    {n[:150]}")
write_out()
