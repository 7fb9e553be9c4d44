"""The NVS branch's Gaussian adapter at the training shape (6 source views of 59x80 feature pixels, one surface, 25 harmonics per
channel = 28 320 Gaussians of 84 floats): forward + backward under autograd of functional.pixel_gaussians on csrc/adapter.hip beside an
ATen restatement of the reference's operator sequence on the same GPU (sigmoid / inverse / einsum / diag_embed / matmul as
gaussian_adapter.py:50-98, gaussians.py:8-44, projection.py:74-114 and mvsdet.py:576-578 spell them, the (v r s) flattening of :615-632
included).  The reference's rotate_sh gets its matrices from e3nn, which is not installed: the ATen form is handed the blocks the HIP
cameras kernel built and applies them degree by degree with the reference's einsum, so the cost of wigner_D itself is NOT in its time.
HIP events, median and minimum of the rounds.  Also counted, for one step of each: device kernels (torch.profiler) and host
synchronisations (torch's sync debug mode).  The two are checked against each other first.  The text goes to --out (default
profiles/adapter_timing.txt) and to stdout.

    python tools/adapter_timing.py [--out FILE] [--rounds N]
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
from mvsdet_amd import functional as F_  # noqa: E402
from mvsdet_amd.ops import adapter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapter_timing.txt"))
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda:0")
V, h, w, S, L = 6, 59, 80, 1, 4
D = (L + 1) ** 2
R, C = h * w, 9 + 3 * D
S_MIN, S_MAX = 0.5, 15.0
gen = torch.Generator().manual_seed(27)


def pose(i):
    a, b = 0.3 * i - 0.8, 0.1 * i + 0.2
    m = torch.eye(4)
    m[:3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]) @ \
        torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    m[:3, 3] = torch.tensor([0.15 * i - 0.5, 0.03 * (i % 3), 0.05 * (i % 2)])
    return m


ext = torch.stack([pose(i) for i in range(V)]).to(dev)
intr = torch.tensor([[0.9, 0.01, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).expand(V, 3, 3).contiguous().to(dev)
raw0 = (1.5 * torch.randn(V, R, S, C, generator=gen)).to(dev)
depth0 = (0.3 + 4.7 * torch.rand(V, R, generator=gen)).to(dev)
opac0 = torch.rand(V, R, generator=gen).to(dev)
G = V * R * S
W_MEANS, W_COVS, W_SH = (torch.randn(*s, generator=gen).to(dev) for s in ((G, 3), (G, 3, 3), (G, 3, D)))
blocks = adapter.adapter_cameras(ext, intr, h, w, L)[:, adapter.ADAPTER_ROT:adapter.ADAPTER_ROT + adapter.rotation_floats(D)].contiguous()
sh_mask = torch.ones(D, device=dev)
for l in range(1, L + 1):
    sh_mask[l * l:(l + 1) ** 2] = 0.1 * 0.25 ** l


def finish(means, covs, harm, opac, leaves):
    ((means * W_MEANS).sum() + (covs * W_COVS).sum() + (harm * W_SH).sum() + opac.sum()).backward()
    return [means.detach(), covs.detach(), harm.detach()], [t.grad for t in leaves]


def hip():
    leaves = [t.detach().requires_grad_(True) for t in (raw0, depth0, opac0)]
    g = F_.pixel_gaussians(ext, intr, *leaves, (h, w), S_MIN, S_MAX, L)
    return finish(g.means[0], g.covariances[0], g.harmonics[0], g.opacities[0], leaves)


def aten():
    leaves = [t.detach().requires_grad_(True) for t in (raw0, depth0, opac0)]
    raw, depth, opac = leaves
    gaussians = raw[None]                                                                    # (1,V,R,S,C)
    # sample_image_grid + mvsdet.py:576-578
    ys, xs = (torch.arange(h, device=dev) + 0.5) / h, (torch.arange(w, device=dev) + 0.5) / w
    xy_ray = torch.stack(torch.meshgrid(xs, ys, indexing="xy"), dim=-1).reshape(R, 1, 2)
    pixel_size = 1 / torch.tensor((w, h), dtype=torch.float32, device=dev)
    xy = (xy_ray + (gaussians[..., :2].sigmoid() - 0.5) * pixel_size)[..., None, :]          # (1,V,R,S,1,2)
    E, K = ext[None, :, None, None, None], intr[None, :, None, None, None]                   # (1,V,1,1,1,*,*)
    depths, opacities = depth[None, :, :, None, None], opac[None, :, :, None, None]
    rest = gaussians[..., 2:][..., None, :]
    scales, rotations, sh = rest.split((3, 4, 3 * D), dim=-1)
    scales = S_MIN + (S_MAX - S_MIN) * scales.sigmoid()
    multiplier = (0.1 * torch.einsum("...ij,j->...i", K[..., :2, :2].inverse(), pixel_size)).sum(dim=-1)
    scales = scales * depths[..., None] * multiplier[..., None]
    rotations = rotations / (rotations.norm(dim=-1, keepdim=True) + 1e-8)
    sh = sh.reshape(*sh.shape[:-1], 3, D).broadcast_to((1, V, R, S, 1, 3, D)) * sh_mask
    # build_covariance / quaternion_to_matrix
    i, j, k, r = torch.unbind(rotations, dim=-1)
    two_s = 2 / ((rotations * rotations).sum(dim=-1) + 1e-8)
    rot = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r), two_s * (i * j + k * r),
                       1 - two_s * (i * i + k * k), two_s * (j * k - i * r), two_s * (i * k - j * r), two_s * (j * k + i * r),
                       1 - two_s * (i * i + j * j)), -1).reshape(*rotations.shape[:-1], 3, 3)
    sc = scales.diag_embed()
    covariances = rot @ sc @ sc.transpose(-1, -2) @ rot.transpose(-1, -2)
    c2w = E[..., :3, :3]
    covariances = c2w @ covariances @ c2w.transpose(-1, -2)
    # get_world_rays
    coords = torch.cat([xy, torch.ones_like(xy[..., :1])], dim=-1)
    directions = torch.einsum("...ij,...j->...i", K.inverse(), coords)
    directions = directions / directions.norm(dim=-1, keepdim=True)
    directions = torch.cat([directions, torch.zeros_like(directions[..., :1])], dim=-1)
    directions = torch.einsum("...ij,...j->...i", E, directions)[..., :-1]
    origins = E[..., :-1, -1].broadcast_to(directions.shape)
    means = origins + directions * depths[..., None]
    # rotate_sh with given blocks: one einsum per degree, then the concatenation
    parts, off = [], 0
    for l in range(L + 1):
        n = 2 * l + 1
        Dl = blocks[:, off:off + n * n].reshape(1, V, 1, 1, 1, 1, n, n)
        parts.append(torch.einsum("...ij,...j->...i", Dl, sh[..., l * l:(l + 1) ** 2]))
        off += n * n
    harmonics = torch.cat(parts, dim=-1)
    return finish(means.reshape(G, 3), covariances.reshape(G, 3, 3), harmonics.reshape(G, 3, D),
                  opacities.expand(1, V, R, S, 1).reshape(G), leaves)


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


(oa, ga), (ob, gb) = hip(), aten()
say(f"{V} source views of {h}x{w}, {S} surface(s), {D} harmonics per channel: {G} Gaussians of {C} floats")
for n, a, b in zip(("means", "covariances", "harmonics"), oa, ob):
    say(f"    {n}: HIP against the ATen form, largest difference {float((a - b).abs().max()):.3g} of {float(b.abs().max()):.3g}")
for n, a, b in zip(("raw", "depth", "opacity"), ga, gb):
    say(f"    d {n}: largest difference {float((a - b).abs().max()):.3g} of {float(b.abs().max()):.3g}")
    assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()), "the two disagree"
for name, fn, steps in (("functional.pixel_gaussians forward + backward (HIP)", hip, 50), ("the ATen form forward + backward", aten, 10)):
    for _ in range(3):
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
        f"{n_kernels if n_kernels is not None else '?'} device kernels (the loss's and autograd's own included)")
    ours = [n for n in names if "adapter" in n]
    if ours:
        say(f"    of these the adapter's own: {len(ours)}")
        for n in ours:
            say(f"        {n[:150]}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
