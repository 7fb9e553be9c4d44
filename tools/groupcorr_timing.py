"""The fused group-wise correlation sweep (ops.sweep.plane_sweep_groupcorr, csrc/groupcorr.hip) at the reference-true shape -- 40 views,
2 neighbours, 256 channels, 12 hypotheses, 60x80 maps -- with G = 8 and G = 32 groups, on plane depths and on a rough per-pixel
depth map, beside two things on the same GPU in the same run: the only route to this result without it -- K ops.homo_warp[_pixel]
calls plus the reshape / product / mean of lss_fpn.py:499-506 as ATen operations -- and ops.plane_sweep_variance_pixel at the
same shape.  Forward, the backward alone, and forward + backward of sum(corr * R) under autograd.  HIP events, median and minimum
of 7 rounds.  The two routes are checked against each other first.

The composed route's backward on plane depths goes through ops.homo_warp_pixel on the broadcast depth map: ops.homo_warp (B,D)
has no autograd formula."""
import os
import statistics
import sys

import torch

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
gen = torch.Generator(device=dev)
gen.manual_seed(5)
DEPTHS = {"plane": planes.contiguous(), "rough": 0.2 + 4.8 * torch.rand(N, D, H, W, device=dev, generator=gen)}
broadcast = planes[:, :, None, None].expand(N, D, H, W).contiguous()
projs = [proj[:, j].contiguous() for j in range(K)]


def composed(f, depth, G, differentiable=False):
    """K warps (2.36 GB each here) and the three statements of lss_fpn.py:499-506 on them."""
    out = []
    for j in range(K):
        if depth.dim() == 2 and not differentiable:
            w = ops.homo_warp(f[nbr[:, j]], projs[j], depth)
        else:
            w = ops.homo_warp_pixel(f[nbr[:, j]], projs[j], depth if depth.dim() == 4 else broadcast)
        w = w.reshape(N, G, C // G, D, H, W)
        out.append(torch.mean(f.reshape(N, G, C // G, H, W).unsqueeze(3) * w, dim=2))
    return torch.stack(out, dim=1)


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
    return statistics.median(ms)


def fwd_bwd(op, f, R):
    f.grad = None
    (op(f) * R).sum().backward()


print(f"shape N={N} K={K} C={C} D={D} {H}x{W}", flush=True)
leaf = feat.clone().requires_grad_(True)
for G in (8, 32):
    # algorithmic bytes of the forward: K + 1 source maps in, K (G,D,H,W) volumes out
    rd = (K + 1) * N * C * H * W * 4
    wr = N * K * G * D * H * W * 4
    gathers = N * K * D * H * W * 4 * C * 4          # 4 taps of C channels per (view, neighbour, hypothesis, pixel)
    flops = N * K * D * H * W * C * (7 + 2)          # tap sum 7, product + add 2
    atomic_bytes = N * K * D * H * W * C * 4 * 4
    print(f"--- G={G} (Cg={C // G}): forward reads {rd / 1e6:.1f} MB, writes {wr / 1e6:.1f} MB ({wr / N / K / 1e6:.2f} MB per view and neighbour; "
          f"the variance writes {N * C * D * H * W * 4 / 1e6:.0f} MB); {gathers / 1e9:.2f} GB of tap gathers from L2, {flops / 1e9:.2f} GFLOP; "
          f"backward {atomic_bytes / 1e9:.2f} GB of float adds if every tap were inside", flush=True)
    R = torch.rand(N, K, G, D, H, W, device=dev, generator=gen)
    for name, depth in DEPTHS.items():
        fused = lambda f: ops.sweep.plane_sweep_groupcorr(f, nbr, proj, depth, G)
        a, b = fused(feat), composed(feat, depth, G)
        ok = torch.isfinite(b)
        print(f"G={G} {name}: max |fused - composed| = {float((a - b)[ok].abs().max()):.3e} over {int(ok.sum())} finite elements of {b.numel()} "
              f"(max |value| {float(b[ok].abs().max()):.3f})", flush=True)
        del a, b, ok
        with torch.no_grad():
            t = timed(f"G={G} {name}: fused forward", lambda: fused(feat), 20)
        print(f"    = {gathers / t / 1e9:.2f} TB/s of tap gathers, {flops / t / 1e9:.2f} TFLOP/s fp32 vector work, {(rd + wr) / t / 1e9:.3f} TB/s of algorithmic bytes")
        with torch.no_grad():
            tb = timed(f"G={G} {name}: fused backward operator alone (pack + memset + kernel + unpack)",
                       lambda: ops.sweep.plane_sweep_groupcorr_backward(feat, nbr, proj, depth, R, G), 5)
        print(f"    = {atomic_bytes / tb / 1e9:.2f} TB/s of float adds if every tap were inside (bound 1.3 TB/s on the bytes actually added)")
        timed(f"G={G} {name}: fused forward + backward (autograd)", lambda: fwd_bwd(fused, leaf, R), 5)
        with torch.no_grad():
            timed(f"G={G} {name}: composed forward (K ops.homo_warp{'_pixel' if depth.dim() == 4 else ''} + ATen reshape / product / mean)",
                  lambda: composed(feat, depth, G), 3)
        comp = lambda f: composed(f, depth, G, differentiable=True)
        leaf.grad = None
        loss = (comp(leaf) * R).sum()
        timed(f"G={G} {name}: composed backward alone (autograd.grad on a kept graph)",
              lambda: torch.autograd.grad(loss, leaf, retain_graph=True), 2)
        del loss
        timed(f"G={G} {name}: composed forward + backward (autograd; warps by ops.homo_warp_pixel)", lambda: fwd_bwd(comp, leaf, R), 2)
    del R
with torch.no_grad():
    timed("plane_sweep_variance_pixel, forward, rough depth (writes 2359 MB)",
          lambda: ops.plane_sweep_variance_pixel(feat, nbr, proj, DEPTHS["rough"]), 20)
    timed("plane_sweep_variance, forward, plane depths", lambda: ops.plane_sweep_variance(feat, nbr, proj, planes), 20)
