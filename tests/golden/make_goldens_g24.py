#!/usr/bin/env python3
"""Generate tests/golden/g24_depth_loss.npz by RUNNING THE REFERENCE on the CPU (build container only: needs the reference tree).

G24: the reference's two depth objectives, unmodified, called directly:

  MVSDet.depth_loss_func_new (mvsdet.py:893-915)  unbound, a SimpleNamespace as `self` (it reads nothing from it), with NON-EMPTY lists.
                                                  An unmodified extract_feat never fills `est_depth_crop` (mvsdet.py:400,698), so the
                                                  reference's own training run only ever sees the empty loop here.
  mvsnet_loss (mvs_models/mvsnet.py:292-294)

Cases (l1: est (N,h,w), gt (N,Hg,Wg)):
  ref_true   N=2, gt 239x320, est the [:59,:80] crop of a 60x80 map (stored whole: `est_full`)
  odd        N=3, gt 23x31 -> 5x7, non-integer scales on both axes
  enlarge    N=2, gt 5x7 -> 11x13: source indices clamp at 0 and at the last row / column
  same       N=2, 7x9, no resize
  batch2     the list [odd, enlarge]: the sum over the batch (stored: the loss alone; the gradients are the single scenes')
  smooth_small, smooth_big   mvsnet_loss at 2x5x7 and 2x59x80, differences on both sides of +-1
Ground truth: a smooth surface in [0.3, 8] cut to steps of 1/32 (it compresses), zero blobs plus isolated zero pixels over about a
fifth of the map.  The two small resized cases stay below 4 m: ATen's CPU kernel and the restatement place their roundings differently,
up to 2 ulp apart on these shapes, and 2 ulp is under the 5e-7 bar only below 4 (ref_true, up to 8 m, is 1 ulp apart at the most).
Stored per case: the inputs, the loss, the count, d loss / d est from the reference's autograd.

ASSERTED here, on the reference's own F.interpolate: every positive resized value >= 1e-3 and every masked |est - g| >= 1e-4 in the
resized cases (no mask bit and no sign hangs on one ulp); F.interpolate and tests/depth_loss_restated.resize agree to 5e-7 with
identical masks; in the smooth-L1 cases no ||d| - 1| < 1e-4.

    python tests/golden/make_goldens_g24.py
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from depth_loss_restated import resize  # noqa: E402
from lcg import lcg_uniform  # noqa: E402

F32 = np.float32


def make_gt(N, H, W, seed, top=8.0):
    """Smooth depth in [0.3, top] in steps of 1/32 with zero blobs and isolated zero pixels over about a fifth of the map."""
    u = lcg_uniform(N * 16 + N * H * W, seed)
    par, salt = u[:N * 16].reshape(N, 16), u[N * 16:].reshape(N, H, W)
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    gt = np.empty((N, H, W), F32)
    for i in range(N):
        p = par[i].astype(np.float64)
        z = 3.6 + 2.2 * np.sin(2.5 * x + 3 * p[0]) * np.cos(2.0 * y + 3 * p[1]) + 1.0 * (x * p[2] + y * p[3])
        z = np.clip(z * (top / 8.0), 0.3, top)
        gt[i] = (np.round(z * 32) / 32).astype(F32)
        for b in range(3):                                     # blobs: ellipses of about 4 % of the map each
            cy, cx = 0.5 + 0.45 * p[4 + 2 * b], 0.5 + 0.45 * p[5 + 2 * b]
            ry, rx = 0.08 + 0.05 * abs(p[10 + b]), 0.12 + 0.06 * abs(p[13 + b])
            gt[i][((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1] = 0
        gt[i][salt[i] > 0.8] = 0                               # isolated pixels: 10 %
    return gt


def make_est(g, seed, lo=0.02, hi=0.6):
    """g + a signed offset of size [lo, hi]; outside the mask (g <= 0) just a depth."""
    u = lcg_uniform(2 * g.size, seed).reshape(2, *g.shape)
    off = np.sign(u[0] + F32(1e-9)) * (lo + (hi - lo) * np.abs(u[1]))
    return np.where(g > 0, g + off, 2.0 + u[1]).astype(F32)


def run_l1(ref, est_views, gts):
    """est_views: list of (N,h,w) tensors (views allowed) -> loss, [grad per scene]."""
    leaves = [e.unsqueeze(1).detach().requires_grad_(True) for e in est_views]
    out = ref.MVSDet.depth_loss_func_new(types.SimpleNamespace(), leaves, [torch.from_numpy(g) for g in gts])
    loss = out["loss_depth"]
    loss.backward()
    return loss.detach().numpy().astype(F32), [l.grad.squeeze(1).numpy().copy() for l in leaves]


def check_l1(est, gt, tag):
    h, w = est.shape[1:]
    g_ref = F.interpolate(torch.from_numpy(gt).unsqueeze(1), size=(h, w), mode="bilinear").squeeze(1).numpy()
    g_our = resize(gt, h, w)
    assert np.array_equal(g_ref > 0, g_our > 0), tag
    dist = float(np.abs(g_ref - g_our).max())
    assert dist <= 5e-7, (tag, dist)
    mask = g_ref > 0
    pos, gap = float(g_ref[mask].min()), float(np.abs(est[mask] - g_ref[mask]).min())
    if gt.shape[1:] != (h, w):
        assert pos >= 1e-3 and gap >= 1e-4, (tag, pos, gap)
    print(f"{tag}: resize vs restatement {dist:.2e}, smallest positive {pos:.4g}, smallest |est - g| {gap:.3g}, "
          f"masked {int(mask.sum())} of {mask.size} ({1 - mask.mean():.2f} outside)")
    return int(mask.sum())


# 5x7 -> 11x13: destination row 5 sits exactly on source row 2 and column 6 on source column 3, so the weight of the next tap is 0 or
# one rounding of the source index.  Holes placed by hand keep rows 2, 3 and columns 3, 4 alike, so that no positive value is such a
# sliver of a neighbour (the >= 1e-3 condition): per view a blob, a 2x2 block on those very rows and columns, isolated pixels.
ENLARGE_HOLES = [[(0, 0), (0, 1), (1, 0), (1, 1), (2, 3), (2, 4), (3, 3), (3, 4), (4, 6), (0, 5)],
                 [(4, 0), (4, 1), (3, 0), (2, 0), (0, 3), (0, 4), (1, 6), (4, 5)]]


def l1_case(ref, arrs, tag, N, Hg, Wg, h, w, seed, full=None, top=8.0, holes=None):
    gt = make_gt(N, Hg, Wg, seed, top)
    if holes is not None:
        gt = make_gt(N, Hg, Wg, seed, top)
        filled = np.where(gt > 0, gt, F32(top / 2))
        for i, cells in enumerate(holes):
            for (r, c) in cells:
                filled[i, r, c] = 0
        gt = filled
    g = F.interpolate(torch.from_numpy(gt).unsqueeze(1), size=(h, w), mode="bilinear").squeeze(1).numpy()
    est = make_est(g, seed + 7)
    if full is not None:                                       # the crop of a padded map: the padding holds a depth too
        pad = np.full((N,) + full, 3.0, F32)
        pad[:, :h, :w] = est
        arrs[f"{tag}:est_full"] = pad
        est_t = torch.from_numpy(pad)[:, :h, :w]
    else:
        arrs[f"{tag}:est"] = est
        est_t = torch.from_numpy(est)
    count = check_l1(est, gt, tag)
    loss, (grad,) = run_l1(ref, [est_t], [gt])
    assert int((grad != 0).sum()) == count
    arrs[f"{tag}:gt"], arrs[f"{tag}:loss"], arrs[f"{tag}:count"], arrs[f"{tag}:grad"] = gt, loss, np.int64(count), grad
    print(f"{tag}: loss {float(loss)!r} count {count}")
    return est, gt


def smooth_case(mvsnet, arrs, tag, N, h, w, seed):
    gt = make_gt(N, h, w, seed)
    gt[gt == 0] = 1.0                                          # mvsnet_loss has its own mask: the map itself has no holes
    u = lcg_uniform(3 * gt.size, seed + 11).reshape(3, *gt.shape)
    size = np.where(u[2] > 0, 0.05 + 0.85 * np.abs(u[1]), 1.1 + 1.4 * np.abs(u[1]))   # |d| in [.05,.9] or [1.1,2.5]
    est = (gt + np.sign(u[0] + F32(1e-9)) * size).astype(F32)
    m = lcg_uniform(gt.size, seed + 12).reshape(gt.shape)
    mask = np.select([m > 0.5, m > 0.0, m > -0.6], [0.75, 0.25, 1.0], 0.0).astype(F32)   # 0 / 0.25 outside, 0.75 / 1 inside
    inside = mask > 0.5
    d = np.abs((est - gt).astype(F32))[inside].astype(np.float64)
    assert np.abs(d - 1).min() >= 1e-4 and (d < 1).sum() > 0 and (d > 1).sum() > 0, tag
    e = torch.from_numpy(est).requires_grad_(True)
    loss = mvsnet.mvsnet_loss(e, torch.from_numpy(gt), torch.from_numpy(mask))
    loss.backward()
    arrs[f"{tag}:est"], arrs[f"{tag}:gt"], arrs[f"{tag}:mask"] = est, gt, mask
    arrs[f"{tag}:loss"], arrs[f"{tag}:count"], arrs[f"{tag}:grad"] = loss.detach().numpy().astype(F32), np.int64(inside.sum()), e.grad.numpy()
    print(f"{tag}: loss {float(loss)!r} count {int(inside.sum())}, {int((d < 1).sum())} quadratic / {int((d > 1).sum())} linear terms, "
          f"smallest ||d| - 1| {np.abs(d - 1).min():.3g}")


if __name__ == "__main__":
    from _ref_loader import load_reference
    torch.set_num_threads(4)
    ref, _ = load_reference()
    mvsnet = sys.modules["refpkg.mvs_models.mvsnet"]
    arrs = dict(torch_version=np.array(torch.__version__), generator=np.array("tests/golden/make_goldens_g24.py"))
    l1_case(ref, arrs, "ref_true", 2, 239, 320, 59, 80, 2401, full=(60, 80))
    odd = l1_case(ref, arrs, "odd", 3, 23, 31, 5, 7, 2402, top=3.9)
    big = l1_case(ref, arrs, "enlarge", 2, 5, 7, 11, 13, 2403, top=3.9, holes=ENLARGE_HOLES)
    l1_case(ref, arrs, "same", 2, 7, 9, 7, 9, 2404)
    loss, grads = run_l1(ref, [torch.from_numpy(odd[0]), torch.from_numpy(big[0])], [odd[1], big[1]])
    assert np.array_equal(grads[0], arrs["odd:grad"]) and np.array_equal(grads[1], arrs["enlarge:grad"])
    arrs["batch2:loss"] = loss
    print(f"batch2: loss {float(loss)!r} = {float(arrs['odd:loss'])!r} + {float(arrs['enlarge:loss'])!r}")
    smooth_case(mvsnet, arrs, "smooth_small", 2, 5, 7, 2405)
    smooth_case(mvsnet, arrs, "smooth_big", 2, 59, 80, 2406)
    path = os.path.join(HERE, "g24_depth_loss.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}  {os.path.getsize(path)} bytes")
