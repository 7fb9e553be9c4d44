#!/usr/bin/env python3
"""Fixture G22: homo_warping with per-pixel depth_values (B,D,H,W) (mvs_models/module.py:130-133) and the variance block
around it (mvsdet.py:439-467), by RUNNING THE REFERENCE on PyTorch-CPU.  Build container only:

    python tests/golden/make_goldens_g22.py

Inputs are those of g2_variance_n3_d8 / g2_variance_n6_d12_arkit (loaded, not stored again).  Per case two depth families,
built from tests/golden/lcg.py seeds and stored: `smooth` (the plane depth + 0.35 interval x a low-frequency pattern + 0.05
interval of noise) and `rough` (every (pixel, hypothesis) independent in [near, far]); each with ~20 planted pixels at a
negative depth and ~20 at 1e6 (and a floor under the others where the case needs one: see CASES).  Stored per (case, family), channel-strided like G2: `warped` of neighbour 0, `variance`,
`R_seed` of the seeded weights R = lcg_uniform(variance.numel(), R_seed), the reference's fp32 autograd gradient of
sum(variance * R) with respect to the feature, `grad_err_fp32` = max |that gradient - the float64 gradient of
tests/sweep_pixel_restated.py| over ALL channels, and `min_abs_z` over all samples.

Two CONDITIONS on the reference alone are asserted (seeds are searched until both hold): min_abs_z >= 0.05 (the division by
Z must not lift last-bit differences past the tests' bars; nothing non-finite enters the goldens), and the fp32 restatement
agrees with the reference within 1e-5.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _ref_loader import load_reference  # noqa: E402
from lcg import lcg_uniform  # noqa: E402
import sweep_pixel_restated as SP  # noqa: E402

torch.set_num_threads(4)
ref, ref_module = load_reference()
META = dict(torch_version=np.array(torch.__version__), generator=np.array("tests/golden/make_goldens_g22.py"))
# G2 case, channel stride of the stored volumes, first seed, floor of the non-planted depths.  The floor: view 2 of n3_d8 has a
# neighbour with r_z in [0.43, 1.2] over the image and t_z = -0.151 m, so Z = r_z d + t_z vanishes at depths 0.13-0.35 m --
# inside that case's first plane band (0.2 +- 0.21 m) and inside [near, far] = [0.2, 5]: no seed can meet min |Z| >= 0.05 there.
# Both families of that case are therefore floored at 0.5 m (Z >= 0.06); the other case needs none.
CASES = [("n3_d8", 32, 100, 0.5), ("n6_d12_arkit", 2, 200, None)]


def depth_family(family, seed, planes, near, far, H, W, floor=None):
    """(N,D,H,W) float32 from LCG seeds only."""
    N, D = planes.shape
    interval = (far - near) / D
    u = lcg_uniform(N * D * H * W, seed).reshape(N, D, H, W).astype(np.float64)
    if family == "smooth":
        ys, xs = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
        ph = lcg_uniform(N * D * 2, seed + 1).reshape(N, D, 2, 1, 1).astype(np.float64) * np.pi
        low = np.sin(2 * np.pi * xs[None, None] + ph[:, :, 0]) * np.cos(2 * np.pi * ys[None, None] + ph[:, :, 1])
        depth = planes.astype(np.float64)[:, :, None, None] + 0.35 * interval * low + 0.05 * interval * u
    else:
        depth = near + (far - near) * (u + 1.0) / 2.0
    if floor is not None:
        depth = np.maximum(depth, floor)
    depth = depth.astype(np.float32)
    # planted pixels: ~20 at a negative depth (behind the camera), ~20 far away (all taps of a neighbour in a few texels)
    where = ((lcg_uniform(40 * 4, seed + 2).reshape(40, 4).astype(np.float64) + 1.0) / 2.0 * np.array([N, D, H, W])).astype(int)
    for i, (n, d, y, x) in enumerate(where):
        depth[n, d, y, x] = -1.5 if i < 20 else 1e6
    return depth


def run_reference(g, depth, need_grad):
    feat = torch.from_numpy(g["feature"]).clone().requires_grad_(need_grad)
    nbr = torch.from_numpy(g["neighbor_ids"])
    ref_proj, nei_projs = torch.from_numpy(g["ref_proj"]), torch.from_numpy(g["nei_projs"])
    N, k = nbr.shape
    D = depth.shape[1]
    dv = torch.from_numpy(depth)
    # mvsdet.py:439-467 restated around the imported homo_warping (inline_restated), training (out-of-place) form
    ref_volume = feat.unsqueeze(2).repeat(1, 1, D, 1, 1)
    volume_sum = ref_volume
    volume_sq_sum = ref_volume ** 2
    nei_features = torch.unbind(feat[nbr.view(-1)].view(N, k, *feat.shape[1:]), dim=1)
    first = None
    for j, nei_fea in enumerate(nei_features):
        warped = ref_module.homo_warping(nei_fea, nei_projs[:, j], ref_proj, dv)
        first = warped if first is None else first
        volume_sum = volume_sum + warped
        volume_sq_sum = volume_sq_sum + warped ** 2
    var = volume_sq_sum / (k + 1) - (volume_sum / (k + 1)) ** 2
    return feat, first, var


def main():
    for tag, cs, seed0, floor in CASES:
        g = np.load(os.path.join(HERE, f"g2_variance_{tag}.npz"))
        N, C, H, W = g["feature"].shape
        near, far = (float(v) for v in g["near_far"])
        nbr, proj = torch.from_numpy(g["neighbor_ids"]), torch.from_numpy(g["proj_rel"])
        for fi, family in enumerate(("smooth", "rough")):
            for seed in range(seed0 + 10 * fi, seed0 + 10 * fi + 10):
                depth = depth_family(family, seed, g["depth_values"], near, far, H, W, floor)
                dt = torch.from_numpy(depth)
                min_abs_z = min(float(SP.sample_grid(proj[:, j], dt, H, W)[1].abs().min()) for j in range(nbr.shape[1]))
                if min_abs_z >= 0.05:
                    break
            else:
                raise SystemExit(f"{tag}/{family}: no seed with min |Z| >= 0.05")
            feat, warped, var = run_reference(g, depth, True)
            assert torch.isfinite(var).all() and torch.isfinite(warped).all()
            R_seed = seed + 5
            R = torch.from_numpy(lcg_uniform(var.numel(), R_seed)).reshape(var.shape)
            (grad,) = torch.autograd.grad((var * R).sum(), feat)
            # condition 2: the restatement against the reference
            ft = torch.from_numpy(g["feature"])
            rw = SP.homo_warp_pixel(ft[nbr[:, 0]], proj[:, 0], dt)
            rv = SP.variance_pixel(ft, nbr, proj, dt)
            err_w, err_v = float((rw - warped).abs().max()), float((rv - var).abs().max())
            assert err_w <= 1e-5 and err_v <= 1e-5, (tag, family, err_w, err_v)
            f64 = ft.double().requires_grad_(True)
            (g64,) = torch.autograd.grad((SP.variance_pixel_f64(f64, nbr, proj, dt) * R.double()).sum(), f64)
            grad_err = float((grad.double() - g64).abs().max())
            out = dict(depth=depth, depth_seed=seed, family=np.array(family), channel_stride=cs, inline_restated=1,
                       warped=warped.detach()[:, ::cs].contiguous().numpy(), variance=var.detach()[:, ::cs].contiguous().numpy(),
                       R_seed=R_seed, grad_feature=grad[:, ::cs].contiguous().numpy(), grad_err_fp32=grad_err,
                       grad_max_abs=float(g64.abs().max()), min_abs_z=min_abs_z, restated_err_warp=err_w, restated_err_var=err_v)
            out.update(META)
            path = os.path.join(HERE, f"g22_sweep_pixel_{tag}_{family}.npz")
            np.savez_compressed(path, **out)
            print(f"wrote {path} {os.path.getsize(path) / 1e6:.2f} MB  seed {seed} min|Z| {min_abs_z:.3f} restated {err_w:.1e} {err_v:.1e} "
                  f"grad_err_fp32 {grad_err:.2e} of {float(g64.abs().max()):.2f}")
            assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
