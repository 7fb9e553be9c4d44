#!/usr/bin/env python3
"""Fixture G23: the group-wise correlation cost volume -- mvs_models/lss_fpn.py:499-506 around the reference's own homo_warping
(mvs_models/module.py:105-146), by RUNNING THE REFERENCE on PyTorch-CPU.  Build container only:

    python tests/golden/make_goldens_g23.py

For every neighbour j: warped_j = homo_warping(feature[neighbor_ids[:, j]], nei_projs[:, j], ref_proj, depth) (imported), then
the three statements of lss_fpn.py:499-506 restated around it (inline_restated): reshape to groups, product with the reshaped
reference feature, mean over the group's channels -> (N,K,G,D,H,W).

Scenes are those of g2_variance_n3_d8 / g2_variance_n6_d12_arkit (loaded, not stored again).  Depths, per case:
  plane  n3_d8: G2's depth_values[:, 1:] -- 7 planes from 0.8 m; the 0.2 m plane is dropped: on these cameras one neighbour reaches
         |Z| = 3e-7 there, against 0.19 at 0.8 m.  n6_d12_arkit: G2's own 12 planes (min |Z| 0.219).
  pixel  the `depth` of g22_sweep_pixel_<case>_rough (loaded, not stored again).
Groups: n3_d8 (C = 32) G in {1, 2, 4, 8}; n6_d12_arkit (C = 8) G in {1, 2}.

Stored per (case, depth kind, G) in g23_groupcorr_<case>_<kind>_g<G>.npz: `corr` = the reference's volume at every
`group_stride`-th group and every `depth_stride`-th hypothesis (both recorded; strides of 1 where the file stays under 1 MiB),
`R_seed` of the weights R = lcg_uniform(N*K*G*D*H*W, R_seed) over the FULL volume, `grad_feature` = the reference's fp32 autograd
gradient of sum(corr * R) with respect to the feature at every `channel_stride`-th channel, `grad_err_fp32` = max |that gradient -
the float64 gradient of tests/groupcorr_restated.py| over ALL channels, `grad_max_abs`, `min_abs_z` over all samples.

CONDITIONS asserted on what is stored: min_abs_z >= 0.05, everything finite, the fp32-warp restatement within 1e-5 of the
reference, every file under 1 MiB.
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
import groupcorr_restated as GR  # noqa: E402
import sweep_pixel_restated as SP  # noqa: E402

torch.set_num_threads(4)
ref, ref_module = load_reference()
META = dict(torch_version=np.array(torch.__version__), generator=np.array("tests/golden/make_goldens_g23.py"))
# G2 case, group counts, channel stride of the stored gradient, first plane of G2's depth_values, R seed base
CASES = [("n3_d8", (1, 2, 4, 8), 32, 1, 2300), ("n6_d12_arkit", (1, 2), 2, 0, 2350)]
MAX_PAIRS = 8   # (group, hypothesis) pairs of the n3_d8 volume a file may hold: 8 x 6 x 48 x 64 floats = 590 KB


def run_reference(g, depth, groups):
    feat = torch.from_numpy(g["feature"]).clone().requires_grad_(True)
    nbr = torch.from_numpy(g["neighbor_ids"])
    ref_proj, nei_projs = torch.from_numpy(g["ref_proj"]), torch.from_numpy(g["nei_projs"])
    N, C, H, W = feat.shape
    D = depth.shape[1]
    out = []
    for j in range(nbr.shape[1]):
        warped = ref_module.homo_warping(feat[nbr[:, j]], nei_projs[:, j], ref_proj, depth)
        # lss_fpn.py:499-506 restated around the imported homo_warping (inline_restated)
        warped = warped.reshape(N, groups, C // groups, D, H, W)
        ref_feat = feat.reshape(N, groups, C // groups, H, W)
        out.append(torch.mean((ref_feat.unsqueeze(3) * warped), axis=2))
    return feat, torch.stack(out, dim=1)


def main():
    for tag, group_counts, cs, first_plane, seed0 in CASES:
        g = np.load(os.path.join(HERE, f"g2_variance_{tag}.npz"))
        N, C, H, W = g["feature"].shape
        nbr, proj = torch.from_numpy(g["neighbor_ids"]), torch.from_numpy(g["proj_rel"])
        ft = torch.from_numpy(g["feature"])
        depths = {"plane": torch.from_numpy(g["depth_values"][:, first_plane:]).contiguous(),
                  "pixel": torch.from_numpy(np.load(os.path.join(HERE, f"g22_sweep_pixel_{tag}_rough.npz"))["depth"])}
        for ki, (kind, depth) in enumerate(depths.items()):
            D = depth.shape[1]
            d4 = GR.depth4(depth, H, W)
            min_abs_z = min(float(SP.sample_grid(proj[:, j], d4, H, W)[1].abs().min()) for j in range(nbr.shape[1]))
            assert min_abs_z >= 0.05, (tag, kind, min_abs_z)
            for groups in group_counts:
                feat, corr = run_reference(g, depth, groups)
                assert torch.isfinite(corr).all()
                R_seed = seed0 + 10 * ki + groups
                R = torch.from_numpy(lcg_uniform(corr.numel(), R_seed)).reshape(corr.shape)
                (grad,) = torch.autograd.grad((corr * R).sum(), feat)
                err = float((GR.groupcorr(ft, nbr, proj, depth, groups) - corr.detach().double()).abs().max())
                assert err <= 1e-5, (tag, kind, groups, err)
                f64 = ft.double().requires_grad_(True)
                (g64,) = torch.autograd.grad((GR.groupcorr_f64(f64, nbr, proj, depth, groups) * R.double()).sum(), f64)
                grad_err = float((grad.double() - g64).abs().max())
                assert torch.isfinite(grad).all() and torch.isfinite(g64).all()
                # what fits: every group_stride-th group, every depth_stride-th hypothesis
                gs = ds = 1
                pairs = MAX_PAIRS * (3 * 2 * 48 * 64) // (N * nbr.shape[1] * H * W)
                while -(-groups // gs) * -(-D // ds) > pairs:
                    if -(-D // ds) > 4:
                        ds *= 2
                    else:
                        gs *= 2
                stored = corr.detach()[:, :, ::gs, ::ds].contiguous().numpy()
                out = dict(kind=np.array(kind), groups=groups, group_stride=gs, depth_stride=ds, channel_stride=cs, first_plane=first_plane,
                           inline_restated=1, corr=stored, R_seed=R_seed, grad_feature=grad[:, ::cs].contiguous().numpy(),
                           grad_err_fp32=grad_err, grad_max_abs=float(g64.abs().max()), min_abs_z=min_abs_z, restated_err=err)
                out.update(META)
                path = os.path.join(HERE, f"g23_groupcorr_{tag}_{kind}_g{groups}.npz")
                np.savez_compressed(path, **out)
                print(f"wrote {path} {os.path.getsize(path) / 1e6:.2f} MB  groups {groups} (stride {gs}) D {D} (stride {ds}) min|Z| {min_abs_z:.3f} "
                      f"restated {err:.1e} grad_err_fp32 {grad_err:.2e} of {float(g64.abs().max()):.2f}")
                assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
