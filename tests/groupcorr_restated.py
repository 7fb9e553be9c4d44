"""PyTorch-CPU restatement of the group-wise correlation cost volume -- TEST INFRASTRUCTURE ONLY.

mvs_models/lss_fpn.py:499-506 around this project's warp: per neighbour j, warped_j = the reference-order fp32 warp of
tests/sweep_pixel_restated.py (imported, not edited), reshaped to (N,G,C/G,D,H,W); the product with the reshaped reference
feature and the mean over a group's channels are taken in float64 (or in `dtype`).  Pinned against the reference's own output by
fixture G23 (tests/golden/make_goldens_g23.py asserts it at generation time, tests/test_groupcorr_host.py on every run).

`groupcorr_f64` samples and reduces in float64 over the SAME fp32 sampling grid: the yardstick of the gradient tests (the grid
carries no gradient, module.py:115, so its fp32 rounding is part of the function being differentiated).
"""
import torch
import torch.nn.functional as F

import sweep_pixel_restated as SP


def depth4(depth, H, W):
    """(N,D) plane depths as the (N,D,H,W) map they stand for; a 4-D depth as it is."""
    return depth if depth.dim() == 4 else depth[:, :, None, None].expand(-1, -1, H, W).contiguous()


def _reduce(feat, warped, groups):
    """lss_fpn.py:499-506: feat (N,C,H,W), warped (N,C,D,H,W) -> (N,G,D,H,W)."""
    N, C, D, H, W = warped.shape
    w = warped.reshape(N, groups, C // groups, D, H, W)
    f = feat.reshape(N, groups, C // groups, H, W)
    return torch.mean(f.unsqueeze(3) * w, dim=2)


def groupcorr(feat, nbr, proj, depth, groups, dtype=torch.float64):
    """feat (N,C,H,W), nbr (N,K), proj (N,K,4,4), depth (N,D) or (N,D,H,W) -> (N,K,G,D,H,W) of `dtype`: the fp32 warp, then
    product and mean in `dtype`."""
    N, C, H, W = feat.shape
    d4 = depth4(depth, H, W)
    out = [_reduce(feat.to(dtype), SP.homo_warp_pixel(feat[nbr[:, j]], proj[:, j], d4).to(dtype), groups) for j in range(nbr.shape[1])]
    return torch.stack(out, dim=1)


def groupcorr_f64(feat, nbr, proj, depth, groups):
    """The same function of `feat` in float64 arithmetic end to end over the fp32 sampling grid; differentiable in feat."""
    N, C, H, W = feat.shape
    d4 = depth4(depth, H, W)
    D = d4.shape[1]
    f = feat.double()
    out = []
    for j in range(nbr.shape[1]):
        grid = SP.sample_grid(proj[:, j], d4, H, W)[0].double()
        w = F.grid_sample(f[nbr[:, j]], grid, mode="bilinear", padding_mode="zeros", align_corners=False).view(N, C, D, H, W)
        out.append(_reduce(f, w, groups))
    return torch.stack(out, dim=1)
