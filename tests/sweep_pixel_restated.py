"""PyTorch-CPU restatement of the per-pixel form of stage 1 -- TEST INFRASTRUCTURE ONLY.

mvs_models/module.py:105-146 with depth_values (B,D,H,W) (the branch at :130-133) and the variance block around it
(mvsdet.py:439-467), in the reference's op order and eager fp32 rounding: oracle/torch_restatement.py::homo_warp with
`depth_values.view(B,1,D,1)` replaced by `depth.reshape(B,1,D,H*W)`.  Pinned against the reference's own output by
fixture G22 (tests/golden/make_goldens_g22.py asserts it at generation time, tests/test_sweep_pixel_host.py on every run).

`variance_pixel_f64` samples and reduces in float64 over the SAME fp32 sampling grid: the yardstick of the gradient tests
(the grid carries no gradient, module.py:115, so its fp32 rounding is part of the function being differentiated).
"""
import torch
import torch.nn.functional as F


def sample_grid(proj, depth, H, W):
    """fp32 sampling grid (B, D*H, W, 2) and the denominators Z (B, D, H*W) of module.py:136.  proj (B,4,4) =
    src_proj @ inverse(ref_proj); depth (B,D,H,W)."""
    B, D = depth.shape[:2]
    # Inputs on a GPU (a test whose volume is too large for the CPU): the grid is still built HERE, on the CPU, and handed to the
    # inputs' device -- it is small (B D H W 2), and it is the arithmetic fixture G22 pins.  torch's GPU kernels do not repeat it:
    # a division by a Python scalar (:137-138) is a multiplication by its reciprocal there, one rounding away in gx and gy.
    dev = depth.device
    proj, depth = proj.cpu(), depth.cpu()
    with torch.no_grad():
        rot, trans = proj[:, :3, :3], proj[:, :3, 3:4]
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        pix = torch.stack((xs.reshape(-1), ys.reshape(-1), torch.ones(H * W)))[None].repeat(B, 1, 1)
        # module.py:126 ray = rot @ pix with the GEMM's inner loop spelled out (oracle/torch_restatement.py explains why)
        x, y = pix[:, 0:1], pix[:, 1:2]
        ray = (rot[:, :, 0:1] * x).double() + rot[:, :, 1:2].double() * y.double()
        ray = ray.float() + rot[:, :, 2:3]
        pts = ray.unsqueeze(2).repeat(1, 1, D, 1) * depth.reshape(B, 1, D, H * W) + trans.view(B, 3, 1, 1)   # :131-135
        xy = pts[:, :2] / pts[:, 2:3]                                           # :136
        gx = xy[:, 0] / ((W - 1) / 2) - 1                                       # :137
        gy = xy[:, 1] / ((H - 1) / 2) - 1                                       # :138
        grid = torch.stack((gx, gy), dim=3).view(B, D * H, W, 2)
    return grid.to(dev), pts[:, 2].to(dev)


def homo_warp_pixel(src_fea, proj, depth):
    """src_fea (B,C,H,W), proj (B,4,4), depth (B,D,H,W) -> (B,C,D,H,W), fp32 as the reference computes it."""
    B, C, H, W = src_fea.shape
    grid, _ = sample_grid(proj, depth, H, W)
    out = F.grid_sample(src_fea, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # :142
    return out.view(B, C, depth.shape[1], H, W)


def _variance(feat, nbr, warp_of):
    N, K = nbr.shape
    D = warp_of.D
    ref = feat.unsqueeze(2).repeat(1, 1, D, 1, 1)                # mvsdet.py:439
    vsum, vsq = ref, ref ** 2                                    # :441-442
    for j in range(K):
        warped = warp_of(feat[nbr[:, j]], j)
        vsum = vsum + warped                                     # :450 (training form: out of place, same values)
        vsq = vsq + warped ** 2                                  # :451
    return vsq / (K + 1) - (vsum / (K + 1)) ** 2                 # :467


def variance_pixel(feat, nbr, proj, depth):
    """feat (N,C,H,W), nbr (N,K) int64, proj (N,K,4,4), depth (N,D,H,W) -> variance (N,C,D,H,W), fp32, differentiable in feat."""
    def warp_of(src, j):
        return homo_warp_pixel(src, proj[:, j], depth)
    warp_of.D = depth.shape[1]
    return _variance(feat, nbr, warp_of)


def variance_pixel_f64(feat, nbr, proj, depth):
    """The same function of `feat` in float64 arithmetic over the fp32 sampling grid; feat may be fp32 or fp64."""
    N, C, H, W = feat.shape
    D = depth.shape[1]
    grids = [sample_grid(proj[:, j], depth, H, W)[0].double() for j in range(nbr.shape[1])]

    def warp_of(src, j):
        return F.grid_sample(src, grids[j], mode="bilinear", padding_mode="zeros", align_corners=False).view(N, C, D, H, W)
    warp_of.D = D
    return _variance(feat.double(), nbr, warp_of)


def homo_warp_pixel_f64(src_fea, proj, depth):
    B, C, H, W = src_fea.shape
    grid = sample_grid(proj, depth, H, W)[0].double()
    return F.grid_sample(src_fea.double(), grid, mode="bilinear", padding_mode="zeros",
                         align_corners=False).view(B, C, depth.shape[1], H, W)
