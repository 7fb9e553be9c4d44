"""The composition case of the adapter's tests: two source views of 5 x 7 feature pixels become 70 Gaussians (adapter_restated), one
target camera renders them (splat_restated) and the NVS loss mean((rgb - gt)^2) closes the chain -- both restatements chained, in
float64 and in float32, with the gradients of the loss in raw, depth and opacity.

Per-pixel decisions of the rasteriser closer than splat_scenes.MARGIN are excluded as splat_scenes does it: the render and the ground
truth are multiplied by the float64 run's `kept` mask before the loss, on both sides of every comparison.  Gaussian-level decisions
cannot be drawn again here (the adapter makes the Gaussians), so the seed is one for which all of them have their margin;
test_adapter_host.py asserts that and the 1 % cap on left-out pixels.
"""
import numpy as np
import torch

import adapter_restated as A
import splat_restated as R
import splat_scenes as S

SEED = 2720
H, W = 24, 32
D_SH = 9
NEAR, FAR = 0.5, 8.0


def composition(seed=SEED):
    """-> the adapter case (2 views, 5 x 7, S = 1) with its source cameras looking down +z from near the origin, and the target's
    fields: tgt_extrinsics (1,4,4), tgt_intrinsics (1,3,3), near, far (1), cams (1,40), bg (3), gt (1,3,H,W)."""
    rng = np.random.RandomState(seed)
    c = A.case(seed, 2, 5, 7, 1, D_SH)
    for v in range(2):                                   # gentle source poses so that the target sees the Gaussians
        ext = np.eye(4)
        ext[:3, :3] = A.rotation(rng, 0.05, 0.2)
        ext[:3, 3] = rng.uniform(-0.2, 0.2, 3)
        c["extrinsics"][v] = ext.astype(np.float32)
    c["depth"] = rng.uniform(1.5, 4.0, c["depth"].shape).astype(np.float32)
    c["s_max"] = 6.0
    ext = np.eye(4)
    ext[:3, :3] = A.rotation(rng, 0.05, 0.15)
    ext[:3, 3] = rng.uniform(-0.1, 0.1, 3)
    tgt_ext = ext[None].astype(np.float32)
    tgt_K = np.array([[[0.9, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]], np.float32)
    near, far = np.array([NEAR], np.float32), np.array([FAR], np.float32)
    tgt = dict(tgt_extrinsics=tgt_ext, tgt_intrinsics=tgt_K, near=near, far=far, cams=R.cameras(tgt_ext, tgt_K, near, far, True),
               bg=np.zeros(3, np.float32), gt=rng.uniform(0, 1, (1, 3, H, W)).astype(np.float32))
    return c, tgt


def chain(c, tgt, sh_rot, dtype, kept=None):
    """Both restatements and the loss in `dtype` -> (loss tensor, image, info, leaves [raw, depth, opacity])."""
    leaves = [torch.from_numpy(c[k]).clone().requires_grad_(True) for k in ("raw", "depth", "opacity")]
    g = A.pixel_gaussians(c["extrinsics"], c["intrinsics"], leaves[0], leaves[1], leaves[2], c["h"], c["w"], c["s_min"], c["s_max"],
                          c["d_sh"], sh_rot, dtype)
    image, info = R.render(g["means"], g["covariances"], g["harmonics"], g["opacities"], torch.from_numpy(tgt["cams"]),
                           torch.from_numpy(tgt["bg"])[None], H, W, dtype)
    if kept is None:
        kept = S.kept(info).numpy()
    mask = torch.from_numpy(kept[:, None].astype(np.float32)).to(dtype)
    loss = torch.mean((image * mask - torch.from_numpy(tgt["gt"]).to(dtype) * mask) ** 2)
    return loss, image, info, leaves, kept, g


_CACHE = {}


def composition_reference():
    """Computed once and shared, unchanged: dict(case, tgt, sh_rot (float64 builder), kept, loss64 / loss32, grads64 / grads32 in raw,
    depth, opacity, gaussian_margin)."""
    if "ref" in _CACHE:
        return _CACHE["ref"]
    c, tgt = composition()
    sh_rot = A.sh_rotation_blocks(c["extrinsics"][:, :3, :3], c["d_sh"])
    loss64, image64, info, l64, kept, g64 = chain(c, tgt, sh_rot, torch.float64)
    grads64 = [g.numpy() for g in torch.autograd.grad(loss64, l64)]
    loss32, _, _, l32, _, _ = chain(c, tgt, sh_rot, torch.float32, kept)
    grads32 = [g.numpy() for g in torch.autograd.grad(loss32, l32)]
    margin = S.gaussian_margin(*[g64[k].detach().float().numpy() for k in ("means", "covariances", "harmonics", "opacities")],
                               tgt["cams"], H, W)
    _CACHE["ref"] = dict(case=c, tgt=tgt, sh_rot=sh_rot, kept=kept, loss64=float(loss64.detach()), loss32=float(loss32.detach()), grads64=grads64,
                         grads32=grads32, gaussian_margin=float(margin.min()), image64=image64.detach().numpy())
    return _CACHE["ref"]
