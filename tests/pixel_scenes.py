"""What tests/test_gpu_sweep_pixel.py and tests/test_gpu_groupcorr.py share: the synthetic scene of a shape and the gradient
bound with its check (|g - g64| <= max(1e-4 |g64| + 1.25e-6 max|g64|, 4 x grad_err_fp32), derived in test_gpu_sweep_pixel.py)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from lcg import lcg_uniform  # noqa: E402


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def scene(shape, nbr_table, seed=5):
    """feat (N,C,H,W), nbr (N,K), proj (N,K,4,4) = src_proj @ inverse(ref_proj) of mildly rotated and shifted cameras, plane
    depths (N,D) in [0.6, 4]: CPU tensors.  shape = (N, K, C, D, H, W), nbr_table the (N,K) neighbour ids."""
    N, K, C, D, H, W = shape
    u = lcg_uniform(N * 6 + 1, seed).astype(np.float64)
    Kmat = np.eye(4)
    Kmat[0, 0] = Kmat[1, 1] = 0.9 * W
    Kmat[0, 2], Kmat[1, 2] = (W - 1) / 2, (H - 1) / 2
    E = []
    for n in range(N):
        e = np.eye(4)
        e[:3, :3] = rot(*(0.08 * u[6 * n:6 * n + 3]))
        e[:3, 3] = 0.25 * u[6 * n + 3:6 * n + 6]
        E.append(Kmat @ e)
    nbr = np.array(nbr_table, np.int64)
    proj = np.stack([np.stack([E[nbr[n, j]] @ np.linalg.inv(E[n]) for j in range(K)]) for n in range(N)]).astype(np.float32)
    feat = torch.from_numpy(lcg_uniform(N * C * H * W, seed + 1)).reshape(N, C, H, W)
    depth = torch.from_numpy(np.tile(np.linspace(0.6, 4.0, D, dtype=np.float32), (N, 1)))
    return feat, torch.from_numpy(nbr), torch.from_numpy(proj), depth


def grad_bound(g64, grad_err_fp32):
    return torch.maximum(1e-4 * g64.abs() + 1.25e-6 * g64.abs().max(), torch.full_like(g64, 4.0 * grad_err_fp32))


def check_grad(got, g64, grad_err_fp32, what):
    got = got.detach().double().cpu()
    excess = (got - g64).abs() / grad_bound(g64, grad_err_fp32)
    print(f"{what}: max |g - g64| = {float((got - g64).abs().max()):.3e} (max |g64| {float(g64.abs().max()):.3f}, "
          f"grad_err_fp32 {grad_err_fp32:.2e}), worst ratio to the bound {float(excess.max()):.3f}")
    assert torch.isfinite(got).all() and float(excess.max()) <= 1.0, what
