"""The Gaussian adapter a second time, in torch on the CPU (float64 or float32, differentiable by autograd): the formulas of
GaussianAdapter.forward (gs_src/model/encoder/common/gaussian_adapter.py:50-98), of quaternion_to_matrix / build_covariance
(gaussians.py:8-44), of get_world_rays (geometry/projection.py:74-114) and of the offset lines mvsdet.py:576-578, restated -- not the
kernel's code, not the reference's.  The rotation of the harmonics is an INPUT here too (blocks per view); `sh_rotation_blocks` is this
file's own float64 builder: a least-squares solve over many random directions of splat_restated.sh_basis.
"""
import numpy as np
import torch

import splat_restated as R

EPS = 1e-8
ROT_OFF = (0, 1, 10, 35, 84, 165)      # first float of degree l's block; ROT_OFF[L + 1] floats in all


def degree_of(d_sh):
    return {1: 0, 4: 1, 9: 2, 16: 3, 25: 4}[int(d_sh)]


def sh_mask(d_sh, dtype=torch.float64):
    m = torch.ones(d_sh, dtype=dtype)
    for l in range(1, degree_of(d_sh) + 1):
        m[l * l:(l + 1) * (l + 1)] = 0.1 * 0.25 ** l
    return m


def sh_rotation_blocks(C, d_sh, seed=5, n_dirs=64):
    """C (V,3,3) rotations (any float array) -> (V, ROT_OFF[L + 1]) float64: per view and degree the (2l+1)^2 block D_l, row-major,
    with sum_j (D c)_j Y_j(C d) = sum_j c_j Y_j(d) for every direction d, i.e. D_l^T Y_l(C d) = Y_l(d): solved in the least-squares
    sense over n_dirs random directions (the system is consistent, so the solution is exact to rounding)."""
    C = np.asarray(C, np.float64)
    L = degree_of(d_sh)
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(n_dirs, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Yd = R.sh_basis(torch.from_numpy(d), d_sh).numpy()                        # (n, d_sh)
    out = np.zeros((C.shape[0], ROT_OFF[L + 1]))
    for v in range(C.shape[0]):
        Ycd = R.sh_basis(torch.from_numpy(d @ C[v].T), d_sh).numpy()          # Y(C d)
        for l in range(L + 1):
            s = slice(l * l, (l + 1) * (l + 1))
            D = np.linalg.lstsq(Ycd[:, s], Yd[:, s], rcond=None)[0]           # one row per direction: Y(C d)^T D = Y(d)^T
            out[v, ROT_OFF[l]:ROT_OFF[l + 1]] = D.reshape(-1)
    return out


def blocks_to_matrix(blocks, d_sh):
    """(V, ROT_OFF[L + 1]) -> (V, d_sh, d_sh) block-diagonal matrices (tensor of the blocks' dtype)."""
    blocks = torch.as_tensor(blocks)
    L = degree_of(d_sh)
    M = torch.zeros(blocks.shape[0], d_sh, d_sh, dtype=blocks.dtype)
    for l in range(L + 1):
        n = 2 * l + 1
        M[:, l * l:l * l + n, l * l:l * l + n] = blocks[:, ROT_OFF[l]:ROT_OFF[l + 1]].reshape(-1, n, n)
    return M


def quaternion_to_matrix(q):
    i, j, k, r = q.unbind(-1)
    two_s = 2.0 / ((q * q).sum(-1) + EPS)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def pixel_gaussians(extrinsics, intrinsics, raw, depth, opacity, h, w, s_min, s_max, d_sh, sh_rot, dtype=torch.float64):
    """extrinsics (V,4,4), intrinsics (V,3,3), raw (V,R,S,9 + 3 d_sh), depth (V,R), opacity (V,R), sh_rot (V, ROT_OFF[L + 1]): tensors
    (leaves may require grad; cast to `dtype` inside autograd) -> dict of means (G,3), covariances (G,3,3), harmonics (G,3,d_sh),
    opacities (G), scales (G,3), rotations (G,4), G = V R S in (v, r, s) order."""
    E, K, t, depth, opacity, sh_rot = (torch.as_tensor(a).to(dtype) for a in (extrinsics, intrinsics, raw, depth, opacity, sh_rot))
    V, Rn, S, _ = t.shape
    assert Rn == h * w
    r = torch.arange(Rn)
    col, row = (r % w).to(dtype), (r // w).to(dtype)
    pix = torch.tensor([1.0 / w, 1.0 / h], dtype=dtype)
    centre = torch.stack([(col + 0.5) / w, (row + 0.5) / h], -1)                              # (R,2)
    xy = centre[None, :, None, :] + (torch.sigmoid(t[..., 0:2]) - 0.5) * pix                    # (V,R,S,2)
    # scales
    K2 = torch.linalg.inv(K[:, :2, :2])
    mult = 0.1 * (K2 @ pix).sum(-1)                                                             # (V)
    sc = (s_min + (s_max - s_min) * torch.sigmoid(t[..., 2:5])) * depth[:, :, None, None] * mult[:, None, None, None]
    # rotation
    q = t[..., 5:9]
    q = q / (q.norm(dim=-1, keepdim=True) + EPS)
    Rq = quaternion_to_matrix(q)
    C = E[:, :3, :3]
    inner = Rq @ torch.diag_embed(sc) @ torch.diag_embed(sc).transpose(-1, -2) @ Rq.transpose(-1, -2)
    Cb = C[:, None, None]
    cov = Cb @ inner @ Cb.transpose(-1, -2)
    # mean
    Ki = torch.linalg.inv(K)
    hom = torch.cat([xy, torch.ones_like(xy[..., :1])], -1)
    d = torch.einsum("vij,vrsj->vrsi", Ki, hom)
    d = d / d.norm(dim=-1, keepdim=True)
    dw = torch.einsum("vij,vrsj->vrsi", C, d)
    mean = E[:, None, None, :3, 3] + dw * depth[:, :, None, None]
    # harmonics
    c = t[..., 9:].reshape(V, Rn, S, 3, d_sh) * sh_mask(d_sh, dtype)
    D = blocks_to_matrix(sh_rot, d_sh)
    harm = torch.einsum("vij,vrscj->vrsci", D, c)
    G = V * Rn * S
    return dict(means=mean.reshape(G, 3), covariances=cov.reshape(G, 3, 3), harmonics=harm.reshape(G, 3, d_sh),
                opacities=opacity[:, :, None].expand(V, Rn, S).reshape(G), scales=sc.reshape(G, 3),
                rotations=q.reshape(G, 4))


def bar(x64, x32):
    return R.bar(x64, x32)


# ------------------------------------------------------------------------------------------- seeded inputs
def rotation(rng, lo=0.4, hi=2.6):
    """A proper rotation by an angle in [lo, hi] rad about a random axis: well away from the identity."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(lo, hi)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def case(seed, V, h, w, S, d_sh, shared_k=False, width=None):
    """Inputs of one case, float32 numpy: raw ~ N(0, 1.5) with quaternion norm >= 0.1, depths in [0.3, 5], proper rotations away from
    the identity, a non-square K with skew per view (or shared)."""
    rng = np.random.RandomState(seed)
    Rn, C = h * w, 9 + 3 * d_sh
    raw = rng.normal(size=(V, Rn, S, C)) * 1.5
    qn = np.linalg.norm(raw[..., 5:9], axis=-1, keepdims=True)
    raw[..., 5:9] *= np.maximum(qn, 0.1) / np.maximum(qn, 1e-12)
    ext = np.zeros((V, 4, 4))
    K = np.zeros((V, 3, 3))
    for v in range(V):
        ext[v, :3, :3] = rotation(rng)
        ext[v, :3, 3] = rng.uniform(-1, 1, 3)
        ext[v, 3, 3] = 1
        K[v] = [[rng.uniform(0.8, 1.1), rng.uniform(-0.02, 0.02), rng.uniform(0.45, 0.55)], [0, rng.uniform(1.0, 1.4), rng.uniform(0.45, 0.55)],
                [0, 0, 1]]
    if shared_k:
        K[:] = K[0]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(V=V, h=h, w=w, S=S, d_sh=d_sh, raw=f32(raw), depth=f32(rng.uniform(0.3, 5.0, (V, Rn))), opacity=f32(rng.uniform(0, 1, (V, Rn))),
                extrinsics=f32(ext), intrinsics=f32(K), s_min=0.5, s_max=15.0, seed=seed)


FIELDS = ("means", "covariances", "harmonics")


def loss_weights(seed, sizes):
    rng = np.random.RandomState(seed + 1000)
    return {k: rng.normal(size=s).astype(np.float32) for k, s in sizes.items()}


def restate(c, sh_rot, dtype, weights=None):
    """The restatement on a case with the given blocks -> (outputs as numpy, gradients of sum_field sum(field * weight) in raw and depth
    or None)."""
    raw = torch.from_numpy(c["raw"]).clone().requires_grad_(weights is not None)
    depth = torch.from_numpy(c["depth"]).clone().requires_grad_(weights is not None)
    out = pixel_gaussians(c["extrinsics"], c["intrinsics"], raw, depth, c["opacity"], c["h"], c["w"], c["s_min"], c["s_max"], c["d_sh"],
                          sh_rot, dtype)
    grads = None
    if weights is not None:
        loss = sum((out[k] * torch.from_numpy(weights[k]).to(dtype)).sum() for k in FIELDS)
        grads = [g.numpy() for g in torch.autograd.grad(loss, [raw, depth])]
    return {k: v.detach().numpy() for k, v in out.items()}, grads
