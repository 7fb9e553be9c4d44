"""The Gaussian head a second time, in plain torch on the CPU (float64 or float32, differentiable by autograd): the inline lines
mvsdet.py:561-569 (index the chosen views, crop, transposing reshape, cat), process_rgb_raw (:319-333: F.interpolate at a quarter
and the crop) and the constructor's nn.Sequential(ReLU, Linear) (:210-216) as relu + nn.functional.linear, restated -- not the kernel's
code.  `four_pixel_mean` is the closed form the kernel uses for the resize; test_gshead_host.py holds it against F.interpolate.

Notation: N(0, s2) is a normal distribution of variance s2.
"""
import numpy as np
import torch
import torch.nn.functional as F

import adapter_restated as A

SH = {1: 12, 4: 21, 9: 36, 16: 57, 25: 84}        # d_sh -> floats per surface, 9 + 3 d_sh


def bar(x64, x32):
    """The adapter tests' bar: elementwise max(1e-4 |x| + 1.25e-6 max|x|, 4 x the float32 restatement's own largest
    distance from float64) -> (bar, own)."""
    return A.bar(x64, x32)


def process_rgb_raw(images, ids, h, w):
    """mvsdet.py:319-333 for ratio 4: (N,3,Hi,Wi) -> (V, h w, 3)."""
    small = F.interpolate(images[ids], scale_factor=0.25, mode="bilinear")[:, :, :h, :w]
    return small.reshape(small.shape[0], 3, -1).transpose(2, 1)


def four_pixel_mean(images, ids, h, w):
    """0.25 ((I[4y+1][4x+1] + I[4y+1][4x+2]) + (I[4y+2][4x+1] + I[4y+2][4x+2])) -> (V, h w, 3), in the images' dtype."""
    I = images[ids]
    ys, xs = 4 * torch.arange(h) + 1, 4 * torch.arange(w) + 1
    top = I[:, :, ys][:, :, :, xs] + I[:, :, ys][:, :, :, xs + 1]
    bot = I[:, :, ys + 1][:, :, :, xs] + I[:, :, ys + 1][:, :, :, xs + 1]
    return (0.25 * (top + bot)).reshape(I.shape[0], 3, -1).transpose(2, 1)


def rows(feature, depth_coding, ids, h, w, rgb_raw=None):
    """mvsdet.py:561-569 -> (V, h w, C + 1 [+ 3])."""
    V = len(ids)
    out = feature[ids, :, :h, :w].reshape(V, feature.shape[1], -1).transpose(1, 2)
    out = torch.cat([out, depth_coding.reshape(depth_coding.shape[0], 1, -1).transpose(2, 1)[ids]], dim=-1)
    if rgb_raw is not None:
        out = torch.cat([out, rgb_raw], dim=-1)
    return out


def gaussian_head(feature, depth_coding, ids, weight, bias, h, w, S, rgb_raw=None, images=None):
    """Tensors of one dtype -> raw (V, h w, S, M / S)."""
    if images is not None:
        rgb_raw = process_rgb_raw(images, ids, h, w)
    x = rows(feature, depth_coding, ids, h, w, rgb_raw)
    out = F.linear(torch.relu(x), weight, bias)
    return out.reshape(out.shape[0], out.shape[1], S, out.shape[2] // S)


# ------------------------------------------------------------------------------------------- seeded inputs
def plant(rng, a):
    """About a tenth of the entries become exactly 0.0, -0.0 or a small negative, in equal parts; returns the mask of the two zeros."""
    pick = rng.uniform(size=a.shape)
    a[pick < 0.1] = -1e-3 * rng.uniform(0.1, 1.0, size=int((pick < 0.1).sum()))
    a[pick < 0.0667] = -0.0
    a[pick < 0.0333] = 0.0
    return pick < 0.0667


def case(seed, N, ids, C, Hf, Wf, h, w, S, d_sh, rgb=None, depth_dims=4):
    """Inputs of one case, float32 numpy: feature, depth_coding and the rgb ~ N(0, 2) with planted zeros and small negatives, weight
    ~ N(0, 1/K), bias ~ N(0, 1/4).  rgb: None, "rows" (rgb_raw (V,R,3)) or "images" ((N,3,4 Hf,4 Wf) denormalised images)."""
    rng = np.random.RandomState(seed)
    K, M, R, V = C + (1 if rgb is None else 4), S * SH[d_sh], h * w, len(ids)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    c = dict(N=N, ids=np.asarray(ids, np.int64), C=C, K=K, M=M, h=h, w=w, S=S, d_sh=d_sh, seed=seed, rgb=rgb)
    c["feature"] = f32(rng.normal(size=(N, C, Hf, Wf)) * np.sqrt(2.0))
    c["depth_coding"] = f32(rng.normal(size=(N, 1, h, w) if depth_dims == 4 else (N, h, w)) * np.sqrt(2.0))
    c["zeros_feature"] = plant(rng, c["feature"])
    c["zeros_depth"] = plant(rng, c["depth_coding"])
    if rgb == "rows":
        c["rgb_raw"] = f32(rng.normal(size=(V, R, 3)) * np.sqrt(2.0))
        plant(rng, c["rgb_raw"])
    elif rgb == "images":
        c["images"] = f32(rng.normal(size=(N, 3, 4 * Hf, 4 * Wf)) * np.sqrt(2.0))
    c["weight"] = f32(rng.normal(size=(M, K)) / np.sqrt(K))
    c["bias"] = f32(rng.normal(size=M) * 0.5)
    return c


def loss_weight(seed, shape):
    return np.random.RandomState(seed + 1000).normal(size=shape).astype(np.float32)


GRADS = ("feature", "depth_coding", "weight", "bias")


def restate(c, dtype, with_grads=True):
    """The restatement on a case -> (raw as numpy (V,R,S,M/S), dict of the gradients of sum(raw * loss_weight) in feature, depth_coding,
    weight and bias, or None)."""
    leaves = {k: torch.from_numpy(c[k]).to(dtype).requires_grad_(with_grads) for k in GRADS}
    extra = {k: torch.from_numpy(c[k]).to(dtype) for k in ("rgb_raw", "images") if k in c}
    ids = torch.from_numpy(c["ids"])
    out = gaussian_head(leaves["feature"], leaves["depth_coding"], ids, leaves["weight"], leaves["bias"], c["h"], c["w"], c["S"], **extra)
    grads = None
    if with_grads:
        lw = torch.from_numpy(loss_weight(c["seed"], tuple(out.shape))).to(dtype)
        grads = dict(zip(GRADS, [g.numpy() for g in torch.autograd.grad((out * lw).sum(), [leaves[k] for k in GRADS])]))
    return out.detach().numpy(), grads
