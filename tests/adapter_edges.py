"""Planted inputs for the Gaussian adapter at the values adapter_restated.case keeps away from: degenerate quaternions, saturated
sigmoids, depths at and around zero, a very large depth.  Plain numpy on top of adapter_restated; imported by test_adapter_host.py
(the restatements alone) and test_gpu_adapter_edges.py (the kernels).

A Gaussian is named (v, r, s): view, pixel, surface; its flat index is (v R + r) S + s.  `planted(name)` starts from
adapter_restated.case(seed, V, h, w, S, d_sh), writes the values of one group onto its Gaussians and returns the case with
{group name: [(v, r, s), ...]}.  Every group has a case of its own (the same seed and sizes: the unplanted Gaussians of all of them
are those of `clean()`), so no group's magnitudes enter another's bar.  A depth belongs to a pixel: a group that plants depths lists all
S Gaussians of each pixel.

`group_bar` is the rule of DESIGN 4.12 (adapter_restated.bar) on the arrays restricted to one group's Gaussians: max|x| and the float32
restatement's own distance come from those rows alone.
"""
import numpy as np
import torch

import adapter_restated as A

SEED, V, H, W, S, D_SH = 160, 2, 5, 7, 2, 4          # 70 Gaussians per view: one full 64-block and a tail of 6
R = H * W
OUT_FIELDS = A.FIELDS + ("scales", "rotations")

# Gaussians at the places where a block's machinery changes: the first and the last of a view, both sides of the 64-Gaussian block
# boundary (g = 63 is (31, 1), g = 64 is (32, 0)), and a few inside
SLOTS = [(0, 0, 0), (0, 31, 1), (0, 32, 0), (1, 34, 1), (1, 31, 1), (1, 32, 0), (0, 17, 1), (1, 10, 0), (0, 34, 0), (1, 0, 1), (0, 5, 0),
         (1, 20, 1)]
PIXELS = [(0, 0), (0, 31), (0, 32), (1, 34), (1, 17)]          # for the depths: first, the block boundary's two pixels, last, inside

ZERO, NEG0 = np.float32(0.0), np.float32(-0.0)
QUATS = {
    "quat_zero": [(ZERO, ZERO, ZERO, ZERO), (ZERO, NEG0, NEG0, ZERO), (NEG0, NEG0, NEG0, NEG0)],
    "quat_underflow": [(1e-24, -2e-24, 3e-24, 1e-24), (1e-30, -2e-30, 3e-30, 1e-30), (0.0, 1e-22, 0.0, 0.0), (0.0, 0.0, 0.0, -1e-22)],
    "quat_near_eps": [(3e-9, -4e-9, 0.0, 0.0), (0.0, 6e-9, 0.0, -8e-9), (6e-8, 0.0, -8e-8, 0.0)],            # norms 5e-9, 1e-8, 1e-7
    "quat_axis": [(0.0, 0.0, 0.0, 2.5), (0.0, 0.0, 0.0, -2.5), (1.0, 0.0, 0.0, 0.0), (6e3, 0.0, -8e3, 0.0), (0.48, -0.6, 0.64, 0.0)],
}
# raw[0:5] (two offsets, three scales): fp32 sigmoid exactly 1 from 16.7 on, expf overflowing to inf at -89 and -104, a denormal
# exp at 88.8; every value of the set stands in an offset slot and in a scale slot at least once
SIGMOIDS = [(16.7, -16.7, 17.0, -17.0, 30.0), (-30.0, 88.8, -89.0, 104.0, -104.0), (104.0, -104.0, 16.7, -16.7, 88.8),
            (-89.0, 30.0, -30.0, 17.0, -17.0), (17.0, -17.0, -30.0, 104.0, -89.0), (88.8, -89.0, 30.0, -104.0, 16.7)]
DEPTHS = {"depth_small": [0.0, -0.0, -1.5, 1e-20, 1e-38], "depth_large": [3e4, 3e4]}
NAMES = tuple(QUATS) + ("sigmoid_saturated",) + tuple(DEPTHS)


def clean(seed=SEED, v=V, h=H, w=W, s=S, d_sh=D_SH):
    return A.case(seed, v, h, w, s, d_sh)


def planted(name):
    """-> (case, {group: [(v, r, s), ...]}) for one of NAMES."""
    c = clean()
    if name in QUATS:
        where = SLOTS[:len(QUATS[name])]
        for (v, r, s), q in zip(where, QUATS[name]):
            c["raw"][v, r, s, 5:9] = np.asarray(q, np.float32)
    elif name == "sigmoid_saturated":
        where = SLOTS[:len(SIGMOIDS)]
        for (v, r, s), t in zip(where, SIGMOIDS):
            c["raw"][v, r, s, 0:5] = np.asarray(t, np.float32)
    else:
        where = []
        for (v, r), d in zip(PIXELS, DEPTHS[name]):
            c["depth"][v, r] = np.float32(d)
            where += [(v, r, s) for s in range(c["S"])]
    return c, {name: where}


def flat(c, gaussians):
    """Flat indices of Gaussians (v, r, s) in (v, r, s) order."""
    Rn, Sn = c["h"] * c["w"], c["S"]
    return np.array(sorted({(v * Rn + r) * Sn + s for v, r, s in gaussians}), np.int64)


def rest(c, groups):
    """The Gaussians no group names, as a list of (v, r, s)."""
    named = {g for gs in groups.values() for g in gs}
    return [(v, r, s) for v in range(c["V"]) for r in range(c["h"] * c["w"]) for s in range(c["S"]) if (v, r, s) not in named]


def rows_of(c, x, idx, per_pixel=False):
    """The rows of x that belong to the Gaussians idx: x is (G, ...), (V,R,S, ...) or, with per_pixel, (V,R) (a depth gradient: the
    pixels of those Gaussians)."""
    x = np.asarray(x)
    G = c["V"] * c["h"] * c["w"] * c["S"]
    if per_pixel:
        return x.reshape(-1)[np.unique(idx // c["S"])]
    return x.reshape(G, -1)[idx]


def group_bar(x64, x32):
    """adapter_restated.bar on arrays already restricted to a group -> (bar, own)."""
    return A.bar(x64, x32)


_REF = {}


def reference(name):
    """Computed once per planted case (or "clean") and shared, unchanged: the case, its groups, the float64 rotation blocks, the weights
    of the linear loss (the same for every case) and both restatements with their gradients."""
    if name not in _REF:
        c, groups = (clean(), {}) if name == "clean" else planted(name)
        _REF[name] = (c, groups) + restated(c)
    return _REF[name]


def restated(c, weights=None):
    """-> (blocks, weights, o64, g64, o32, g32) of a case."""
    G = c["V"] * c["h"] * c["w"] * c["S"]
    blocks = A.sh_rotation_blocks(c["extrinsics"][:, :3, :3], c["d_sh"])
    if weights is None:
        weights = A.loss_weights(c["seed"], dict(means=(G, 3), covariances=(G, 3, 3), harmonics=(G, 3, c["d_sh"])))
    o64, g64 = A.restate(c, blocks, torch.float64, weights)
    o32, g32 = A.restate(c, blocks.astype(np.float32), torch.float32, weights)
    return blocks, weights, o64, g64, o32, g32


def quantities(c, out, grads):
    """Everything a run yields, as (name, array, per_pixel) triples: the five fields and the two gradients."""
    return [(k, out[k], False) for k in OUT_FIELDS] + [("d raw", grads[0], False), ("d depth", grads[1], True)]
