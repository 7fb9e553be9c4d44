"""Ground-truth depth maps for the depth-diagnostics tests, made from the integer LCG of tests/golden/lcg.py so that none is stored:
a smooth surface near the first depth candidate plus noise, rectangular holes of exact zeros larger than the resize footprint, and
(optionally) one view that is all zeros.  `plant` then moves single source pixels until every decision that hangs on the resized map
has a margin: no original_valid voxel has z within WINDOW_MARGIN of an edge g -+ vz of its window, no resized value lies in
(0, POSITIVE_MARGIN).  The moved pixels are returned (and stored in the fixture), so a map is rebuilt from its seed and that list.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from lcg import lcg_uniform  # noqa: E402

from depth_diag_restated import F32, original_valid, resize_aten_cpu  # noqa: E402

WINDOW_MARGIN = 1e-4      # asserted; `plant` works to twice that
POSITIVE_MARGIN = 1e-5
BUMP = 1.0 / 1024         # metres per step, exact in fp32


def base_gt(first_candidate, Hg, Wg, seed, zero_view=None, holes=2, noise=0.03):
    """first_candidate (N,h,w) float32 -> gt (N,Hg,Wg) float32: its 3x3 box mean (float64), sampled at the nearest pixel, plus
    `noise` * U(-1,1), at least 0.1 m; `holes` zero rectangles per view; view `zero_view` all zeros."""
    c = np.asarray(first_candidate, np.float64)
    N, h, w = c.shape
    p = np.pad(c, ((0, 0), (1, 1), (1, 1)), mode="edge")
    smooth = sum(p[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    ys = np.minimum(np.arange(Hg) * h // Hg, h - 1)
    xs = np.minimum(np.arange(Wg) * w // Wg, w - 1)
    r = lcg_uniform(N * Hg * Wg + 4 * N * holes, seed).astype(np.float64)
    gt = smooth[:, ys][:, :, xs] + noise * r[:N * Hg * Wg].reshape(N, Hg, Wg)
    gt = np.maximum(gt, 0.1).astype(F32)
    u = (r[N * Hg * Wg:].reshape(N, holes, 4) + 1.0) / 2.0                      # [0,1)
    hh = min(Hg, 3 * -(-Hg // h) + 3)                                          # three footprints and a border
    hw = min(Wg, 3 * -(-Wg // w) + 3)
    for i in range(N):
        for k in range(holes):
            y0 = int(u[i, k, 0] * (Hg - hh + 1))
            x0 = int(u[i, k, 1] * (Wg - hw + 1))
            gt[i, y0:y0 + hh, x0:x0 + hw] = 0.0
    if zero_view is not None:
        gt[zero_view] = 0.0
    return gt


def apply_bumps(gt, bumps):
    """bumps (K,4) int: view, row, column, steps of BUMP."""
    for i, Y, X, k in np.asarray(bumps, np.int64).reshape(-1, 4):
        gt[i, Y, X] = F32(gt[i, Y, X] + F32(k * BUMP))
    return gt


def _taps(d, n_in, n_out):
    if n_in == n_out:
        return d, d
    src = max((n_in / n_out) * (d + 0.5) - 0.5, 0.0)
    i0 = min(int(np.floor(src)), n_in - 1)
    lo = max(i0 - 1, 0)                                                         # one more either side: the fp32 index may round the other way
    return lo, min(i0 + 2, n_in - 1)


def violations(x, y, z, g, vz, factor=2.0):
    """Output pixels (view, y, x) at which a decision lacks `factor` times its margin."""
    h, w = g.shape[1:]
    vz = F32(vz)
    bad = set()
    for i in range(z.shape[0]):
        ov = original_valid(x[i], y[i], z[i], h, w)
        yy, xx = y[i][ov].astype(np.int64), x[i][ov].astype(np.int64)
        gi = g[i][yy, xx]
        zi = z[i][ov].astype(np.float64)
        with np.errstate(invalid="ignore"):
            d = np.minimum(np.abs(zi - (gi - vz).astype(F32)), np.abs(zi - (gi + vz).astype(F32)))
            near = d < factor * WINDOW_MARGIN
        bad.update((i, int(a), int(b)) for a, b in zip(yy[near], xx[near]))
        with np.errstate(invalid="ignore"):
            tiny = (g[i] > 0) & (g[i] < factor * POSITIVE_MARGIN)
        bad.update((i, int(a), int(b)) for a, b in zip(*np.nonzero(tiny)))
    return sorted(bad)


def plant(gt, x, y, z, h, w, vz, max_rounds=40):
    """Move source pixels of gt (in place) until no decision lacks its margin -> bumps (K,4) int32.  Zero pixels (holes) stay zero."""
    bumps = []
    Hg, Wg = gt.shape[1:]
    for rnd in range(max_rounds):
        g = resize_aten_cpu(gt, h, w)
        bad = violations(x, y, z, g, vz)
        if not bad:
            return np.asarray(bumps, np.int32).reshape(-1, 4)
        for i, py, px in bad:
            ya, yb = _taps(py, Hg, h)
            xa, xb = _taps(px, Wg, w)
            moved = False
            for Y in range(ya, yb + 1):
                for X in range(xa, xb + 1):
                    if gt[i, Y, X] > 0:
                        k = 1 + (rnd + Y + 2 * X) % 5
                        gt[i, Y, X] = F32(gt[i, Y, X] + F32(k * BUMP))
                        bumps.append((i, Y, X, k))
                        moved = True
            if not moved:
                raise RuntimeError(f"depth_diag_planted: pixel {(i, py, px)} lies in a hole and a voxel sits on its window's edge")
    raise RuntimeError("depth_diag_planted: margins not reached")
