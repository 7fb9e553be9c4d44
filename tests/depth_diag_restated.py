"""Float64 restatement of the gt_depth branch of the reference's backproject_Weigh (mvsdet.py:1435-1484), shared by
test_depth_diag_host.py, test_depth_diag_integration.py and test_gpu_depth_diag.py.

It restates the REDUCTIONS, not the decisions: the voxel -> pixel indices x, y, the depth z (mvsdet.py:1386-1390), the window weight
w_iv and the refined validity valid' (:1393-1428) come from the oracle (stage 3 is pinned to it bit for bit elsewhere), the resized
ground truth g from ATen-CPU's F.interpolate, as the reference calls it (:1437).  Every term -- difference and square -- is formed in
fp32 as the reference forms it; the sums are exact (math.fsum of the fp32 terms), so what is left between this file and a
summation in any order is the summation's own rounding.
"""
import math

import numpy as np

F32 = np.float32


def original_valid(x, y, z, h, w):
    """mvsdet.py:1391."""
    return (x >= 0) & (y >= 0) & (x < w) & (y < h) & (z > 0)


def resize_aten_cpu(gt_depth, h, w):
    """mvsdet.py:1437-1439 with ATen-CPU.  gt_depth: torch tensor or array (N,Hg,Wg), strides kept -> (N,h,w) float32 array."""
    import torch
    import torch.nn.functional as F
    t = gt_depth if isinstance(gt_depth, torch.Tensor) else torch.from_numpy(np.asarray(gt_depth))
    return F.interpolate(t.detach().cpu().unsqueeze(1), size=(h, w), mode="bilinear").squeeze(1).numpy()


def gt_window(z, g, vz):
    """(z > g - vz) & (z < g + vz) with the fp32 edges the reference forms (:1470-1471)."""
    vz = F32(vz)
    with np.errstate(invalid="ignore"):
        return (z > (g - vz).astype(F32)) & (z < (g + vz).astype(F32))


def summation_bound(n):
    """Relative distance between an fp32 summation of n non-negative terms in any pairwise / sequential-by-blocks order (plus the
    final division and one rounding of the result) and the exact sum: (ceil(log2 n) + 3) * 2^-24."""
    return (math.ceil(math.log2(max(int(n), 2))) + 3) * 2.0 ** -24


def restate(x, y, z, g, weight, valid2, depth_mean, vz):
    """x, y (N,V) int; z, weight (N,V) float32; valid2 (N,V) bool; g, depth_mean (N,h,w) float32 ->
    dict(scalars (2) f32, per_view (N,4) f32, sums (N,6) f64, n_skipped, n_gap_terms, n_rmse_terms)."""
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    z, weight = np.asarray(z, F32), np.asarray(weight, F32)
    g, depth_mean = np.asarray(g, F32), np.asarray(depth_mean, F32)
    valid2 = np.asarray(valid2).astype(bool).reshape(z.shape)
    N, V = z.shape
    h, w = g.shape[1:]
    sums = np.zeros((N, 6), np.float64)
    per_view = np.zeros((N, 4), F32)
    for i in range(N):
        ov = original_valid(x[i], y[i], z[i], h, w)
        gt_valid = np.zeros(V, bool)
        gt_valid[ov] = gt_window(z[i][ov], g[i][y[i][ov], x[i][ov]], vz)                  # :1468-1471
        t = gt_valid[ov].astype(F32) - weight[i][ov]                                      # :1473, fp32
        t2 = (t * t).astype(F32)
        with np.errstate(invalid="ignore"):
            mask = g[i] > 0                                                               # :1444 (NaN stays out)
        e = depth_mean[i][mask] - g[i][mask]                                              # :1445, fp32
        e2 = (e * e).astype(F32)
        n_orig, n_valid, n_gt = int(ov.sum()), int(valid2[i].sum()), int(gt_valid.sum())
        n_neq = int((gt_valid != valid2[i]).sum())
        sums[i] = [_fsum(t2), n_orig, n_valid, _fsum(e2), int(mask.sum()), n_neq]
        per_view[i, 0] = F32(sums[i, 0] / n_orig) if n_valid > 0 else F32(np.nan)        # :1464 skips a view without valid'
        per_view[i, 1] = F32((n_orig - n_gt) / V)                                         # :1477 (gt_valid is a subset of original_valid)
        per_view[i, 2] = F32(n_neq / V)                                                   # :1478
        per_view[i, 3] = F32(n_orig - n_valid)                                            # :1479
    kept = [i for i in range(N) if sums[i, 2] > 0]
    acc = F32(0)
    for i in kept:                                                                        # :1484 sum(gap_all) / len(gap_all), fp32
        acc = F32(acc + per_view[i, 0])
    gap_all = F32(acc / F32(len(kept))) if kept else F32(np.nan)
    n_mask = sums[:, 4].sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = F32(np.float64(_fsum(sums[:, 3])) / np.float64(n_mask))                    # empty mask: 0 / 0 = NaN
    return dict(scalars=np.array([gap_all, rmse], F32), per_view=per_view, sums=sums, n_skipped=N - len(kept),
                n_gap_terms=int(sums[kept, 1].sum()) if kept else 0, n_rmse_terms=int(n_mask))


def _fsum(a):
    a = np.asarray(a, np.float64).ravel()
    if not np.isfinite(a).all():
        return float(a.sum())
    return math.fsum(a.tolist())


def margins(x, y, z, g, vz):
    """(smallest distance of an original_valid voxel's z to an edge g -+ vz of its ground-truth window, smallest positive resized
    value): the two decisions of the branch that hang on g.  inf where there is nothing to measure."""
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    h, w = g.shape[1:]
    vz = F32(vz)
    best = np.inf
    for i in range(z.shape[0]):
        ov = original_valid(x[i], y[i], z[i], h, w)
        gi = g[i][y[i][ov], x[i][ov]]
        zi = z[i][ov].astype(np.float64)
        with np.errstate(invalid="ignore"):
            d = np.minimum(np.abs(zi - (gi - vz).astype(F32)), np.abs(zi - (gi + vz).astype(F32)))
        d = d[np.isfinite(d)]
        if d.size:
            best = min(best, float(d.min()))
    with np.errstate(invalid="ignore"):
        pos = g[g > 0]
    return best, (float(pos.min()) if pos.size else np.inf)
