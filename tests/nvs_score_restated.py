"""Restatement of the reference's view-synthesis scores for the tests (test_nvs_score_host.py, test_gpu_nvs_score.py).

What is restated: compute_psnr / compute_ssim / save_rendered_img_Image / save_rendered_depth of the reference's
nerf_utils/save_rendered_img.py:17-44, 178-235 and the reductions of NVSMetric / MVSMetric (mmdet3d/evaluation/metrics/Indoor_NVS.py:94-103,
273-280).  That module imports skimage, cv2 and matplotlib, none of which is installed where this package is developed, so no fixture
could be recorded from the reference's own code and there is no tests/golden file for this: the defaults that
structural_similarity(channel_axis=-1, data_range=1) selects (win_size 7, uniform_filter, sample covariance, K1 0.01, K2 0.03, crop
by 3) are written out instead, twice and independently:

  (a) the scipy form -- uniform_filter(size=7) on whole planes and the crop [3:H-3, 3:W-3], in float64 and in float32.  The
      float32 form follows the reference's own order: skimage keeps float32 images in float32 and averages S with
      mean(dtype=float64); PSNR is torch's float32 `mean` and `log`.
  (b) a direct float64 form that adds the 49 shifted slices of every plane: each 7x7 window taken by plain slicing, no filter and
      no border mode anywhere.

Inputs are made by `scene`: gt uniform in [0,1], pred = clip(gt + 0.1 normal) (PSNR near 20 dB), one quadrant 0.5 in both images --
the flat region where float32 cancels in uxx - ux ux.
"""
import numpy as np
import torch
from scipy.ndimage import uniform_filter

WIN = 7
COV_NORM = WIN * WIN / (WIN * WIN - 1.0)
C1, C2 = (0.01 * 1) ** 2, (0.03 * 1) ** 2


def _s_map(ux, uy, uxx, uyy, uxy):
    vx = COV_NORM * (uxx - ux * ux)
    vy = COV_NORM * (uyy - uy * uy)
    vxy = COV_NORM * (uxy - ux * uy)
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def _check(x, y):
    if x.shape != y.shape:
        raise ValueError("Input images must have the same dimensions.")
    if min(x.shape[0], x.shape[1]) < WIN:
        raise ValueError("win_size exceeds image extent.")


def ssim_plane_filter(x, y, dtype=np.float64):
    """(a): one channel, (H,W) planes."""
    _check(x, y)
    x, y = x.astype(dtype), y.astype(dtype)
    u = lambda a: uniform_filter(a, size=WIN)   # noqa: E731
    S = _s_map(u(x), u(y), u(x * x), u(y * y), u(x * y))
    pad = (WIN - 1) // 2
    return S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64)


def window_means(a):
    """The mean of every 7x7 window that lies inside a (H,W) float64 plane -> (H-6, W-6)."""
    H, W = a.shape
    acc = np.zeros((H - WIN + 1, W - WIN + 1), np.float64)
    for di in range(WIN):
        for dj in range(WIN):
            acc += a[di:di + H - WIN + 1, dj:dj + W - WIN + 1]
    return acc / (WIN * WIN)


def ssim_plane_direct(x, y):
    """(b): one channel, float64."""
    _check(x, y)
    x, y = x.astype(np.float64), y.astype(np.float64)
    m = window_means
    return _s_map(m(x), m(y), m(x * x), m(y * y), m(x * y)).mean()


def compute_ssim(pred, target, form="filter", dtype=np.float64):
    """One (H,W,3) view: the mean of the three channel values (skimage: mssim.mean())."""
    assert pred.shape == target.shape and pred.shape[-1] == 3
    plane = (lambda x, y: ssim_plane_filter(x, y, dtype)) if form == "filter" else ssim_plane_direct
    return np.array([plane(pred[..., c], target[..., c]) for c in range(3)]).mean()


def compute_psnr(pred, target, dtype=torch.float64):
    """One view; the reference's expression on torch tensors of `dtype` (float32: its own order)."""
    p, t = torch.from_numpy(np.ascontiguousarray(pred)).to(dtype), torch.from_numpy(np.ascontiguousarray(target)).to(dtype)
    mse = ((p - t) ** 2).mean()
    return (-10.0 * torch.log(mse) / np.log(10.0)).numpy()


def save_rendered_img_Image(pred, gt, form="filter", f32=False):
    """pred, gt (n_tgt,3,H,W) float32 arrays -> (psnr, ssim, 0) and the per-view (n_tgt,2) values."""
    n = pred.shape[0]
    p, g = pred.transpose(0, 2, 3, 1), gt.transpose(0, 2, 3, 1)
    psnr_total, ssim_total, views = 0, 0, []
    for v in range(n):
        psnr = compute_psnr(p[v], g[v], torch.float32 if f32 else torch.float64)
        ssim = compute_ssim(p[v], g[v], form, np.float32 if f32 else np.float64)
        psnr_total += psnr
        ssim_total += ssim
        views.append((float(psnr), float(ssim)))
    return (float(psnr_total / n), float(ssim_total / n), 0), np.array(views, np.float64)


def save_rendered_depth(pred, gt, f32=False):
    """pred, gt (n_tgt,H,W): the mean over views of mean((pred_v - gt_v)^2) -- the reference's `rmse`, no root."""
    assert pred.shape == gt.shape
    dtype = np.float32 if f32 else np.float64
    rmse = 0
    for v in range(pred.shape[0]):
        rmse += np.mean((pred[v].astype(dtype) - gt[v].astype(dtype)) ** 2)
    return float(rmse / pred.shape[0])


def scene_triple(pred, gt, pred_depth=None, gt_depth=None, form="filter", f32=False):
    """What MVSDet.predict stores for a scene (mvsdet.py:1020-1024) and the per-view values."""
    (psnr, ssim, rmse), views = save_rendered_img_Image(pred, gt, form, f32)
    if pred_depth is not None:
        rmse = save_rendered_depth(pred_depth, gt_depth, f32)
    return (psnr, ssim, rmse), views


def nvs_metric(results):
    """NVSMetric.compute_metrics over [(psnr, ssim, rmse), ...]."""
    return {"psnr": sum(r[0] for r in results) / len(results), "ssim": sum(r[1] for r in results) / len(results),
            "rmse": sum(r[2] for r in results) / len(results)}


def mvs_metric(results):
    """MVSMetric.compute_metrics over [(weight_gap, src_rmse), ...]: the mean of weight_gap is computed and NOT returned -- the dict
    carries the loop variable, the last scene's value."""
    final_weight_gap, final_src_rmse = [], []
    for weight_gap, src_rmse in results:
        final_weight_gap.append(weight_gap)
        final_src_rmse.append(src_rmse)
    final_weight_gap = sum(final_weight_gap) / len(final_weight_gap)
    final_src_rmse = sum(final_src_rmse) / len(final_src_rmse)
    return {"weight_gap": weight_gap, "src_rmse": final_src_rmse}


# ------------------------------------------------------------------------------------------------ inputs
def scene(n, H, W, seed=0, depth=True):
    """-> dict(pred, gt (n,3,H,W) float32 in [0,1]; pred_depth, gt_depth (n,H,W) float32 or None)."""
    rng = np.random.RandomState(1000 * seed + 31 * n + 7 * H + W)
    gt = rng.uniform(0, 1, (n, 3, H, W)).astype(np.float32)
    pred = np.clip(gt + 0.1 * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)
    gt[:, :, :H // 2, :W // 2] = 0.5
    pred[:, :, :H // 2, :W // 2] = 0.5
    out = dict(pred=pred, gt=gt, pred_depth=None, gt_depth=None)
    if depth:
        out["gt_depth"] = rng.uniform(0.5, 6.0, (n, H, W)).astype(np.float32)
        out["pred_depth"] = (out["gt_depth"] + 0.2 * rng.standard_normal((n, H, W))).astype(np.float32)
    return out


_CACHE = {}


def reference(n, H, W, seed=0, depth=True):
    """Computed once per shape and shared, unchanged: the scene and its float64 (a) triple and per-view values."""
    key = (n, H, W, seed, depth)
    if key not in _CACHE:
        sc = scene(n, H, W, seed, depth)
        triple, views = scene_triple(sc["pred"], sc["gt"], sc["pred_depth"], sc["gt_depth"])
        _CACHE[key] = dict(scene=sc, triple=triple, views=views)
    return _CACHE[key]
