"""Float64-accumulating restatement of the reference's two depth objectives, shared by tests/golden/make_goldens_g24.py,
test_depth_loss_host.py and test_gpu_depth_loss.py.

  l1         MVSDet.depth_loss_func_new (mvsdet.py:893-915), one scene: g = F.interpolate(gt, (h,w), 'bilinear'), mask = g > 0,
             mean |est - g| over the mask
  smooth_l1  mvsnet_loss (mvs_models/mvsnet.py:292-294): mask > 0.5, smooth-L1 with beta = 1, mean

Every term is formed in fp32 in the reference's order; the sum is exact (math.fsum of the fp32 terms) and divided in float64, one
rounding to fp32 at the end.  The gradient is the reference's autograd spelled out: fl32(g_loss / count) * sign(est - g) (mean's
backward, then abs's: sign(0) = 0), or * clamp(d, -1, 1) for smooth-L1.

`resize` restates at::native::compute_source_index_and_lambda (UpSample.h) + the bilinear blend in fp32 numpy, each operation
rounded once: scale = fl(in / out); src = fma(scale, dst + 0.5, -0.5) clamped at 0; i0 = floor(src) capped at in - 1; l1 = src - i0;
value = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d).  Equal sizes are the identity.
"""
import math

import numpy as np

F32 = np.float32
L1, SMOOTH_L1 = 0, 1


def resize_taps(out, inn):
    """-> i0, i1 (int64), l0, l1 (float32) for every destination index 0..out-1 of an axis resized from `inn`."""
    dst = np.arange(out)
    if inn == out:
        return dst, dst.copy(), np.ones(out, F32), np.zeros(out, F32)
    scale = F32(F32(inn) / F32(out))                                    # area_pixel_compute_scale
    centre = (dst.astype(F32) + F32(0.5)).astype(F32)
    src = (np.float64(scale) * centre.astype(np.float64) - 0.5).astype(F32)   # one fused multiply-add: the product is exact in float64
    src = np.maximum(src, F32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), inn - 1)
    l1 = np.clip((src - i0.astype(F32)).astype(F32), F32(0), F32(1))
    i1 = i0 + (i0 < inn - 1)
    return i0, i1, (F32(1) - l1).astype(F32), l1


def resize(gt, h, w):
    """gt (N,Hg,Wg) float32 array -> (N,h,w) float32, ATen's upsample_bilinear2d(align_corners=False) op by op."""
    gt = np.asarray(gt, F32)
    y0, y1, ly0, ly1 = resize_taps(h, gt.shape[1])
    x0, x1, lx0, lx1 = resize_taps(w, gt.shape[2])
    a, b = gt[:, y0][:, :, x0], gt[:, y0][:, :, x1]
    c, d = gt[:, y1][:, :, x0], gt[:, y1][:, :, x1]
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    lx0, lx1 = lx0[None, None, :], lx1[None, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        top = ((lx0 * a).astype(F32) + (lx1 * b).astype(F32)).astype(F32)
        bot = ((lx0 * c).astype(F32) + (lx1 * d).astype(F32)).astype(F32)
        return ((ly0 * top).astype(F32) + (ly1 * bot).astype(F32)).astype(F32)


def _fsum(a):
    a = np.asarray(a, np.float64).ravel()
    if not np.isfinite(a).all():
        with np.errstate(invalid="ignore"):
            return float(a.sum())
    return math.fsum(a.tolist())


def restate(est, gt, mask=None, kind=L1, g_loss=1.0):
    """est (N,h,w); gt (N,Hg,Wg) (l1) or (N,h,w) (smooth_l1); mask (N,h,w) for smooth_l1 ->
    dict(loss f32, count int, grad (N,h,w) f32, inside (N,h,w) bool, g the target map, d est - g inside the mask (0 outside))."""
    est = np.asarray(est, F32)
    N, h, w = est.shape
    with np.errstate(invalid="ignore"):
        if kind == L1:
            g = resize(gt, h, w)
            inside = g > 0                                                  # NaN stays out (mvsdet.py:912)
        else:
            g = np.asarray(gt, F32)
            inside = np.asarray(mask, F32) > F32(0.5)                       # mvsnet.py:293
        d = np.zeros_like(est)
        d[inside] = (est[inside] - g[inside]).astype(F32)
        a = np.abs(d[inside])
        if kind == L1:
            terms = a
        else:
            terms = np.where(a < 1, (F32(0.5) * a * a).astype(F32), (a - F32(0.5)).astype(F32))
        count = int(inside.sum())
        with np.errstate(divide="ignore"):
            loss = F32(np.float64(_fsum(terms)) / np.float64(count))         # empty mask: 0 / 0 = NaN
        grad = np.zeros_like(est)
        if count:
            per_term = F32(F32(g_loss) / F32(count))
            s = np.sign(d[inside]) if kind == L1 else np.clip(d[inside], F32(-1), F32(1))
            s = np.where(np.isnan(d[inside]) & (kind == L1), F32(0), s)     # ATen's sgn of NaN is 0
            grad[inside] = (per_term * s.astype(F32)).astype(F32)
    return dict(loss=loss, count=count, grad=grad, inside=inside, g=g, d=d)


def margins(est, gt, mask=None, kind=L1):
    """The decisions that could hang on one ulp: (smallest positive target value, smallest |est - g| inside the mask) for l1,
    (smallest |mask - 0.5|, smallest ||d| - 1| inside the mask) for smooth_l1.  inf where there is nothing to measure."""
    r = restate(est, gt, mask, kind)
    d = np.abs(r["d"][r["inside"]]).astype(np.float64)
    if kind == L1:
        with np.errstate(invalid="ignore"):
            pos = r["g"][r["g"] > 0]
        return (float(pos.min()) if pos.size else np.inf), (float(d.min()) if d.size else np.inf)
    m = np.abs(np.asarray(mask, np.float64) - 0.5)
    return float(m.min()), (float(np.abs(d - 1).min()) if d.size else np.inf)
