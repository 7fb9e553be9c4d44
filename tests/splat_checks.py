"""What the Gaussian rasteriser's GPU tests share (test_gpu_splat.py, test_gpu_splat_edges.py): one call of ops.splat.rasterize on a
scene of splat_scenes.py, and the comparison of its image and gradients with the float64 restatement under the bar of DESIGN 4.12 /
4.15 (splat_restated.bar)."""
import numpy as np
import torch

import splat_restated as R

NAMES = ("means", "covs", "sh", "opac")


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def run(sc, gpu, weights=None, max_keys=None, use_sh=True, leaves=None):
    """ops.splat.rasterize on a scene with the scene's own camera block -> image, the four gradients (numpy), the workspace."""
    from mvsdet_amd.ops import splat
    if leaves is None:
        leaves = [dev(sc[k], gpu) for k in NAMES]
    leaves = [t.detach().requires_grad_(True) for t in leaves]
    keys = splat.default_max_keys(sc["G"]) if max_keys is None else max_keys
    image, ws = splat.rasterize(*leaves, dev(sc["cams"], gpu), dev(sc["bg"], gpu), sc["H"], sc["W"], keys, use_sh)
    assert not ws.requires_grad and image.dtype == torch.float32 and tuple(image.shape) == (sc["V"], 3, sc["H"], sc["W"])
    grads = None
    if weights is not None:
        grads = [g.cpu().numpy() for g in torch.autograd.grad((image * dev(weights, gpu)).sum(), leaves)]
    return image.detach().cpu().numpy(), grads, ws


def compare(tag, got, o64, o32, keep=None):
    """got against the float64 value under the bar; prints the figures first."""
    x64, x32 = np.asarray(o64, np.float64), np.asarray(o32, np.float64)
    if keep is not None:
        got, x64, x32 = got[keep], x64[keep], x32[keep]
    bar, own = R.bar(x64, x32)
    err = np.abs(got.astype(np.float64) - x64)
    worst = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    print(f"{tag}: max|x| {np.abs(x64).max():.4g}  kernel-f64 {err.max():.3g}  restated f32-f64 {own:.3g}  worst err/bar {worst:.3f}")
    assert np.isfinite(got).all(), tag
    assert (err <= bar).all(), (tag, worst)


def check_case(sc, o64, o32, w, gpu, use_sh=True):
    image, grads, ws = run(sc, gpu, w, use_sh=use_sh)
    keep = np.broadcast_to(o64["kept"][:, None], image.shape)
    compare("image", image, o64["image"], o32["image"], keep)
    for n, g, g64, g32 in zip(NAMES, grads, o64["grads"], o32["grads"]):
        compare("d " + n, g, g64, g32)
    lower = grads[1][:, [1, 2, 2], [0, 0, 1]]
    assert np.array_equal(bits(lower), np.zeros_like(bits(lower))), "the lower triangle of the covariance gradient is exactly 0"
    return image, grads, ws
