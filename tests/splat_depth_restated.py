"""render_depth_cuda (gs_src/model/decoder/cuda_splatting.py:237-280) restated in torch on the CPU, on top of the
rasteriser's restatement (tests/splat_restated.py): in float64 or float32, differentiable by autograd through the value into the means.

    fake_colour(...)    cuda_splatting.py:250-262: every Gaussian's camera-space z per view, mapped by the mode -> (V,G)
    render_depth(...)   splat_restated.render(use_sh=False) on that value as a (G,3,1) colour over a zero background, channel 0
    with_gradients(...) both restatements of a scene with the gradients of sum(depth * g_depth * kept) in means, covs, opac

Nothing here is taken from the kernels.  The kept mask (splat_scenes.kept) and the comparison bar (splat_restated.bar) are the colour's:
no per-pixel decision depends on a colour, so the same pixels are left out, and no new tolerance is introduced.
"""
import numpy as np
import torch

import splat_restated as R
import splat_scenes as S

MODES = ("depth", "disparity", "relative_disparity", "log")
NAMES = ("means", "covs", "opac")


def fake_colour(means, extrinsics, near, far, mode, dtype=torch.float64):
    """means (G,3) tensor (may require grad), extrinsics (V,4,4) camera-to-world, near / far (V) -> (V,G) in `dtype`, every operation in
    `dtype` and in the reference's order: inverse(extrinsics) . [mean, 1], third component, then the mode."""
    if mode not in MODES:
        raise ValueError(mode)
    ext = torch.as_tensor(extrinsics).to(means.device, dtype)
    near, far = torch.as_tensor(near).to(means.device, dtype)[:, None], torch.as_tensor(far).to(means.device, dtype)[:, None]
    m = means.to(dtype)
    hom = torch.cat([m, torch.ones_like(m[:, :1])], dim=-1)                     # homogenize_points
    cam = torch.einsum("vij,gj->vgi", ext.inverse(), hom)
    value = cam[..., 2]
    if mode == "disparity":
        value = 1 / value
    elif mode == "relative_disparity":                                          # conversions.py:17-27
        eps = 1e-10
        disp_near, disp_far, disp = 1 / (near + eps), 1 / (far + eps), 1 / (value + eps)
        value = 1 - (disp - disp_far) / (disp_near - disp_far + eps)
    elif mode == "log":                                                         # the reference's clamp, as written: min near, max far
        value = value.minimum(near).maximum(far).log()
    return value


def render_depth(means, covs, opac, cams, extrinsics, near, far, H, W, mode, dtype=torch.float64):
    """-> depth (V,H,W), the value (V,G), info as splat_restated.render gives it (one view at a time, joined): the value is a colour of
    its own per view."""
    value = fake_colour(means, extrinsics, near, far, mode, dtype)
    cams = torch.as_tensor(cams)
    planes, infos = [], []
    for v in range(cams.shape[0]):
        colour = value[v][:, None, None].expand(-1, 3, 1)
        image, info = R.render(means, covs, colour, opac, cams[v:v + 1], torch.zeros(1, 3), H, W, dtype, use_sh=False)
        planes.append(image[0, 0])
        infos.append(info)
    info = dict(ok=torch.cat([i["ok"] for i in infos]), pixel=torch.cat([i["pixel"] for i in infos]), keys=[i["keys"][0] for i in infos],
                stopped=torch.cat([i["stopped"] for i in infos]), n_contrib=torch.cat([i["n_contrib"] for i in infos]))
    return torch.stack(planes), value, info


def g_depth(sc):
    """The scene's depth weights: the first channel of its image weights."""
    return np.ascontiguousarray(sc["g_image"][:, 0])


def restate(sc, mode, dtype=torch.float64, grad=True):
    leaves = [torch.from_numpy(sc[k]).clone().requires_grad_(grad) for k in NAMES]
    depth, value, info = render_depth(*leaves, sc["cams"], sc["extrinsics"], sc["near"], sc["far"], sc["H"], sc["W"], mode, dtype)
    out = dict(depth=depth.detach().numpy(), values=value.detach().numpy(), info=info)
    if dtype == torch.float64:
        out["kept"] = S.kept(info).numpy()
    return out, depth, leaves


def with_gradients(sc, mode):
    """(o64, o32, weights): both restatements with the gradients of sum(depth * g_depth * kept); the kept mask is the float64 run's."""
    o64, d64, l64 = restate(sc, mode, torch.float64)
    w = torch.from_numpy(g_depth(sc) * o64["kept"].astype(np.float32))
    o64["grads"] = [g.numpy() for g in torch.autograd.grad((d64 * w.double()).sum(), l64, allow_unused=True, materialize_grads=True)]
    o32, d32, l32 = restate(sc, mode, torch.float32)
    o32["grads"] = [g.numpy() for g in torch.autograd.grad((d32 * w).sum(), l32, allow_unused=True, materialize_grads=True)]
    return o64, o32, w.numpy()


_CACHE = {}


def reference(kind, name, mode):
    """Computed once per (scene, mode) and shared, unchanged.  kind: "case", "special" or "edge" of splat_scenes."""
    key = (kind, name, mode)
    if key not in _CACHE:
        sc = {"case": lambda: S.scene(**S.CASES[name]), "special": lambda: S.SPECIAL[name](), "edge": lambda: S.EDGES[name]()}[kind]()
        _CACHE[key] = (sc,) + with_gradients(sc, mode)
    return _CACHE[key]
