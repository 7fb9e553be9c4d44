"""Gaussian adapter (csrc/adapter.hip): the pixel Gaussians the rasteriser renders -- GaussianAdapter.forward
(gs_src/model/encoder/common/gaussian_adapter.py:50-98) with the offset lines of mvsdet.py:576-578.

The names live in this module only (`ops.adapter.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from ._common import _NS, _lib, camera_inputs, req, stream

ADAPTER_CAM = 192         # floats per view: C 9, origin 3, K^-1 9, multiplier, 2 unused, rotation blocks of the harmonics 165, 3 unused
ADAPTER_ROT = 24          # first float of the rotation blocks
ADAPTER_SH = (1, 4, 9, 16, 25)


def rotation_floats(d_sh: int) -> int:
    """sum_{l <= L} (2l + 1)^2: the floats of one view's rotation blocks, degree after degree."""
    L = ADAPTER_SH.index(d_sh)
    return sum((2 * l + 1) ** 2 for l in range(L + 1))


def row_floats(d_sh: int) -> int:
    return 9 + 3 * d_sh


def _d_sh(name: str, sh_degree: int) -> int:
    if not 0 <= int(sh_degree) <= 4:
        raise ValueError(f"{name}: sh_degree = {sh_degree} must be 0 .. 4")
    return (int(sh_degree) + 1) ** 2


# ------------------------------------------------------------------------------------------- cameras
@torch.library.custom_op(f"{_NS}::adapter_cameras", mutates_args=(), device_types="cuda")
def adapter_cameras(extrinsics: Tensor, intrinsics: Tensor, h: int, w: int, sh_degree: int, sh_rot: Optional[Tensor] = None) -> Tensor:
    """extrinsics (V,4,4) camera-to-world, intrinsics (V,3,3) normalised -> cams (V,192): C_v, the origin, K_v^-1, the scale multiplier
    of an h x w map and the rotation blocks D_l of the harmonics.  sh_rot None: the blocks that are right for the basis this project
    renders with (csrc/sh_basis.h); sh_rot (V, rotation_floats(d_sh)): the caller's blocks, row-major, degree after degree (degree 0
    included), applied as given.  One launch of one thread per view, float64 inside, rounded once; nothing returns to the host."""
    extrinsics, intrinsics, V, (e_view, k_view, k_row) = camera_inputs("adapter_cameras", extrinsics, intrinsics)
    d_sh = _d_sh("adapter_cameras", sh_degree)
    if h < 1 or w < 1:
        raise ValueError(f"adapter_cameras: h and w must be positive (got {h}, {w})")
    if sh_rot is not None:
        req(sh_rot, "sh_rot", dim=2)
        if tuple(sh_rot.shape) != (V, rotation_floats(d_sh)):
            raise ValueError(f"adapter_cameras: sh_rot {tuple(sh_rot.shape)} must be {(V, rotation_floats(d_sh))}")
        sh_rot = sh_rot.contiguous()
    cams = torch.empty((V, ADAPTER_CAM), dtype=torch.float32, device=extrinsics.device)
    with torch.cuda.device(extrinsics.device):
        _lib.check(_lib.load().mvsdet_adapter_cameras_f32(
            _lib.ptr(extrinsics), e_view, _lib.ptr(intrinsics), k_view, k_row, _lib.ptr(sh_rot), _lib.ptr(cams), V, int(h), int(w), d_sh,
            stream(extrinsics)), "adapter_cameras")
    return cams


@adapter_cameras.register_fake
def _(extrinsics, intrinsics, h, w, sh_degree, sh_rot=None):
    return extrinsics.new_empty((extrinsics.shape[0], ADAPTER_CAM))


# ------------------------------------------------------------------------------------------- pixel Gaussians
def _check(name: str, raw: Tensor, depth: Tensor, cams: Tensor, h: int, w: int, sh_degree: int):
    req(raw, "raw", dim=4)
    req(depth, "depth", dim=2)
    req(cams, "cams", dim=2)
    d_sh = _d_sh(name, sh_degree)
    V, R, S, C = raw.shape
    if C != row_floats(d_sh) or R != h * w or tuple(depth.shape) != (V, R) or tuple(cams.shape) != (V, ADAPTER_CAM) or min(V, R, S) < 1:
        raise ValueError(f"{name}: raw {tuple(raw.shape)}, depth {tuple(depth.shape)} and cams {tuple(cams.shape)} must be "
                         f"(V, {h * w}, S, {row_floats(d_sh)}), (V, {h * w}) and (V,{ADAPTER_CAM}) from adapter_cameras")
    if V > 65535 or R * S * (C + 1) >= 2 ** 31 or V * R * S * 3 * d_sh >= 2 ** 31:
        raise ValueError(f"{name}: V={V} R={R} S={S} d_sh={d_sh} exceeds the limits (V <= 65535, R S (10 + 3 d_sh) and 3 V R S d_sh < 2^31)")
    return V, R, S, d_sh


def _rows(t: Tensor) -> Tuple[Tensor, int, int]:
    """A (V,R,S,C) tensor whose rows the kernels can walk with two strides -> (tensor, view stride, row stride); anything else is
    copied.  A slice of a wider buffer along the last axis is read in place."""
    V, R, S, C = t.shape
    row = t.stride(2) if S > 1 else t.stride(1) if R > 1 else C
    ok = t.stride(3) == 1 and row >= C and (S == 1 or R == 1 or t.stride(1) == S * row) and (V == 1 or t.stride(0) >= 0)
    if not ok:
        t = t.contiguous()
        row = C
    return t, (t.stride(0) if V > 1 else 0), row


def forward_into(raw: Tensor, depth: Tensor, cams: Tensor, h: int, w: int, s_min: float, s_max: float, sh_degree: int, means: Tensor,
                 covariances: Tensor, harmonics: Tensor, scales: Optional[Tensor] = None, rotations: Optional[Tensor] = None) -> None:
    """The forward launch into the caller's contiguous outputs: what `pixel_gaussians` does after allocating them."""
    V, R, S, d_sh = _check("pixel_gaussians", raw, depth, cams, h, w, sh_degree)
    raw, view, row = _rows(raw)
    depth, cams = depth.contiguous(), cams.contiguous()
    with torch.cuda.device(raw.device):
        _lib.check(_lib.load().mvsdet_adapter_forward_f32(
            _lib.ptr(raw), view, row, _lib.ptr(depth), _lib.ptr(cams), _lib.ptr(means), _lib.ptr(covariances), _lib.ptr(harmonics),
            _lib.ptr(scales), _lib.ptr(rotations), V, int(h), int(w), S, d_sh, float(s_min), float(s_max), stream(raw)), "pixel_gaussians")


def backward_into(raw: Tensor, depth: Tensor, cams: Tensor, g_means: Optional[Tensor], g_covariances: Optional[Tensor],
                  g_harmonics: Optional[Tensor], h: int, w: int, s_min: float, s_max: float, sh_degree: int, g_raw: Tensor,
                  g_depth: Tensor) -> None:
    """The backward launch into the caller's g_raw (V,R,S,9 + 3 d_sh: any view `raw` itself could be, written through its strides) and
    contiguous g_depth (V,R,S)."""
    V, R, S, d_sh = _check("pixel_gaussians_backward", raw, depth, cams, h, w, sh_degree)
    raw, view, row = _rows(raw)
    g_same, g_view, g_row = _rows(g_raw)
    if g_same is not g_raw or tuple(g_raw.shape) != tuple(raw.shape):
        raise ValueError(f"pixel_gaussians_backward: g_raw {tuple(g_raw.shape)} with strides {g_raw.stride()} cannot be written in place")
    depth, cams = depth.contiguous(), cams.contiguous()
    grads = [None if g is None else g.contiguous() for g in (g_means, g_covariances, g_harmonics)]
    with torch.cuda.device(raw.device):
        _lib.check(_lib.load().mvsdet_adapter_backward_f32(
            _lib.ptr(raw), view, row, _lib.ptr(depth), _lib.ptr(cams), _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(grads[2]),
            _lib.ptr(g_raw), g_view, g_row, _lib.ptr(g_depth), V, int(h), int(w), S, d_sh, float(s_min), float(s_max), stream(raw)),
            "pixel_gaussians_backward")


@torch.library.custom_op(f"{_NS}::adapter_pixel_gaussians", mutates_args=(), device_types="cuda")
def _pixel_gaussians(raw: Tensor, depth: Tensor, cams: Tensor, h: int, w: int, s_min: float, s_max: float, sh_degree: int,
                     with_scales: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    V, R, S, d_sh = _check("pixel_gaussians", raw, depth, cams, h, w, sh_degree)
    G, dev = V * R * S, raw.device
    means = torch.empty((G, 3), dtype=torch.float32, device=dev)
    covs = torch.empty((G, 3, 3), dtype=torch.float32, device=dev)
    harm = torch.empty((G, 3, d_sh), dtype=torch.float32, device=dev)
    scales = torch.empty((G if with_scales else 0, 3), dtype=torch.float32, device=dev)
    rots = torch.empty((G if with_scales else 0, 4), dtype=torch.float32, device=dev)
    forward_into(raw, depth, cams, h, w, s_min, s_max, sh_degree, means, covs, harm, scales if with_scales else None,
                 rots if with_scales else None)
    return means, covs, harm, scales, rots


@_pixel_gaussians.register_fake
def _(raw, depth, cams, h, w, s_min, s_max, sh_degree, with_scales):
    V, R, S, _ = raw.shape
    G, d_sh = V * R * S, (sh_degree + 1) ** 2
    n = G if with_scales else 0
    return raw.new_empty((G, 3)), raw.new_empty((G, 3, 3)), raw.new_empty((G, 3, d_sh)), raw.new_empty((n, 3)), raw.new_empty((n, 4))


@torch.library.custom_op(f"{_NS}::adapter_pixel_gaussians_backward", mutates_args=(), device_types="cuda")
def pixel_gaussians_backward(raw: Tensor, depth: Tensor, cams: Tensor, g_means: Optional[Tensor], g_covariances: Optional[Tensor],
                             g_harmonics: Optional[Tensor], h: int, w: int, s_min: float, s_max: float,
                             sh_degree: int) -> Tuple[Tensor, Tensor]:
    """Gradients of `pixel_gaussians` -> (g_raw (V,R,S,9 + 3 d_sh), g_depth (V,R,S)).  g_covariances is any 3x3 gradient: the upper
    triangle the rasteriser sends, or all nine entries.  A gradient that is None counts as zeros.  One launch, no atomics."""
    V, R, S, d_sh = _check("pixel_gaussians_backward", raw, depth, cams, h, w, sh_degree)
    G = V * R * S
    for g, name, shape in ((g_means, "g_means", (G, 3)), (g_covariances, "g_covariances", (G, 3, 3)), (g_harmonics, "g_harmonics", (G, 3, d_sh))):
        if g is not None:
            req(g, name)
            if tuple(g.shape) != shape:
                raise ValueError(f"pixel_gaussians_backward: {name} {tuple(g.shape)} must be {shape}")
    g_raw = torch.empty(tuple(raw.shape), dtype=torch.float32, device=raw.device)
    g_depth = torch.empty((V, R, S), dtype=torch.float32, device=raw.device)
    backward_into(raw, depth, cams, g_means, g_covariances, g_harmonics, h, w, s_min, s_max, sh_degree, g_raw, g_depth)
    return g_raw, g_depth


@pixel_gaussians_backward.register_fake
def _(raw, depth, cams, g_means, g_covariances, g_harmonics, h, w, s_min, s_max, sh_degree):
    return raw.new_empty(tuple(raw.shape)), raw.new_empty(tuple(raw.shape[:3]))


def _pg_setup(ctx, inputs, output):
    raw, depth, cams, h, w, s_min, s_max, sh_degree, with_scales = inputs
    if cams.requires_grad:
        raise RuntimeError("pixel_gaussians: the cameras carry no gradient here; detach them")
    ctx.mark_non_differentiable(output[3], output[4])   # scales, rotations: kept for the visualisation dump only
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(raw, depth, cams)
    ctx.args = (h, w, s_min, s_max, sh_degree)


def _pg_bwd(ctx, g_means, g_covs, g_harm, g_scales, g_rots):
    if g_means is None and g_covs is None and g_harm is None:
        return (None,) * 9
    raw, depth, cams = ctx.saved_tensors
    g_raw, g_depth = pixel_gaussians_backward(raw, depth, cams, g_means, g_covs, g_harm, *ctx.args)
    return g_raw, g_depth.sum(dim=2), None, None, None, None, None, None, None


_pixel_gaussians.register_autograd(_pg_bwd, setup_context=_pg_setup)

for _op in (adapter_cameras, _pixel_gaussians):
    _op.register_autocast("cuda", torch.float32)
del _op


def pixel_gaussians(raw: Tensor, depth: Tensor, cams: Tensor, h: int, w: int, s_min: float, s_max: float, sh_degree: int,
                    with_scales: bool = False):
    """raw (V,R,S,9 + 3 d_sh) -- offset 2, scales 3, quaternion xyzw 4, harmonics (3,d_sh); a slice of a wider buffer along the last
    axis is read in place --, depth (V,R) along the ray, cams (V,192) from `adapter_cameras`, R = h w -> (means (G,3), covariances
    (G,3,3), harmonics (G,3,d_sh)) with G = V R S in (v, r, s) order, and with `with_scales` also (scales (G,3), rotations (G,4)), which
    carry no gradient.  One launch; one more for the backward.  Differentiable in raw and depth."""
    means, covs, harm, scales, rots = _pixel_gaussians(raw, depth, cams, int(h), int(w), float(s_min), float(s_max), int(sh_degree),
                                                       bool(with_scales))
    return (means, covs, harm, scales, rots) if with_scales else (means, covs, harm)
