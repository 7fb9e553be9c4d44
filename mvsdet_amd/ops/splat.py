"""Gaussian rasteriser (csrc/splat.hip): what gs_src/model/decoder/cuda_splatting.py::render_cuda asks of `diff_gaussian_rasterization`.

The names live in this module only (`ops.splat.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

import ctypes
from typing import List, Tuple

import torch
from torch import Tensor

from ._common import _NS, _lib, req, stream

SPLAT_CAM = 40            # floats per view: view matrix 16, full projection 16, tan fov x / y, camera position 3, scale, 2 unused
SPLAT_SLOT = 9            # floats per (tile, Gaussian) gradient slot of the backward
SPLAT_TILE = 16
SPLAT_KEYS_PER_GAUSSIAN = 8   # default key capacity of a view: 8 (Gaussian, tile) pairs per Gaussian (DESIGN 4.15 has the measured need)
SPLAT_SH = (1, 4, 9, 16, 25)


def default_max_keys(G: int) -> int:
    return SPLAT_KEYS_PER_GAUSSIAN * int(G)


def _strides(t: Tensor) -> ctypes.Array:
    return (ctypes.c_int64 * t.dim())(*[int(s) for s in t.stride()])


def _check(name: str, means: Tensor, covariances: Tensor, harmonics: Tensor, opacities: Tensor, cams: Tensor, background: Tensor,
           H: int, W: int, max_keys: int, use_sh: bool):
    req(means, "means", dim=2)
    req(covariances, "covariances", dim=3)
    req(harmonics, "harmonics", dim=3)
    req(opacities, "opacities", dim=1)
    req(cams, "cams", dim=2)
    req(background, "background", dim=2)
    G, V = means.shape[0], cams.shape[0]
    d_sh = harmonics.shape[2]
    if means.shape[1] != 3 or tuple(covariances.shape) != (G, 3, 3) or tuple(harmonics.shape[:2]) != (G, 3) or opacities.shape[0] != G:
        raise ValueError(f"{name}: means {tuple(means.shape)}, covariances {tuple(covariances.shape)}, harmonics {tuple(harmonics.shape)} "
                         f"and opacities {tuple(opacities.shape)} must be (G,3), (G,3,3), (G,3,d_sh) and (G)")
    if d_sh not in SPLAT_SH:
        raise ValueError(f"{name}: d_sh = {d_sh} must be one of {SPLAT_SH}")
    if not use_sh and d_sh != 1:
        raise ValueError(f"{name}: precomputed colours come as (G,3,1), got d_sh = {d_sh}")
    if cams.shape[1] != SPLAT_CAM or tuple(background.shape) != (V, 3) or min(V, G, H, W, max_keys) < 1:
        raise ValueError(f"{name}: cams {tuple(cams.shape)} must be (V,{SPLAT_CAM}) from splat_cameras, background {tuple(background.shape)} "
                         f"(V,3), and H, W, max_keys positive (got {H}, {W}, {max_keys})")
    tiles = -(-H // SPLAT_TILE) * -(-W // SPLAT_TILE)
    if V > 65535 or max(V * G, V * tiles, SPLAT_SLOT * V * max_keys, 3 * V * H * W, 3 * G * d_sh) >= 2 ** 31:
        raise ValueError(f"{name}: V={V} G={G} {H}x{W} max_keys={max_keys} exceeds the limits (V G, V tiles, 9 V max_keys, 3 V H W < 2^31)")
    return V, G, d_sh, cams.contiguous(), background.contiguous()


# ------------------------------------------------------------------------------------------- cameras
@torch.library.custom_op(f"{_NS}::splat_cameras", mutates_args=(), device_types="cuda")
def splat_cameras(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, scale_invariant: bool) -> Tensor:
    """cuda_splatting.py:66-90 for V views -> cams (V,40): the transposed view matrix and full projection, tan(fov / 2) in x and y
    (get_fov), the camera position and the scale 1 / near (1 without scale_invariant) that the rasteriser applies to means, covariances
    and the translation itself.  extrinsics (V,4,4) camera-to-world, intrinsics (V,3,3) normalised, near / far (V).  One launch of one
    thread per view, float64 inside, rounded once; nothing returns to the host."""
    req(extrinsics, "extrinsics", dim=3)
    req(intrinsics, "intrinsics", dim=3)
    req(near, "near", dim=1)
    req(far, "far", dim=1)
    V = extrinsics.shape[0]
    if tuple(extrinsics.shape[1:]) != (4, 4) or tuple(intrinsics.shape) != (V, 3, 3) or near.shape[0] != V or far.shape[0] != V or V < 1:
        raise ValueError(f"splat_cameras: extrinsics {tuple(extrinsics.shape)}, intrinsics {tuple(intrinsics.shape)}, near {tuple(near.shape)} "
                         f"and far {tuple(far.shape)} must be (V,4,4), (V,3,3), (V) and (V)")
    if extrinsics.stride(2) != 1 or extrinsics.stride(1) != 4:
        extrinsics = extrinsics.contiguous()
    if intrinsics.stride(2) != 1:
        intrinsics = intrinsics.contiguous()
    near, far = near.contiguous(), far.contiguous()
    cams = torch.empty((V, SPLAT_CAM), dtype=torch.float32, device=extrinsics.device)
    with torch.cuda.device(extrinsics.device):
        _lib.check(_lib.load().mvsdet_splat_cameras_f32(
            _lib.ptr(extrinsics), extrinsics.stride(0), _lib.ptr(intrinsics), intrinsics.stride(0), intrinsics.stride(1), _lib.ptr(near),
            _lib.ptr(far), int(scale_invariant), _lib.ptr(cams), V, stream(extrinsics)), "splat_cameras")
    return cams


@splat_cameras.register_fake
def _(extrinsics, intrinsics, near, far, scale_invariant):
    return extrinsics.new_empty((extrinsics.shape[0], SPLAT_CAM))


# ------------------------------------------------------------------------------------------- render
def workspace_bytes(V: int, G: int, H: int, W: int, max_keys: int) -> int:
    n = int(_lib.load().mvsdet_splat_workspace_bytes(V, G, H, W, max_keys))
    if n == 0:
        raise ValueError(f"splat: no workspace for V={V} G={G} {H}x{W} max_keys={max_keys}: "
                         + _lib.load().mvsdet_last_error().decode("utf-8", "replace"))
    return n


def rasterize_into(means: Tensor, covariances: Tensor, harmonics: Tensor, opacities: Tensor, cams: Tensor, background: Tensor, H: int,
                   W: int, max_keys: int, use_sh: bool, image: Tensor, workspace: Tensor) -> None:
    """The forward launch sequence into a caller's `image` (V,3,H,W) and `workspace` (uint8 or int32, 256-byte aligned, at least
    workspace_bytes(...)): what `rasterize` does after allocating both."""
    V, G, d_sh, cams, background = _check("rasterize", means, covariances, harmonics, opacities, cams, background, H, W, max_keys, use_sh)
    with torch.cuda.device(means.device):
        _lib.check(_lib.load().mvsdet_splat_forward_f32(
            _lib.ptr(means), _strides(means), _lib.ptr(covariances), _strides(covariances), _lib.ptr(harmonics), _strides(harmonics),
            _lib.ptr(opacities), opacities.stride(0), _lib.ptr(cams), _lib.ptr(background), _lib.ptr(image), _lib.ptr(workspace),
            workspace.numel() * workspace.element_size(), V, G, d_sh, int(use_sh), H, W, max_keys, stream(means)), "rasterize")


@torch.library.custom_op(f"{_NS}::splat_rasterize", mutates_args=(), device_types="cuda")
def rasterize(means: Tensor, covariances: Tensor, harmonics: Tensor, opacities: Tensor, cams: Tensor, background: Tensor, H: int, W: int,
              max_keys: int, use_sh: bool) -> Tuple[Tensor, Tensor]:
    """V views of one set of G Gaussians -> (image (V,3,H,W), workspace uint8).  means (G,3), covariances (G,3,3: the upper triangle
    is read), harmonics (G,3,d_sh), opacities (G), any strides, read in place; cams (V,40) from `splat_cameras`; background (V,3).
    use_sh False: harmonics (G,3,1) are the colours.  max_keys: the (Gaussian, tile) pairs a view may have (`default_max_keys`); a view
    that needs more comes out NaN, with NaN gradients, and `status(workspace)` says so.  No host synchronisation.  Differentiable in
    means, covariances (gradient on the upper triangle, off-diagonals with both symmetric terms), harmonics and opacities."""
    V, G, d_sh, cams, background = _check("rasterize", means, covariances, harmonics, opacities, cams, background, H, W, max_keys, use_sh)
    image = torch.empty((V, 3, H, W), dtype=torch.float32, device=means.device)
    workspace = torch.empty((workspace_bytes(V, G, H, W, max_keys),), dtype=torch.uint8, device=means.device)
    rasterize_into(means, covariances, harmonics, opacities, cams, background, H, W, max_keys, use_sh, image, workspace)
    return image, workspace


@rasterize.register_fake
def _(means, covariances, harmonics, opacities, cams, background, H, W, max_keys, use_sh):
    V, G = cams.shape[0], means.shape[0]
    return means.new_empty((V, 3, H, W)), means.new_empty((workspace_bytes(V, G, H, W, max_keys),), dtype=torch.uint8)


@torch.library.custom_op(f"{_NS}::splat_rasterize_backward", mutates_args=(), device_types="cuda")
def rasterize_backward(means: Tensor, covariances: Tensor, harmonics: Tensor, opacities: Tensor, cams: Tensor, background: Tensor,
                       workspace: Tensor, g_image: Tensor, H: int, W: int, max_keys: int,
                       use_sh: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Gradients of `rasterize` -> (means (G,3), covariances (G,3,3), harmonics (G,3,d_sh), opacities (G)), summed over the views in
    ascending order; every (tile, Gaussian) pair is reduced inside its block and added in tile order: no float atomics, the same
    bits on every run.  Two launches."""
    V, G, d_sh, cams, background = _check("rasterize_backward", means, covariances, harmonics, opacities, cams, background, H, W, max_keys,
                                          use_sh)
    req(g_image, "g_image", dim=4)
    req(workspace, "workspace", dtype=torch.uint8, dim=1)
    if tuple(g_image.shape) != (V, 3, H, W):
        raise ValueError(f"rasterize_backward: g_image {tuple(g_image.shape)} must be {(V, 3, H, W)}")
    g_image = g_image.contiguous()
    dev = means.device
    slots = torch.empty((V * max_keys * SPLAT_SLOT,), dtype=torch.float32, device=dev)
    g_means = torch.empty((G, 3), dtype=torch.float32, device=dev)
    g_cov = torch.empty((G, 3, 3), dtype=torch.float32, device=dev)
    g_sh = torch.empty((G, 3, d_sh), dtype=torch.float32, device=dev)
    g_op = torch.empty((G,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_splat_backward_f32(
            _lib.ptr(means), _strides(means), _lib.ptr(covariances), _strides(covariances), _lib.ptr(harmonics), _strides(harmonics),
            _lib.ptr(opacities), opacities.stride(0), _lib.ptr(cams), _lib.ptr(background), _lib.ptr(g_image), _lib.ptr(workspace),
            workspace.numel(), _lib.ptr(slots), _lib.ptr(g_means), _lib.ptr(g_cov), _lib.ptr(g_sh), _lib.ptr(g_op), V, G, d_sh,
            int(use_sh), H, W, max_keys, stream(means)), "rasterize_backward")
    return g_means, g_cov, g_sh, g_op


@rasterize_backward.register_fake
def _(means, covariances, harmonics, opacities, cams, background, workspace, g_image, H, W, max_keys, use_sh):
    G = means.shape[0]
    return means.new_empty((G, 3)), means.new_empty((G, 3, 3)), means.new_empty(tuple(harmonics.shape)), means.new_empty((G,))


def _rz_setup(ctx, inputs, output):
    means, covariances, harmonics, opacities, cams, background, H, W, max_keys, use_sh = inputs
    if cams.requires_grad or background.requires_grad:
        raise RuntimeError("rasterize: the cameras and the background carry no gradient here; detach them")
    ctx.mark_non_differentiable(output[1])   # the workspace
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(means, covariances, harmonics, opacities, cams, background, output[1])
    ctx.args = (H, W, max_keys, use_sh)


def _rz_bwd(ctx, g_image, g_workspace):
    if g_image is None:
        return (None,) * 10
    means, covariances, harmonics, opacities, cams, background, workspace = ctx.saved_tensors
    gm, gc, gs, go = rasterize_backward(means, covariances, harmonics, opacities, cams, background, workspace, g_image, *ctx.args)
    return gm, gc, gs, go, None, None, None, None, None, None


rasterize.register_autograd(_rz_bwd, setup_context=_rz_setup)

for _op in (splat_cameras, rasterize):
    _op.register_autocast("cuda", torch.float32)
del _op


def status(workspace: Tensor, V: int) -> List[dict]:
    """The status words of a `rasterize` workspace, one dict per view: needed keys, capacity, overflow.  This read is a host
    synchronisation -- the only one; the render itself never waits for it."""
    words = workspace.view(torch.uint8)[:16 * V].view(torch.int32).view(V, 4).cpu()
    return [dict(needed=int(n), capacity=int(c), overflow=bool(o)) for n, c, o, _ in words.tolist()]


def radii(workspace: Tensor, V: int, G: int) -> Tensor:
    """(V,G) int32 view into a `rasterize` workspace: every Gaussian's radius in pixels, 0 where it was culled (what the extension
    returns as `radii`).  No copy, no synchronisation."""
    start = (16 * V + 255) // 256 * 256
    return workspace.view(torch.uint8)[start:start + 4 * V * G].view(torch.int32).view(V, G)
