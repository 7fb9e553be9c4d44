"""Gaussian rasteriser (csrc/splat.hip): what gs_src/model/decoder/cuda_splatting.py::render_cuda asks of `diff_gaussian_rasterization`,
and render_depth_cuda's depth as a fourth blended channel of the same pass (`rasterize_depth`) or alone (`depth_only`).

The names live in this module only (`ops.splat.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from ._common import _NS, _lib, camera_inputs, req, stream

SPLAT_CAM = 40            # floats per view: view matrix 16, full projection 16, tan fov x / y, camera position 3, scale, 2 unused
SPLAT_SLOT = 9            # floats per (tile, Gaussian) gradient slot of the backward
SPLAT_SLOT_DEPTH = 10     # the same in the depth forms: one more float, dL/dd
DEPTH_MODES = ("depth", "disparity", "relative_disparity", "log")   # render_depth_cuda's modes, in the C ABI's numbering
SPLAT_TILE = 16
SPLAT_KEYS_PER_GAUSSIAN = 8   # default key capacity of a view: 8 (Gaussian, tile) pairs per Gaussian (DESIGN 4.15 has the measured need)
SPLAT_SH = (1, 4, 9, 16, 25)


def default_max_keys(G: int) -> int:
    return SPLAT_KEYS_PER_GAUSSIAN * int(G)


def _depth_mode(name: str, mode: str) -> int:
    if mode not in DEPTH_MODES:
        raise ValueError(f"{name}: mode {mode!r} must be one of {DEPTH_MODES}")
    return DEPTH_MODES.index(mode)


def _bounds(name: str, near: Tensor, far: Tensor, V: int):
    req(near, "near", dim=1)
    req(far, "far", dim=1)
    if near.shape[0] != V or far.shape[0] != V:
        raise ValueError(f"{name}: near {tuple(near.shape)} and far {tuple(far.shape)} must be ({V})")
    return near.contiguous(), far.contiguous()


def _check(name: str, means: Tensor, covariances: Tensor, harmonics: Optional[Tensor], opacities: Tensor, cams: Tensor,
           background: Optional[Tensor], H: int, W: int, max_keys: int, use_sh: bool, near: Optional[Tensor] = None,
           far: Optional[Tensor] = None, mode: Optional[str] = None):
    """The checks of every form.  harmonics and background None: no colour (d_sh counts as 1); mode None: no depth, near and far are
    not looked at.  -> V, G, d_sh, the mode's number in the C ABI (0 without depth) and cams, near, far, background as the C entries
    read them (contiguous; None where the form has none)."""
    code = 0 if mode is None else _depth_mode(name, mode)
    colour = harmonics is not None
    req(means, "means", dim=2)
    req(covariances, "covariances", dim=3)
    if colour:
        req(harmonics, "harmonics", dim=3)
    req(opacities, "opacities", dim=1)
    req(cams, "cams", dim=2)
    if colour:
        req(background, "background", dim=2)
    G, V = means.shape[0], cams.shape[0]
    d_sh = harmonics.shape[2] if colour else 1
    sh_fits = not colour or tuple(harmonics.shape[:2]) == (G, 3)
    if means.shape[1] != 3 or tuple(covariances.shape) != (G, 3, 3) or not sh_fits or opacities.shape[0] != G:
        raise ValueError(f"{name}: means {tuple(means.shape)}, covariances {tuple(covariances.shape)}, harmonics "
                         f"{tuple(harmonics.shape) if colour else None} and opacities {tuple(opacities.shape)} must be (G,3), (G,3,3), "
                         "(G,3,d_sh) and (G)")
    if d_sh not in SPLAT_SH:
        raise ValueError(f"{name}: d_sh = {d_sh} must be one of {SPLAT_SH}")
    if colour and not use_sh and d_sh != 1:
        raise ValueError(f"{name}: precomputed colours come as (G,3,1), got d_sh = {d_sh}")
    if cams.shape[1] != SPLAT_CAM or (colour and tuple(background.shape) != (V, 3)) or min(V, G, H, W, max_keys) < 1:
        raise ValueError(f"{name}: cams {tuple(cams.shape)} must be (V,{SPLAT_CAM}) from splat_cameras, background "
                         f"{tuple(background.shape) if colour else None} (V,3), and H, W, max_keys positive (got {H}, {W}, {max_keys})")
    if mode is not None:
        near, far = _bounds(name, near, far, V)
    tiles = -(-H // SPLAT_TILE) * -(-W // SPLAT_TILE)
    slot = SPLAT_SLOT if mode is None else SPLAT_SLOT_DEPTH
    if V > 65535 or max(V * G, V * tiles, slot * V * max_keys, 3 * V * H * W, 3 * G * d_sh) >= 2 ** 31:
        raise ValueError(f"{name}: V={V} G={G} {H}x{W} max_keys={max_keys} exceeds the limits (V G, V tiles, {slot} V max_keys, 3 V H W "
                         "< 2^31)")
    return V, G, d_sh, code, cams.contiguous(), near, far, background.contiguous() if colour else None


def _gaussians(means: Tensor, covariances: Tensor, harmonics: Optional[Tensor], opacities: Tensor) -> tuple:
    """The first eight arguments of both C entries: the Gaussian tensors in place, each with its element strides."""
    return (_lib.ptr(means), _lib.strides(means), _lib.ptr(covariances), _lib.strides(covariances), _lib.ptr(harmonics),
            None if harmonics is None else _lib.strides(harmonics), _lib.ptr(opacities), opacities.stride(0))


# ------------------------------------------------------------------------------------------- cameras
@torch.library.custom_op(f"{_NS}::splat_cameras", mutates_args=(), device_types="cuda")
def splat_cameras(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, scale_invariant: bool) -> Tensor:
    """cuda_splatting.py:66-90 for V views -> cams (V,40): the transposed view matrix and full projection, tan(fov / 2) in x and y
    (get_fov), the camera position and the scale 1 / near (1 without scale_invariant) that the rasteriser applies to means, covariances
    and the translation itself.  extrinsics (V,4,4) camera-to-world, intrinsics (V,3,3) normalised, near / far (V).  One launch of one
    thread per view, float64 inside, rounded once; nothing returns to the host."""
    extrinsics, intrinsics, V, (e_view, k_view, k_row) = camera_inputs("splat_cameras", extrinsics, intrinsics)
    near, far = _bounds("splat_cameras", near, far, V)
    cams = torch.empty((V, SPLAT_CAM), dtype=torch.float32, device=extrinsics.device)
    with torch.cuda.device(extrinsics.device):
        _lib.check(_lib.load().mvsdet_splat_cameras_f32(
            _lib.ptr(extrinsics), e_view, _lib.ptr(intrinsics), k_view, k_row, _lib.ptr(near), _lib.ptr(far), int(scale_invariant),
            _lib.ptr(cams), V, stream(extrinsics)), "splat_cameras")
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


def _forward(name: str, means, covariances, harmonics, opacities, cams, near, far, background, H, W, max_keys, use_sh, mode,
             image=None, workspace=None):
    """The forward of every form through the one C entry -> (image, depth, values, workspace), None for what the form does not give.
    harmonics None: depth alone; mode None: colour alone.  image and workspace are allocated unless the caller brings them."""
    V, G, d_sh, code, cams, near, far, background = _check(name, means, covariances, harmonics, opacities, cams, background, H, W, max_keys,
                                                           use_sh, near, far, mode)
    dev, colour, with_depth = means.device, harmonics is not None, mode is not None
    if colour and image is None:
        image = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev) if with_depth else None
    values = torch.empty((V, G), dtype=torch.float32, device=dev) if with_depth else None
    if workspace is None:
        workspace = torch.empty((workspace_bytes(V, G, H, W, max_keys),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_splat_forward_f32(
            *_gaussians(means, covariances, harmonics, opacities), _lib.ptr(cams), _lib.ptr(near), _lib.ptr(far), _lib.ptr(background),
            _lib.ptr(image), _lib.ptr(depth), _lib.ptr(values), _lib.ptr(workspace), workspace.numel() * workspace.element_size(), V, G,
            d_sh, int(use_sh), int(colour), int(with_depth), code, H, W, max_keys, stream(means)), name)
    return image, depth, values, workspace


def _backward(name: str, means, covariances, harmonics, opacities, cams, near, far, background, values, workspace, g_image, g_depth, H, W,
              max_keys, use_sh, mode):
    """The backward of every form through the one C entry -> (g_means, g_covariances, g_harmonics or None, g_opacities)."""
    V, G, d_sh, code, cams, near, far, background = _check(name, means, covariances, harmonics, opacities, cams, background, H, W, max_keys,
                                                           use_sh, near, far, mode)
    dev, colour, with_depth = means.device, harmonics is not None, mode is not None
    req(workspace, "workspace", dtype=torch.uint8, dim=1)
    if with_depth:
        req(g_depth, "g_depth", dim=3)
        req(values, "values", dim=2)
        if tuple(g_depth.shape) != (V, H, W) or tuple(values.shape) != (V, G):
            raise ValueError(f"{name}: g_depth {tuple(g_depth.shape)} and values {tuple(values.shape)} must be {(V, H, W)} and {(V, G)}")
        g_depth, values = g_depth.contiguous(), values.contiguous()
    if colour:
        req(g_image, "g_image", dim=4)
        if tuple(g_image.shape) != (V, 3, H, W):
            raise ValueError(f"{name}: g_image {tuple(g_image.shape)} must be {(V, 3, H, W)}")
        g_image = g_image.contiguous()
    slots = torch.empty((V * max_keys * (SPLAT_SLOT_DEPTH if with_depth else SPLAT_SLOT),), dtype=torch.float32, device=dev)
    g_means = torch.empty((G, 3), dtype=torch.float32, device=dev)
    g_cov = torch.empty((G, 3, 3), dtype=torch.float32, device=dev)
    g_sh = torch.empty((G, 3, d_sh), dtype=torch.float32, device=dev) if colour else None
    g_op = torch.empty((G,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_splat_backward_f32(
            *_gaussians(means, covariances, harmonics, opacities), _lib.ptr(cams), _lib.ptr(near), _lib.ptr(far), _lib.ptr(background),
            _lib.ptr(g_image), _lib.ptr(g_depth), _lib.ptr(values), _lib.ptr(workspace), workspace.numel(), _lib.ptr(slots),
            _lib.ptr(g_means), _lib.ptr(g_cov), _lib.ptr(g_sh), _lib.ptr(g_op), V, G, d_sh, int(use_sh), int(colour), int(with_depth), code,
            H, W, max_keys, stream(means)), name)
    return g_means, g_cov, g_sh, g_op


def rasterize_into(means: Tensor, covariances: Tensor, harmonics: Tensor, opacities: Tensor, cams: Tensor, background: Tensor, H: int,
                   W: int, max_keys: int, use_sh: bool, image: Tensor, workspace: Tensor) -> None:
    """The forward launch sequence into a caller's `image` (V,3,H,W) and `workspace` (uint8 or int32, 256-byte aligned, at least
    workspace_bytes(...)): what `rasterize` does after allocating both."""
    _forward("rasterize", means, covariances, harmonics, opacities, cams, None, None, background, H, W, max_keys, use_sh, None, image,
             workspace)


@torch.library.custom_op(f"{_NS}::splat_rasterize", mutates_args=(), device_types="cuda")
def rasterize(means: Tensor, covariances: Tensor, harmonics: Tensor, opacities: Tensor, cams: Tensor, background: Tensor, H: int, W: int,
              max_keys: int, use_sh: bool) -> Tuple[Tensor, Tensor]:
    """V views of one set of G Gaussians -> (image (V,3,H,W), workspace uint8).  means (G,3), covariances (G,3,3: the upper triangle
    is read), harmonics (G,3,d_sh), opacities (G), any strides, read in place; cams (V,40) from `splat_cameras`; background (V,3).
    use_sh False: harmonics (G,3,1) are the colours.  max_keys: the (Gaussian, tile) pairs a view may have (`default_max_keys`); a view
    that needs more comes out NaN, with NaN gradients, and `status(workspace)` says so.  No host synchronisation.  Differentiable in
    means, covariances (gradient on the upper triangle, off-diagonals with both symmetric terms), harmonics and opacities."""
    image, _, _, workspace = _forward("rasterize", means, covariances, harmonics, opacities, cams, None, None, background, H, W, max_keys,
                                      use_sh, None)
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
    return _backward("rasterize_backward", means, covariances, harmonics, opacities, cams, None, None, background, None, workspace, g_image,
                     None, H, W, max_keys, use_sh, None)


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

# ------------------------------------------------------------------------------------------- rendered depth
@torch.library.custom_op(f"{_NS}::splat_rasterize_depth", mutates_args=(), device_types="cuda")
def rasterize_depth(means: Tensor, covariances: Tensor, harmonics: Tensor, opacities: Tensor, cams: Tensor, near: Tensor, far: Tensor,
                    background: Tensor, H: int, W: int, max_keys: int, use_sh: bool, mode: str) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """`rasterize` with the rendered depth of render_depth_cuda as a fourth blended channel of the same pass -> (image (V,3,H,W),
    depth (V,H,W), values (V,G), workspace).  near / far (V): the unscaled bounds `splat_cameras` was given; mode: one of
    DEPTH_MODES.  values is what the reference calls fake_color -- every Gaussian's camera-space z (before the scale_invariant
    scaling) mapped by the mode, 0 where culled; it is returned to be looked at and carries no gradient.  depth = sum values alpha T
    over a background of 0, with the colour's alpha, T, skips and early stop; NaN for a view over its key capacity.  image has the
    bits of `rasterize`, and the workspace is the same (`status`, `radii`).  Differentiable in means, covariances, harmonics and
    opacities, through both outputs."""
    return _forward("rasterize_depth", means, covariances, harmonics, opacities, cams, near, far, background, H, W, max_keys, use_sh, mode)


@rasterize_depth.register_fake
def _(means, covariances, harmonics, opacities, cams, near, far, background, H, W, max_keys, use_sh, mode):
    V, G = cams.shape[0], means.shape[0]
    return (means.new_empty((V, 3, H, W)), means.new_empty((V, H, W)), means.new_empty((V, G)),
            means.new_empty((workspace_bytes(V, G, H, W, max_keys),), dtype=torch.uint8))


@torch.library.custom_op(f"{_NS}::splat_rasterize_depth_backward", mutates_args=(), device_types="cuda")
def rasterize_depth_backward(means: Tensor, covariances: Tensor, harmonics: Tensor, opacities: Tensor, cams: Tensor, near: Tensor,
                             far: Tensor, background: Tensor, values: Tensor, workspace: Tensor, g_image: Tensor, g_depth: Tensor, H: int,
                             W: int, max_keys: int, use_sh: bool, mode: str) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Gradients of `rasterize_depth` for g_image (V,3,H,W) and g_depth (V,H,W) -> (means, covariances, harmonics, opacities).  The
    depth enters the recurrence as one more channel and leaves one more per-(tile, Gaussian) partial sum, dL/dd, chained to the means
    through the mode's derivative (0 for log); the fixed summation order of `rasterize_backward`, the same bits on every run."""
    return _backward("rasterize_depth_backward", means, covariances, harmonics, opacities, cams, near, far, background, values, workspace,
                     g_image, g_depth, H, W, max_keys, use_sh, mode)


@rasterize_depth_backward.register_fake
def _(means, covariances, harmonics, opacities, cams, near, far, background, values, workspace, g_image, g_depth, H, W, max_keys, use_sh, mode):
    G = means.shape[0]
    return means.new_empty((G, 3)), means.new_empty((G, 3, 3)), means.new_empty(tuple(harmonics.shape)), means.new_empty((G,))


@torch.library.custom_op(f"{_NS}::splat_depth_only", mutates_args=(), device_types="cuda")
def depth_only(means: Tensor, covariances: Tensor, opacities: Tensor, cams: Tensor, near: Tensor, far: Tensor, H: int, W: int,
               max_keys: int, mode: str) -> Tuple[Tensor, Tensor, Tensor]:
    """The depth of `rasterize_depth` alone -> (depth (V,H,W), values (V,G), workspace): no harmonics are read, no colour is staged
    or blended.  The same bits as the fused call's depth.  Differentiable in means, covariances and opacities."""
    return _forward("depth_only", means, covariances, None, opacities, cams, near, far, None, H, W, max_keys, False, mode)[1:]


@depth_only.register_fake
def _(means, covariances, opacities, cams, near, far, H, W, max_keys, mode):
    V, G = cams.shape[0], means.shape[0]
    return means.new_empty((V, H, W)), means.new_empty((V, G)), means.new_empty((workspace_bytes(V, G, H, W, max_keys),), dtype=torch.uint8)


@torch.library.custom_op(f"{_NS}::splat_depth_only_backward", mutates_args=(), device_types="cuda")
def depth_only_backward(means: Tensor, covariances: Tensor, opacities: Tensor, cams: Tensor, near: Tensor, far: Tensor, values: Tensor,
                        workspace: Tensor, g_depth: Tensor, H: int, W: int, max_keys: int, mode: str) -> Tuple[Tensor, Tensor, Tensor]:
    """Gradients of `depth_only` -> (means (G,3), covariances (G,3,3), opacities (G)).  Also the backward of a `rasterize_depth` whose
    image received no gradient: the workspace is the same."""
    gm, gc, _, go = _backward("depth_only_backward", means, covariances, None, opacities, cams, near, far, None, values, workspace, None,
                              g_depth, H, W, max_keys, False, mode)
    return gm, gc, go


@depth_only_backward.register_fake
def _(means, covariances, opacities, cams, near, far, values, workspace, g_depth, H, W, max_keys, mode):
    G = means.shape[0]
    return means.new_empty((G, 3)), means.new_empty((G, 3, 3)), means.new_empty((G,))


def _no_grad_inputs(name, **tensors):
    bad = [k for k, t in tensors.items() if t.requires_grad]
    if bad:
        raise RuntimeError(f"{name}: {', '.join(bad)} carry no gradient here; detach them")


def _rd_setup(ctx, inputs, output):
    means, covariances, harmonics, opacities, cams, near, far, background, H, W, max_keys, use_sh, mode = inputs
    _no_grad_inputs("rasterize_depth", cams=cams, near=near, far=far, background=background)
    ctx.mark_non_differentiable(output[2], output[3])   # the values and the workspace
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(means, covariances, harmonics, opacities, cams, near, far, background, output[2], output[3])
    ctx.args = (H, W, max_keys, use_sh, mode)


def _rd_bwd(ctx, g_image, g_depth, g_values, g_workspace):
    none = (None,) * 9
    if g_image is None and g_depth is None:
        return (None,) * 13
    means, covariances, harmonics, opacities, cams, near, far, background, values, workspace = ctx.saved_tensors
    H, W, max_keys, use_sh, mode = ctx.args
    if g_depth is None:      # the image alone was used: the colour-only backward reads the same workspace
        return rasterize_backward(means, covariances, harmonics, opacities, cams, background, workspace, g_image, H, W, max_keys, use_sh) + none
    if g_image is None:      # the depth alone was used
        gm, gc, go = depth_only_backward(means, covariances, opacities, cams, near, far, values, workspace, g_depth, H, W, max_keys, mode)
        return (gm, gc, torch.zeros_like(harmonics), go) + none
    return rasterize_depth_backward(means, covariances, harmonics, opacities, cams, near, far, background, values, workspace, g_image,
                                    g_depth, H, W, max_keys, use_sh, mode) + none


def _do_setup(ctx, inputs, output):
    means, covariances, opacities, cams, near, far, H, W, max_keys, mode = inputs
    _no_grad_inputs("depth_only", cams=cams, near=near, far=far)
    ctx.mark_non_differentiable(output[1], output[2])
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(means, covariances, opacities, cams, near, far, output[1], output[2])
    ctx.args = (H, W, max_keys, mode)


def _do_bwd(ctx, g_depth, g_values, g_workspace):
    if g_depth is None:
        return (None,) * 10
    means, covariances, opacities, cams, near, far, values, workspace = ctx.saved_tensors
    return depth_only_backward(means, covariances, opacities, cams, near, far, values, workspace, g_depth, *ctx.args) + (None,) * 7


rasterize_depth.register_autograd(_rd_bwd, setup_context=_rd_setup)
depth_only.register_autograd(_do_bwd, setup_context=_do_setup)

for _op in (splat_cameras, rasterize, rasterize_depth, depth_only):
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
