"""Photometric consistency (csrc/photoloss.hip): mvs_models/homography.py and MVSDet.photometric_loss (mvsdet.py:845-874).

The names live in this module only (`ops.photo.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from ._common import _NS, _lib, req, stream

PHOTO_GEO = 24          # floats per pair: K_left^-1 (9), K_left [R_rel | t_rel] (12), 3 unused
PHOTO_MAX_SCENES = 32   # photometric_select

_GRID: dict = {}


def pixel_grid(h: int, w: int, device=None) -> Tuple[Tensor, Tensor]:
    """homography.py:66-77: the pixel coordinates the reference warps from, (linspace(-1,1,W) + 1) * 0.5 * (W-1) and the same for
    the rows, evaluated with the reference's own torch ops on the CPU (they are not the integers: linspace rounds).  With a device:
    uploaded once per (h, w, device) and kept."""
    key = (h, w, None if device is None else str(device))
    hit = _GRID.get(key)
    if hit is None:
        xg = (torch.linspace(-1.0, 1.0, w) + 1.0) * 0.5 * (w - 1)
        yg = (torch.linspace(-1.0, 1.0, h) + 1.0) * 0.5 * (h - 1)
        hit = _GRID[key] = (xg, yg) if device is None else (xg.to(device), yg.to(device))
    return hit


def _index(name: str, idx: Optional[Tensor], like: Tensor, B: Optional[int] = None):
    if idx is None:
        return None
    if idx.dtype != torch.int64 or idx.dim() != 1 or idx.device != like.device:
        raise ValueError(f"{name}: must be a 1-D int64 tensor on {like.device} (got {idx.dtype}, shape {tuple(idx.shape)}, {idx.device})")
    if B is not None and idx.shape[0] != B:
        raise ValueError(f"{name}: {idx.shape[0]} indices for {B} pairs")
    return idx.contiguous()


def _rows4(t: Tensor, name: str) -> Tensor:
    """(n, >=3, 4) camera rows with a row stride of 4 elements: a (N,4,4) stack or the [:,0] / [:,1] plane of packed (B,2,3,4)."""
    req(t, name, dim=3)
    if t.shape[1] < 3 or t.shape[2] != 4:
        raise ValueError(f"{name}: must be (n, 3 or 4, 4), got {tuple(t.shape)}")
    return t if (t.stride(2) == 1 and t.stride(1) == 4 and t.stride(0) >= 0) else t.contiguous()


# ------------------------------------------------------------------------------------------- geometry
@torch.library.custom_op(f"{_NS}::photo_geometry", mutates_args=(), device_types="cuda")
def photo_geometry(ext_left: Tensor, k_left: Tensor, ext_right: Tensor, left_idx: Optional[Tensor],
                   right_idx: Optional[Tensor]) -> Tensor:
    """homography.py:11-30,56-58 for B (left, right) pairs -> geo (B,24): K_left^-1 and K_left [R_right R_left^T | t_right - R_rel t_left]
    (the LEFT intrinsics project into the right view, as the reference has it), float64 rounded once.  ext_* (n,3|4,4) world-to-camera
    rows; k_left (3|4, 3|4) for all views or (n_left, 3|4, 3|4); left_idx / right_idx (B) int64 choose the views (None: pair b is view
    b of both).  One launch of one thread per pair; nothing returns to the host."""
    ext_left, ext_right = _rows4(ext_left, "ext_left"), _rows4(ext_right, "ext_right")
    req(k_left, "k_left")
    if k_left.dim() not in (2, 3) or k_left.shape[-1] < 3 or k_left.shape[-2] < 3:
        raise ValueError(f"photo_geometry: k_left must be (3|4,3|4) or (n,3|4,3|4), got {tuple(k_left.shape)}")
    if k_left.stride(-1) != 1:
        k_left = k_left.contiguous()
    if k_left.dim() == 3 and k_left.shape[0] != ext_left.shape[0]:
        raise ValueError(f"photo_geometry: {k_left.shape[0]} intrinsics for {ext_left.shape[0]} left views")
    if (left_idx is None) != (right_idx is None):
        raise ValueError("photo_geometry: left_idx and right_idx come together")
    if left_idx is None and ext_left.shape[0] != ext_right.shape[0]:
        raise ValueError(f"photo_geometry: {ext_left.shape[0]} left and {ext_right.shape[0]} right views and no index")
    B = ext_left.shape[0] if left_idx is None else left_idx.shape[0]
    left_idx, right_idx = _index("left_idx", left_idx, ext_left, B), _index("right_idx", right_idx, ext_left, B)
    geo = torch.empty((B, PHOTO_GEO), dtype=torch.float32, device=ext_left.device)
    k_view = k_left.stride(0) if k_left.dim() == 3 else 0
    with torch.cuda.device(ext_left.device):
        _lib.check(_lib.load().mvsdet_photo_geometry_f32(
            _lib.ptr(ext_left), ext_left.stride(0), _lib.ptr(k_left), k_view, k_left.stride(-2), _lib.ptr(ext_right),
            ext_right.stride(0), _lib.ptr(left_idx), _lib.ptr(right_idx), ext_left.shape[0], ext_right.shape[0], _lib.ptr(geo), B,
            stream(ext_left)), "photo_geometry")
    return geo


@photo_geometry.register_fake
def _(ext_left, k_left, ext_right, left_idx, right_idx):
    return ext_left.new_empty((ext_left.shape[0] if left_idx is None else left_idx.shape[0], PHOTO_GEO))


# ------------------------------------------------------------------------------------------- warp
def _check_warp(name: str, img: Tensor, depth: Tensor, geo: Tensor, src_idx, depth_idx):
    req(img, "img", dim=4)
    req(depth, "depth", dim=3)
    req(geo, "geo", dim=2)
    B = geo.shape[0]
    if geo.shape[1] != PHOTO_GEO or B < 1:
        raise ValueError(f"{name}: geo must be (B,{PHOTO_GEO}) from photo_geometry, got {tuple(geo.shape)}")
    h, w, C = img.shape[1:]
    if tuple(depth.shape[1:]) != (h, w) or min(h, w, C) < 1:
        raise ValueError(f"{name}: img {tuple(img.shape)} must be (n,h,w,C) and depth {tuple(depth.shape)} (n,h,w) of one h, w")
    src_idx, depth_idx = _index("src_idx", src_idx, img, B), _index("depth_idx", depth_idx, img, B)
    if src_idx is None and img.shape[0] != B:
        raise ValueError(f"{name}: {img.shape[0]} images for {B} pairs and no src_idx")
    if depth_idx is None and depth.shape[0] != B:
        raise ValueError(f"{name}: {depth.shape[0]} depth maps for {B} pairs and no depth_idx")
    if max(B, depth.shape[0]) * h * w * C >= 2 ** 31:
        raise ValueError(f"{name}: {max(B, depth.shape[0])}x{h}x{w}x{C} exceeds 2^31 elements")
    return B, h, w, C, geo.contiguous(), src_idx, depth_idx


@torch.library.custom_op(f"{_NS}::inverse_warp", mutates_args=(), device_types="cuda")
def inverse_warp(img: Tensor, depth: Tensor, geo: Tensor, src_idx: Optional[Tensor], depth_idx: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """inverse_warping (homography.py:6-63, 104-201) -> warped (B,h,w,C), mask (B,h,w,1) float 0/1.  img (n,h,w,C) ANY strides
    (channel-last, or the permuted view of planar NCHW) and depth (n,h,w) any strides (the crop of a padded map) are read in place;
    pair b samples image src_idx[b] at the positions depth map depth_idx[b] projects to (None: b).  geo from `photo_geometry`.
    The reference's fp32 operation order, its mask (the last test on y0) and its clamped-index weights; outside the mask warped is the
    same formula, an extrapolation.  One launch.  Differentiable in depth only."""
    B, h, w, C, geo, src_idx, depth_idx = _check_warp("inverse_warp", img, depth, geo, src_idx, depth_idx)
    dev = img.device
    xg, yg = pixel_grid(h, w, dev)
    warped = torch.empty((B, h, w, C), dtype=torch.float32, device=dev)
    mask = torch.empty((B, h, w, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_photo_warp_f32(
            _lib.ptr(img), _lib.strides4(img), _lib.ptr(src_idx), img.shape[0], _lib.ptr(depth), _lib.strides3(depth),
            _lib.ptr(depth_idx), depth.shape[0], _lib.ptr(geo), _lib.ptr(xg), _lib.ptr(yg), _lib.ptr(warped), _lib.ptr(mask), B, h, w, C,
            stream(img)), "inverse_warp")
    return warped, mask


@inverse_warp.register_fake
def _(img, depth, geo, src_idx, depth_idx):
    B, (h, w, C) = geo.shape[0], img.shape[1:]
    return img.new_empty((B, h, w, C)), img.new_empty((B, h, w, 1))


@torch.library.custom_op(f"{_NS}::inverse_warp_backward", mutates_args=(), device_types="cuda")
def inverse_warp_backward(img: Tensor, depth: Tensor, geo: Tensor, src_idx: Optional[Tensor], depth_idx: Optional[Tensor],
                          g_warped: Tensor) -> Tensor:
    """d / d depth of `inverse_warp` -> (n,h,w) fp32 at depth's shape, dense: through the four weights to (x, y) and through the
    quotient to depth (floor, clamp and the mask carry none); a depth map no pair reads gets 0, one that several read their sum in
    ascending pair order.  A pixel whose g_warped is 0 in every channel gets exactly 0.  One launch, no atomics."""
    B, h, w, C, geo, src_idx, depth_idx = _check_warp("inverse_warp_backward", img, depth, geo, src_idx, depth_idx)
    req(g_warped, "g_warped", dim=4)
    if tuple(g_warped.shape) != (B, h, w, C):
        raise ValueError(f"inverse_warp_backward: g_warped {tuple(g_warped.shape)} must be {(B, h, w, C)}")
    g_warped = g_warped.contiguous()
    dev = img.device
    xg, yg = pixel_grid(h, w, dev)
    grad = torch.empty(tuple(depth.shape), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_photo_warp_bwd_f32(
            _lib.ptr(img), _lib.strides4(img), _lib.ptr(src_idx), img.shape[0], _lib.ptr(depth), _lib.strides3(depth),
            _lib.ptr(depth_idx), depth.shape[0], _lib.ptr(geo), _lib.ptr(xg), _lib.ptr(yg), _lib.ptr(g_warped), _lib.ptr(grad), B, h, w,
            C, stream(img)), "inverse_warp_backward")
    return grad


@inverse_warp_backward.register_fake
def _(img, depth, geo, src_idx, depth_idx, g_warped):
    return depth.new_empty(tuple(depth.shape))


def _iw_setup(ctx, inputs, output):
    img, depth, geo, src_idx, depth_idx = inputs
    if img.requires_grad or geo.requires_grad:
        raise RuntimeError("inverse_warp: the image and the cameras carry no gradient here (depth only); detach them")
    ctx.mark_non_differentiable(output[1])   # the mask
    ctx.set_materialize_grads(False)         # no zero fill for the gradient of an output nobody used
    ctx.save_for_backward(img, depth, geo, src_idx, depth_idx)


def _iw_bwd(ctx, g_warped, g_mask):
    if g_warped is None:
        return None, None, None, None, None
    img, depth, geo, src_idx, depth_idx = ctx.saved_tensors
    return None, inverse_warp_backward(img, depth, geo, src_idx, depth_idx, g_warped), None, None, None


inverse_warp.register_autograd(_iw_bwd, setup_context=_iw_setup)


# ------------------------------------------------------------------------------------------- loss
def _check_loss(name: str, warped: Tensor, ref: Tensor, mask: Tensor):
    req(warped, "warped", dim=4)
    req(ref, "ref", dim=4)
    req(mask, "mask", dim=4)
    B, h, w, C = warped.shape
    if ref.shape != warped.shape or tuple(mask.shape) != (B, h, w, 1) or min(B, h, w, C) < 1:
        raise ValueError(f"{name}: warped {tuple(warped.shape)} and ref {tuple(ref.shape)} must be one (B,h,w,C) and mask "
                         f"{tuple(mask.shape)} (B,h,w,1)")
    if B * h * w * C >= 2 ** 31:
        raise ValueError(f"{name}: {B}x{h}x{w}x{C} exceeds 2^31 elements")
    return B, h, w, C, warped.contiguous(), mask.contiguous()


@torch.library.custom_op(f"{_NS}::reconstr_loss", mutates_args=(), device_types="cuda")
def reconstr_loss(warped: Tensor, ref: Tensor, mask: Tensor, simple: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """compute_reconstr_loss (homography.py:204-225) -> (L () fp32, terms (3) fp32, count () int32).  wm = warped * mask, rm = ref *
    mask; terms = the means of smooth_l1 (beta 1) of wm - rm and of its forward differences along w and along h, each over its own
    element count; L = terms[0] (simple) or 0.5 terms[0] + 0.5 (terms[1] + terms[2]); count = pixels inside the mask.  ref any
    strides.  Two launches, float64 sums in a fixed order, no atomics.  Differentiable in warped only."""
    B, h, w, C, warped, mask = _check_loss("reconstr_loss", warped, ref, mask)
    dev = warped.device
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    terms = torch.empty((3,), dtype=torch.float32, device=dev)
    count = torch.empty((), dtype=torch.int32, device=dev)
    ws_bytes = int(lib.mvsdet_photo_loss_workspace_bytes(B, h, w))
    workspace = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_photo_loss_f32(_lib.ptr(warped), _lib.ptr(mask), _lib.ptr(ref), _lib.strides4(ref), _lib.ptr(loss),
                                             _lib.ptr(terms), _lib.ptr(count), _lib.ptr(workspace), ws_bytes, B, h, w, C, int(simple),
                                             stream(warped)), "reconstr_loss")
    return loss, terms, count


@reconstr_loss.register_fake
def _(warped, ref, mask, simple):
    return warped.new_empty(()), warped.new_empty((3,)), warped.new_empty((), dtype=torch.int32)


@torch.library.custom_op(f"{_NS}::reconstr_loss_backward", mutates_args=(), device_types="cuda")
def reconstr_loss_backward(warped: Tensor, ref: Tensor, mask: Tensor, g_loss: Tensor, simple: bool) -> Tensor:
    """d L / d warped of `reconstr_loss` times g_loss (() fp32, read on the device) -> (B,h,w,C): the photo term and the transposed
    difference stencils, times the mask -- exactly 0 outside it.  One launch."""
    B, h, w, C, warped, mask = _check_loss("reconstr_loss_backward", warped, ref, mask)
    req(g_loss, "g_loss")
    if g_loss.numel() != 1 or g_loss.device != warped.device:
        raise ValueError("reconstr_loss_backward: g_loss must be one float32 on the device of warped")
    grad = torch.empty((B, h, w, C), dtype=torch.float32, device=warped.device)
    with torch.cuda.device(warped.device):
        _lib.check(_lib.load().mvsdet_photo_loss_bwd_f32(_lib.ptr(warped), _lib.ptr(mask), _lib.ptr(ref), _lib.strides4(ref),
                                                         _lib.ptr(g_loss), _lib.ptr(grad), B, h, w, C, int(simple), stream(warped)),
                   "reconstr_loss_backward")
    return grad


@reconstr_loss_backward.register_fake
def _(warped, ref, mask, g_loss, simple):
    return warped.new_empty(tuple(warped.shape))


def _rl_setup(ctx, inputs, output):
    warped, ref, mask, simple = inputs
    if ref.requires_grad:
        raise RuntimeError("reconstr_loss: the reference image carries no gradient here (warped only); detach it")
    ctx.mark_non_differentiable(output[1], output[2])   # the gradient goes through L
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(warped, ref, mask)
    ctx.simple = simple


def _rl_bwd(ctx, g_loss, g_terms, g_count):
    if g_loss is None:
        return None, None, None, None
    warped, ref, mask = ctx.saved_tensors
    return reconstr_loss_backward(warped, ref, mask, g_loss.contiguous(), ctx.simple), None, None, None


reconstr_loss.register_autograd(_rl_bwd, setup_context=_rl_setup)


# ------------------------------------------------------------------------------------------- selection over scenes
def _check_select(name: str, masks: Tensor, L: Tensor):
    req(masks, "masks", dim=2)
    req(L, "L", dim=1)
    n, total = masks.shape
    if L.shape[0] != n or not (1 <= n <= PHOTO_MAX_SCENES) or total < 1 or total >= 2 ** 31:
        raise ValueError(f"{name}: masks {tuple(masks.shape)} must be (n, pixels) and L {tuple(L.shape)} (n), 1 <= n <= "
                         f"{PHOTO_MAX_SCENES}")
    return n, total


@torch.library.custom_op(f"{_NS}::photometric_select", mutates_args=(), device_types="cuda")
def photometric_select(masks: Tensor, L: Tensor) -> Tuple[Tensor, Tensor]:
    """MVSDet.photometric_loss (mvsdet.py:845-874) on the n scalars L_i and the n masks (n, B*h*w) -> (loss_pc () fp32, wins (n)
    int32): per pixel the smallest L_i + 1e4 (1 - mask_i) (the lower scene on a tie), dropped where it is not < 1e4, and the mean
    over the pixels = sum_i wins_i L_i / pixels.  Two launches, integer counts, no atomics.  Differentiable in L."""
    n, total = _check_select("photometric_select", masks, L)
    masks, L = masks.contiguous(), L.contiguous()
    dev = masks.device
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    wins = torch.empty((n,), dtype=torch.int32, device=dev)
    ws_bytes = int(lib.mvsdet_photo_select_workspace_bytes(n, total))
    workspace = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_photo_select_f32(_lib.ptr(masks), _lib.ptr(L), _lib.ptr(wins), _lib.ptr(loss), _lib.ptr(workspace),
                                               ws_bytes, n, total, stream(masks)), "photometric_select")
    return loss, wins


@photometric_select.register_fake
def _(masks, L):
    return L.new_empty(()), L.new_empty((L.shape[0],), dtype=torch.int32)


@torch.library.custom_op(f"{_NS}::photometric_select_backward", mutates_args=(), device_types="cuda")
def photometric_select_backward(wins: Tensor, g_loss: Tensor, total: int) -> Tensor:
    """d loss_pc / d L_i times g_loss (() fp32 on the device) = g_loss * wins_i / pixels: the share of pixels scene i wins."""
    req(wins, "wins", dtype=torch.int32, dim=1)
    req(g_loss, "g_loss")
    n = wins.shape[0]
    if g_loss.numel() != 1 or not (1 <= n <= PHOTO_MAX_SCENES) or total < 1:
        raise ValueError("photometric_select_backward: g_loss must be one float32, wins (n <= 32) and total >= 1")
    grad = torch.empty((n,), dtype=torch.float32, device=wins.device)
    with torch.cuda.device(wins.device):
        _lib.check(_lib.load().mvsdet_photo_select_bwd_f32(_lib.ptr(wins.contiguous()), _lib.ptr(g_loss), _lib.ptr(grad), n, total,
                                                           stream(wins)), "photometric_select_backward")
    return grad


@photometric_select_backward.register_fake
def _(wins, g_loss, total):
    return g_loss.new_empty((wins.shape[0],))


def _ps_setup(ctx, inputs, output):
    masks, L = inputs
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(output[1])
    ctx.total = masks.shape[1]


def _ps_bwd(ctx, g_loss, g_wins):
    if g_loss is None:
        return None, None
    (wins,) = ctx.saved_tensors
    return None, photometric_select_backward(wins, g_loss.contiguous(), ctx.total)


photometric_select.register_autograd(_ps_bwd, setup_context=_ps_setup)

for _op in (inverse_warp, reconstr_loss, photometric_select):
    _op.register_autocast("cuda", torch.float32)
del _op
