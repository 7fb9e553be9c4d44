"""a9 / a9+a10: the lifting block and its diagnostics against ground-truth depth (csrc/backproject.hip)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from ._common import _NS, _lib, req, stream


def _check_stage3(features, points, projection, est_depth, est_dens):
    req(features, "features", dim=4)
    req(points, "points")
    req(projection, "projection", dim=3)
    req(est_depth, "est_depth", dim=4)
    req(est_dens, "est_dens", dim=4)
    N, C, h, w = features.shape
    if points.shape[0] != 3:
        raise ValueError("backproject_weigh: points must be (3, ...)")
    V = points.numel() // 3
    J = est_depth.shape[1]
    if projection.shape != (N, 3, 4):
        raise ValueError(f"backproject_weigh: projection {tuple(projection.shape)} != ({N},3,4)")
    if est_depth.shape != (N, J, h, w) or est_dens.shape != (N, J, h, w):
        raise ValueError(f"backproject_weigh: est_depth/est_dens must be ({N},J,{h},{w}), got "
                         f"{tuple(est_depth.shape)} / {tuple(est_dens.shape)}")
    if est_depth.stride() != est_dens.stride():
        est_dens = est_dens.contiguous()
        est_depth = est_depth.contiguous()
    return N, C, h, w, V, J, est_depth, est_dens


@torch.library.custom_op(f"{_NS}::backproject_weigh", mutates_args=(), device_types="cuda")
def backproject_weigh(features: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor, est_dens: Tensor,
                      vz: float) -> Tuple[Tensor, Tensor]:
    """a9 (mvsdet.py:1372): features (N,C,h,w) any strides; points (3,X,Y,Z); projection (N,3,4);
    est_depth/est_dens (N,J,h,w) any strides -> volume (N,C,V) fp32, valid (N,V) bool."""
    N, C, h, w, V, J, est_depth, est_dens = _check_stage3(features, points, projection, est_depth, est_dens)
    points, projection = points.contiguous(), projection.contiguous()
    dev = features.device
    volume = torch.empty((N, C, V), dtype=torch.float32, device=dev)
    valid = torch.empty((N, V), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_backproject_weigh_f32(
            _lib.ptr(features), _lib.strides4(features), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth),
            _lib.ptr(est_dens), _lib.strides4(est_depth), _lib.ptr(volume), _lib.ptr(valid), None, None,
            N, C, h, w, V, J, vz, stream(features)), "backproject_weigh")
    return volume, valid.bool()


@backproject_weigh.register_fake
def _(features, points, projection, est_depth, est_dens, vz):
    N, C = features.shape[:2]
    V = points.numel() // 3
    return features.new_empty((N, C, V)), features.new_empty((N, V), dtype=torch.bool)


@torch.library.custom_op(f"{_NS}::backproject_weigh_backward", mutates_args=(), device_types="cuda")
def backproject_weigh_backward(features: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor,
                               est_dens: Tensor, vz: float, grad: Tensor) -> Tuple[Tensor, Tensor]:
    N, C, h, w, V, J, est_depth, est_dens = _check_stage3(features, points, projection, est_depth, est_dens)
    points, projection, grad = points.contiguous(), projection.contiguous(), grad.contiguous()
    dev = features.device
    gfeat = torch.empty((N, C, h, w), dtype=torch.float32, device=dev)
    gdens = torch.empty((N, J, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_backproject_weigh_bwd_f32(
            _lib.ptr(features), _lib.strides4(features), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth),
            _lib.ptr(est_dens), _lib.strides4(est_depth), _lib.ptr(grad), _lib.ptr(gfeat), _lib.ptr(gdens),
            N, C, h, w, V, J, vz, stream(features)), "backproject_weigh_backward")
    return gfeat, gdens


@backproject_weigh_backward.register_fake
def _(features, points, projection, est_depth, est_dens, vz, grad):
    N, C, h, w = features.shape
    return features.new_empty((N, C, h, w)), features.new_empty((N, est_depth.shape[1], h, w))


def _bp_setup(ctx, inputs, output):
    features, points, projection, est_depth, est_dens, vz = inputs
    ctx.save_for_backward(features, points, projection, est_depth, est_dens)
    ctx.vz = vz


def _bp_bwd(ctx, g_volume, g_valid):
    features, points, projection, est_depth, est_dens = ctx.saved_tensors
    gfeat, gdens = backproject_weigh_backward(features, points, projection, est_depth, est_dens, ctx.vz, g_volume)
    return gfeat, None, None, None, gdens, None


backproject_weigh.register_autograd(_bp_bwd, setup_context=_bp_setup)


# ------------------------------------------------------------------------------------------- a9 against ground-truth depth
@torch.library.custom_op(f"{_NS}::depth_diagnostics", mutates_args=(), device_types="cuda")
def depth_diagnostics(points: Tensor, projection: Tensor, est_depth: Tensor, est_dens: Tensor, depth_mean: Tensor,
                      gt_depth: Tensor, vz: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The gt_depth branch of backproject_Weigh (mvsdet.py:1435-1484): points (3,X,Y,Z); projection (N,3,4); est_depth / est_dens
    (N,J,h,w) any strides; depth_mean (N,h,w) any strides (the cropped depth expectation); gt_depth (N,Hg,Wg) any strides, any size
    -> scalars (2) {gap_all ("weight_gap"), rmse ("src_rmse")}, per_view (N,4) {gap_i, orig_gap, new_gap, n_reduce}, sums (N,6)
    float64 (include/mvsdet_hip.h), gt_resized (N,h,w).  Three launches on the current stream, no host synchronisation; no autograd
    (the reference runs the branch under no_grad).  gap_all is NaN when no view keeps a voxel (the reference raises there)."""
    req(points, "points")
    req(projection, "projection", dim=3)
    req(est_depth, "est_depth", dim=4)
    req(est_dens, "est_dens", dim=4)
    req(depth_mean, "depth_mean", dim=3)
    req(gt_depth, "gt_depth", dim=3)
    N, J, h, w = est_depth.shape
    if points.shape[0] != 3:
        raise ValueError("depth_diagnostics: points must be (3, ...)")
    V = points.numel() // 3
    if projection.shape != (N, 3, 4) or est_dens.shape != (N, J, h, w):
        raise ValueError(f"depth_diagnostics: projection {tuple(projection.shape)} / est_dens {tuple(est_dens.shape)} do not match "
                         f"est_depth {tuple(est_depth.shape)}")
    if depth_mean.shape != (N, h, w) or gt_depth.shape[0] != N:
        raise ValueError(f"depth_diagnostics: depth_mean {tuple(depth_mean.shape)} must be ({N},{h},{w}) and gt_depth "
                         f"{tuple(gt_depth.shape)} ({N},Hg,Wg)")
    if est_depth.stride() != est_dens.stride():
        est_depth, est_dens = est_depth.contiguous(), est_dens.contiguous()
    points, projection = points.contiguous(), projection.contiguous()
    Hg, Wg = int(gt_depth.shape[1]), int(gt_depth.shape[2])
    dev = est_depth.device
    lib = _lib.load()
    scalars = torch.empty((2,), dtype=torch.float32, device=dev)
    per_view = torch.empty((N, 4), dtype=torch.float32, device=dev)
    sums = torch.empty((N, 6), dtype=torch.float64, device=dev)
    gt_resized = torch.empty((N, h, w), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.mvsdet_depth_diagnostics_workspace_bytes(N, h, w, V))
    workspace = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_depth_diagnostics_f32(
            _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth), _lib.ptr(est_dens), _lib.strides4(est_depth),
            _lib.ptr(depth_mean), _lib.strides3(depth_mean), _lib.ptr(gt_depth), _lib.strides3(gt_depth), _lib.ptr(scalars),
            _lib.ptr(per_view), _lib.ptr(sums), _lib.ptr(gt_resized), _lib.ptr(workspace), ws_bytes, N, h, w, V, J, Hg, Wg, vz,
            stream(est_depth)), "depth_diagnostics")
    return scalars, per_view, sums, gt_resized


@depth_diagnostics.register_fake
def _(points, projection, est_depth, est_dens, depth_mean, gt_depth, vz):
    N, _, h, w = est_depth.shape
    return (est_depth.new_empty((2,)), est_depth.new_empty((N, 4)), est_depth.new_empty((N, 6), dtype=torch.float64),
            est_depth.new_empty((N, h, w)))


# ------------------------------------------------------------------------------------------- a9+a10
@torch.library.custom_op(f"{_NS}::backproject_weigh_mean", mutates_args=(), device_types="cuda")
def backproject_weigh_mean(features: Tensor, packed: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor,
                           est_dens: Tensor, H: int, W: int, vz: float) -> Tuple[Tensor, Tensor]:
    """a9+a10 fused (mvsdet.py:1372 + 511-515).  `features` is the (N,C,h,w) crop view (used for shapes and by
    the backward pass), `packed` = pack_features(full (N,C,H,W) maps).  -> mean (C,V) fp32, count (V) int32."""
    N, C, h, w, V, J, est_depth, est_dens = _check_stage3(features, points, projection, est_depth, est_dens)
    req(packed, "packed", dim=1)
    lib = _lib.load()
    if packed.numel() * 4 != lib.mvsdet_packed_bytes(N, C, H, W):
        raise ValueError("backproject_weigh_mean: packed buffer does not match (N,C,H,W)")
    points, projection = points.contiguous(), projection.contiguous()
    dev = features.device
    mean = torch.empty((C, V), dtype=torch.float32, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_backproject_weigh_mean_packed_f32(
            _lib.ptr(packed), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth), _lib.ptr(est_dens),
            _lib.strides4(est_depth), _lib.ptr(mean), _lib.ptr(count), N, C, H, W, h, w, V, J, vz, stream(features)),
            "backproject_weigh_mean")
    return mean, count


@backproject_weigh_mean.register_fake
def _(features, packed, points, projection, est_depth, est_dens, H, W, vz):
    C = features.shape[1]
    V = points.numel() // 3
    return features.new_empty((C, V)), features.new_empty((V,), dtype=torch.int32)


@torch.library.custom_op(f"{_NS}::backproject_weigh_sum_shard", mutates_args=(), device_types="cuda")
def backproject_weigh_sum_shard(packed: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor, est_dens: Tensor,
                                n_src: int, ref_first: int, C: int, H: int, W: int, vz: float) -> Tuple[Tensor, Tensor]:
    """a9 summed over the M views ref_first .. ref_first+M-1 only, NOT divided (the a10 division happens after the
    ranks' sums and counts are all-reduced).  projection (M,3,4), est_depth / est_dens (M,J,h,w) are the shard's;
    `packed` holds all n_src views.  -> sum (C,V) fp32, count (V) int32.  Forward only."""
    req(packed, "packed", dim=1)
    req(points, "points")
    req(projection, "projection", dim=3)
    req(est_depth, "est_depth", dim=4)
    req(est_dens, "est_dens", dim=4)
    M, J, h, w = est_depth.shape
    V = points.numel() // 3
    lib = _lib.load()
    if packed.numel() * 4 != lib.mvsdet_packed_bytes(n_src, C, H, W):
        raise ValueError("backproject_weigh_sum_shard: packed buffer does not match (n_src,C,H,W)")
    if points.shape[0] != 3 or projection.shape != (M, 3, 4) or est_dens.shape != est_depth.shape:
        raise ValueError("backproject_weigh_sum_shard: points / projection / est_dens shape mismatch")
    if M < 1 or ref_first < 0 or ref_first + M > n_src:
        raise ValueError(f"backproject_weigh_sum_shard: views [{ref_first},{ref_first + M}) outside the {n_src} packed views")
    if est_depth.stride() != est_dens.stride():
        est_depth, est_dens = est_depth.contiguous(), est_dens.contiguous()
    points, projection = points.contiguous(), projection.contiguous()
    dev = packed.device
    total = torch.empty((C, V), dtype=torch.float32, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    view_floats = lib.mvsdet_packed_bytes(1, C, H, W) // 4
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_backproject_weigh_sum_packed_f32(
            _lib.ptr(packed[view_floats * ref_first:]), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth),
            _lib.ptr(est_dens), _lib.strides4(est_depth), _lib.ptr(total), _lib.ptr(count), M, C, H, W, h, w, V, J, vz,
            stream(packed)), "backproject_weigh_sum_shard")
    return total, count


@backproject_weigh_sum_shard.register_fake
def _(packed, points, projection, est_depth, est_dens, n_src, ref_first, C, H, W, vz):
    V = points.numel() // 3
    return packed.new_empty((C, V)), packed.new_empty((V,), dtype=torch.int32)


@torch.library.custom_op(f"{_NS}::backproject_weigh_mean_backward", mutates_args=(), device_types="cuda")
def backproject_weigh_mean_backward(features: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor,
                                    est_dens: Tensor, count: Tensor, vz: float, grad: Tensor) -> Tuple[Tensor, Tensor]:
    N, C, h, w, V, J, est_depth, est_dens = _check_stage3(features, points, projection, est_depth, est_dens)
    points, projection, grad = points.contiguous(), projection.contiguous(), grad.contiguous()
    dev = features.device
    gfeat = torch.empty((N, C, h, w), dtype=torch.float32, device=dev)
    gdens = torch.empty((N, J, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_backproject_weigh_mean_bwd_f32(
            _lib.ptr(features), _lib.strides4(features), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth),
            _lib.ptr(est_dens), _lib.strides4(est_depth), _lib.ptr(count), _lib.ptr(grad), _lib.ptr(gfeat),
            _lib.ptr(gdens), N, C, h, w, V, J, vz, stream(features)), "backproject_weigh_mean_backward")
    return gfeat, gdens


@backproject_weigh_mean_backward.register_fake
def _(features, points, projection, est_depth, est_dens, count, vz, grad):
    N, C, h, w = features.shape
    return features.new_empty((N, C, h, w)), features.new_empty((N, est_depth.shape[1], h, w))


def _bpm_setup(ctx, inputs, output):
    features, packed, points, projection, est_depth, est_dens, H, W, vz = inputs
    mean, count = output
    ctx.save_for_backward(features, points, projection, est_depth, est_dens, count)
    ctx.vz = vz


def _bpm_bwd(ctx, g_mean, g_count):
    features, points, projection, est_depth, est_dens, count = ctx.saved_tensors
    gfeat, gdens = backproject_weigh_mean_backward(features, points, projection, est_depth, est_dens, count, ctx.vz,
                                                   g_mean)
    return gfeat, None, None, None, None, gdens, None, None, None


backproject_weigh_mean.register_autograd(_bpm_bwd, setup_context=_bpm_setup)
