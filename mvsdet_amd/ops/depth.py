"""a5-a7: ray depth and the depth distribution (csrc/depthprob.hip)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from ._common import _NS, _lib, req, stream


def _ray_depth_launch(intr: Tensor, est_depth: Optional[Tensor], h: int, w: int):
    """The kernel launch of `ray_depth` -> depth_scale (N,h*w,1), est_ray_depth (N,J,h*w) or None."""
    req(intr, "intr", dim=2)
    N = intr.shape[0]
    intr = intr.contiguous()
    scale = torch.empty((N, h * w, 1), dtype=torch.float32, device=intr.device)
    ray = None
    J, H, W = 0, h, w
    if est_depth is not None:
        req(est_depth, "est_depth", dim=4)
        if est_depth.shape[0] != N:
            raise ValueError("ray_depth: est_depth and intr disagree on the number of views")
        est_depth = est_depth.contiguous()
        J, H, W = est_depth.shape[1:]
        ray = torch.empty((N, J, h * w), dtype=torch.float32, device=intr.device)
    with torch.cuda.device(intr.device):
        _lib.check(_lib.load().mvsdet_ray_depth_f32(_lib.ptr(intr), _lib.ptr(est_depth), _lib.ptr(scale), _lib.ptr(ray), N, J, H, W,
                                                    h, w, stream(intr)), "ray_depth")
    return scale, ray


class _RayDepthGrad(torch.autograd.Function):
    """est_ray_depth under autograd: the forward is the same launch as the no-grad path; the backward is that of the
    reference's `est_depth / (scale + 1e-8)` (mvsdet.py:494): g / (scale + 1e-8) on the cropped (h, w) window of est_depth,
    zero on its padding.  depth_scale depends on the intrinsics alone and carries no gradient."""

    @staticmethod
    def forward(ctx, est_depth, intr, h, w):
        scale, ray = _ray_depth_launch(intr, est_depth, h, w)
        ctx.mark_non_differentiable(scale)
        ctx.save_for_backward(scale)
        ctx.geometry = (tuple(est_depth.shape), h, w)
        return scale, ray

    @staticmethod
    def backward(ctx, g_scale, g_ray):
        (scale,) = ctx.saved_tensors
        (N, J, H, W), h, w = ctx.geometry
        grad = g_ray.new_zeros((N, J, H, W))
        grad[:, :, :h, :w] = (g_ray / (scale.view(N, 1, h * w) + 1e-8)).view(N, J, h, w)
        return grad, None, None, None


def ray_depth(intr: Tensor, est_depth: Optional[Tensor], h: int, w: int):
    """mvsdet.py:1158-1216 + :494: intr (N,5) {fx,fy,cx,cy,skew} at feature level -> depth_scale (N,h*w,1) and, when
    est_depth (N,J,H,W) is given, est_ray_depth (N,h*w,1,J) in the layout extract_feat hands to the Gaussian adapter.
    Differentiable in est_depth only (when it requires grad): d est_ray_depth / d est_depth = 1 / (depth_scale + 1e-8) on
    the (h, w) window, 0 on the padding, as the reference's division; depth_scale and the intrinsics carry no gradient.
    The forward values are those of the no-grad path, bit for bit (the same launch)."""
    if est_depth is not None and est_depth.requires_grad and torch.is_grad_enabled():
        scale, ray = _RayDepthGrad.apply(est_depth, intr, h, w)
    else:
        scale, ray = _ray_depth_launch(intr, est_depth, h, w)
    return scale, (None if ray is None else ray.transpose(2, 1).unsqueeze(2))


# ------------------------------------------------------------------------------------------- a5-a7
@torch.library.custom_op(f"{_NS}::depth_prob_topk", mutates_args=(), device_types="cuda")
def depth_prob_topk(cost_reg: Tensor, off_logit: Tensor, near: float, interval: float,
                    topk: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """a5-a7 (mvsdet.py:470-475, 266-283, 298-317) -> prob, off (N,D,H,W); est_depth, est_dens (N,topk,H,W);
    est_idx (N,topk,H,W) int32; avg_depth (N,H,W)."""
    req(cost_reg, "cost_reg", dim=4)
    req(off_logit, "off_logit", dim=4)
    if cost_reg.shape != off_logit.shape:
        raise ValueError("depth_prob_topk: cost_reg / off_logit shape mismatch")
    N, D, H, W = cost_reg.shape
    # the slices of one (N, 2, D, H, W) tensor (the network's output) are read in place: dense (D, H, W) blocks, one stride
    # between the views; anything else is made contiguous first
    dense = (W * H * D, W * H, W, 1)
    if not (cost_reg.stride()[1:] == dense[1:] == off_logit.stride()[1:] and cost_reg.stride(0) == off_logit.stride(0) >= dense[0]):
        cost_reg, off_logit = cost_reg.contiguous(), off_logit.contiguous()
    view_stride = cost_reg.stride(0) if N > 1 else dense[0]
    dev = cost_reg.device
    prob = torch.empty((N, D, H, W), dtype=torch.float32, device=dev)
    off = torch.empty((N, D, H, W), dtype=torch.float32, device=dev)
    est_depth = torch.empty((N, topk, H, W), dtype=torch.float32, device=dev)
    est_dens = torch.empty((N, topk, H, W), dtype=torch.float32, device=dev)
    est_idx = torch.empty((N, topk, H, W), dtype=torch.int32, device=dev)
    avg = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_depth_prob_topk_strided_f32(_lib.ptr(cost_reg), _lib.ptr(off_logit), view_stride,
                                                                  _lib.ptr(prob), _lib.ptr(off), _lib.ptr(est_depth),
                                                                  _lib.ptr(est_dens), _lib.ptr(est_idx), _lib.ptr(avg), N, D, H,
                                                                  W, topk, near, interval, stream(cost_reg)), "depth_prob_topk")
    return prob, off, est_depth, est_dens, est_idx, avg


@depth_prob_topk.register_fake
def _(cost_reg, off_logit, near, interval, topk):
    N, D, H, W = cost_reg.shape
    e = cost_reg.new_empty
    return (e((N, D, H, W)), e((N, D, H, W)), e((N, topk, H, W)), e((N, topk, H, W)),
            cost_reg.new_empty((N, topk, H, W), dtype=torch.int32), e((N, H, W)))


@torch.library.custom_op(f"{_NS}::sample_depth_prob", mutates_args=(), device_types="cuda")
def sample_depth_prob(prob: Tensor, off: Tensor, near: float, interval: float,
                      topk: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """a6+a7 on ready-made probabilities (mvsdet.py:266-283, 298-317) -> est_depth, est_dens (N,topk,H,W),
    est_idx int32, avg_depth (N,H,W)."""
    req(prob, "prob", dim=4)
    req(off, "off", dim=4)
    if prob.shape != off.shape:
        raise ValueError("sample_depth_prob: prob / off shape mismatch")
    N, D, H, W = prob.shape
    prob, off = prob.contiguous(), off.contiguous()
    dev = prob.device
    est_depth = torch.empty((N, topk, H, W), dtype=torch.float32, device=dev)
    est_dens = torch.empty((N, topk, H, W), dtype=torch.float32, device=dev)
    est_idx = torch.empty((N, topk, H, W), dtype=torch.int32, device=dev)
    avg = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_sample_depth_prob_f32(_lib.ptr(prob), _lib.ptr(off), _lib.ptr(est_depth),
                                                            _lib.ptr(est_dens), _lib.ptr(est_idx), _lib.ptr(avg), N, D, H,
                                                            W, topk, near, interval, stream(prob)), "sample_depth_prob")
    return est_depth, est_dens, est_idx, avg


@sample_depth_prob.register_fake
def _(prob, off, near, interval, topk):
    N, D, H, W = prob.shape
    e = prob.new_empty
    return e((N, topk, H, W)), e((N, topk, H, W)), prob.new_empty((N, topk, H, W), dtype=torch.int32), e((N, H, W))


def _sdp_setup(ctx, inputs, output):
    prob, off, near, interval, topk = inputs
    ctx.save_for_backward(prob, off, output[2])
    ctx.near, ctx.interval = near, interval


def _sdp_bwd(ctx, g_depth, g_dens, g_idx, g_avg):
    # gradients w.r.t. prob and off directly (no softmax / sigmoid Jacobian), in plain tensor ops:
    # est_dens = prob[idx]; est_depth = idx*iv + near + off[idx]*iv; avg = sum_d prob_d * depth_d
    prob, off, est_idx = ctx.saved_tensors
    iv, near = ctx.interval, ctx.near
    idx = est_idx.long()
    gp = torch.zeros_like(prob)
    go = torch.zeros_like(prob)
    if g_dens is not None:
        gp.scatter_add_(1, idx, g_dens)
    if g_depth is not None:
        go.scatter_add_(1, idx, g_depth * iv)
    if g_avg is not None:
        d = torch.arange(prob.shape[1], device=prob.device, dtype=torch.float32).view(1, -1, 1, 1)
        gp += g_avg.unsqueeze(1) * ((d * iv + near) + off * iv)
        go += g_avg.unsqueeze(1) * prob * iv
    return gp, go, None, None, None


sample_depth_prob.register_autograd(_sdp_bwd, setup_context=_sdp_setup)


@torch.library.custom_op(f"{_NS}::depth_prob_topk_backward", mutates_args=(), device_types="cuda")
def depth_prob_topk_backward(prob: Tensor, off: Tensor, est_idx: Tensor, g_prob: Tensor, g_depth: Tensor,
                             g_dens: Tensor, g_avg: Tensor, near: float, interval: float) -> Tuple[Tensor, Tensor]:
    N, D, H, W = prob.shape
    topk = est_idx.shape[1]
    g_cost = torch.empty_like(prob)
    g_off = torch.empty_like(prob)
    g_prob, g_depth, g_dens, g_avg = g_prob.contiguous(), g_depth.contiguous(), g_dens.contiguous(), g_avg.contiguous()
    with torch.cuda.device(prob.device):
        _lib.check(_lib.load().mvsdet_depth_prob_topk_bwd_f32(
            _lib.ptr(prob), _lib.ptr(off), _lib.ptr(est_idx), _lib.ptr(g_prob), _lib.ptr(g_depth), _lib.ptr(g_dens),
            _lib.ptr(g_avg), _lib.ptr(g_cost), _lib.ptr(g_off), N, D, H, W, topk, near, interval, stream(prob)),
            "depth_prob_topk_backward")
    return g_cost, g_off


@depth_prob_topk_backward.register_fake
def _(prob, off, est_idx, g_prob, g_depth, g_dens, g_avg, near, interval):
    return torch.empty_like(prob), torch.empty_like(prob)


def _dp_setup(ctx, inputs, output):
    cost_reg, off_logit, near, interval, topk = inputs
    prob, off, est_depth, est_dens, est_idx, avg = output
    ctx.save_for_backward(prob, off, est_idx)
    ctx.near, ctx.interval = near, interval


def _dp_bwd(ctx, g_prob, g_off, g_depth, g_dens, g_idx, g_avg):
    prob, off, est_idx = ctx.saved_tensors

    def z(g, like_shape):
        return torch.zeros(like_shape, dtype=torch.float32, device=prob.device) if g is None else g

    N, D, H, W = prob.shape
    k = est_idx.shape[1]
    g_cost, g_offl = depth_prob_topk_backward(prob, off, est_idx, z(g_prob, prob.shape), z(g_depth, (N, k, H, W)),
                                              z(g_dens, (N, k, H, W)), z(g_avg, (N, H, W)), ctx.near, ctx.interval)
    if g_off is not None:  # direct gradient on the sigmoid output
        g_offl = g_offl + g_off * off * (1.0 - off)
    return g_cost, g_offl, None, None, None


depth_prob_topk.register_autograd(_dp_bwd, setup_context=_dp_setup)


# ------------------------------------------------------------------------------------------- depth supervision (csrc/depthloss.hip)
DEPTH_LOSS_L1, DEPTH_LOSS_SMOOTH_L1 = 0, 1   # include/mvsdet_hip.h: MVSDET_DEPTH_LOSS_*


def _check_depth_loss(name: str, est: Tensor, gt: Tensor, mask: Optional[Tensor], kind: int):
    req(est, "est", dim=3)
    req(gt, "gt", dim=3)
    if kind not in (DEPTH_LOSS_L1, DEPTH_LOSS_SMOOTH_L1):
        raise ValueError(f"{name}: kind must be {DEPTH_LOSS_L1} (l1) or {DEPTH_LOSS_SMOOTH_L1} (smooth_l1), got {kind}")
    if gt.shape[0] != est.shape[0]:
        raise ValueError(f"{name}: est {tuple(est.shape)} and gt {tuple(gt.shape)} disagree on the number of views")
    if kind == DEPTH_LOSS_SMOOTH_L1:
        if mask is None:
            raise ValueError(f"{name}: smooth_l1 needs a mask")
        req(mask, "mask", dim=3)
        if gt.shape != est.shape or mask.shape != est.shape:
            raise ValueError(f"{name}: smooth_l1 takes gt and mask at the shape of est {tuple(est.shape)}, got {tuple(gt.shape)} / "
                             f"{tuple(mask.shape)}")
    elif mask is not None:
        raise ValueError(f"{name}: l1 takes its mask from the resized gt (> 0); pass mask=None")
    N, h, w = est.shape
    return N, h, w, int(gt.shape[1]), int(gt.shape[2])


@torch.library.custom_op(f"{_NS}::depth_loss", mutates_args=(), device_types="cuda")
def depth_loss(est: Tensor, gt: Tensor, mask: Optional[Tensor], kind: int) -> Tuple[Tensor, Tensor]:
    """One scene of the reference's depth objectives -> (loss () fp32, count () int32).  est (N,h,w) any strides (the crop of a
    padded map is read in place).  kind 0 (l1, MVSDet.depth_loss_func_new, mvsdet.py:893-915): gt (N,Hg,Wg) any strides and size is
    resized to (h,w) as F.interpolate(mode='bilinear') does; mask = resized > 0; mean of |est - resized|; `mask` must be None.
    kind 1 (smooth_l1, mvsnet_loss, mvs_models/mvsnet.py:292-294): gt, mask (N,h,w); mean over mask > 0.5 of smooth-L1 (beta 1).
    Two launches on the current stream, no atomics, no host synchronisation; an empty mask gives NaN and count 0.
    Differentiable in est only."""
    N, h, w, Hg, Wg = _check_depth_loss("depth_loss", est, gt, mask, kind)
    dev = est.device
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    count = torch.empty((), dtype=torch.int32, device=dev)
    ws_bytes = int(lib.mvsdet_depth_loss_workspace_bytes(N, h, w))
    workspace = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_depth_loss_f32(
            _lib.ptr(est), _lib.strides3(est), _lib.ptr(gt), _lib.strides3(gt), _lib.ptr(mask),
            None if mask is None else _lib.strides3(mask), _lib.ptr(loss), _lib.ptr(count), _lib.ptr(workspace), ws_bytes,
            N, h, w, Hg, Wg, kind, stream(est)), "depth_loss")
    return loss, count


@depth_loss.register_fake
def _(est, gt, mask, kind):
    return est.new_empty(()), est.new_empty((), dtype=torch.int32)


@torch.library.custom_op(f"{_NS}::depth_loss_backward", mutates_args=(), device_types="cuda")
def depth_loss_backward(est: Tensor, gt: Tensor, mask: Optional[Tensor], count: Tensor, g_loss: Tensor, kind: int) -> Tensor:
    """d loss / d est of `depth_loss` -> (N,h,w) fp32, dense: 0 outside the mask, (g_loss / count) * sign(est - g) (l1) or
    * clamp(est - gt, -1, 1) (smooth_l1) inside.  count () int32 as the forward returned it and g_loss () fp32 are read on the
    device.  One launch."""
    N, h, w, Hg, Wg = _check_depth_loss("depth_loss_backward", est, gt, mask, kind)
    req(g_loss, "g_loss")
    if count.dtype != torch.int32 or count.numel() != 1 or g_loss.numel() != 1 or count.device != est.device:
        raise ValueError("depth_loss_backward: count must be one int32 and g_loss one float32 on the device of est")
    grad = torch.empty((N, h, w), dtype=torch.float32, device=est.device)
    with torch.cuda.device(est.device):
        _lib.check(_lib.load().mvsdet_depth_loss_bwd_f32(
            _lib.ptr(est), _lib.strides3(est), _lib.ptr(gt), _lib.strides3(gt), _lib.ptr(mask),
            None if mask is None else _lib.strides3(mask), _lib.ptr(g_loss), _lib.ptr(count), _lib.ptr(grad), N, h, w, Hg, Wg, kind,
            stream(est)), "depth_loss_backward")
    return grad


@depth_loss_backward.register_fake
def _(est, gt, mask, count, g_loss, kind):
    return est.new_empty(tuple(est.shape))


def _dl_setup(ctx, inputs, output):
    est, gt, mask, kind = inputs
    if gt.requires_grad or (mask is not None and mask.requires_grad):
        raise RuntimeError("depth_loss: the ground truth and the mask carry no gradient (the reference gives them none); "
                           "detach them")
    ctx.save_for_backward(est, gt, mask, output[1])
    ctx.kind = kind


def _dl_bwd(ctx, g_loss, g_count):
    est, gt, mask, count = ctx.saved_tensors
    return depth_loss_backward(est, gt, mask, count, g_loss.contiguous(), ctx.kind), None, None, None


depth_loss.register_autograd(_dl_bwd, setup_context=_dl_setup)
