"""NerfDetHead._get_targets / _loss_by_feat_single (nerfdet_head.py:206-257, 473-562) on csrc/assign.hip: three launches for the
targets, two for the losses' sums, one for their gradients, on the current stream, no host synchronisation, the same bits from run
to run.  The `_rotated` functions are ImVoxelHead_ARKit's (:779-846, 1029-1185; RotatedIoU3DLoss) on the same kernels instantiated
for 7-value boxes."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch
from torch import Tensor

from ._common import _lib, req, stream, to_device
from .detect import DETECT_MAX_LEVELS, detect_level_geometry


ASSIGN_MAX_BOXES = 1024   # MVSDET_ASSIGN_MAX_BOXES: ground-truth boxes of one scene (staged in LDS by assign_pick_kernel)


class HeadTargets(NamedTuple):
    """Targets of every point of a batch (P = the levels' points concatenated in order, a level's voxels x-major): labels (B,P)
    int64 (-1: no box), box_index (B,P) int32 (-1), center_targets (B,P), bbox_targets (B,P,6) (x1, y1, z1, x2, y2, z2; zero
    where no box), and geom (B,L,6), the device copy of detect_level_geometry the targets were made with.  From
    head_targets_rotated: bbox_targets (B,P,7) = the chosen ground-truth row (x, y, z, dx, dy, dz, yaw), center_targets -1 where no
    box is assigned."""
    labels: Tensor
    box_index: Tensor
    center_targets: Tensor
    bbox_targets: Tensor
    geom: Tensor


class HeadLossSums(NamedTuple):
    """Unnormalised sums of every scene: center (B,) = the centerness BCE over positive points, bbox (B,) = centerness target *
    (1 - IoU) over positive points, cls (B,) = the focal loss over valid points and classes -- these three carry gradients to the
    nine maps -- and weight_sum (B,) = the positive points' centerness targets, n_pos, n_valid (B,) int32."""
    center: Tensor
    bbox: Tensor
    cls: Tensor
    weight_sum: Tensor
    n_pos: Tensor
    n_valid: Tensor


def check_box_limit(n_boxes: int) -> None:
    if n_boxes > ASSIGN_MAX_BOXES:
        raise ValueError(f"head_targets: {n_boxes} ground-truth boxes in one scene, above the limit ASSIGN_MAX_BOXES = "
                         f"{ASSIGN_MAX_BOXES} (MVSDET_ASSIGN_MAX_BOXES: the boxes of a scene are staged in LDS)")


def head_targets(featmap_sizes, origins, gt_boxes: Tensor, gt_volumes: Tensor, gt_labels: Tensor, gt_counts: Tensor,
                 pts_assign_threshold: int, pts_center_threshold: int) -> HeadTargets:
    """NerfDetHead._get_targets of every scene of a batch (nerfdet_head.py:473-562).  featmap_sizes: (X, Y, Z) per level; origins:
    one float32 (3,) origin per scene; gt_boxes (B,G,6) = cat(gravity_center, tensor[:, 3:6]), gt_volumes (B,G), gt_labels (B,G)
    int64, padded to the batch's largest G <= ASSIGN_MAX_BOXES (checked on the shape, before any launch); gt_counts (B,) int32 =
    the boxes of every scene.  CUDA tensors only.  Equal volumes: the lowest box index wins (torch.min on the CPU; the reference
    leaves it to the backend).  A scene without boxes gets label -1 everywhere (the reference raises on the empty min).  A box with
    at most pts_center_threshold points inside on its best level keeps them all."""
    return _head_targets(featmap_sizes, origins, gt_boxes, None, gt_volumes, gt_labels, gt_counts, pts_assign_threshold,
                         pts_center_threshold)


def head_targets_rotated(featmap_sizes, origins, gt_boxes: Tensor, gt_rot: Tensor, gt_volumes: Tensor, gt_labels: Tensor,
                         gt_counts: Tensor, pts_assign_threshold: int, pts_center_threshold: int) -> HeadTargets:
    """ImVoxelHead_ARKit._get_targets of every scene of a batch (nerfdet_head.py:1107-1185): as head_targets, with gt_boxes (B,G,7) =
    cat(gravity_center, tensor[:, 3:7]) and gt_rot (B,G,2) = (cos(yaw), sin(yaw)), which the caller computes (torch.cos / torch.sin,
    as rotation_3d_in_axis does) so that no transcendental is evaluated on the way to a label.  Face distances in the box's own
    frame; the top-k takes min(pts_center_threshold + 1, P) values; bbox_targets (B,P,7) are the chosen ground-truth rows,
    center_targets -1 where no box is assigned."""
    return _head_targets(featmap_sizes, origins, gt_boxes, gt_rot, gt_volumes, gt_labels, gt_counts, pts_assign_threshold,
                         pts_center_threshold)


def _head_targets(featmap_sizes, origins, gt_boxes, gt_rot, gt_volumes, gt_labels, gt_counts, pts_assign_threshold,
                  pts_center_threshold):
    rotated = gt_rot is not None
    fname, nbox = ("head_targets_rotated", 7) if rotated else ("head_targets", 6)
    B = len(origins)
    L = len(featmap_sizes)
    if not (1 <= L <= DETECT_MAX_LEVELS):
        raise ValueError(f"{fname}: 1..{DETECT_MAX_LEVELS} levels needed")
    if gt_boxes.dim() != 3:
        raise ValueError(f"{fname}: gt_boxes must be (B, G, {nbox}) (got shape {tuple(gt_boxes.shape)})")
    G = int(gt_boxes.shape[1])
    check_box_limit(G)   # from the shape, before anything else
    req(gt_boxes, "gt_boxes", dim=3)
    req(gt_volumes, "gt_volumes", dim=2)
    req(gt_labels, "gt_labels", dtype=torch.int64, dim=2)
    req(gt_counts, "gt_counts", dtype=torch.int32, dim=1)
    if rotated:
        req(gt_rot, "gt_rot", dim=3)
    if gt_boxes.shape != (B, G, nbox) or gt_volumes.shape != (B, G) or gt_labels.shape != (B, G) or gt_counts.shape != (B,) \
            or (rotated and gt_rot.shape != (B, G, 2)):
        raise ValueError(f"{fname}: gt_boxes {tuple(gt_boxes.shape)}, gt_volumes {tuple(gt_volumes.shape)}, gt_labels "
                         f"{tuple(gt_labels.shape)}, gt_counts {tuple(gt_counts.shape)} for {B} scenes")
    dev = gt_boxes.device
    sizes = [tuple(int(v) for v in s) for s in featmap_sizes]
    dims = [v for s in sizes for v in s]
    P = sum(s[0] * s[1] * s[2] for s in sizes)
    geom = to_device(detect_level_geometry(sizes, origins), dev)
    lib = _lib.load()
    ws = torch.empty(int(lib.mvsdet_head_targets_workspace_bytes(B, G)), dtype=torch.uint8, device=dev)
    labels = torch.empty((B, P), dtype=torch.int64, device=dev)
    box_index = torch.empty((B, P), dtype=torch.int32, device=dev)
    center_t = torch.empty((B, P), dtype=torch.float32, device=dev)
    bbox_t = torch.empty((B, P, nbox), dtype=torch.float32, device=dev)
    boxes, volumes, glabels = gt_boxes.contiguous(), gt_volumes.contiguous(), gt_labels.contiguous()
    gt = [_lib.ptr(boxes) if G else None]
    if rotated:
        rot = gt_rot.contiguous()
        gt.append(_lib.ptr(rot) if G else None)
    entry = lib.mvsdet_head_targets_rotated_f32 if rotated else lib.mvsdet_head_targets_f32
    with torch.cuda.device(dev):
        _lib.check(entry(
            (ctypes.c_int * len(dims))(*dims), _lib.ptr(geom), B, L, *gt, _lib.ptr(volumes) if G else None,
            _lib.ptr(glabels) if G else None, _lib.ptr(gt_counts.contiguous()), G, int(pts_assign_threshold), int(pts_center_threshold),
            _lib.ptr(labels), _lib.ptr(box_index), _lib.ptr(center_t), _lib.ptr(bbox_t), _lib.ptr(ws) if ws.numel() else None,
            ws.numel(), stream(gt_boxes)), fname)
    return HeadTargets(labels, box_index, center_t, bbox_t, geom)


def _loss_maps(center_preds, bbox_preds, cls_preds, valid_pred, targets: HeadTargets, nreg: int = 6):
    L = len(center_preds)
    if not (1 <= L <= DETECT_MAX_LEVELS) or len(bbox_preds) != L or len(cls_preds) != L:
        raise ValueError(f"head_loss: 1..{DETECT_MAX_LEVELS} levels of center / bbox / cls maps needed")
    req(valid_pred, "valid_pred", dtype=valid_pred.dtype, dim=5)
    B = valid_pred.shape[0]
    maps = []
    for lvl, (c, r, k) in enumerate(zip(center_preds, bbox_preds, cls_preds)):
        for t, name, ch in ((c, "center", 1), (r, "bbox", nreg), (k, "cls", int(cls_preds[0].shape[1]))):
            req(t, f"{name}_preds[{lvl}]", dim=5)
            if t.shape[0] != B or t.shape[1] != ch or t.shape[2:] != c.shape[2:]:
                raise ValueError(f"head_loss: {name}_preds[{lvl}] has shape {tuple(t.shape)}")
        maps += [c, r, k]
    P = sum(int(c.shape[2] * c.shape[3] * c.shape[4]) for c in center_preds)
    if targets.labels.shape != (B, P) or targets.geom.shape != (B, L, 6) or targets.bbox_targets.shape != (B, P, nreg):
        raise ValueError(f"head_loss: targets of shape {tuple(targets.labels.shape)} for {B} scenes of {P} points")
    return maps


class _HeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, valid, labels, center_t, bbox_t, geom, gamma, alpha, rotated, *maps):
        L = len(maps) // 3
        maps = [m.contiguous() for m in maps]
        B, C = int(valid.shape[0]), int(maps[2].shape[1])
        dims = [int(v) for l in range(L) for v in maps[3 * l].shape[2:]]
        P = int(labels.shape[1])
        dev = valid.device
        lib = _lib.load()
        ws = torch.empty(int(lib.mvsdet_head_loss_workspace_bytes(B, P)), dtype=torch.uint8, device=dev)
        sums = torch.empty((B, 4), dtype=torch.float32, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
        arr = ctypes.c_void_p * L
        ctx.args = (arr, dims, B, L, C, [int(v) for v in valid.shape[2:]], float(gamma), float(alpha), bool(rotated))
        with torch.cuda.device(dev):
            _lib.check((lib.mvsdet_head_loss_rotated_f32 if rotated else lib.mvsdet_head_loss_f32)(
                arr(*[maps[3 * l].data_ptr() for l in range(L)]), arr(*[maps[3 * l + 1].data_ptr() for l in range(L)]),
                arr(*[maps[3 * l + 2].data_ptr() for l in range(L)]), (ctypes.c_int * len(dims))(*dims), _lib.ptr(valid), _lib.ptr(geom),
                B, L, C, *ctx.args[5], _lib.ptr(labels), _lib.ptr(center_t), _lib.ptr(bbox_t), float(gamma), float(alpha),
                _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), stream(valid)), "head_loss")
        ctx.save_for_backward(valid, labels, center_t, bbox_t, geom, *maps)
        out = (sums[:, 0], sums[:, 1], sums[:, 2], sums[:, 3], counts[:, 0], counts[:, 1])
        ctx.mark_non_differentiable(*out[3:])
        return out

    @staticmethod
    def backward(ctx, g_center, g_bbox, g_cls, *unused):
        valid, labels, center_t, bbox_t, geom, *maps = ctx.saved_tensors
        arr, dims, B, L, C, vdims, gamma, alpha, rotated = ctx.args
        lib = _lib.load()
        coef = torch.stack([g_center, g_bbox, g_cls], dim=1).float().contiguous()
        grads = [torch.empty_like(m) for m in maps]
        with torch.cuda.device(valid.device):
            _lib.check((lib.mvsdet_head_loss_rotated_backward_f32 if rotated else lib.mvsdet_head_loss_backward_f32)(
                arr(*[maps[3 * l].data_ptr() for l in range(L)]), arr(*[maps[3 * l + 1].data_ptr() for l in range(L)]),
                arr(*[maps[3 * l + 2].data_ptr() for l in range(L)]), (ctypes.c_int * len(dims))(*dims), _lib.ptr(valid), _lib.ptr(geom),
                B, L, C, *vdims, _lib.ptr(labels), _lib.ptr(center_t), _lib.ptr(bbox_t), gamma, alpha, _lib.ptr(coef),
                arr(*[grads[3 * l].data_ptr() for l in range(L)]), arr(*[grads[3 * l + 1].data_ptr() for l in range(L)]),
                arr(*[grads[3 * l + 2].data_ptr() for l in range(L)]), stream(valid)), "head_loss_backward")
        return (None,) * 8 + tuple(grads)


def head_loss(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, targets: HeadTargets, gamma: float = 2.0,
              alpha: float = 0.25) -> HeadLossSums:
    """The sums of NerfDetHead._loss_by_feat_single (nerfdet_head.py:206-257) for every scene of a batch, with gradients to the nine
    maps.  center_preds / bbox_preds / cls_preds: per level (B,1|6|C,X,Y,Z) float32 CUDA maps, read in place; valid_pred
    (B,1,X,Y,Z): the stacked view counts; targets: ops.head_targets of the same level sizes.  Positive = label >= 0 and
    nn.Upsample(trilinear)(valid_pred).round().bool().  The caller divides: center / n_pos', cls / n_pos' with n_pos' =
    max(n_pos, 1) (averaged over the ranks first), bbox / weight_sum (NerfDetHeadConvs.loss_by_feat)."""
    maps = _loss_maps(center_preds, bbox_preds, cls_preds, valid_pred, targets)
    valid = valid_pred.float().contiguous()
    return HeadLossSums(*_HeadLoss.apply(valid, targets.labels, targets.center_targets, targets.bbox_targets, targets.geom,
                                         float(gamma), float(alpha), False, *maps))


def head_loss_rotated(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, targets: HeadTargets, gamma: float = 2.0,
                      alpha: float = 0.25) -> HeadLossSums:
    """The sums of ImVoxelHead_ARKit._loss_by_feat_single (nerfdet_head.py:779-846) for every scene of a batch, with gradients to
    the nine maps: as head_loss, with bbox maps of 7 channels (six distances, heading) and targets of ops.head_targets_rotated.
    bbox (B,) = centerness target * (1 - IoU3D) over positive points, IoU3D the rotated 3-D IoU of RotatedIoU3DLoss between the
    decoded box (_bbox_pred_to_bbox, :1029-1055) and its ground-truth row: the true intersection area of the two rectangles times
    the z overlap over the union of the volumes.  Finite values and gradients at every pair, degenerate ones included (identical
    boxes, shared or touching edges, headings a multiple of pi/2 apart, a target of zero size: csrc/assign.hip's header); the
    targets receive no gradient."""
    maps = _loss_maps(center_preds, bbox_preds, cls_preds, valid_pred, targets, nreg=7)
    valid = valid_pred.float().contiguous()
    return HeadLossSums(*_HeadLoss.apply(valid, targets.labels, targets.center_targets, targets.bbox_targets, targets.geom,
                                         float(gamma), float(alpha), True, *maps))
