"""The convolutions of the detection head that consume the neck's outputs ("neck + head"):
`NerfDetHead._init_layers / _forward_single / forward` of projects/NeRF-Det/nerfdet/nerfdet_head.py:90-118, and the 7-DoF
`ImVoxelHead_ARKit` (:663-700: the same three layers with n_reg_outs = 7; `arkit_head=True`).  Per neck level:

    centerness = conv_center(x)               Conv3d(C -> 1,         k=3, p=1, no bias)
    bbox       = exp(scale_l(conv_reg(x)))    Conv3d(C -> n_reg_outs, k=3, p=1, no bias), one learnable scalar per level;
                                              ImVoxelHead_ARKit: exp(scale_l(.)) on the 6 distances, the angle channel raw
    cls        = conv_cls(x)                  Conv3d(C -> n_classes,  k=3, p=1, bias)

Target assignment and the three losses (`loss_by_feat`, nerfdet_head.py:152-257, 473-562: AxisAlignedIoULoss, FocalLoss, sigmoid
CrossEntropyLoss) run on csrc/assign.hip for the ScanNet head (`ops.head_targets`, `ops.head_loss`): six launches per batch, no host
synchronisation, the same bits from run to run.  The ARKit head's objective (:779-846, 1029-1185: targets in each box's rotated
frame, RotatedIoU3DLoss) runs on the same kernels instantiated for 7-value boxes (`ops.head_targets_rotated`,
`ops.head_loss_rotated`), on ROCm tensors only.
`predict_by_feat` (nerfdet_head.py:301-420, 564-628: scores, top-k, decode, aligned 3-D NMS) runs on csrc/detect.hip for the
ScanNet head (`ops.head_predict`), and for the ARKit head (:902-1056, 1190-1243: all class scores of a top-k point, rotated decode,
mmcv's nms3d per class) on its rotated kernels (`ops.head_predict_rotated`).  Parameter names equal the reference's
(`conv_center.weight`, `conv_reg.weight`, `conv_cls.weight/bias`, `scales.<l>.scale`), so a checkpoint's `bbox_head.*` entries load.

1 + 6 + 18 = 25 output channels are no GEMM shape for a library (nine launches per scene).  In eval mode without
autograd, on a ROCm device, the three convolutions of a level run as ONE 3x3x3 MFMA convolution whose 64 output channels
are [center | reg | cls | zeros] -- the input is read once, the neck's small grids take the split over input channels of
csrc/costreg_conv0.hip -- followed by the slices, the exponential and the bias: 5 GFLOP per scene, 13 GFLOP padded.

Under autograd with `autograd_route` "hip" (initial value from MVSDET_DETECTOR_AUTOGRAD, "aten" by default; neck.py), any CUDA fp32
call runs the same fused convolution on the bf16x3 forward / input-gradient / weight-gradient kernels (`layers.ConvK3S1`) on
torch.cat(conv_center.weight, conv_reg.weight, conv_cls.weight, zeros to 64 rows), concatenated per call: autograd hands the weight
gradient back to the three parameters, and the bias, `Scale` and exp stay elementwise ATen operations.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import layers, ops
from .ops._common import to_device
from .layers import ConvK3S1, DerivedTensorsMixin, autograd_route_from_env, await_made, check_route, fp32_under_autocast, mark_made


class Scale(nn.Module):
    """mmcv.cnn.Scale: a learnable scalar factor (parameter name `scale`)."""

    def __init__(self, scale: float = 1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x: Tensor) -> Tensor:
        return x * self.scale


# The fused 128 -> 25 (padded to 64) convolution of a level on the bf16 matrix cores with three-term split operands
# (outputs within ~1e-5 of the fp32 sums' scale; the small levels split over the input channels) instead of the fp32 MFMA.
HEAD_BF16X3 = True


class NerfDetHeadConvs(DerivedTensorsMixin, nn.Module):
    """The learnable layers of NerfDetHead and their forward pass (nerfdet_head.py:94-118)."""

    def __init__(self, n_classes: int = 18, n_levels: int = 3, n_channels: int = 128, n_reg_outs: int = 6,
                 arkit_head: bool = False, test_cfg=None, pts_assign_threshold: int = 27, pts_center_threshold: int = 18,
                 center_loss_weight: float = 1.0, bbox_loss_weight: float = 1.0, cls_loss_weight: float = 1.0,
                 focal_gamma: float = 2.0, focal_alpha: float = 0.25):
        super().__init__()
        # loss_by_feat: both thresholds of _get_targets, loss_weight of the three terms, FocalLoss' gamma and alpha
        self.pts_assign_threshold, self.pts_center_threshold = int(pts_assign_threshold), int(pts_center_threshold)
        self.center_loss_weight, self.bbox_loss_weight = float(center_loss_weight), float(bbox_loss_weight)
        self.cls_loss_weight, self.focal_gamma, self.focal_alpha = float(cls_loss_weight), float(focal_gamma), float(focal_alpha)
        self.test_cfg = test_cfg   # nms_pre, score_thr, iou_thr (mvsdet_res50_2x_low_res_depth.py:61): predict_by_feat
        self.n_classes, self.n_levels, self.n_reg_outs = n_classes, n_levels, n_reg_outs
        self.arkit_head = bool(arkit_head)   # ImVoxelHead_ARKit._forward_single (nerfdet_head.py:677-692)
        self.conv_center = nn.Conv3d(n_channels, 1, 3, padding=1, bias=False)
        self.conv_reg = nn.Conv3d(n_channels, n_reg_outs, 3, padding=1, bias=False)
        self.conv_cls = nn.Conv3d(n_channels, n_classes, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in range(n_levels)])
        self._fused = None   # (key, permuted fused weight); dropped on train()/eval() and load_state_dict
        self.autograd_route = autograd_route_from_env()   # "aten" | "hip": the route under autograd (module docstring)
        self._init_derived_hooks()

    def init_weights(self):
        """nerfdet_head.py:104-108: normal_init(std=0.01), classification bias for a prior probability of 0.01."""
        for conv in (self.conv_center, self.conv_reg, self.conv_cls):
            nn.init.normal_(conv.weight, 0.0, 0.01)
        nn.init.constant_(self.conv_cls.bias, float(-torch.log(torch.tensor((1 - 0.01) / 0.01))))

    def _fused_weight(self) -> Tensor:
        ws = (self.conv_center.weight, self.conv_reg.weight, self.conv_cls.weight)
        key = tuple((w.data_ptr(), w._version, w.device) for w in ws)
        if self._fused is None or self._fused[0] != key or self._fused[2] != HEAD_BF16X3:
            w = torch.cat([t.detach() for t in ws], 0)
            pad = (-w.shape[0]) % 64
            if pad:
                w = torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], 0)
            # cut into bf16 pieces in the bf16x3 kernel's layout (csrc/costreg_bf16.hip; HEAD_BF16X3), or permuted for the fp32 MFMA
            self._fused = (key, ops.split_conv_weight(w) if HEAD_BF16X3 else ops.permute_conv_weight(w), HEAD_BF16X3)
            mark_made(self._fused[1])
        await_made(self._fused[1])   # computed on another stream a moment ago: this stream waits for it (layers._PENDING)
        return self._fused[1]

    def _route(self, x) -> str:   # the autograd kernels: keyed on autograd, whatever `training` is (`layers.decide`)
        return layers.decide(layers.call_facts(x, self), other=check_route(self) == "hip")

    def _fused_weight_autograd(self) -> Tensor:
        """[center | reg | cls | zeros] as ONE (64 m, C, 3, 3, 3) weight in the autograd graph (made per call: the weights change
        every step)."""
        w = torch.cat([self.conv_center.weight, self.conv_reg.weight, self.conv_cls.weight], 0)
        pad = (-w.shape[0]) % 64
        if pad:
            w = torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], 0)
        return w

    def _forward_single_hip(self, x: Tensor, scale: Scale, w: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        if x.shape[1] % 64:
            raise ValueError(f"NerfDetHeadConvs (autograd_route='hip'): {x.shape[1]} input channels, a multiple of 64 needed")
        layers.count_hip()
        y = ConvK3S1.apply(x, w, True)
        r, c = self.n_reg_outs, self.n_classes
        center = y[:, :1]
        cls = y[:, 1 + r:1 + r + c] + self.conv_cls.bias.view(1, -1, 1, 1, 1)
        if self.arkit_head:
            reg = torch.cat((torch.exp(scale(y[:, 1:7])), y[:, 7:1 + r]), dim=1)
        else:
            reg = torch.exp(scale(y[:, 1:1 + r]))
        return center, reg, cls

    def _forward_single(self, x: Tensor, scale: Scale, route: str) -> Tuple[Tensor, Tensor, Tensor]:
        if route == "eval":
            layers.count_hip()
            if HEAD_BF16X3:
                y = ops.conv3d_k3_bf16x3(x, self._fused_weight(), None, None, False)
            else:
                y = ops.conv3d_k3_mfma(x, self._fused_weight(), None, None, False)
            r, c = self.n_reg_outs, self.n_classes
            center = y[:, :1].contiguous()
            cls = y[:, 1 + r:1 + r + c] + self.conv_cls.bias.detach().view(1, -1, 1, 1, 1)
            if self.arkit_head:
                reg = torch.cat((torch.exp(y[:, 1:7] * scale.scale.detach()), y[:, 7:1 + r]), dim=1)
            else:
                reg = torch.exp(y[:, 1:1 + r] * scale.scale.detach())
            return center, reg, cls
        layers.record(self, route, "conv_center", "conv_reg", "conv_cls")
        if self.arkit_head:
            reg_final = self.conv_reg(x)
            return self.conv_center(x), torch.cat((torch.exp(scale(reg_final[:, :6])), reg_final[:, 6:]), dim=1), self.conv_cls(x)
        return self.conv_center(x), torch.exp(scale(self.conv_reg(x))), self.conv_cls(x)

    @fp32_under_autocast
    def forward(self, x: Sequence[Tensor]) -> Tuple[List[Tensor], List[Tensor], List[Tensor]]:
        """mmdet's multi_apply(self._forward_single, x, self.scales): a tuple of three per-level lists."""
        routes = [self._route(xi) for xi in x]
        w = self._fused_weight_autograd() if "grad" in routes else None
        res = [self._forward_single_hip(xi, s, w) if r == "grad" else self._forward_single(xi, s, r)
               for xi, s, r in zip(x, self.scales, routes)]
        return tuple(map(list, zip(*res)))

    def predict_by_feat(self, center_preds: List[List[Tensor]], bbox_preds: List[List[Tensor]], cls_preds: List[List[Tensor]],
                        valid_pred: Tensor, batch_input_metas: List[dict], **kwargs) -> List["SceneDetections"]:
        """NerfDetHead.predict_by_feat (nerfdet_head.py:301-420): boxes, scores and labels of every scene from the head's maps (per
        level (B,...) tensors) and valid_pred = torch.stack(valids).float() (B,1,X,Y,Z), on the HIP kernels of csrc/detect.hip.
        The selection is the reference's; the walk visits NaN scores first whatever their sign, takes -0 and +0 as equal, and
        orders equal scores by level, then voxel index (the reference's argsort leaves them unordered).  One host sync per batch.
        CUDA float32 maps only.
        ARKit head (ImVoxelHead_ARKit.predict_by_feat, nerfdet_head.py:902-1056, 1190-1243): 7-DoF boxes (x, y, z, dx, dy, dz,
        heading), class-major, per class in mmcv nms3d's pick order (equal class scores by level, then voxel index), boxed with
        box_dim=7, with_yaw=True.  Labels are int64 also for a scene without boxes, where the reference returns float32
        new_zeros((0,)).  Maps that are not on a ROCm device raise NotImplementedError: mmcv's nms3d has no CPU path either."""
        if self.arkit_head and not all(t.is_cuda for t in center_preds):
            raise NotImplementedError(
                "predict_by_feat: ImVoxelHead_ARKit's 7-DoF boxes go through mmcv's rotated BEV nms3d (nerfdet_head.py:1190-1243), "
                "which runs on ROCm tensors only (ops.nms3d); there is no CPU path")
        pred = predict_head_maps(center_preds, bbox_preds, cls_preds, valid_pred, batch_input_metas, self.test_cfg,
                                 rotated=self.arkit_head)
        return unpad_predictions(pred, batch_input_metas)

    def loss_by_feat(self, center_preds: List[Tensor], bbox_preds: List[Tensor], cls_preds: List[Tensor], valid_pred: Tensor,
                     batch_gt_instances_3d, batch_input_metas: List[dict], batch_gt_instances_ignore=None, **kwargs) -> dict:
        """NerfDetHead.loss_by_feat (nerfdet_head.py:152-257): dict(center_loss, bbox_loss, cls_loss), each the mean over the
        batch's scenes, from the head's maps (per level (B,...) CUDA float32 tensors), valid_pred (B,1,X,Y,Z) and per scene anything
        with `bboxes_3d` (`gravity_center`, `tensor`, `volume`) and `labels_3d`.  Targets and sums on csrc/assign.hip, no host
        synchronisation.  Per scene: center_loss = BCE-with-logits over positive points / (n_pos + eps), cls_loss = mmcv's sigmoid
        focal loss over valid points and classes / (n_pos + eps), n_pos = max(positive points, 1), averaged over the ranks of an
        initialised process group first (mmdet's reduce_mean); bbox_loss = sum w (1 - IoU) / (sum w + eps), w = the centerness
        target; eps = float32's machine epsilon, mmdet 3.x's weight_reduce_loss.  A scene without valid or positive points gives 0
        with zero gradients; one without boxes has no positive point (the reference raises there).  Equal box volumes at a point:
        the lowest box index.  batch_gt_instances_ignore is not read, as in the reference.
        ARKit head (ImVoxelHead_ARKit.loss_by_feat, nerfdet_head.py:779-900, 1029-1185): bbox maps of 7 channels, ground truth with
        yaw (`tensor[:, 3:7]`, with_yaw boxes), face distances and centerness in each box's own frame, the ground-truth row as box
        target, IoU = the rotated 3-D IoU of RotatedIoU3DLoss (mmcv's diff_iou_rotated_3d: the true intersection of the two
        rectangles times the z overlap).  Maps that are not on a ROCm device raise NotImplementedError: the rotated IoU has no CPU
        path here, as mmcv's own op has none."""
        if self.arkit_head and not all(t.is_cuda for t in center_preds):
            raise NotImplementedError(
                "loss_by_feat: ImVoxelHead_ARKit's RotatedIoU3DLoss (nerfdet_head.py:779-846, mmcv's diff_iou_rotated_3d) runs on "
                "ROCm tensors only (ops.head_loss_rotated); there is no CPU path")
        B = len(batch_input_metas)
        if len(batch_gt_instances_3d) != B:
            raise ValueError(f"loss_by_feat: {len(batch_gt_instances_3d)} ground-truth sets for {B} scenes")
        ops.check_box_limit(max([len(g.labels_3d) for g in batch_gt_instances_3d], default=0))   # before anything is launched
        for t in list(center_preds) + list(bbox_preds) + list(cls_preds) + [valid_pred]:
            if not t.is_cuda:
                raise RuntimeError(f"loss_by_feat: the head's maps must live on a ROCm device (got {t.device}); this package has no "
                                   "CPU path")
        if torch.is_autocast_enabled("cuda"):   # --amp: the loss computes in float32 (layers.fp32_under_autocast's rule)
            with torch.autocast("cuda", enabled=False):
                up = lambda ts: [t.float() for t in ts]
                return self.loss_by_feat(up(center_preds), up(bbox_preds), up(cls_preds), valid_pred, batch_gt_instances_3d,
                                         batch_input_metas, batch_gt_instances_ignore, **kwargs)
        dev = valid_pred.device
        sizes = [tuple(c.shape[2:]) for c in center_preds]
        origins = [scene_origin(m) for m in batch_input_metas]
        if self.arkit_head:
            gt_boxes, gt_rot, gt_volumes, gt_labels, gt_counts = pad_ground_truth_rotated(batch_gt_instances_3d, dev)
            targets = ops.head_targets_rotated(sizes, origins, gt_boxes, gt_rot, gt_volumes, gt_labels, gt_counts,
                                               self.pts_assign_threshold, self.pts_center_threshold)
            sums = ops.head_loss_rotated(center_preds, bbox_preds, cls_preds, valid_pred, targets, self.focal_gamma, self.focal_alpha)
        else:
            gt_boxes, gt_volumes, gt_labels, gt_counts = pad_ground_truth(batch_gt_instances_3d, dev)
            targets = ops.head_targets(sizes, origins, gt_boxes, gt_volumes, gt_labels, gt_counts, self.pts_assign_threshold,
                                       self.pts_center_threshold)
            sums = ops.head_loss(center_preds, bbox_preds, cls_preds, valid_pred, targets, self.focal_gamma, self.focal_alpha)
        eps = torch.finfo(torch.float32).eps
        n_pos = sums.n_pos.float()
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            torch.distributed.all_reduce(n_pos.div_(torch.distributed.get_world_size()), op=torch.distributed.ReduceOp.SUM)
        n_avg = n_pos.clamp(min=1.0) + eps
        return dict(center_loss=torch.mean(sums.center / n_avg * self.center_loss_weight),
                    bbox_loss=torch.mean(sums.bbox / (sums.weight_sum + eps) * self.bbox_loss_weight),
                    cls_loss=torch.mean(sums.cls / n_avg * self.cls_loss_weight))

    @staticmethod
    def flops(grid: Sequence[int], n_classes: int = 18, n_levels: int = 3, n_channels: int = 128, n_reg_outs: int = 6) -> float:
        v = sum((grid[0] >> i) * (grid[1] >> i) * (grid[2] >> i) for i in range(n_levels))
        return 54.0 * n_channels * (1 + n_reg_outs + n_classes) * v


def cfg_value(cfg, name: str):
    """test_cfg.<name> of an mmengine ConfigDict, a dict or any object with the attribute."""
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def scene_origin(meta: dict):
    """input_meta['lidar2img']['origin'] as the reference's torch.tensor(origin): float32 only (the dataset builds it so,
    scannet_multiview_dataset.py:153-157; a float64 origin would make the reference decode the boxes in float64)."""
    o = meta["lidar2img"]["origin"]
    t = o if isinstance(o, Tensor) else torch.tensor(o)
    if t.dtype != torch.float32:
        raise ValueError(f"predict_by_feat: lidar2img['origin'] must be float32 (got {t.dtype}); the reference would decode "
                         "the boxes in float64")
    return t


def predict_head_maps(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, batch_input_metas, test_cfg,
                      rotated: bool = False) -> ops.HeadPrediction:
    """The padded device result of predict_by_feat for the whole batch (no host sync): ops.head_predict (ARKit head, `rotated`:
    ops.head_predict_rotated) with the test_cfg's values."""
    if test_cfg is None:
        raise ValueError("predict_by_feat: a test_cfg with nms_pre, score_thr and iou_thr is needed")
    origins = [scene_origin(m) for m in batch_input_metas]
    predict = ops.head_predict_rotated if rotated else ops.head_predict
    return predict(center_preds, bbox_preds, cls_preds, valid_pred, origins, int(cfg_value(test_cfg, "nms_pre")),
                   float(cfg_value(test_cfg, "score_thr")), float(cfg_value(test_cfg, "iou_thr")))


def pad_ground_truth(batch_gt_instances_3d, device) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """What _get_targets reads of every scene's ground truth, by the reference's own torch expressions (nerfdet_head.py:497-500),
    padded to the batch's largest box count: boxes (B,G,6) = cat(gravity_center, tensor[:, 3:6]), volumes (B,G), labels (B,G) int64
    and the counts (B,) int32, made from the shapes; on `device` without a host synchronisation."""
    boxes, _, volumes, labels, counts = _pad_ground_truth(batch_gt_instances_3d, device, 6)
    return boxes, volumes, labels, counts


def pad_ground_truth_rotated(batch_gt_instances_3d, device) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """pad_ground_truth for ImVoxelHead_ARKit._get_targets (nerfdet_head.py:1133-1134): boxes (B,G,7) = cat(gravity_center,
    tensor[:, 3:7]), rot (B,G,2) = (cos(yaw), sin(yaw)) by torch.cos / torch.sin on the ground truth's own tensors where they
    live (what rotation_3d_in_axis calls), volumes, labels, counts."""
    return _pad_ground_truth(batch_gt_instances_3d, device, 7)


def _pad_ground_truth(batch_gt_instances_3d, device, nbox: int):
    rows = []
    for gt in batch_gt_instances_3d:
        b = gt.bboxes_3d
        if nbox == 7 and b.tensor.shape[1] < 7:
            raise ValueError(f"loss_by_feat: the ARKit head needs ground-truth boxes with yaw (tensor of 7 values, got "
                             f"{tuple(b.tensor.shape)})")
        boxes = torch.cat((b.gravity_center, b.tensor[:, 3:nbox]), dim=1).float()
        yaw = boxes[:, 6] if nbox == 7 else boxes[:, :0].reshape(-1)
        rot = torch.stack((torch.cos(yaw), torch.sin(yaw)), dim=-1) if nbox == 7 else boxes[:, :0]
        rows.append((boxes, b.volume.float().reshape(-1), gt.labels_3d.long().reshape(-1), rot))
    G = max([int(r[0].shape[0]) for r in rows], default=0)
    counts = torch.tensor([int(r[0].shape[0]) for r in rows], dtype=torch.int32)

    def pad(ts, width, dtype):
        out = [torch.cat([t.reshape((t.shape[0],) + width), t.new_zeros((G - t.shape[0],) + width)]) for t in ts]
        return to_device(torch.stack(out).to(dtype), device)

    return (pad([r[0] for r in rows], (nbox,), torch.float32), pad([r[3] for r in rows], (2,), torch.float32) if nbox == 7 else None,
            pad([r[1] for r in rows], (), torch.float32), pad([r[2] for r in rows], (), torch.int64), to_device(counts, device))


class SceneDetections:
    """mmengine's InstanceData as the reference fills it: bboxes_3d, scores_3d, labels_3d."""

    def __init__(self, bboxes_3d, scores_3d: Tensor, labels_3d: Tensor):
        self.bboxes_3d, self.scores_3d, self.labels_3d = bboxes_3d, scores_3d, labels_3d

    def keys(self):
        return ["bboxes_3d", "scores_3d", "labels_3d"]

    def __len__(self):
        return int(self.scores_3d.shape[0])

    def __repr__(self):
        return f"SceneDetections({len(self)} boxes)"


def unpad_predictions(pred: ops.HeadPrediction, batch_input_metas) -> List[SceneDetections]:
    """Per scene the first `count` rows (ONE host sync for the batch: the counts), boxed by meta['box_type_3d'] where given
    (box_dim 6 without yaw, or 7 with yaw for the ARKit head's boxes)."""
    counts = pred.counts.cpu().tolist()
    results = []
    for i, n in enumerate(counts):
        if n < 0:
            raise RuntimeError(f"predict_by_feat: scene {i} has {-n} boxes above score_thr (in one class, for the ARKit head), "
                               f"more than the candidate limit "
                               f"{ops.DETECT_MAX_CANDIDATES} of one sort (MVSDET_DETECT_MAX_CANDIDATES)")
        bboxes = pred.boxes[i, :n]
        meta = batch_input_metas[i]
        if "box_type_3d" in meta:
            dim = int(bboxes.shape[-1])   # 7: the ARKit head's boxes with their heading
            bboxes = meta["box_type_3d"](bboxes, box_dim=dim, with_yaw=dim == 7, origin=(.5, .5, .5))
        results.append(SceneDetections(bboxes, pred.scores[i, :n], pred.labels[i, :n]))
    return results
