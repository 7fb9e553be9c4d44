#!/usr/bin/env python3
"""Generate tests/golden/g18_head_loss.npz by RUNNING THE REFERENCE (build container only: needs the reference tree).

G18: the ScanNet head's training objective, NerfDetHead.loss_by_feat -> _loss_by_feat_single -> _get_targets with
_get_face_distances, _get_centerness, _bbox_pred_to_bbox, _get_points, _upsample_valid_preds and get_points
(projects/NeRF-Det/nerfdet/nerfdet_head.py:21-34, 152-257, 392-562) and axis_aligned_bbox_overlaps_3d
(mmdet3d/structures/ops/iou3d_calculator.py:210-329), executed where they lie on the CPU.  Stand-ins (mmdet, mmcv and mmengine are
not installed), each named in the fixture's `stand_in` entry:
  * the ground-truth box holder: tests/head_loss_restated.DepthBoxes (tensor, gravity_center, volume of DepthInstance3DBoxes);
  * mmdet.utils.reduce_mean: the identity (one process);
  * mmdet's weighted_loss / weight_reduce_loss for reduction='mean' with an avg_factor: (loss * weight).sum() / (avg_factor + eps),
    eps = float32's machine epsilon -- mmdet 3.x's form; mmdet 2.x divides by avg_factor alone, 1.2e-7 relative apart;
  * mmdet's CrossEntropyLoss(use_sigmoid=True): F.binary_cross_entropy_with_logits(pred, label.float(), reduction='none') through
    the same reduction (its weight is the mask label >= 0, all ones for centerness targets);
  * mmdet's FocalLoss (gamma 2, alpha .25) through mmcv's sigmoid focal loss op: the forward and backward formulas of its kernel
    per (point, class), positive iff label == class, so -1 is background everywhere;
  * torch.sqrt inside the reference's text: the correctly rounded float32 square root (head_loss_restated.ieee_sqrt).  This
    machine's CPU torch takes sqrt from MKL's vector maths, which is within an ulp but not correctly rounded (6 values in 1000
    differ from numpy's), where torch on a GPU, numpy and IEEE 754 agree; every other torch function is the real one;
  * AxisAlignedIoULoss: its forward restated around the reference's own axis_aligned_bbox_overlaps_3d (its file imports mmdet).

Inputs are made from LCG seeds by tests/head_loss_restated.scene (the GPU test rebuilds them); only seeds and the reference's
outputs are stored: labels and chosen box of every point, the targets' rows at assigned points, the losses per scene and batch,
the losses of a float64 evaluation of the same formulas, and of the gradients of center_loss + bbox_loss + cls_loss by the nine maps
the rows at positive points, every 61st element elsewhere and each map's sum and absolute sum.  A scene in which a face distance
lies within 4 ulp of 0 or a centerness within 4 ulp of its box's boundary value is rejected and reseeded.

    python tests/golden/make_goldens_g18.py
"""
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import head_loss_restated as R  # noqa: E402

PTS_ASSIGN_THRESHOLD, PTS_CENTER_THRESHOLD = 27, 18
STRIDE = 61

# name -> scene kinds; one base seed per case
CASES = {
    "one": ("one",),
    "twelve": ("twelve",),
    "sixty": ("sixty",),
    "no_valid": ("no_valid",),
    "valid_no_pos": ("valid_no_pos",),
    "batch2": ("twelve", "five"),
}
BASE_SEED = {"one": 1800, "twelve": 1810, "sixty": 1820, "no_valid": 1830, "valid_no_pos": 1840, "batch2": 1850}


# ------------------------------------------------------------------------------------------------------------ the stand-ins
EPS = torch.finfo(torch.float32).eps


def weight_reduce_mean(loss, weight, avg_factor):
    if weight is not None:
        loss = loss * weight
    return loss.sum() / (avg_factor + EPS)


class SigmoidFocal(torch.autograd.Function):
    """mmcv.ops.sigmoid_focal_loss, reduction 'none', no class weight: the kernel's formulas."""

    @staticmethod
    def forward(ctx, x, target, gamma, alpha):
        tiny = torch.finfo(torch.float32).tiny
        p = torch.sigmoid(x)
        pos = target.view(-1, 1) == torch.arange(x.shape[1]).view(1, -1)
        term_p = -alpha * (1 - p).pow(gamma) * torch.log(p.clamp(min=tiny))
        term_n = -(1 - alpha) * p.pow(gamma) * torch.log((1 - p).clamp(min=tiny))
        ctx.save_for_backward(p, pos)
        ctx.ga = (gamma, alpha)
        return torch.where(pos, term_p, term_n)

    @staticmethod
    def backward(ctx, g):
        tiny = torch.finfo(torch.float32).tiny
        p, pos = ctx.saved_tensors
        gamma, alpha = ctx.ga
        gp = -alpha * (1 - p).pow(gamma) * (1 - p - gamma * p * torch.log(p.clamp(min=tiny)))
        gn = -(1 - alpha) * p.pow(gamma) * (gamma * (1 - p) * torch.log((1 - p).clamp(min=tiny)) - p)
        return g * torch.where(pos, gp, gn), None, None, None


class FocalLoss:
    def __init__(self, gamma=2.0, alpha=0.25, loss_weight=1.0):
        self.gamma, self.alpha, self.loss_weight = gamma, alpha, loss_weight

    def __call__(self, pred, target, weight=None, avg_factor=None):
        loss = SigmoidFocal.apply(pred.contiguous(), target.contiguous(), self.gamma, self.alpha)
        return self.loss_weight * weight_reduce_mean(loss, weight, avg_factor)


class SigmoidCrossEntropyLoss:
    def __init__(self, loss_weight=1.0):
        self.loss_weight = loss_weight

    def __call__(self, pred, label, weight=None, avg_factor=None):
        mask = ((label >= 0) & (label != -100)).float()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, label.float(), reduction="none")
        return self.loss_weight * weight_reduce_mean(loss, mask if weight is None else weight * mask, avg_factor)


def load_reference_loss():
    """RefLoss(): a bare object with the reference's loss_by_feat and everything it calls, executed where it lies."""
    from _ref_loader import REF_ROOT
    path = os.path.join(REF_ROOT, "projects", "NeRF-Det", "nerfdet", "nerfdet_head.py")
    iou_path = os.path.join(REF_ROOT, "mmdet3d", "structures", "ops", "iou3d_calculator.py")
    if not (os.path.isfile(path) and os.path.isfile(iou_path)):
        raise FileNotFoundError(path)
    src = open(path).read().splitlines()
    find = lambda start, prefix: next(i for i in range(start, len(src)) if src[i].startswith(prefix))  # noqa: E731
    cls_line = find(0, "class NerfDetHead(")
    gp0 = find(0, "def get_points(") - 1          # with its @torch.no_grad()
    gp1 = find(gp0, "@MODELS")
    a0 = find(cls_line, "    def loss_by_feat(")
    a1 = find(a0, "    def predict(")
    b0 = next(i for i in range(a1, len(src)) if src[i].startswith("    def _upsample_valid_preds(")) - 1   # with its @staticmethod
    b1 = find(b0, "    def _nms(")
    from typing import List
    from torch import Tensor, nn
    iou_src = open(iou_path).read().splitlines()
    i0 = next(i for i, l in enumerate(iou_src) if l.startswith("def axis_aligned_bbox_overlaps_3d("))
    iou_ns = dict(torch=torch)
    exec(compile("\n".join(iou_src[i0:]), iou_path, "exec"), iou_ns)
    overlaps = iou_ns["axis_aligned_bbox_overlaps_3d"]

    class AxisAlignedIoULoss:   # mmdet3d/models/losses/axis_aligned_iou_loss.py:51-85 for reduction 'mean'
        def __init__(self, loss_weight=1.0):
            self.loss_weight = loss_weight

        def __call__(self, pred, target, weight=None, avg_factor=None):
            if (weight is not None) and (not torch.any(weight > 0)):
                return (pred * weight).sum()
            return weight_reduce_mean(1 - overlaps(pred, target, is_aligned=True), weight, avg_factor) * self.loss_weight

    class TorchWithIeeeSqrt:   # `torch` as the reference's text sees it: everything forwarded, sqrt correctly rounded
        sqrt = staticmethod(R.ieee_sqrt)

        def __getattr__(self, name):
            return getattr(torch, name)

    ns = dict(torch=TorchWithIeeeSqrt(), nn=nn, Tensor=Tensor, List=List, InstanceList=list, OptInstanceList=list, reduce_mean=lambda t: t)
    exec(compile("\n".join(src[gp0:gp1]), path, "exec"), ns)
    exec(compile(textwrap.dedent("\n".join(src[a0:a1] + [""] + src[b0:b1])), path, "exec"), ns)

    class RefLoss:
        loss_by_feat, _loss_by_feat_single, _get_targets = ns["loss_by_feat"], ns["_loss_by_feat_single"], ns["_get_targets"]
        _upsample_valid_preds, _get_points = staticmethod(ns["_upsample_valid_preds"]), ns["_get_points"]
        _bbox_pred_to_bbox, _bbox_pred_to_loss = ns["_bbox_pred_to_bbox"], ns["_bbox_pred_to_loss"]
        _get_face_distances, _get_centerness = staticmethod(ns["_get_face_distances"]), staticmethod(ns["_get_centerness"])

        def __init__(self, n_levels=3, pts_assign_threshold=PTS_ASSIGN_THRESHOLD, pts_center_threshold=PTS_CENTER_THRESHOLD):
            self.n_levels = n_levels
            self.pts_assign_threshold, self.pts_center_threshold = pts_assign_threshold, pts_center_threshold
            self.center_loss, self.bbox_loss, self.cls_loss = SigmoidCrossEntropyLoss(), AxisAlignedIoULoss(), FocalLoss()

    return RefLoss


def run_reference(RefLoss, kinds, seeds, levels=R.SCANNET_LEVELS, n_classes=18, thresholds=(PTS_ASSIGN_THRESHOLD, PTS_CENTER_THRESHOLD)):
    """The reference on a batch made from the seeds: the losses (batch), per scene the losses and the targets, the maps' gradients."""
    c, r, k, v, origins, gts = R.batch(kinds, seeds, levels, n_classes)
    maps = [t.requires_grad_(True) for t in c + r + k]
    head = RefLoss(len(levels), *thresholds)
    metas = R.metas_for(origins)
    losses = head.loss_by_feat(c, r, k, v, gts, metas)
    (losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]).backward()
    grads = [m.grad for m in maps]
    sizes = [tuple(t.shape[2:]) for t in c]
    scenes = []
    valid_preds = head._upsample_valid_preds(v, c)
    for b in range(len(kinds)):
        pts = head._get_points(featmap_sizes=sizes, origin=metas[b]["lidar2img"]["origin"], device=torch.device("cpu"))
        center_t, bbox_t, labels = head._get_targets(pts, gts[b].bboxes_3d, gts[b].labels_3d)
        with torch.no_grad():
            per = head._loss_by_feat_single([x[b] for x in c], [x[b] for x in r], [x[b] for x in k], [x[b] for x in valid_preds],
                                            metas[b], gts[b].bboxes_3d, gts[b].labels_3d)
        scenes.append(dict(labels=labels, center_t=center_t, bbox_t=bbox_t, losses=torch.stack([t.detach() for t in per])))
    return losses, scenes, grads, (c, r, k, v, origins, gts)


def chosen_boxes(scene_ref, sizes, origin, gt):
    """The reference's min_area_inds where a box was chosen (label >= 0), else -1: _get_targets does not return it, so it is
    identified from the returned box targets -- the box whose faces give exactly this row (the equal-volume pair differs there)."""
    boxes = R.gt_triplet(gt)[0]
    pts = torch.cat([R.level_points(s, l, origin) for l, s in enumerate(sizes)])
    idx = torch.full((len(pts),), -1, dtype=torch.int64)
    for p in torch.nonzero(scene_ref["labels"] >= 0).squeeze(1).tolist():
        rows = []
        for g in range(len(boxes)):
            dg = R.face_distances(pts[p:p + 1], boxes[g])[0]
            rows.append(torch.stack((pts[p, 0] - dg[0], pts[p, 1] - dg[2], pts[p, 2] - dg[4], pts[p, 0] + dg[1], pts[p, 1] + dg[3],
                                     pts[p, 2] + dg[5])))
        hit = torch.nonzero((torch.stack(rows) == scene_ref["bbox_t"][p]).all(dim=1)).squeeze(1)
        assert len(hit) == 1, (p, hit)
        idx[p] = int(hit[0])
    return idx


def grad_sample(grad, pos_voxels):
    """Flat indices into one map's gradient: all channels of the positive voxels of every scene, and every 61st element."""
    B, C = grad.shape[:2]
    N = grad[0, 0].numel()
    idx = set(range(0, grad.numel(), STRIDE))
    for b in range(B):
        for v in pos_voxels[b]:
            idx.update((b * C + ch) * N + v for ch in range(C))
    return np.array(sorted(idx), dtype=np.int64)


def main():
    torch.set_num_threads(4)
    RefLoss = load_reference_loss()
    out = {}
    sizes = [tuple(s) for s in R.SCANNET_LEVELS]
    offs = np.cumsum([0] + [s[0] * s[1] * s[2] for s in sizes])
    for name, kinds in CASES.items():
        for attempt in range(40):
            seeds = [BASE_SEED[name] + 7 * attempt + 3 * i for i in range(len(kinds))]
            _, _, _, _, origins, gts = R.batch(kinds, seeds)
            why = [w for o, gt in zip(origins, gts) for w in R.near_decisions(sizes, o, R.gt_triplet(gt), PTS_ASSIGN_THRESHOLD,
                                                                              PTS_CENTER_THRESHOLD)]
            if not why:
                break
            print(f"{name}: seeds {seeds} rejected: {why[0]}")
        else:
            raise RuntimeError(f"{name}: no acceptable seed")
        losses, scenes, grads, (c, r, k, v, origins, gts) = run_reference(RefLoss, kinds, seeds)
        out[f"{name}:kinds"] = np.array(kinds)
        out[f"{name}:seeds"] = np.array(seeds, dtype=np.int64)
        out[f"{name}:losses"] = np.array([float(losses[n].detach()) for n in ("center_loss", "bbox_loss", "cls_loss")], dtype=np.float32)
        l64, _ = R.loss_by_feat([t.detach() for t in c], [t.detach() for t in r], [t.detach() for t in k], v,
                                [R.gt_triplet(g) for g in gts], origins, dtype=torch.float64)
        out[f"{name}:losses_f64"] = np.array([float(l64[n]) for n in ("center_loss", "bbox_loss", "cls_loss")], dtype=np.float64)
        pos_voxels = [[[] for _ in kinds] for _ in sizes]
        for b, sc in enumerate(scenes):
            labels = sc["labels"]
            assert int(labels.max()) < 127
            box = chosen_boxes(sc, sizes, origins[b], gts[b])
            assigned = torch.nonzero(labels >= 0).squeeze(1)
            out[f"{name}:{b}:labels"] = labels.numpy().astype(np.int8)
            out[f"{name}:{b}:box_index"] = box.numpy().astype(np.int16)
            out[f"{name}:{b}:center_targets"] = sc["center_t"][assigned].numpy()
            out[f"{name}:{b}:bbox_targets"] = sc["bbox_t"][assigned].numpy()
            out[f"{name}:{b}:scene_losses"] = sc["losses"].numpy()
            valid = R.upsampled_valid(v, sizes, b)
            for p in torch.nonzero((labels >= 0) & valid).squeeze(1).tolist():
                l = int(np.searchsorted(offs, p, side="right") - 1)
                pos_voxels[l][b].append(p - int(offs[l]))
        for j, kind in enumerate(("center", "bbox", "cls")):
            for l in range(len(sizes)):
                g = grads[j * len(sizes) + l]
                idx = grad_sample(g, pos_voxels[l])
                out[f"{name}:grad:{kind}:{l}:index"] = idx.astype(np.int32)
                out[f"{name}:grad:{kind}:{l}:values"] = g.reshape(-1)[idx].numpy()
                out[f"{name}:grad:{kind}:{l}:sums"] = np.array([float(g.double().sum()), float(g.double().abs().sum()),
                                                                float(g.abs().max())], dtype=np.float64)
        print(name, "seeds", seeds, "losses", out[f"{name}:losses"], "f64", out[f"{name}:losses_f64"], "assigned",
              [int((sc["labels"] >= 0).sum()) for sc in scenes])
    out.update(pts_assign_threshold=np.int64(PTS_ASSIGN_THRESHOLD), pts_center_threshold=np.int64(PTS_CENTER_THRESHOLD),
               stride=np.int64(STRIDE), torch_version=np.array(torch.__version__),
               generator=np.array("tests/golden/make_goldens_g18.py"),
               stand_in=np.array("ground-truth boxes: tests/head_loss_restated.DepthBoxes; reduce_mean: identity; weight_reduce_loss: "
                                 "sum / (avg_factor + float32 eps), mmdet 3.x's form (mmdet 2.x: / avg_factor, 1.2e-7 relative apart); "
                                 "CrossEntropyLoss(use_sigmoid): F.binary_cross_entropy_with_logits; FocalLoss: the forward / backward "
                                 "formulas of mmcv's sigmoid focal loss kernel (gamma 2, alpha .25, label -1 = background); "
                                 "AxisAlignedIoULoss: its forward around the reference's axis_aligned_bbox_overlaps_3d; torch.sqrt in the "
                                 "reference's text: the correctly rounded float32 square root (this CPU build's is MKL's, within an ulp)"))
    path = os.path.join(HERE, "g18_head_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
