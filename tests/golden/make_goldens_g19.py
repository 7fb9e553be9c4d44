#!/usr/bin/env python3
"""Generate tests/golden/g19_head_loss_arkit.npz by RUNNING THE REFERENCE (build container only: needs the reference tree).

G19: the ARKit head's training objective, ImVoxelHead_ARKit.loss_by_feat -> _loss_by_feat_single -> _get_targets with
_get_face_distances, _get_centerness, _bbox_pred_to_bbox, _get_points, _upsample_valid_preds and get_points
(projects/NeRF-Det/nerfdet/nerfdet_head.py:21-34, 779-900, 1000-1185), rotation_3d_in_axis
(mmdet3d/structures/bbox_3d/utils.py:32-124) and the RotatedIoU3DLoss wrapper (mmdet3d/models/losses/rotated_iou_loss.py), executed
where they lie on the CPU.  Stand-ins (mmdet, mmcv and mmengine are not installed), each named in the fixture's `stand_in` entry:
  * G18's (tests/golden/make_goldens_g18.py): reduce_mean, weight_reduce_loss behind weighted_loss, the sigmoid BCE, the focal loss,
    the IEEE square root;
  * the ground-truth box holder: tests/head_loss_arkit_restated.RotatedDepthBoxes (tensor, gravity_center, volume, with_yaw);
  * array_converter on rotation_3d_in_axis: left out (it passes tensors through);
  * mmcv.ops.diff_iou_rotated_3d: tests/rotated_iou_restated.diff_iou_rotated_3d -- THE MATHEMATICAL FUNCTION, NOT MMCV'S
    ROUNDING.  mmcv's compiled sort_vertices op has no CPU path and none of its text is at hand; the stand-in returns the exact
    intersection area of the two rectangles by autograd-differentiable torch.  The fixture therefore holds "the true rotated IoU
    and its gradient", not "mmcv's bits"; nobody here can measure the distance to mmcv's own float32 result.

Inputs are made from LCG seeds by tests/head_loss_arkit_restated.scene (the GPU test rebuilds them); only seeds and results are
stored, in G18's layout: labels and chosen box of every point, the targets' rows at assigned points, the losses per scene and batch
in float32 and from a float64 evaluation of the same formulas, and of the gradients of center_loss + bbox_loss + cls_loss by the nine
maps the rows at positive points, every 89th element elsewhere and each map's sum, absolute sum and maximum.

Conditions on the inputs (not tolerances; a scene that fails one is rejected and reseeded, the count is printed): no face distance
within 4 ulp of 0, no centerness within 4 ulp of its box's top-k boundary value, no point claimed by two boxes of equal volume; for
every box the pts_center_threshold-th and the next centerness on its best level at least 1e-5 relative apart; for every positive
point |sin(2 (yaw_p - yaw_t))| and the distance of every corner of one rectangle to every edge of the other at least
head_loss_arkit_restated.DEGENERATE_MARGIN = 1e-5 (degenerate pairs are tested on their own).

    python tests/golden/make_goldens_g19.py
"""
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import head_loss_arkit_restated as A  # noqa: E402
import head_loss_restated as R  # noqa: E402
import rotated_iou_restated as RI  # noqa: E402
from make_goldens_g18 import FocalLoss, SigmoidCrossEntropyLoss, weight_reduce_mean, grad_sample  # noqa: E402,F401

PTS_ASSIGN_THRESHOLD, PTS_CENTER_THRESHOLD = 27, 18
STRIDE = 89
N_CLASSES = 17

CASES = {
    "one": ("one",),
    "twelve": ("twelve",),
    "sixty": ("sixty",),
    "no_valid": ("no_valid",),
    "valid_no_pos": ("valid_no_pos",),
    "batch2": ("twelve", "five"),
}
BASE_SEED = {"one": 1900, "twelve": 1910, "sixty": 1920, "no_valid": 1930, "valid_no_pos": 1940, "batch2": 1950}


def weighted_loss(fn):
    """mmdet.models.losses.utils.weighted_loss for reduction='mean' with an avg_factor (G18's weight_reduce_mean)."""
    def wrapper(pred, target, weight=None, reduction="mean", avg_factor=None, **kwargs):
        assert reduction == "mean" and avg_factor is not None
        return weight_reduce_mean(fn(pred, target, **kwargs), weight, avg_factor)
    return wrapper


class _Models:
    @staticmethod
    def register_module():
        return lambda cls: cls


def load_reference_loss():
    """RefLoss(): a bare object with the reference's ARKit loss_by_feat and everything it calls, executed where it lies."""
    from _ref_loader import REF_ROOT
    path = os.path.join(REF_ROOT, "projects", "NeRF-Det", "nerfdet", "nerfdet_head.py")
    rot_path = os.path.join(REF_ROOT, "mmdet3d", "structures", "bbox_3d", "utils.py")
    loss_path = os.path.join(REF_ROOT, "mmdet3d", "models", "losses", "rotated_iou_loss.py")
    if not all(os.path.isfile(p) for p in (path, rot_path, loss_path)):
        raise FileNotFoundError(path)
    from typing import List, Optional, Tuple, Union
    from torch import Tensor, nn

    class TorchWithIeeeSqrt:   # `torch` as the reference's text sees it: everything forwarded, sqrt correctly rounded
        sqrt = staticmethod(R.ieee_sqrt)

        def __getattr__(self, name):
            return getattr(torch, name)

    find = lambda src, start, prefix: next(i for i in range(start, len(src)) if src[i].startswith(prefix))  # noqa: E731
    rsrc = open(rot_path).read().splitlines()
    r0 = find(rsrc, 0, "def rotation_3d_in_axis(")
    r1 = find(rsrc, r0, "@array_converter")
    rot_ns = dict(torch=torch, np=np, Tensor=Tensor, Union=Union, Tuple=Tuple)
    exec(compile("\n".join(rsrc[r0:r1]), rot_path, "exec"), rot_ns)

    lsrc = [l for l in open(loss_path).read().splitlines() if not l.startswith(("import ", "from "))]
    loss_ns = dict(torch=torch, nn=nn, Tensor=Tensor, Optional=Optional, MODELS=_Models, weighted_loss=weighted_loss,
                   diff_iou_rotated_3d=lambda a, b: RI.diff_iou_rotated_3d(a[0], b[0]).unsqueeze(0))
    exec(compile("\n".join(lsrc), loss_path, "exec"), loss_ns)

    src = open(path).read().splitlines()
    cls_line = find(src, 0, "class ImVoxelHead_ARKit(")
    gp0 = find(src, 0, "def get_points(") - 1          # with its @torch.no_grad()
    gp1 = find(src, gp0, "@MODELS")
    a0 = find(src, cls_line, "    def _loss_by_feat_single(")
    a1 = find(src, a0, "    def _predict_by_feat_single(")
    b0 = find(src, a1, "    def _upsample_valid_preds(") - 1   # with its @staticmethod
    b1 = find(src, b0, "    # Originally ImVoxelNet utilizes 2d nms")
    ns = dict(torch=TorchWithIeeeSqrt(), nn=nn, Tensor=Tensor, List=List, InstanceList=list, OptInstanceList=list,
              reduce_mean=lambda t: t, rotation_3d_in_axis=rot_ns["rotation_3d_in_axis"])
    exec(compile("\n".join(src[gp0:gp1]), path, "exec"), ns)
    exec(compile(textwrap.dedent("\n".join(src[a0:a1] + [""] + src[b0:b1])), path, "exec"), ns)

    class RefLoss:
        loss_by_feat, _loss_by_feat_single, _get_targets = ns["loss_by_feat"], ns["_loss_by_feat_single"], ns["_get_targets"]
        _upsample_valid_preds, _get_points = staticmethod(ns["_upsample_valid_preds"]), ns["_get_points"]
        _bbox_pred_to_bbox = staticmethod(ns["_bbox_pred_to_bbox"])
        _get_face_distances, _get_centerness = staticmethod(ns["_get_face_distances"]), staticmethod(ns["_get_centerness"])

        def __init__(self, n_levels=3, pts_assign_threshold=PTS_ASSIGN_THRESHOLD, pts_center_threshold=PTS_CENTER_THRESHOLD):
            self.n_levels = n_levels
            self.pts_assign_threshold, self.pts_center_threshold = pts_assign_threshold, pts_center_threshold
            self.center_loss, self.cls_loss = SigmoidCrossEntropyLoss(), FocalLoss()
            self.bbox_loss = loss_ns["RotatedIoU3DLoss"]()

    return RefLoss


def run_reference(RefLoss, kinds, seeds, levels=A.ARKIT_LEVELS, n_classes=N_CLASSES,
                  thresholds=(PTS_ASSIGN_THRESHOLD, PTS_CENTER_THRESHOLD)):
    """The reference on a batch made from the seeds: the losses (batch), per scene the losses and the targets, the maps' gradients."""
    c, r, k, v, origins, gts = A.batch(kinds, seeds, levels, n_classes)
    maps = [t.requires_grad_(True) for t in c + r + k]
    head = RefLoss(len(levels), *thresholds)
    metas = A.metas_for(origins)
    losses = head.loss_by_feat(c, r, k, v, gts, metas)
    (losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]).backward()
    grads = [m.grad if m.grad is not None else torch.zeros_like(m) for m in maps]
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


def chosen_boxes(scene_ref, gt):
    """The reference's min_inds where a box was chosen (label >= 0), else -1, identified from the returned box targets: the one
    ground-truth row equal to it."""
    boxes = A.gt_triplet(gt)[0]
    idx = torch.full((len(scene_ref["labels"]),), -1, dtype=torch.int64)
    for p in torch.nonzero(scene_ref["labels"] >= 0).squeeze(1).tolist():
        hit = torch.nonzero((boxes == scene_ref["bbox_t"][p]).all(dim=1)).squeeze(1)
        assert len(hit) == 1, (p, hit)
        idx[p] = int(hit[0])
    return idx


def positive_pairs(c, r, v, origins, gts, sizes, thresholds=(PTS_ASSIGN_THRESHOLD, PTS_CENTER_THRESHOLD)):
    """(predicted boxes, target boxes) of every positive point of the batch, by the restatement."""
    pred, tgt = [], []
    for b, (o, gt) in enumerate(zip(origins, gts)):
        labels, _, _, bbox_t = A.assign(sizes, o, *A.gt_triplet(gt), *thresholds)
        pos = (labels >= 0) & R.upsampled_valid(v, sizes, b)
        _, bbox, _ = R.flatten_maps(c, r, c, b)
        points = torch.cat([R.level_points(s, l, o) for l, s in enumerate(sizes)])
        pred.append(A.pred_to_box(points[pos], bbox[pos].detach()))
        tgt.append(bbox_t[pos])
    return torch.cat(pred), torch.cat(tgt)


def acceptable(kinds, seeds, sizes):
    c, r, k, v, origins, gts = A.batch(kinds, seeds)
    why = [w for o, gt in zip(origins, gts) for w in A.near_decisions(sizes, o, A.gt_triplet(gt), PTS_ASSIGN_THRESHOLD,
                                                                      PTS_CENTER_THRESHOLD)]
    return why + A.near_degenerate(*positive_pairs(c, r, v, origins, gts, sizes))


def main():
    torch.set_num_threads(4)
    RefLoss = load_reference_loss()
    out = {}
    sizes = [tuple(s) for s in A.ARKIT_LEVELS]
    offs = np.cumsum([0] + [s[0] * s[1] * s[2] for s in sizes])
    for name, kinds in CASES.items():
        for attempt in range(12):
            seeds = [BASE_SEED[name] + 7 * attempt + 3 * i for i in range(len(kinds))]
            why = acceptable(kinds, seeds, sizes)
            if not why:
                break
            print(f"{name}: seeds {seeds} rejected: {why[0]}")
        else:
            raise RuntimeError(f"{name}: no acceptable seed")
        print(f"{name}: {attempt + 1} seed(s) tried")
        losses, scenes, grads, (c, r, k, v, origins, gts) = run_reference(RefLoss, kinds, seeds)
        out[f"{name}:kinds"] = np.array(kinds)
        out[f"{name}:seeds"] = np.array(seeds, dtype=np.int64)
        out[f"{name}:seeds_tried"] = np.int64(attempt + 1)
        out[f"{name}:losses"] = np.array([float(losses[n].detach()) for n in ("center_loss", "bbox_loss", "cls_loss")], dtype=np.float32)
        l64, _ = A.loss_by_feat([t.detach() for t in c], [t.detach() for t in r], [t.detach() for t in k], v,
                                [A.gt_triplet(g) for g in gts], origins, dtype=torch.float64)
        out[f"{name}:losses_f64"] = np.array([float(l64[n]) for n in ("center_loss", "bbox_loss", "cls_loss")], dtype=np.float64)
        pos_voxels = [[[] for _ in kinds] for _ in sizes]
        for b, sc in enumerate(scenes):
            labels = sc["labels"]
            assert int(labels.max()) < 127
            box = chosen_boxes(sc, gts[b])
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
                B, C = g.shape[:2]
                N = g[0, 0].numel()
                idx = set(range(0, g.numel(), STRIDE))
                for b in range(B):
                    for vx in pos_voxels[l][b]:
                        idx.update((b * C + ch) * N + vx for ch in range(C))
                idx = np.array(sorted(idx), dtype=np.int64)
                out[f"{name}:grad:{kind}:{l}:index"] = idx.astype(np.int32)
                out[f"{name}:grad:{kind}:{l}:values"] = g.reshape(-1)[idx].numpy()
                out[f"{name}:grad:{kind}:{l}:sums"] = np.array([float(g.double().sum()), float(g.double().abs().sum()),
                                                                float(g.abs().max())], dtype=np.float64)
        print(name, "seeds", seeds, "losses", out[f"{name}:losses"], "f64", out[f"{name}:losses_f64"], "assigned",
              [int((sc["labels"] >= 0).sum()) for sc in scenes])
    out.update(pts_assign_threshold=np.int64(PTS_ASSIGN_THRESHOLD), pts_center_threshold=np.int64(PTS_CENTER_THRESHOLD),
               stride=np.int64(STRIDE), n_classes=np.int64(N_CLASSES), degenerate_margin=np.float64(A.DEGENERATE_MARGIN),
               torch_version=np.array(torch.__version__), generator=np.array("tests/golden/make_goldens_g19.py"),
               stand_in=np.array("mmcv.ops.diff_iou_rotated_3d: tests/rotated_iou_restated.diff_iou_rotated_3d, the mathematical "
                                 "function, not mmcv's rounding (the exact intersection area of the two rectangles in plain torch; "
                                 "mmcv's sort_vertices op has no CPU path); ground-truth boxes: "
                                 "tests/head_loss_arkit_restated.RotatedDepthBoxes; array_converter on rotation_3d_in_axis: left out; "
                                 "reduce_mean: identity; weighted_loss / weight_reduce_loss: sum / (avg_factor + float32 eps), mmdet "
                                 "3.x's form; CrossEntropyLoss(use_sigmoid): F.binary_cross_entropy_with_logits; FocalLoss: the forward "
                                 "/ backward formulas of mmcv's sigmoid focal loss kernel (gamma 2, alpha .25, label -1 = background); "
                                 "torch.sqrt in the reference's text: the correctly rounded float32 square root"))
    path = os.path.join(HERE, "g19_head_loss_arkit.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
