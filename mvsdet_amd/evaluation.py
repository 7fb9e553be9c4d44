"""Indoor detection metrics on the device: mmdet3d's `indoor_eval` (IndoorMetric.compute_metrics -> per-class AP and recall, mAP and
mAR at IoU thresholds) over csrc/evalmap.hip.

`IndoorEvaluator.update` appends a batch's detections and ground truth to device state without a host synchronisation; `compute`
orders and scores them on the device and assembles the reference's `ret_dict` on the host from the per-label values, with the
reference's NumPy expressions and dtypes.  `indoor_eval` has the reference's signature; `integration.patch_reference_indoor_eval`
rebinds it in an imported reference module.

What is computed is BaseInstance3DBoxes.overlaps as a mathematical function, in float32: the intersection of the two footprints is
computed directly, where the reference recovers it from mmcv's box_iou_rotated.  mmcv's own float32 rounding is not reproduced (it
is not installed where this package is developed; the distance to it is not measured).  Equal scores inside a label are visited by
(scene, row); the reference's np.argsort leaves that order open.  A label that is predicted and has no ground truth anywhere gives
NaN AP and recall, and with them NaN mAP and mAR, as the reference does.

The view-synthesis side (the reference's NVSMetric and MVSMetric) is at the end of the module: `NVSEvaluator`, `MVSEvaluator` and
`nvs_eval` over csrc/nvsmetric.hip (ops.nvsmetric)."""
from __future__ import annotations

import logging
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import ops
from .ops._common import req, to_device


def _get(obj, *names):
    for n in names:
        if isinstance(obj, dict):
            if n in obj:
                return obj[n]
        elif hasattr(obj, n):
            return getattr(obj, n)
    raise KeyError(f"indoor evaluation: none of {names} in {type(obj).__name__}")


def _rows7(boxes) -> Tensor:
    """A box object's own rows (bottom-centred `.tensor`), or a tensor, as (n,7) float32 with yaw 0 where there is none."""
    t = boxes.tensor if hasattr(boxes, "tensor") else torch.as_tensor(boxes)
    if t.numel() == 0:
        return t.new_zeros((0, 7), dtype=torch.float32)
    t = t.float().reshape(-1, t.shape[-1])
    if t.shape[1] not in (6, 7):
        raise ValueError(f"indoor evaluation: boxes of 6 or 7 values needed (got {tuple(t.shape)})")
    return t if t.shape[1] == 7 else torch.cat((t, t.new_zeros((t.shape[0], 1))), dim=1)


def _bottom_centred(boxes: Tensor) -> Tensor:
    """(B,N,6|7) gravity-centred rows to the box classes' layout, by their own expression: z + dz * (0 - 0.5) in float32."""
    z = boxes[..., 2] + boxes[..., 5] * (0 - 0.5)
    yaw = boxes[..., 6:7] if boxes.shape[-1] == 7 else boxes.new_zeros(boxes.shape[:-1] + (1,))
    return torch.cat((boxes[..., :2], z.unsqueeze(-1), boxes[..., 3:6], yaw), dim=-1)


def _pad(rows, width, dtype, dev) -> Tensor:
    n = max([int(r.shape[0]) for r in rows], default=0)
    out = [torch.cat([r.reshape((r.shape[0],) + width).to(dtype), r.new_zeros((n - r.shape[0],) + width, dtype=dtype)]) for r in rows]
    return to_device(torch.stack(out), dev)


class IndoorEvaluator:
    """Accumulates detections and ground truth of any number of batches on `device` and scores them as mmdet3d's indoor_eval.

    n_labels: labels are 0 .. n_labels-1; iou_thr: the IoU thresholds; capacity / gt_capacity: detections / ground-truth boxes the
    evaluator can hold in all (<= 2**20 detections) -- running over either, or a negative count in a HeadPrediction (the heads' flag
    for more than DETECT_MAX_CANDIDATES boxes), raises at compute(); label2cat: names of the labels (default: their numbers)."""

    def __init__(self, n_labels: int, iou_thr: Sequence[float] = (0.25, 0.5), capacity: int = 1 << 16, gt_capacity: int = 1 << 14,
                 device="cuda", label2cat=None):
        self.iou_thr = tuple(iou_thr)
        self.label2cat = label2cat if label2cat is not None else {i: str(i) for i in range(int(n_labels))}
        self._st = ops.eval_state(n_labels, capacity, gt_capacity, len(self.iou_thr), device)
        self._scenes = 0     # the next scene's serial number
        self._bound = 0      # host-side upper bound of the detections fed (padded rows included)
        self.last_result: Optional[ops.EvalResult] = None

    @property
    def device(self) -> torch.device:
        return self._st.state.device

    def reset(self) -> None:
        ops.eval_reset(self._st)
        self._scenes, self._bound, self.last_result = 0, 0, None

    def update(self, pred, gt) -> None:
        """One batch, no host synchronisation.  Either a HeadPrediction (gravity-centred boxes (B,N,6|7), scores, labels, counts)
        with the padded ground truth of head.pad_ground_truth[_rotated] (the tuple it returns, gravity-centred), or two lists with
        one entry per scene: detections with `bboxes_3d` (a box object's `.tensor`, bottom-centred), `scores_3d`, `labels_3d`, and
        ground truth with `bboxes_3d` / `gt_bboxes_3d` and `labels_3d` / `gt_labels_3d` (objects or dicts)."""
        dev = self.device
        if isinstance(pred, ops.HeadPrediction):
            if not isinstance(gt, (tuple, list)) or len(gt) not in (4, 5):
                raise TypeError("IndoorEvaluator.update: a HeadPrediction goes with the tuple of head.pad_ground_truth[_rotated]")
            gt_boxes, gt_labels, gt_counts = gt[0], gt[-2], gt[-1]
            req(pred.boxes, "pred.boxes", dim=3)
            req(gt_boxes, "gt_boxes", dim=3)
            boxes, scores, labels, counts = _bottom_centred(pred.boxes), pred.scores, pred.labels, pred.counts
            gt_boxes = _bottom_centred(gt_boxes)
        else:
            dets, gts = list(pred), list(gt)
            if len(dets) != len(gts):
                raise ValueError(f"IndoorEvaluator.update: {len(dets)} scenes of detections, {len(gts)} of ground truth")
            if not dets:
                return
            db = [_rows7(_get(d, "bboxes_3d")) for d in dets]
            gb = [_rows7(_get(g, "gt_bboxes_3d", "bboxes_3d")) for g in gts]
            boxes, gt_boxes = _pad(db, (7,), torch.float32, dev), _pad(gb, (7,), torch.float32, dev)
            scores = _pad([torch.as_tensor(_get(d, "scores_3d")).reshape(-1) for d in dets], (), torch.float32, dev)
            labels = _pad([torch.as_tensor(_get(d, "labels_3d")).reshape(-1) for d in dets], (), torch.int64, dev)
            gt_labels = _pad([torch.as_tensor(_get(g, "gt_labels_3d", "labels_3d")).reshape(-1) for g in gts], (), torch.int64, dev)
            counts = to_device(torch.tensor([int(b.shape[0]) for b in db], dtype=torch.int32), dev)
            gt_counts = to_device(torch.tensor([int(b.shape[0]) for b in gb], dtype=torch.int32), dev)
        ops.eval_match(self._st, boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, self._scenes)
        self._scenes += int(boxes.shape[0])
        self._bound = min(self._bound + int(boxes.shape[0]) * int(boxes.shape[1]), self._st.capacity)

    def compute(self) -> Dict[str, float]:
        """The reference's ret_dict: per threshold `<cat>_AP_<t>` of every label in the order the reference's dicts meet them
        (a scene's detections, then its ground truth), `mAP_<t>`, `<cat>_rec_<t>`, `mAR_<t>`.  One host synchronisation."""
        res = ops.eval_compute(self._st, self.iou_thr, self._bound)
        self.last_result = res
        info = res.info.cpu().tolist()
        if info[2]:
            what = "; ".join(v for k, v in ops.EVAL_FLAGS.items() if info[2] & k)
            raise RuntimeError(f"IndoorEvaluator.compute: {what} (capacity {self._st.capacity}, gt_capacity {self._st.gt_capacity}, "
                               f"n_labels {self._st.n_labels}); reset() and feed again")
        ap, recall = res.ap.cpu().numpy(), res.recall.cpu().numpy()
        ndet, first = res.ndet.cpu().numpy(), res.first.cpu().numpy()
        labels = [int(l) for l in np.argsort(first.view(np.uint64), kind="stable") if first[l] != -1]
        return assemble(labels, ap[:, labels], recall[:, labels], ndet[labels], self.iou_thr, self.label2cat)


def assemble(labels, ap, rec_last, ndet, thresholds, label2cat) -> Dict[str, float]:
    """indoor_eval's ret_dict (indoor_eval.py:266-289) from per-label values with the reference's NumPy expressions and dtypes: a
    label with ground truth and no prediction contributes eval_map_recall's float64 zeros(1), the others average_precision's
    float32 arrays of one value and eval_det_cls' float64 recall; np.mean rounds mAP in the dtype that follows from them."""
    ret = {}
    for t, thr in enumerate(thresholds):
        aps = [np.zeros(1) if ndet[k] == 0 else np.array([ap[t][k]], np.float32) for k in range(len(labels))]
        recs = [np.float64(0.0) if ndet[k] == 0 else np.float64(rec_last[t][k]) for k in range(len(labels))]
        for k, lab in enumerate(labels):
            ret[f"{label2cat[lab]}_AP_{thr:.2f}"] = float(aps[k][0])
        ret[f"mAP_{thr:.2f}"] = float(np.mean(aps))
        for k, lab in enumerate(labels):
            ret[f"{label2cat[lab]}_rec_{thr:.2f}"] = float(recs[k])
        ret[f"mAR_{thr:.2f}"] = float(np.mean(recs))
    return ret


def _table(ret: Dict[str, float], thresholds) -> str:
    cats = [k[:-len(f"_AP_{thresholds[0]:.2f}")] for k in ret if k.endswith(f"_AP_{thresholds[0]:.2f}") and not k.startswith("mAP_")]
    head = ["classes"] + [f"{m}_{t:.2f}" for t in thresholds for m in ("AP", "AR")]
    rows = [[c] + [f"{ret[f'{c}_{m}_{t:.2f}']:.4f}" for t in thresholds for m in ("AP", "rec")] for c in cats]
    rows.append(["Overall"] + [f"{ret[f'{m}_{t:.2f}']:.4f}" for t in thresholds for m in ("mAP", "mAR")])
    width = [max(len(r[i]) for r in [head] + rows) for i in range(len(head))]
    return "\n".join(" | ".join(v.ljust(w) for v, w in zip(r, width)) for r in [head] + rows)


def indoor_eval(gt_annos, dt_annos, metric, label2cat, logger=None, box_mode_3d=None, device="cuda") -> Dict[str, float]:
    """mmdet3d's indoor_eval (same arguments and return value) on the device.  gt_annos: dicts with `gt_bboxes_3d`, `gt_labels_3d`;
    dt_annos: dicts with `bboxes_3d`, `scores_3d`, `labels_3d`; the detections' boxes go through `convert_to(box_mode_3d)` as in the
    reference.  The table is logged through `logging` (`logger`: a Logger, a logger's name, or None for this module's)."""
    assert len(dt_annos) == len(gt_annos)
    dets = []
    for d in dt_annos:
        b = d["bboxes_3d"]
        dets.append(dict(bboxes_3d=b.convert_to(box_mode_3d) if hasattr(b, "convert_to") else b, scores_3d=d["scores_3d"],
                         labels_3d=d["labels_3d"]))
    n_det = sum(int(torch.as_tensor(d["labels_3d"]).numel()) for d in dets)
    n_max = max([int(torch.as_tensor(d["labels_3d"]).numel()) for d in dets], default=0)
    n_gt = sum(len(g["gt_labels_3d"]) for g in gt_annos)
    keys = list(label2cat.keys()) if isinstance(label2cat, dict) else list(range(len(label2cat)))
    seen = [int(torch.as_tensor(d["labels_3d"]).max()) for d in dets if torch.as_tensor(d["labels_3d"]).numel()]
    seen += [int(np.max(np.asarray(g["gt_labels_3d"]))) for g in gt_annos if len(g["gt_labels_3d"])]
    n_labels = max(keys + seen, default=0) + 1
    ev = IndoorEvaluator(n_labels, tuple(metric), capacity=max(n_det, n_max, 1), gt_capacity=max(n_gt, 1), device=device,
                         label2cat=label2cat)
    for d, g in zip(dets, gt_annos):
        ev.update([d], [g])
    ret = ev.compute()
    log = logger if isinstance(logger, logging.Logger) else logging.getLogger(logger if isinstance(logger, str) else __name__)
    log.info("\n%s", _table(ret, tuple(metric)))
    return ret


# ------------------------------------------------------------------------------------------- view synthesis (NVSMetric, MVSMetric)
def _scene_list(x, name: str, dims) -> list:
    """A tensor of one scene, or a list of scenes; None entries stay."""
    if x is None:
        return []
    scenes = [x] if isinstance(x, Tensor) else list(x)
    out = []
    for t in scenes:
        if t is not None:
            t = torch.as_tensor(t)
            t = t[0] if t.dim() == dims + 1 and t.shape[0] == 1 else t
            if t.dim() != dims:
                raise ValueError(f"NVS evaluation: {name} {tuple(t.shape)}: one scene is "
                                 f"{'(n_tgt,3,H,W) or (1,n_tgt,3,H,W)' if dims == 4 else '(n_tgt,H,W) or (1,n_tgt,H,W)'}")
        out.append(t)
    return out


class NVSEvaluator:
    """The reference's NVSMetric (mmdet3d/evaluation/metrics/Indoor_NVS.py:15-106) over the triples its test loop stores per scene
    (mvsdet.py:1017-1040: save_rendered_img_Image, and save_rendered_depth where a rendered depth exists), scored and accumulated on
    `device` (csrc/nvsmetric.hip; a CPU device takes ops.nvsmetric.nvs_score's torch float64 route).  `update` makes no host synchronisation,
    `compute` one read-back.  PSNR and SSIM are evaluated in float64: the reference's float32 route lies up to 1.4e-7 (SSIM) and
    2.3e-6 dB (PSNR) from them.  `last_scene`: the device row (psnr, ssim, rmse) of the scene fed last;
    `last_views`: its (n_tgt,2) psnr and ssim per view."""

    def __init__(self, device="cuda"):
        self._st = ops.nvsmetric.nvs_state(device)
        self._scenes = 0
        self.last_scene: Optional[Tensor] = None
        self.last_views: Optional[Tensor] = None

    @property
    def device(self) -> torch.device:
        return self._st.device

    def reset(self) -> None:
        ops.nvsmetric.nvs_reset(self._st)
        self._scenes, self.last_scene, self.last_views = 0, None, None

    def update(self, rgb_pred, gt_rgb, depth_pred=None, gt_depth=None) -> None:
        """One scene -- rgb_pred (1,n_tgt,3,H,W) as `MVSDetHotPath.novel_views` returns it, or (n_tgt,3,H,W); gt_rgb the same shape
        without the leading 1; depth_pred / gt_depth (n_tgt,H,W) or None -- or lists with one entry per scene (a depth entry may be
        None: that scene counts rmse 0, as the reference's triple does).  Shapes may differ from scene to scene."""
        preds, gts = _scene_list(rgb_pred, "rgb_pred", 4), _scene_list(gt_rgb, "gt_rgb", 4)
        dps, dgs = _scene_list(depth_pred, "depth_pred", 3), _scene_list(gt_depth, "gt_depth", 3)
        if len(preds) != len(gts) or len(dps) != len(dgs) or (dps and len(dps) != len(preds)):
            raise ValueError(f"NVSEvaluator.update: {len(preds)} renders, {len(gts)} ground truths, {len(dps)} / {len(dgs)} depth maps")
        for i, (p, g) in enumerate(zip(preds, gts)):
            dp, dg = (dps[i], dgs[i]) if dps else (None, None)
            dev = self.device
            p, g, dp, dg = (None if t is None else (t if t.device == dev else to_device(t, dev)) for t in (p, g, dp, dg))
            self.last_views, self.last_scene = ops.nvsmetric.nvs_score(self._st, p, g, dp, dg)
            self._scenes += 1

    def compute(self) -> Dict[str, float]:
        """NVSMetric.compute_metrics' dict {'psnr', 'ssim', 'rmse'}: the plain means over the scenes fed, as Python floats."""
        if self._scenes == 0:
            raise RuntimeError("NVSEvaluator.compute: no scene was fed")
        psnr, ssim, rmse = ops.nvsmetric.nvs_result(self._st).cpu().tolist()
        return {"psnr": psnr, "ssim": ssim, "rmse": rmse}


class MVSEvaluator:
    """The reference's MVSMetric (Indoor_NVS.py:232-283) over the depth diagnostics of the lifting block, accumulated on the device.
    The reference's quirk is kept: `src_rmse` is the mean over the scenes, but `weight_gap` is the LAST scene's value -- it computes
    the mean (final_weight_gap, :277) and then returns the loop variable (:280).  `update` makes no host synchronisation, `compute`
    one read-back."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self._acc: Optional[Tensor] = None     # (2) float64 on the inputs' device: the last scene's weight_gap, the sum of src_rmse
        self._scenes = 0

    def update(self, outputs_or_pair) -> None:
        """A scene's `SceneOutputs` (or any mapping with "weight_gap" and "src_rmse"), or the pair (weight_gap, src_rmse)."""
        if hasattr(outputs_or_pair, "keys"):
            gap, rmse = outputs_or_pair["weight_gap"], outputs_or_pair["src_rmse"]
        else:
            gap, rmse = outputs_or_pair
        gap, rmse = (torch.as_tensor(t).detach().reshape(()).to(torch.float64) for t in (gap, rmse))
        if self._acc is None:
            self._acc = torch.stack((gap, rmse))
        else:
            self._acc = torch.stack((gap.to(self._acc.device), self._acc[1] + rmse.to(self._acc.device)))
        self._scenes += 1

    def compute(self) -> Dict[str, float]:
        """MVSMetric.compute_metrics' dict {'weight_gap': the last scene's, 'src_rmse': the mean}, as Python floats."""
        if self._scenes == 0:
            raise RuntimeError("MVSEvaluator.compute: no scene was fed")
        gap, total = self._acc.cpu().tolist()
        return {"weight_gap": gap, "src_rmse": total / self._scenes}


def nvs_eval(rgb_preds, gt_rgbs, depth_preds=None, gt_depths=None, device="cuda") -> Dict[str, float]:
    """The function form beside `indoor_eval`: the scenes' renders and ground truth (lists, or one scene's tensors; depth lists may
    hold None) -> NVSMetric's dict {'psnr', 'ssim', 'rmse'}."""
    ev = NVSEvaluator(device)
    ev.update(rgb_preds, gt_rgbs, depth_preds, gt_depths)
    return ev.compute()
