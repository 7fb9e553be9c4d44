#!/usr/bin/env python3
"""Generate tests/golden/g16_detect_arkit.npz by RUNNING THE REFERENCE (build container only: needs the reference tree).

G16: the ARKit head's post-processing, ImVoxelHead_ARKit.predict_by_feat -> _predict_by_feat_single -> _bbox_pred_to_bbox ->
_single_scene_multiclass_nms (projects/NeRF-Det/nerfdet/nerfdet_head.py:902-1056, 1190-1243, get_points :21-34) with the real
rotation_3d_in_axis (mmdet3d/structures/bbox_3d/utils.py), executed where they lie on CPU with these stand-ins: mmengine's
InstanceData (an attribute holder), the test_cfg (a SimpleNamespace), `box_type_3d` (the identity, so the raw (n, 7) tensor comes
back), `@array_converter` (a pass-through: the inputs are tensors already) and mmcv.ops.nms3d, whose compiled op has no CPU path:
the float32 NumPy restatement of tests/nms3d_restated.py (STAND_IN below; flagged in the fixture).

Inputs are head maps at the ARKit level sizes (40x40x16, 20x20x8, 10x10x4) with 17 classes and 7 regression channels (the angle
raw, over [-pi, pi] and beyond), made from LCG seeds by `scene_inputs` below (the GPU test rebuilds them from the stored seeds);
only the seeds and the reference's outputs are stored.  A scene whose result hangs on a decision within rounding is rejected and
reseeded (`near_decisions`).

    python tests/golden/make_goldens_g16.py
"""
import math
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import nms3d_restated as R  # noqa: E402
from lcg import lcg_uniform  # noqa: E402

LEVELS = ((40, 40, 16), (20, 20, 8), (10, 10, 4))
N_CLASSES = 17
VOXEL = (.16, .16, .2)
SCORE_THR, IOU_THR = 0.01, 0.25
STAND_IN = ("mmcv.ops.nms3d as the float32 NumPy restatement of tests/nms3d_restated.py; mmengine's InstanceData as an attribute "
            "holder, the test_cfg as a SimpleNamespace, box_type_3d as the identity, array_converter as a pass-through "
            "(tests/golden/make_goldens_g16.py)")

# name -> (scene kinds, nms_pre); one base seed per case
CASES = {
    "planted": (("planted",), 1000),
    "random": (("random",), 1000),
    "empty": (("empty",), 1000),
    "half": (("half",), 1000),
    "batch2": (("planted", "random"), 1000),
    "nms_pre_big": (("sparse",), 30000),
    "nms_pre_zero": (("sparse",), 0),
}
BASE_SEED = {"planted": 1600, "random": 1610, "empty": 1620, "half": 1630, "batch2": 1640, "nms_pre_big": 1660, "nms_pre_zero": 1670}


def _u(shape, seed):
    return torch.from_numpy(lcg_uniform(int(np.prod(shape)), seed)).reshape(shape)


def level_points(size, level, origin):
    """get_points of one level as (3, X, Y, Z) float32 (our own restatement, for planting objects and the screen)."""
    n = torch.tensor(size)
    vs = torch.tensor(VOXEL) * (2 ** level)
    new_origin = origin - n / 2. * vs
    grid = torch.stack(torch.meshgrid([torch.arange(s) for s in size], indexing="ij"))
    return grid * vs.view(3, 1, 1, 1) + new_origin.view(3, 1, 1, 1)


def scene_inputs(kind: str, seed: int):
    """(center, bbox, cls) lists over the levels of (1, c, X, Y, Z) float32, valid counts (1, 1, 40, 40, 16) float32, origin (3,)."""
    origin = (torch.tensor([3.0, 3.0, 1.5]) + _u((3,), seed * 10) * torch.tensor([0.5, 0.5, 0.2])).float()
    vshape = (1, 1) + LEVELS[0]
    uv = _u(vshape, seed * 10 + 1)
    if kind in ("half", "sparse"):
        valid = (uv > (0.4 if kind == "sparse" else 0.0)).float()       # 0 / 1 views: level means of exactly 0.5 occur
    elif kind == "planted":
        valid = torch.full(vshape, 3.0)
    else:
        valid = torch.floor((uv + 1) * 2.5)                              # 0 .. 4 views
    objs = []
    if kind == "planted":   # rotated boxes: centre, half sizes, heading over [-pi, pi] (one beyond), label
        uo = _u((5, 8), seed * 10 + 2)
        for o in range(5):
            c = origin + uo[o, :3] * torch.tensor([2.0, 2.0, 0.6])
            half = 0.3 + 0.3 * (uo[o, 3:6] + 1)
            heading = float(uo[o, 6]) * math.pi * (1.3 if o == 4 else 1.0)
            objs.append((c, half, heading, int((uo[o, 7] + 1) * 8.5) % N_CLASSES))
    centers, bboxes, clss = [], [], []
    for lvl, size in enumerate(LEVELS):
        s = 100 * (lvl + 1) + seed * 10
        uc, ur, uk = _u((1, 1) + size, s + 3), _u((1, 7) + size, s + 4), _u((1, N_CLASSES) + size, s + 5)
        if kind == "empty":
            cls, ctr, reg = uk - 10.0, uc, 0.3 + 0.1 * ur
        elif kind == "planted":
            cls, ctr = 0.5 * uk - 9.0, 0.5 * uc
            reg = 0.2 + 0.05 * (ur + 1)
            p = level_points(size, lvl, origin)
            for c, half, heading, label in objs:
                d = p - c.view(3, 1, 1, 1)
                co, si = math.cos(heading), math.sin(heading)
                lx, ly, lz = d[0] * co + d[1] * si, -d[0] * si + d[1] * co, d[2]
                ins = (lx.abs() <= half[0]) & (ly.abs() <= half[1]) & (lz.abs() <= half[2])
                cls[0, label][ins] = (2.0 + uk[0, label])[ins]
                ctr[0, 0][ins] = (1.0 + 0.5 * uc[0, 0])[ins]
                faces = torch.stack([half[0] + lx, half[0] - lx, half[1] + ly, half[1] - ly, half[2] + lz, half[2] - lz])
                reg[0, :6][:, ins] = (faces * (1 + 0.15 * ur[0, :6]))[:, ins]
                reg[0, 6][ins] = (heading + 0.05 * ur[0, 6])[ins]
        elif kind == "sparse":
            cls, ctr, reg = 3.5 * uk - 7.7, 2.0 * uc, 0.1 + 0.15 * (ur + 1)
        else:   # a few dozen survivors per class: same-class pairs at iou_thr or in the margin band stay rare
            cls, ctr, reg = 3.5 * uk - 7.5, 2.0 * uc, 0.1 + 0.15 * (ur + 1)
        if kind != "planted":
            reg[0, 6] = 4.0 * ur[0, 6]   # headings over [-4, 4]
        centers.append(ctr.float().contiguous())
        bboxes.append(reg.float().contiguous())
        clss.append(cls.float().contiguous())
    return centers, bboxes, clss, valid, origin


def batch_inputs(kinds, seeds):
    scenes = [scene_inputs(k, s) for k, s in zip(kinds, seeds)]
    cat = lambda j: [torch.cat([sc[j][lvl] for sc in scenes]) for lvl in range(len(LEVELS))]  # noqa: E731
    return cat(0), cat(1), cat(2), torch.cat([sc[3] for sc in scenes]), [sc[4] for sc in scenes]


def nms3d_stand_in(boxes, scores, iou_threshold):
    """mmcv.ops.nms3d's stand-in: the NumPy restatement on the CPU tensors."""
    return torch.from_numpy(R.nms3d(boxes.numpy(), scores.numpy(), iou_threshold))


# ------------------------------------------------------------------------------------------------------------ the reference
def _slice(src, start, stop_pred):
    i1 = next(i for i in range(start + 1, len(src)) if stop_pred(src[i]))
    return src[start:i1]


def load_reference_predict(nms3d=nms3d_stand_in):
    """ImVoxelHead_ARKit's predict_by_feat .. _single_scene_multiclass_nms, get_points and rotation_3d_in_axis, executed where they
    lie as methods of a bare object: RefPredict(test_cfg).predict_by_feat(...)."""
    from typing import List, Tuple, Union

    from _ref_loader import REF_ROOT
    from torch import Tensor, nn
    path = os.path.join(REF_ROOT, "projects", "NeRF-Det", "nerfdet", "nerfdet_head.py")
    upath = os.path.join(REF_ROOT, "mmdet3d", "structures", "bbox_3d", "utils.py")
    for p in (path, upath):
        if not os.path.isfile(p):
            raise FileNotFoundError(p)
    usrc = open(upath).read().splitlines()
    r0 = next(i for i, l in enumerate(usrc) if l.startswith("def rotation_3d_in_axis("))
    while usrc[r0 - 1].startswith("@"):
        r0 -= 1
    rot = _slice(usrc, r0 + 1, lambda l: l.startswith("@") or l.startswith("def ") or l.startswith("class "))
    src = open(path).read().splitlines()
    cls_line = next(i for i, l in enumerate(src) if l.startswith("class ImVoxelHead_ARKit("))
    gp0 = next(i for i, l in enumerate(src) if l.startswith("def get_points("))
    gp1 = next(i for i in range(gp0, len(src)) if src[i].startswith("@MODELS"))
    a0 = next(i for i in range(cls_line, len(src)) if src[i].startswith("    def _predict_by_feat_single("))
    a1 = next(i for i in range(a0, len(src)) if src[i].startswith("    def _get_face_distances("))
    while src[a1 - 1].startswith("    @") or src[a1 - 1].strip().startswith("#"):
        a1 -= 1
    b0 = next(i for i in range(cls_line, len(src)) if src[i].startswith("    def _single_scene_multiclass_nms("))
    b1 = next((i for i in range(b0 + 1, len(src)) if src[i].startswith("@") or src[i].startswith("class ")), len(src))

    class InstanceData:                     # mmengine.structures.InstanceData: an attribute holder here
        pass

    def array_converter(**kwargs):          # mmdet3d's decorator: the inputs are tensors already
        return lambda fn: fn

    def nms3d_normal(*args):
        raise AssertionError("the ARKit head's boxes have 7 values: nms3d_normal is never called")

    ns = dict(torch=torch, nn=nn, np=np, Tensor=Tensor, List=List, Tuple=Tuple, Union=Union, InstanceData=InstanceData,
              array_converter=array_converter, nms3d=nms3d, nms3d_normal=nms3d_normal)
    exec(compile("\n".join(usrc[r0:r0 + 1] + rot), upath, "exec"), ns)
    exec(compile("\n".join(src[gp0:gp1]), path, "exec"), ns)
    exec(compile(textwrap.dedent("\n".join(src[a0:a1] + [""] + src[b0:b1])), path, "exec"), ns)

    class RefPredict:
        predict_by_feat, _predict_by_feat_single = ns["predict_by_feat"], ns["_predict_by_feat_single"]
        _upsample_valid_preds, _get_points = ns["_upsample_valid_preds"], ns["_get_points"]
        _bbox_pred_to_bbox, _single_scene_multiclass_nms = ns["_bbox_pred_to_bbox"], ns["_single_scene_multiclass_nms"]

        def __init__(self, test_cfg):
            self.test_cfg = test_cfg

    return RefPredict


def metas_for(origins):
    ident = lambda t, box_dim, with_yaw, origin: t  # noqa: E731  (box_type_3d stand-in: the raw tensor)
    return [{"lidar2img": {"origin": o.numpy().astype(np.float32)}, "box_type_3d": ident} for o in origins]


def make_test_cfg(nms_pre):
    return types.SimpleNamespace(nms_pre=nms_pre, score_thr=SCORE_THR, iou_thr=IOU_THR)


def run_reference(RefPredict, kinds, seeds, nms_pre):
    c, r, k, v, origins = batch_inputs(kinds, seeds)
    with torch.no_grad():
        res = RefPredict(make_test_cfg(nms_pre)).predict_by_feat(c, r, k, v, metas_for(origins))
    return res, (c, r, k, v, origins)


def scene_candidates(inputs, b, nms_pre):
    """One scene's candidates as the reference forms them (float32 torch): boxes (n, 7) decoded by our own arithmetic, class
    scores (n, C), the upsampled valid values of every level, per level the sorted max-scores (for the top-k screen)."""
    c, r, k, v, origins = inputs
    boxes, scores, ups, tops = [], [], [], []
    for lvl, size in enumerate(LEVELS):
        up = torch.nn.Upsample(size=size, mode="trilinear")(v[b:b + 1])
        ups.append(up.reshape(-1))
        vm = up.round().bool()[0]
        s = (k[lvl][b].sigmoid() * c[lvl][b].sigmoid() * vm).reshape(N_CLASSES, -1).t()
        ms = s.max(1).values
        ids = torch.arange(ms.numel())
        if ms.numel() > nms_pre > 0:
            tops.append(ms.sort(descending=True).values)
            ids = ms.topk(nms_pre).indices.sort().values
        p = level_points(size, lvl, origins[b]).reshape(3, -1).t()[ids]
        d = r[lvl][b].reshape(7, -1).t()[ids]
        shift = torch.stack(((d[:, 1] - d[:, 0]) / 2, (d[:, 3] - d[:, 2]) / 2), 1)
        co, si = d[:, 6].cos(), d[:, 6].sin()
        ctr = torch.stack((p[:, 0] + (shift[:, 0] * co - shift[:, 1] * si), p[:, 1] + (shift[:, 0] * si + shift[:, 1] * co),
                           p[:, 2]), 1)
        size_ = torch.stack((d[:, 0] + d[:, 1], d[:, 2] + d[:, 3], d[:, 4] + d[:, 5]), 1)
        boxes.append(torch.cat((ctr, size_, d[:, 6:7]), 1))
        scores.append(s[ids])
    return torch.cat(boxes).numpy(), torch.cat(scores).numpy(), ups, tops


def near_decisions(inputs, nms_pre):
    """Reasons a scene's result could flip under an ulp of sigmoid / sin / cos: an upsampled count near 0.5, a level's top-k
    boundary, a class score within 1e-5 of score_thr (relative: 1e-7, a hundred ulps), equal survivor scores in a class, a same-class IoU of the walk within 1e-4 of
    iou_thr, or a pair whose restated IoU and exact float64 clipping IoU fall on opposite sides of iou_thr."""
    why = []
    for b in range(inputs[3].shape[0]):
        boxes, scores, ups, tops = scene_candidates(inputs, b, nms_pre)
        for lvl, up in enumerate(ups):
            dist = (up - 0.5).abs()
            if ((dist > 0) & (dist < 1e-4)).any():
                why.append(f"scene {b} level {lvl}: an upsampled count near 0.5")
        for srt in tops:
            if abs(float(srt[nms_pre - 1] - srt[nms_pre])) <= 1e-5 * float(srt[nms_pre - 1]):
                why.append(f"scene {b}: top-k boundary")
        if (np.abs(scores.astype(np.float64) - SCORE_THR) < 1e-5 * SCORE_THR).any():
            why.append(f"scene {b}: a class score at score_thr")
        for cl in range(N_CLASSES):
            sel = scores[:, cl] > SCORE_THR
            if not sel.any():
                continue
            bx, sc = boxes[sel], scores[sel, cl]
            if len(np.unique(sc)) != len(sc):
                why.append(f"scene {b} class {cl}: equal survivor scores")
                continue
            bad = []

            def visit(i, js, iou):
                if bad:
                    return
                if (np.abs(iou.astype(np.float64) - IOU_THR) < 1e-4).any():
                    bad.append("an IoU at iou_thr")
                    return
                for j in js[iou > 0]:
                    if (R.exact_iou(bx[i], bx[j]) > IOU_THR) != (iou[js == j][0] > IOU_THR):
                        bad.append("restated and exact IoU on opposite sides of iou_thr")
                        return

            R.nms3d(bx, sc, IOU_THR, visit=visit)
            if bad:
                why.append(f"scene {b} class {cl}: {bad[0]}")
                break
    return why


def main():
    torch.set_num_threads(4)
    RefPredict = load_reference_predict()
    out = {}
    for name, (kinds, nms_pre) in CASES.items():
        for attempt in range(40):
            seeds = [BASE_SEED[name] + 7 * attempt + 3 * i for i in range(len(kinds))]
            res, inputs = run_reference(RefPredict, kinds, seeds, nms_pre)
            why = near_decisions(inputs, nms_pre)
            if not why:
                break
            print(f"{name}: seeds {seeds} rejected: {why[0]}")
        else:
            raise RuntimeError(f"{name}: no acceptable seed")
        out[f"{name}:kinds"] = np.array(kinds)
        out[f"{name}:seeds"] = np.array(seeds, dtype=np.int64)
        out[f"{name}:nms_pre"] = np.int64(nms_pre)
        for b, rs in enumerate(res):
            out[f"{name}:{b}:boxes"] = rs.bboxes_3d.numpy()
            out[f"{name}:{b}:scores"] = rs.scores_3d.numpy()
            out[f"{name}:{b}:labels"] = rs.labels_3d.numpy()
        print(name, "seeds", seeds, "kept", [len(rs.scores_3d) for rs in res],
              "classes", [len(np.unique(rs.labels_3d.numpy())) for rs in res])
    out.update(score_thr=np.float32(SCORE_THR), iou_thr=np.float32(IOU_THR), torch_version=np.array(torch.__version__),
               generator=np.array("tests/golden/make_goldens_g16.py"), stand_in=np.array(STAND_IN))
    path = os.path.join(HERE, "g16_detect_arkit.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
