#!/usr/bin/env python3
"""Generate tests/golden/g15_detect.npz by RUNNING THE REFERENCE (build container only: needs the reference tree).

G15: the ScanNet head's post-processing, NerfDetHead.predict_by_feat -> _predict_by_feat_single -> _nms -> aligned_3d_nms
(projects/NeRF-Det/nerfdet/nerfdet_head.py:301-428, 564-628, and get_points :21-34), executed where it lies on CPU with three
stand-ins: mmengine's InstanceData (an attribute holder), the test_cfg (an attribute holder with nms_pre, score_thr, iou_thr) and
no `box_type_3d` (the meta carries an identity callable, so the reference returns its raw (n, 6) tensor).

Inputs are head maps at the ScanNet level sizes (40x40x16, 20x20x8, 10x10x4) with 18 classes, made from LCG seeds by
`scene_inputs` below (the GPU test rebuilds them from the stored seeds); only the seeds and the reference's outputs are stored.
A scene whose result hangs on a decision within rounding of a threshold is rejected and reseeded (`near_decisions`): CPU and
GPU sigmoid / exp may differ by an ulp.

    python tests/golden/make_goldens_g15.py
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from lcg import lcg_uniform  # noqa: E402

LEVELS = ((40, 40, 16), (20, 20, 8), (10, 10, 4))
N_CLASSES = 18
VOXEL = (.16, .16, .2)
SCORE_THR, IOU_THR = 0.01, 0.25

# name -> (scene kinds, nms_pre); one base seed per scene
CASES = {
    "planted": (("planted",), 1000),
    "random": (("random",), 1000),
    "empty": (("empty",), 1000),
    "half": (("half",), 1000),
    "batch2": (("planted", "random"), 1000),
    "nms_pre_big": (("sparse",), 30000),
    "nms_pre_zero": (("sparse",), 0),
}
BASE_SEED = {"planted": 1500, "random": 1510, "empty": 1520, "half": 1530, "batch2": 1540, "nms_pre_big": 1560, "nms_pre_zero": 1570}


def _u(shape, seed):
    return torch.from_numpy(lcg_uniform(int(np.prod(shape)), seed)).reshape(shape)


def level_points(size, level, origin):
    """get_points of one level as (3, X, Y, Z) float32 (our own restatement, for planting objects only)."""
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
    centers, bboxes, clss = [], [], []
    objs = []
    if kind == "planted":
        uo = _u((5, 8), seed * 10 + 2)
        for o in range(5):
            c = origin + uo[o, :3] * torch.tensor([2.0, 2.0, 0.6])
            half = 0.3 + 0.3 * (uo[o, 3:6] + 1)
            objs.append((c - half, c + half, int((uo[o, 6] + 1) * 9) % N_CLASSES))
    for lvl, size in enumerate(LEVELS):
        s = 100 * (lvl + 1) + seed * 10
        uc, ur, uk = _u((1, 1) + size, s + 3), _u((1, 6) + size, s + 4), _u((1, N_CLASSES) + size, s + 5)
        if kind == "empty":
            cls, ctr, reg = uk - 10.0, uc, 0.3 + 0.1 * ur
        elif kind == "planted":
            cls, ctr = 0.5 * uk - 9.0, 0.5 * uc
            reg = 0.2 + 0.05 * (ur + 1)
            p = level_points(size, lvl, origin)
            for lo, hi, label in objs:
                ins = ((p >= lo.view(3, 1, 1, 1)) & (p <= hi.view(3, 1, 1, 1))).all(0)
                cls[0, label][ins] = (2.0 + uk[0, label])[ins]
                ctr[0, 0][ins] = (1.0 + 0.5 * uc[0, 0])[ins]
                faces = torch.stack([p[0] - lo[0], hi[0] - p[0], p[1] - lo[1], hi[1] - p[1], p[2] - lo[2], hi[2] - p[2]])
                reg[0][:, ins] = (faces * (1 + 0.15 * ur[0]))[:, ins]
        elif kind == "sparse":
            cls, ctr, reg = 3.5 * uk - 6.5, 2.0 * uc, 0.05 + 0.1 * (ur + 1)
        else:
            cls, ctr, reg = 3.5 * uk - 4.5, 2.0 * uc, 0.05 + 0.1 * (ur + 1)
        centers.append(ctr.float().contiguous())
        bboxes.append(reg.float().contiguous())
        clss.append(cls.float().contiguous())
    return centers, bboxes, clss, valid, origin


def batch_inputs(kinds, seeds):
    scenes = [scene_inputs(k, s) for k, s in zip(kinds, seeds)]
    cat = lambda j: [torch.cat([sc[j][lvl] for sc in scenes]) for lvl in range(len(LEVELS))]  # noqa: E731
    return cat(0), cat(1), cat(2), torch.cat([sc[3] for sc in scenes]), [sc[4] for sc in scenes]


# ------------------------------------------------------------------------------------------------------------ the reference
def load_reference_predict():
    """NerfDetHead's predict_by_feat .. aligned_3d_nms and get_points, executed where they lie (nerfdet_head.py:21-34, 301-428,
    564-633) as methods of a bare object: RefPredict(test_cfg).predict_by_feat(...)."""
    from _ref_loader import REF_ROOT
    path = os.path.join(REF_ROOT, "projects", "NeRF-Det", "nerfdet", "nerfdet_head.py")
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    src = open(path).read().splitlines()
    cls_line = next(i for i, l in enumerate(src) if l.startswith("class NerfDetHead("))
    gp0 = next(i for i, l in enumerate(src) if l.startswith("def get_points("))
    gp1 = next(i for i in range(gp0, len(src)) if src[i].startswith("@MODELS"))
    a0 = next(i for i in range(cls_line, len(src)) if src[i].startswith("    def predict_by_feat("))
    a1 = next(i for i in range(a0, len(src)) if src[i].startswith("    def _bbox_pred_to_loss("))
    b0 = next(i for i in range(a1, len(src)) if src[i].startswith("    def _nms("))
    b1 = next(i for i in range(b0, len(src)) if src[i].startswith("@MODELS") or src[i].startswith("class "))
    from typing import List
    from torch import Tensor, nn

    class InstanceData:                     # mmengine.structures.InstanceData: an attribute holder here
        pass

    ns = dict(torch=torch, nn=nn, Tensor=Tensor, List=List, InstanceData=InstanceData)
    exec(compile("\n".join(src[gp0:gp1]), path, "exec"), ns)
    exec(compile(textwrap.dedent("\n".join(src[a0:a1] + [""] + src[b0:b1])), path, "exec"), ns)

    class RefPredict:
        predict_by_feat, _predict_by_feat_single = ns["predict_by_feat"], ns["_predict_by_feat_single"]
        _upsample_valid_preds, _get_points = ns["_upsample_valid_preds"], ns["_get_points"]
        _bbox_pred_to_bbox, _nms, aligned_3d_nms = ns["_bbox_pred_to_bbox"], ns["_nms"], ns["aligned_3d_nms"]

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


def near_decisions(inputs, nms_pre):
    """Reasons a scene's result could flip under an ulp of sigmoid: max-scores near score_thr, a level's top-k boundary, equal
    survivor scores, a same-class pair of the greedy walk with |IoU - iou_thr| < 1e-4 (float64 restatement)."""
    c, r, k, v, origins = inputs
    why = []
    for b in range(v.shape[0]):
        boxes, scores, labels = [], [], []
        for lvl, size in enumerate(LEVELS):
            vm = torch.nn.Upsample(size=size, mode="trilinear")(v[b:b + 1]).round().bool()[0]
            s = (k[lvl][b].sigmoid() * c[lvl][b].sigmoid() * vm).reshape(N_CLASSES, -1).double()
            ms, lab = s.max(0)
            if ((ms - SCORE_THR).abs() < 1e-5 * SCORE_THR).any():
                why.append(f"scene {b} level {lvl}: a max-score at score_thr")
            ids = torch.arange(ms.numel())
            if ms.numel() > nms_pre > 0:
                srt = ms.sort(descending=True).values
                if abs(float(srt[nms_pre - 1] - srt[nms_pre])) <= 1e-5 * float(srt[nms_pre - 1]):
                    why.append(f"scene {b} level {lvl}: top-k boundary")
                ids = ms.topk(nms_pre).indices
            p = level_points(size, lvl, origins[b]).reshape(3, -1).t().double()[ids]
            d = r[lvl][b].reshape(6, -1).t().double()[ids]
            boxes.append(torch.stack([p[:, 0] - d[:, 0], p[:, 1] - d[:, 2], p[:, 2] - d[:, 4],
                                      p[:, 0] + d[:, 1], p[:, 1] + d[:, 3], p[:, 2] + d[:, 5]], 1))
            scores.append(ms[ids])
            labels.append(lab[ids])
        bx, sc, lb = torch.cat(boxes), torch.cat(scores), torch.cat(labels)
        keep = sc > SCORE_THR
        bx, sc, lb = bx[keep].numpy(), sc[keep].numpy(), lb[keep].numpy()
        if len(np.unique(sc.astype(np.float32))) != len(sc):
            why.append(f"scene {b}: equal survivor scores")
        order = np.argsort(-sc, kind="stable")
        bx, lb = bx[order], lb[order]
        area = (bx[:, 3] - bx[:, 0]) * (bx[:, 4] - bx[:, 1]) * (bx[:, 5] - bx[:, 2])
        alive = np.ones(len(sc), bool)
        for i in range(len(sc)):
            if not alive[i]:
                continue
            j = np.nonzero(alive[i + 1:] & (lb[i + 1:] == lb[i]))[0] + i + 1
            if len(j) == 0:
                continue
            lo, hi = np.maximum(bx[i, :3], bx[j, :3]), np.minimum(bx[i, 3:], bx[j, 3:])
            inter = np.prod(np.maximum(hi - lo, 0), axis=1)
            iou = inter / (area[i] + area[j] - inter)
            if (np.abs(iou - IOU_THR) < 1e-4).any():
                why.append(f"scene {b}: an IoU at iou_thr")
                break
            alive[j[iou > IOU_THR]] = False
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
        if name == "half":   # the case exists for round-half-to-even: some upsampled level-1 / level-2 value is exactly 0.5
            v = inputs[3]
            assert any((torch.nn.Upsample(size=sz, mode="trilinear")(v) == 0.5).any() for sz in LEVELS[1:])
        out[f"{name}:kinds"] = np.array(kinds)
        out[f"{name}:seeds"] = np.array(seeds, dtype=np.int64)
        out[f"{name}:nms_pre"] = np.int64(nms_pre)
        for b, rs in enumerate(res):
            out[f"{name}:{b}:boxes"] = rs.bboxes_3d.numpy()
            out[f"{name}:{b}:scores"] = rs.scores_3d.numpy()
            out[f"{name}:{b}:labels"] = rs.labels_3d.numpy()
        print(name, "seeds", seeds, "kept", [len(rs.scores_3d) for rs in res])
    out.update(score_thr=np.float32(SCORE_THR), iou_thr=np.float32(IOU_THR), torch_version=np.array(torch.__version__),
               generator=np.array("tests/golden/make_goldens_g15.py"),
               stand_in=np.array("mmengine's InstanceData as an attribute holder, the test_cfg as a SimpleNamespace, box_type_3d as "
                                 "the identity (tests/golden/make_goldens_g15.py)"))
    path = os.path.join(HERE, "g15_detect.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
