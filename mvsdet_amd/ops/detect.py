"""NerfDetHead.predict_by_feat -> _nms -> aligned_3d_nms (nerfdet_head.py:301-420, 564-628) on csrc/detect.hip: head maps -> kept
boxes in four launches per batch on the current stream, no host synchronisation."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch
from torch import Tensor

from ._common import _lib, req, stream


DETECT_MAX_CANDIDATES = 16384   # MVSDET_DETECT_MAX_CANDIDATES: boxes of one scene above score_thr
DETECT_MAX_LEVELS = 4
DETECT_VOXEL_SIZE = (.16, .16, .2)   # NerfDetHead._get_points: tmp_voxel_size, doubled per level


class HeadPrediction(NamedTuple):
    """Padded detections of a batch: boxes (B,Nmax,6) (cx, cy, cz, dx, dy, dz), scores (B,Nmax), labels (B,Nmax) int64 and the
    kept count of every scene (B,) int32 -- a negative count -n: n boxes above score_thr, more than DETECT_MAX_CANDIDATES."""
    boxes: Tensor
    scores: Tensor
    labels: Tensor
    counts: Tensor


def detect_level_geometry(featmap_sizes, origins) -> Tensor:
    """(B, L, 6) host float32: per scene and level the voxel size and get_points' new_origin, from the reference's own torch ops
    (nerfdet_head.py:22-34, 408-419: torch.tensor(featmap_size) / 2. * voxel size, subtracted from the float32 origin)."""
    rows = []
    for origin in origins:
        o = origin if isinstance(origin, Tensor) else torch.tensor(origin)
        if o.dtype != torch.float32:
            raise ValueError(f"detection: lidar2img['origin'] must be float32 (got {o.dtype}); a float64 origin would make the "
                             "reference decode the boxes in float64")
        o = o.cpu().reshape(3)
        per = []
        for i, size in enumerate(featmap_sizes):
            n_voxels = torch.tensor(list(size))
            voxel_size = torch.tensor(DETECT_VOXEL_SIZE) * (2 ** i)
            new_origin = o - n_voxels / 2. * voxel_size
            per.append(torch.cat([voxel_size, new_origin]))
        rows.append(torch.stack(per))
    return torch.stack(rows).float()


def detect_candidates(featmap_sizes, nms_pre: int) -> int:
    """A scene's candidate capacity: per level nms_pre points if the level has more than nms_pre > 0 of them, else all."""
    n = 0
    for s in featmap_sizes:
        v = int(s[0]) * int(s[1]) * int(s[2])
        n += nms_pre if v > nms_pre > 0 else v
    return n


def head_predict(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, origins, nms_pre: int, score_thr: float,
                 iou_thr: float) -> HeadPrediction:
    """The ScanNet head's predict_by_feat up to the boxes, for every scene of the batch, on the current stream without a host sync.
    center_preds / bbox_preds / cls_preds: per level (B,1|6|C,X,Y,Z) float32; valid_pred (B,1,X,Y,Z): the stacked view counts (any
    dtype; taken as float, as the reference's torch.stack(valids).float()); origins: one float32 (3,) origin per scene.
    Kept boxes of a scene in pick order.  Visiting order of the walk: NaN scores first, whatever their sign; -0 and +0 equal; equal
    scores by level, then voxel index.  (The head's scores are >= +0 and a NaN never passes score_thr.)"""
    return _detect_head(center_preds, bbox_preds, cls_preds, valid_pred, origins, nms_pre, score_thr, iou_thr, rotated=False)


def head_predict_rotated(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, origins, nms_pre: int, score_thr: float,
                         iou_thr: float) -> HeadPrediction:
    """ImVoxelHead_ARKit's predict_by_feat up to the boxes (nerfdet_head.py:902-1056, 1190-1243), for every scene of the batch, on
    the current stream without a host sync: as head_predict, with bbox maps of 7 channels.  A top-k point keeps all its class
    scores; per class (ascending) the points with that score > score_thr go through nms3d (ops.nms3d).  HeadPrediction with boxes
    (B,Nmax,7) (x, y, z, dx, dy, dz, heading), Nmax = n_classes * min(candidates, DETECT_MAX_CANDIDATES), class-major rows.
    Visiting order inside a class: its score descending, equal scores by level, then voxel index.  A negative count -n: one class
    of the scene has n boxes above score_thr, more than DETECT_MAX_CANDIDATES."""
    return _detect_head(center_preds, bbox_preds, cls_preds, valid_pred, origins, nms_pre, score_thr, iou_thr, rotated=True)


def _detect_head(center_preds, bbox_preds, cls_preds, valid_pred, origins, nms_pre, score_thr, iou_thr, rotated: bool):
    fname = "head_predict_rotated" if rotated else "head_predict"
    nreg = 7 if rotated else 6
    L = len(center_preds)
    if not (1 <= L <= DETECT_MAX_LEVELS) or len(bbox_preds) != L or len(cls_preds) != L:
        raise ValueError(f"{fname}: 1..{DETECT_MAX_LEVELS} levels of center / bbox / cls maps needed")
    req(valid_pred, "valid_pred", dtype=valid_pred.dtype, dim=5)
    B = valid_pred.shape[0]
    valid = valid_pred.float().contiguous()
    centers, bboxes, clss, dims = [], [], [], []
    for lvl, (c, r, k) in enumerate(zip(center_preds, bbox_preds, cls_preds)):
        for t, name, ch in ((c, "center", 1), (r, "bbox", nreg), (k, "cls", None)):
            req(t, f"{name}_preds[{lvl}]", dim=5)
            if t.shape[0] != B or (ch is not None and t.shape[1] != ch) or t.shape[2:] != c.shape[2:]:
                raise ValueError(f"{fname}: {name}_preds[{lvl}] has shape {tuple(t.shape)}")
        if k.shape[1] != cls_preds[0].shape[1]:
            raise ValueError(f"{fname}: every level needs the same class count")
        centers.append(c.contiguous())
        bboxes.append(r.contiguous())
        clss.append(k.contiguous())
        dims += [int(v) for v in c.shape[2:]]
    sizes = [tuple(c.shape[2:]) for c in centers]
    if len(origins) != B:
        raise ValueError(f"{fname}: {len(origins)} origins for {B} scenes")
    dev = valid.device
    geom = detect_level_geometry(sizes, origins).pin_memory().to(dev, non_blocking=True)
    nms_pre = int(nms_pre)
    points = sum(s[0] * s[1] * s[2] for s in sizes)
    ncap = detect_candidates(sizes, nms_pre)
    n_classes = int(clss[0].shape[1])
    lib = _lib.load()
    if rotated:
        nmax = max(1, n_classes * min(ncap, DETECT_MAX_CANDIDATES))
        wsb, entry = lib.mvsdet_detect_rotated_workspace_bytes(B, points, ncap, n_classes), lib.mvsdet_detect_head_rotated_f32
    else:
        nmax = max(1, min(ncap, DETECT_MAX_CANDIDATES))
        wsb, entry = lib.mvsdet_detect_workspace_bytes(B, points, ncap), lib.mvsdet_detect_head_f32
    ws = torch.empty(int(wsb), dtype=torch.uint8, device=dev)
    boxes = torch.empty((B, nmax, nreg), dtype=torch.float32, device=dev)
    scores = torch.empty((B, nmax), dtype=torch.float32, device=dev)
    labels = torch.empty((B, nmax), dtype=torch.int64, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    arr = ctypes.c_void_p * L
    with torch.cuda.device(dev):
        _lib.check(entry(
            arr(*[t.data_ptr() for t in centers]), arr(*[t.data_ptr() for t in bboxes]), arr(*[t.data_ptr() for t in clss]),
            (ctypes.c_int * len(dims))(*dims), _lib.ptr(valid), _lib.ptr(geom), B, L, n_classes, *[int(v) for v in valid.shape[2:]],
            nms_pre, float(score_thr), float(iou_thr), _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(labels), _lib.ptr(counts), nmax,
            _lib.ptr(ws), ws.numel(), stream(valid)), fname)
    return HeadPrediction(boxes, scores, labels, counts)


def aligned_3d_nms(boxes: Tensor, scores: Tensor, classes: Tensor, thresh: float) -> Tensor:
    """NerfDetHead.aligned_3d_nms (nerfdet_head.py:580-628): boxes (n,6) (x1,y1,z1,x2,y2,z2), scores (n,), classes (n,) ->
    the kept indices in pick order (LongTensor).  CUDA float32 only; n <= DETECT_MAX_CANDIDATES.  Reads the kept count back
    (one host sync, as the reference's loop syncs on every box).  Visiting order: NaN scores first, whatever their sign (the
    reference's argsort puts NaN last and its loop takes from the end); -0 and +0 equal; equal scores by lower index first."""
    req(boxes, "boxes", dim=2)
    req(scores, "scores", dim=1)
    if not classes.is_cuda:
        raise RuntimeError(f"mvsdet_amd: `classes` must live on a ROCm device (got {classes.device}); this package has no CPU path")
    n = boxes.shape[0]
    if boxes.shape[1] != 6 or scores.shape[0] != n or classes.numel() != n:
        raise ValueError(f"aligned_3d_nms: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}, classes {tuple(classes.shape)}")
    if n > DETECT_MAX_CANDIDATES:
        raise ValueError(f"aligned_3d_nms: {n} boxes, above the candidate limit {DETECT_MAX_CANDIDATES}")
    b, s, c = boxes.contiguous(), scores.contiguous(), classes.reshape(-1).to(torch.int64).contiguous()
    lib = _lib.load()
    ws = torch.empty(int(lib.mvsdet_detect_workspace_bytes(1, 0, n)), dtype=torch.uint8, device=boxes.device)
    out = torch.empty((max(n, 1),), dtype=torch.int64, device=boxes.device)
    count = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(lib.mvsdet_aligned_3d_nms_f32(_lib.ptr(b), _lib.ptr(s), _lib.ptr(c), n, float(thresh), _lib.ptr(out),
                                                 _lib.ptr(count), _lib.ptr(ws), ws.numel(), stream(boxes)), "aligned_3d_nms")
    return out[:int(count.item())]


def nms3d(boxes: Tensor, scores: Tensor, iou_threshold: float) -> Tensor:
    """mmcv.ops.nms3d (mmcv 2.1.0) on csrc/detect.hip: boxes (n,7) (x, y, z, dx, dy, dz, heading), scores (n,) -> the kept indices
    in pick order (LongTensor).  Greedy by score; a later box goes when its bird's-eye-view IoU with a kept box is > iou_threshold
    (z and dz unused).  Equal scores by lower index first (mmcv's sort leaves them unordered); NaN scores first.  CUDA float32
    only; n <= DETECT_MAX_CANDIDATES.  Reads the kept count back (one host sync, as mmcv's own op)."""
    req(boxes, "boxes", dim=2)
    req(scores, "scores", dim=1)
    n = boxes.shape[0]
    if boxes.shape[1] != 7 or scores.shape[0] != n:
        raise ValueError(f"nms3d: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}")
    if n > DETECT_MAX_CANDIDATES:
        raise ValueError(f"nms3d: {n} boxes, above the candidate limit {DETECT_MAX_CANDIDATES}")
    b, s = boxes.contiguous(), scores.contiguous()
    lib = _lib.load()
    ws = torch.empty(int(lib.mvsdet_detect_rotated_workspace_bytes(1, 0, n, 1)), dtype=torch.uint8, device=boxes.device)
    out = torch.empty((max(n, 1),), dtype=torch.int64, device=boxes.device)
    count = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(lib.mvsdet_nms3d_f32(_lib.ptr(b), _lib.ptr(s), n, float(iou_threshold), _lib.ptr(out), _lib.ptr(count),
                                        _lib.ptr(ws), ws.numel(), stream(boxes)), "nms3d")
    return out[:int(count.item())]


def bev_iou_rotated(a: Tensor, b: Tensor) -> Tensor:
    """(n, m) bird's-eye-view IoU of the boxes a (n,7) and b (m,7), iou_bev of mmcv's nms3d (the device function the NMS uses,
    a first, early exit included).  CUDA float32 only; no host sync."""
    req(a, "a", dim=2)
    req(b, "b", dim=2)
    if a.shape[1] != 7 or b.shape[1] != 7:
        raise ValueError(f"bev_iou_rotated: boxes of 7 values needed, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, m = a.shape[0], b.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=a.device)
    x, y = a.contiguous(), b.contiguous()
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().mvsdet_bev_iou_rotated_f32(_lib.ptr(x), n, _lib.ptr(y), m, _lib.ptr(out), stream(a)), "bev_iou_rotated")
    return out
