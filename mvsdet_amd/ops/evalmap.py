"""mmdet3d's indoor_eval on csrc/evalmap.hip: eval_match appends a batch's detections to an evaluator's device state (two launches),
eval_compute orders them and returns the per-label values (a key fill, a bitonic sort, a claim and an AP launch), all on the
current stream without a host synchronisation or a device allocation of the library's.  mvsdet_amd.evaluation builds the
reference's ret_dict from them."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch
from torch import Tensor

from ._common import _lib, req, stream


EVAL_MAX_RECORDS = 1 << 20    # MVSDET_EVAL_MAX_RECORDS
EVAL_MAX_LABELS = 4095        # MVSDET_EVAL_MAX_LABELS
EVAL_MAX_THRESHOLDS = 8       # MVSDET_EVAL_MAX_THRESHOLDS
EVAL_FLAGS = {1: "more detections than `capacity`", 2: "more ground-truth boxes than `gt_capacity`",
              4: "a negative count (the heads' flag for more than DETECT_MAX_CANDIDATES boxes) or a count above the padded size",
              8: "a scene serial below one already fed", 16: "a label outside [0, n_labels)",
              32: "more records than the bound given to eval_compute"}


class EvalState(NamedTuple):
    """An evaluator's device memory: `state` (records, counts; mvsdet_eval_state_bytes) and the `workspace` of eval_compute at full
    capacity, both uint8, and the sizes every call on it repeats."""
    state: Tensor
    workspace: Tensor
    n_labels: int
    capacity: int
    gt_capacity: int
    n_thr: int


class EvalResult(NamedTuple):
    """Device outputs of eval_compute: ap (T,L) float32, recall (T,L) float64, npos, ndet (L) int32, first (L) int64 (where a label
    was first seen; -1 never), tp (T,n_bound) uint8 and order (n_bound) int32 in visiting order, info (4) int32 = records,
    ground-truth slots, flags (EVAL_FLAGS), next scene serial."""
    ap: Tensor
    recall: Tensor
    npos: Tensor
    ndet: Tensor
    first: Tensor
    tp: Tensor
    order: Tensor
    info: Tensor


def _eval_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"mvsdet_amd: the evaluator lives on a ROCm device (got {dev}); this package has no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def eval_state(n_labels: int, capacity: int, gt_capacity: int, n_thr: int, device) -> EvalState:
    """Allocate and clear an evaluator's state for up to `capacity` detections and `gt_capacity` ground-truth boxes in all."""
    dev = _eval_device(device)
    lib = _lib.load()
    n_labels, capacity, gt_capacity, n_thr = int(n_labels), int(capacity), int(gt_capacity), int(n_thr)
    nbytes = int(lib.mvsdet_eval_state_bytes(n_labels, capacity, gt_capacity))
    wbytes = int(lib.mvsdet_eval_workspace_bytes(n_labels, capacity, gt_capacity, n_thr)) if nbytes else 0
    if nbytes == 0 or wbytes == 0:
        raise ValueError(f"eval_state: n_labels={n_labels} (1..{EVAL_MAX_LABELS}), capacity={capacity} (1..{EVAL_MAX_RECORDS}), "
                         f"gt_capacity={gt_capacity} (1..{1 << 24}), {n_thr} thresholds (1..{EVAL_MAX_THRESHOLDS})")
    st = EvalState(torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(wbytes, dtype=torch.uint8, device=dev),
                   n_labels, capacity, gt_capacity, n_thr)
    eval_reset(st)
    return st


def eval_reset(st: EvalState) -> None:
    with torch.cuda.device(st.state.device):
        _lib.check(_lib.load().mvsdet_eval_reset(_lib.ptr(st.state), st.state.numel(), st.n_labels, st.capacity, st.gt_capacity,
                                                 stream(st.state)), "eval_reset")


def eval_match(st: EvalState, boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, gt_boxes: Tensor, gt_labels: Tensor,
               gt_counts: Tensor, scene0: int) -> None:
    """Append a batch to the state: boxes (B,N,7) and gt_boxes (B,G,7) float32 rows (x, y, BOTTOM z, dx, dy, dz, yaw), scores (B,N),
    labels (B,N) / gt_labels (B,G) int64, counts / gt_counts (B,) int32; scene0: the serial number of the batch's first scene."""
    req(boxes, "boxes", dim=3)
    req(scores, "scores", dim=2)
    req(labels, "labels", dtype=torch.int64, dim=2)
    req(counts, "counts", dtype=torch.int32, dim=1)
    req(gt_boxes, "gt_boxes", dim=3)
    req(gt_labels, "gt_labels", dtype=torch.int64, dim=2)
    req(gt_counts, "gt_counts", dtype=torch.int32, dim=1)
    B, N, G = int(boxes.shape[0]), int(boxes.shape[1]), int(gt_boxes.shape[1])
    if boxes.shape != (B, N, 7) or scores.shape != (B, N) or labels.shape != (B, N) or counts.shape != (B,) \
            or gt_boxes.shape != (B, G, 7) or gt_labels.shape != (B, G) or gt_counts.shape != (B,):
        raise ValueError(f"eval_match: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}, labels {tuple(labels.shape)}, counts "
                         f"{tuple(counts.shape)}, gt_boxes {tuple(gt_boxes.shape)}, gt_labels {tuple(gt_labels.shape)}, gt_counts "
                         f"{tuple(gt_counts.shape)}: (B,N,7), (B,N), (B,N), (B,), (B,G,7), (B,G), (B,) wanted")
    if boxes.device != st.state.device or gt_boxes.device != st.state.device:
        raise RuntimeError(f"eval_match: inputs on {boxes.device} / {gt_boxes.device}, the evaluator on {st.state.device}")
    t = [x.contiguous() for x in (boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts)]
    with torch.cuda.device(st.state.device):
        _lib.check(_lib.load().mvsdet_eval_match_f32(
            _lib.ptr(st.state), st.n_labels, st.capacity, st.gt_capacity, _lib.ptr(t[0]) if N else None, _lib.ptr(t[1]) if N else None,
            _lib.ptr(t[2]) if N else None, _lib.ptr(t[3]), B, N, _lib.ptr(t[4]) if G else None, _lib.ptr(t[5]) if G else None,
            _lib.ptr(t[6]), G, int(scene0), stream(st.state)), "eval_match")


def eval_compute(st: EvalState, thresholds, n_bound: int) -> EvalResult:
    """Per-label AP and recall of everything fed so far (the state is left as it is).  n_bound: a host-side upper bound of the
    detections fed (<= capacity), which sizes the sort and the per-record outputs."""
    thr = [float(v) for v in thresholds]
    if len(thr) != st.n_thr:
        raise ValueError(f"eval_compute: {len(thr)} thresholds, the state was made for {st.n_thr}")
    dev, T, L, n = st.state.device, st.n_thr, st.n_labels, int(n_bound)
    ap = torch.empty((T, L), dtype=torch.float32, device=dev)
    recall = torch.empty((T, L), dtype=torch.float64, device=dev)
    npos = torch.empty(L, dtype=torch.int32, device=dev)
    ndet = torch.empty(L, dtype=torch.int32, device=dev)
    first = torch.empty(L, dtype=torch.int64, device=dev)
    tp = torch.empty((T, n), dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_eval_compute(
            _lib.ptr(st.state), L, st.capacity, st.gt_capacity, n, (ctypes.c_float * T)(*thr), T, _lib.ptr(ap), _lib.ptr(recall),
            _lib.ptr(npos), _lib.ptr(ndet), _lib.ptr(first), _lib.ptr(tp) if n else None, _lib.ptr(order) if n else None, _lib.ptr(info),
            _lib.ptr(st.workspace), st.workspace.numel(), stream(st.state)), "eval_compute")
    return EvalResult(ap, recall, npos, ndet, first, tp, order, info)


def eval_iou(a: Tensor, b: Tensor) -> Tensor:
    """(n, m) IoU of boxes a (n,7) and b (m,7) (x, y, bottom z, dx, dy, dz, yaw) as the evaluator takes it: BaseInstance3DBoxes.overlaps
    as a mathematical function in float32 -- not mmcv's box_iou_rotated rounding, and not iou_bev of bev_iou_rotated."""
    req(a, "a", dim=2)
    req(b, "b", dim=2)
    if a.shape[1] != 7 or b.shape[1] != 7:
        raise ValueError(f"eval_iou: boxes of 7 values needed, got {tuple(a.shape)} and {tuple(b.shape)}")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    x, y = a.contiguous(), b.contiguous()
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().mvsdet_eval_iou_f32(_lib.ptr(x), int(a.shape[0]), _lib.ptr(y), int(b.shape[0]), _lib.ptr(out), stream(a)),
                   "eval_iou")
    return out
