"""Stage 2 of the hot path (depth_prob_topk / sample_depth_prob) restated in plain float64 torch: mvsdet.py:470-475 (softmax over
the planes, sigmoid of the offset logits), :266-283 (top-k planes, their densities and depths, depth = (d * iv + near) + off * iv)
and :298-317 (the depth expectation).  The reference of test_gpu_lift_forward_edges.py; test_lift_forward_host.py pins it against
the reference's own outputs (fixture g4_depth_prob) and against the CPU oracle before anything runs on a GPU.

The ranking is DEFINED here, not inherited from torch.topk, whose order among equal values is unspecified:
  * descending value;
  * NaN above every number (what torch.topk does: the reference hands a NaN probability on to the volume);
  * the lower plane first among equals and among NaNs.
"""
import numpy as np
import torch


def rank(prob, topk):
    """prob (N, D, H, W), any float type -> (N, topk, H, W) int64 plane indices under the rule above."""
    nan = torch.isnan(prob)
    by_value = torch.sort(torch.where(nan, torch.zeros_like(prob), prob), dim=1, descending=True, stable=True).indices
    # a second stable sort on "is NaN" lifts the NaN planes above every number and keeps each group's order
    nan_first = torch.sort(nan.gather(1, by_value).to(torch.int8), dim=1, descending=True, stable=True).indices
    return by_value.gather(1, nan_first)[:, :topk]


def depth_of_planes(off, near, iv):
    """(d * iv + near) + off * iv for every plane d, in off's dtype; near and iv are the float32 values the kernels receive."""
    near, iv = float(np.float32(near)), float(np.float32(iv))
    d = torch.arange(off.shape[1], dtype=off.dtype, device=off.device).view(1, -1, 1, 1)
    return (d * iv + near) + off * iv


def restated(a, b, near, iv, topk, from_logits=True, idx=None):
    """a, b: cost and offset logits (from_logits) or ready-made prob and off, (N, D, H, W).
    -> dict of float64 prob, off, est_depth, est_dens, avg_depth and int64 est_idx (`idx` if given, else `rank` of prob)."""
    a, b = a.double(), b.double()
    prob, off = (torch.softmax(a, dim=1), torch.sigmoid(b)) if from_logits else (a, b)
    depth = depth_of_planes(off, near, iv)
    if idx is None:
        idx = rank(prob, topk)
    idx = idx.long()
    return dict(prob=prob, off=off, est_depth=depth.gather(1, idx), est_dens=prob.gather(1, idx), est_idx=idx,
                avg_depth=(prob * depth).sum(dim=1))
