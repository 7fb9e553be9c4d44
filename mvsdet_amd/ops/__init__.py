"""PyTorch-ROCm custom operators over the C ABI (torch.ops.mvsdet_amd.*), one module per stage.

Every operator enqueues hand-written gfx950 kernels of libmvsdet_hip.so on the current HIP stream through ctypes; torch supplies
device memory, streams and autograd plumbing only.  Operators raise if their inputs are not float32 tensors on a ROCm device --
there is no CPU implementation here (one exception: ops.nvsmetric scores CPU tensors in torch float64).  Callers look a name up as `ops.<name>` at call time: every public name is re-exported.
"""
from __future__ import annotations

import torch

from .sweep import (  # noqa: F401
    _check_sweep, pack_features, homo_warp, validate_neighbors, plane_sweep_variance_packed, plane_sweep_variance_shard, plane_sweep_table,
    plane_sweep_variance_tabled, plane_sweep_variance_tabled_f16, sweep_flags, sweep_inside_count, sweep_stall_events, sweep_row_pitch,
    plane_sweep_table_pitched, plane_sweep_table_pooled, plane_sweep_variance_tabled_pitched, plane_sweep_variance,
    plane_sweep_variance_backward, plane_sweep_variance_keep, plane_sweep_variance_backward_packed, homo_warp_pixel,
    homo_warp_pixel_backward, plane_sweep_variance_pixel_packed, plane_sweep_variance_pixel, plane_sweep_variance_pixel_backward,
    device_copy, store_pattern_probe)
from .depth import ray_depth, depth_prob_topk, sample_depth_prob, depth_prob_topk_backward  # noqa: F401
from .lift import (  # noqa: F401
    backproject_weigh, backproject_weigh_backward, depth_diagnostics, backproject_weigh_mean, backproject_weigh_sum_shard,
    backproject_weigh_mean_backward)
from .costnet import (  # noqa: F401
    split_bf16, ROW_CHANNEL, split_conv_weight, split_conv_weights, SclTensor, PsclTensor, scl_geometry, pscl_geometry, scl_empty,
    pscl_empty, pscl_from_tensor, scl_pack, gemm_split_weight, gemm_layer_ok, conv3d_k1_s2_bf16x3, convT3d_k2_s2_bf16x3,
    conv3d_k1_s2_dx_bf16x3, convT3d_k2_s2_dx_bf16x3, neck_gemm_dw_splits, neck_gemm_dw_bf16x3, conv3d_k3_bf16x3, split_conv_weight_mx,
    conv3d_k3_fp16mx_ok, conv3d_k3_fp16mx, conv3d_k3_bf16x3_stats, conv3d_k3_s2_bf16x3, convT3d_k3_s2_bf16x3, convT3d_k3_s2_bf16x3_stats,
    conv3d_k3_cout2_sum, conv3d_k3_cout2, permute_conv_weight, conv3d_k3_mfma, permute_convT_weight, convT3d_k3_s2_mfma, conv3d_k3_dw,
    conv3d_k3_cout2_backward, bn3d_relu_train, bn3d_relu_backward, bn3d_res_relu_train, bn3d_res_relu_backward)
from .detect import (  # noqa: F401
    DETECT_MAX_CANDIDATES, DETECT_MAX_LEVELS, DETECT_VOXEL_SIZE, HeadPrediction, detect_level_geometry, detect_candidates, head_predict,
    head_predict_rotated, aligned_3d_nms, nms3d, bev_iou_rotated)
from .head_train import (  # noqa: F401
    ASSIGN_MAX_BOXES, HeadTargets, HeadLossSums, check_box_limit, head_targets, head_targets_rotated, head_loss, head_loss_rotated)
from .evalmap import (  # noqa: F401
    EVAL_MAX_RECORDS, EVAL_MAX_LABELS, EVAL_MAX_THRESHOLDS, EVAL_FLAGS, EvalState, EvalResult, eval_state, eval_reset, eval_match,
    eval_compute, eval_iou)
from . import nvsmetric  # noqa: F401  (ops.nvsmetric.<name>: not re-exported)
from . import photo  # noqa: F401  (ops.photo.<name>: not re-exported)
from . import splat  # noqa: F401  (ops.splat.<name>: not re-exported)
from . import adapter  # noqa: F401  (ops.adapter.<name>: not re-exported)
from . import gshead  # noqa: F401  (ops.gshead.<name>: not re-exported)
from . import fpn  # noqa: F401  (ops.fpn.<name>: not re-exported)
from . import resnet  # noqa: F401  (ops.resnet.<name>: not re-exported)

# ------------------------------------------------------------------------------------------- --amp (tools/train.py:24-28)
# Under torch.autocast the 2-D backbone hands out float16 / bfloat16 maps.  The hot path computes in float32 -- the rule torch's own
# autocast applies to `grid_sampler`, `softmax` and the reductions the reference runs here -- so these operators CAST low-precision
# floating inputs to float32 while autocast is on (and return float32), instead of raising the TypeError a non-float32 tensor gets
# outside autocast.  The fp16-STORAGE sweep (pack_features on float16 maps, plane_sweep_variance_shard(half_out=True)) is an explicit
# opt-in and keeps its dtypes: it has no autocast rule.
AUTOCAST_FP32_OPS = (homo_warp, plane_sweep_variance, plane_sweep_variance_keep, depth_prob_topk, sample_depth_prob,
                     backproject_weigh, backproject_weigh_mean)
# the evaluation-only diagnostics of the lifting block run under the same rule (no gradient, so not a forward operator of the path)
AUTOCAST_FP32_DIAGNOSTICS = (depth_diagnostics,)
# the per-pixel forms of a3 / a3+a4 (kept apart: AUTOCAST_FP32_OPS lists the operators of the shipped path)
AUTOCAST_FP32_PIXEL_OPS = (homo_warp_pixel, plane_sweep_variance_pixel)
for _op in AUTOCAST_FP32_OPS + AUTOCAST_FP32_PIXEL_OPS + AUTOCAST_FP32_DIAGNOSTICS:
    _op.register_autocast("cuda", torch.float32)
del _op
