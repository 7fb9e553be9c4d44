"""ctypes binding of libmvsdet_hip.so (include/mvsdet_hip.h) -- the stub a maintainer of the reference
would add to call the HIP path from Python.

There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVSDET_HIP_LIB: load another build of the same C ABI (kernel A/B runs); the default is the in-tree library
LIB_PATH = os.environ.get("MVSDET_HIP_LIB") or os.path.join(_HERE, "libmvsdet_hip.so")
_lib = None

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_i64p = ctypes.POINTER(ctypes.c_int64)
_i64 = ctypes.c_int64

# name -> argtypes (all return int unless listed in _RESTYPE); mirrors include/mvsdet_hip.h one to one
SIGNATURES = {
    "mvsdet_version": [],
    "mvsdet_last_error": [],
    "mvsdet_set_option": [ctypes.c_char_p, _i],
    "mvsdet_get_option": [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)],
    "mvsdet_validate_neighbors": [_i64p, _i, _i, _i],
    "mvsdet_packed_bytes": [_i, _i, _i, _i],
    "mvsdet_pack_features_f32": [_vp, _i64p, _vp, _i, _i, _i, _i, _vp],
    "mvsdet_pack_features_f16": [_vp, _i64p, _vp, _i, _i, _i, _i, _vp],
    "mvsdet_homo_warp_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_scratch_bytes": [_i, _i, _i, _i, _i],
    "mvsdet_plane_sweep_workspace_bytes": [_i, _i, _i, _i, _i, _i],
    "mvsdet_plane_sweep_variance_packed_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_variance_shard_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_variance_shard_f16": [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_table_f32": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_variance_tabled_f32": [_vp, _vp, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_variance_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_bwd_workspace_bytes": [_i, _i, _i, _i, _i, _i],
    "mvsdet_plane_sweep_variance_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_variance_bwd_packed_f32": [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_depth_prob_topk_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "mvsdet_depth_prob_topk_strided_f32": [_vp, _vp, ctypes.c_longlong, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "mvsdet_sample_depth_prob_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "mvsdet_ray_depth_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_depth_prob_topk_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "mvsdet_convT3d_k3_s2_mfma_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_tile_shape": [_i, _i, _i, _i, _vp, _vp, _vp],
    "mvsdet_conv3d_k3_mfma_workspace_bytes": [_i, _i, _i, _i, _i, _i, _i],
    "mvsdet_bn3d_workspace_bytes": [_i],
    "mvsdet_bn3d_relu_train_fwd_res_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, ctypes.c_longlong, _f, _f, _i, _vp],
    "mvsdet_bn3d_relu_train_fwd_parts_f32": [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, ctypes.c_longlong, _f, _f, _i, _vp],
    "mvsdet_bn3d_relu_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, ctypes.c_longlong, _i, _vp],
    "mvsdet_bn3d_res_relu_train_fwd_f32": [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, ctypes.c_longlong, _f, _f, _i, _vp],
    "mvsdet_bn3d_res_relu_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, ctypes.c_longlong, _i, _vp],
    "mvsdet_conv3d_k3_mfma_ws_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_dw_partial_bytes": [_i, _i, _i],
    "mvsdet_conv3d_k3_dw_mfma_f32": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_dw_bf16x3": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_s2_dw_mfma_f32": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_s2_dw_bf16x3": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_cout2_dx_f32": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_cout2_dw_f32": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_cout2_dw_bf16x3": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_cout2_dw_bf16x3_ok": [_i, _i],
    "mvsdet_gemm_split_weight_bytes": [_i, _i],
    "mvsdet_gemm_split_weight": [_vp, _vp, _i, _i, _vp],
    "mvsdet_conv3d_k1_s2_bf16x3": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_convT3d_k2_s2_bf16x3": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k1_s2_dx_bf16x3": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_convT3d_k2_s2_dx_bf16x3": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_neck_gemm_dw_partial_bytes": [_i, _i, _i, _i],
    "mvsdet_neck_gemm_dw_bf16x3": [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_fpn_lateral_bf16x3": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_fpn_conv3x3_bf16x3": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "mvsdet_fpn_dw_splits": [_i, _i, _i, _i, _i, _i],
    "mvsdet_fpn_dw_workspace_bytes": [_i, _i, _i, _i, _i, _i],
    "mvsdet_fpn_dw_bf16x3": [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_fpn_top_down_grad_f32": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_fpn_bias_grad_f32": [_vp, _vp, _i, _i, _i, _i, _vp],
    "mvsdet_resnet_conv1x1_bf16x3": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_resnet_conv3x3_bf16x3": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_resnet_relu_gate_f32": [_vp, _vp, _vp, ctypes.c_longlong, _vp],
    "mvsdet_resnet_conv1x1_dx_bf16x3": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_resnet_conv3x3_dx_bf16x3": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_resnet_dw_s2_splits": [_i, _i, _i, _i, _i, _i],
    "mvsdet_resnet_dw_s2_workspace_bytes": [_i, _i, _i, _i, _i, _i],
    "mvsdet_resnet_dw_s2_bf16x3": [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_cout2_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_cout2_sum_f32": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "mvsdet_backproject_weigh_f32": [_vp, _i64p, _vp, _vp, _vp, _vp, _i64p, _vp, _vp, _vp, _vp,
                                     _i, _i, _i, _i, _i, _i, _f, _vp],
    "mvsdet_backproject_weigh_mean_packed_f32": [_vp, _vp, _vp, _vp, _vp, _i64p, _vp, _vp,
                                                 _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp],
    "mvsdet_backproject_weigh_sum_packed_f32": [_vp, _vp, _vp, _vp, _vp, _i64p, _vp, _vp,
                                                _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp],
    "mvsdet_backproject_weigh_bwd_f32": [_vp, _i64p, _vp, _vp, _vp, _vp, _i64p, _vp, _vp, _vp,
                                         _i, _i, _i, _i, _i, _i, _f, _vp],
    "mvsdet_backproject_weigh_mean_bwd_f32": [_vp, _i64p, _vp, _vp, _vp, _vp, _i64p, _vp, _vp, _vp, _vp,
                                              _i, _i, _i, _i, _i, _i, _f, _vp],
    "mvsdet_depth_diagnostics_workspace_bytes": [_i, _i, _i, _i],
    "mvsdet_depth_diagnostics_f32": [_vp, _vp, _vp, _vp, _i64p, _vp, _i64p, _vp, _i64p, _vp, _vp, _vp, _vp, _vp, _sz,
                                     _i, _i, _i, _i, _i, _i, _i, _f, _vp],
    "mvsdet_depth_loss_workspace_bytes": [_i, _i, _i],
    "mvsdet_depth_loss_f32": [_vp, _i64p, _vp, _i64p, _vp, _i64p, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_depth_loss_bwd_f32": [_vp, _i64p, _vp, _i64p, _vp, _i64p, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_photo_geometry_f32": [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _i, _i, _vp, _i, _vp],
    "mvsdet_photo_warp_f32": [_vp, _i64p, _vp, _i, _vp, _i64p, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "mvsdet_photo_warp_bwd_f32": [_vp, _i64p, _vp, _i, _vp, _i64p, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "mvsdet_photo_loss_workspace_bytes": [_i, _i, _i],
    "mvsdet_photo_loss_f32": [_vp, _vp, _vp, _i64p, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp],
    "mvsdet_photo_loss_bwd_f32": [_vp, _vp, _vp, _i64p, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "mvsdet_photo_select_workspace_bytes": [_i, _i],
    "mvsdet_photo_select_f32": [_vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _vp],
    "mvsdet_photo_select_bwd_f32": [_vp, _vp, _vp, _i, _i, _vp],
    "mvsdet_splat_workspace_bytes": [_i, _i, _i, _i, _i],
    "mvsdet_splat_cameras_f32": [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _i, _vp, _i, _vp],
    "mvsdet_splat_forward_f32": [_vp, _i64p, _vp, _i64p, _vp, _i64p, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i,
                                 _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_splat_backward_f32": [_vp, _i64p, _vp, _i64p, _vp, _i64p, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp,
                                  _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_adapter_cameras_f32": [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _i, _i, _i, _i, _vp],
    "mvsdet_adapter_forward_f32": [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "mvsdet_adapter_backward_f32": [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "mvsdet_gshead_forward_f32": [_vp, _i64p, _vp, _i64p, _vp, _vp, _i64p, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_gshead_rgb_rows_f32": [_vp, _i64p, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_gshead_backward_input_f32": [_vp, _i64p, _vp, _i64p, _vp, _vp, _vp, _vp, _i64p, _vp, _i64p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_gshead_partial_bytes": [_i, _i, _i, _i, _i],
    "mvsdet_gshead_backward_weight_f32": [_vp, _i64p, _vp, _i64p, _vp, _vp, _i64p, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i,
                                          _i, _i, _i, _i, _vp],
    "mvsdet_copy_f32": [_vp, _vp, _sz, _vp],
    "mvsdet_store_pattern_probe_f32": [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_store_pattern_probe_f16": [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_scl_bytes": [_i, _i, _i, _i, _i, _vp, _vp, _vp],
    "mvsdet_pscl_bytes": [_i, _i, _i, _i, _i, _vp, _vp, _vp],
    "mvsdet_conv3d_k3_bf16x3_io": [_vp, _vp, _i64p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_bf16x3_stats_parts": [_i, _i, _i, _i, _i],
    "mvsdet_conv3d_k3_bf16x3_stats": [_vp, _vp, _i64p, _vp, _vp, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_convT3d_k3_s2_bf16x3_stats_parts": [_i, _i, _i, _i],
    "mvsdet_convT3d_k3_s2_bf16x3_stats": [_vp, _vp, _vp, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_s2_bf16x3_io": [_vp, _i64p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_convT3d_k3_s2_bf16x3_io": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_split_conv_weight_bytes": [_i, _i],
    "mvsdet_split_conv_weight_ordered": [_vp, _vp, _i, _i, _i, _vp],
    "mvsdet_split_conv_weights_batched": [_vp, _vp, _vp, _vp, _vp, _i, _vp],
    "mvsdet_scl_pack_f32": [_vp, _i64p, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_table_pitched_f32": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_variance_tabled_f16": [_vp, _vp, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_table_pooled_f32": [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_variance_tabled_pitched_f32": [_vp, _vp, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_bf16x3_workspace_bytes": [_i, _i, _i, _i, _i, _i],
    "mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes": [_i, _i, _i, _i, _i, _i],
    "mvsdet_split_conv_weight_mx_bytes": [_i, _i],
    "mvsdet_split_conv_weight_mx": [_vp, _vp, _i, _i, _vp],
    "mvsdet_conv3d_k3_fp16mx_f32in": [_vp, _i64p, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_conv3d_k3_fp16mx_ok": [_i, _i, _i, _i, _i, _i64p],
    "mvsdet_detect_workspace_bytes": [_i, _i, _i],
    "mvsdet_detect_head_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp],
    "mvsdet_aligned_3d_nms_f32": [_vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _sz, _vp],
    "mvsdet_detect_rotated_workspace_bytes": [_i, _i, _i, _i],
    "mvsdet_detect_head_rotated_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _i, _vp, _sz,
                                       _vp],
    "mvsdet_nms3d_f32": [_vp, _vp, _i, _f, _vp, _vp, _vp, _sz, _vp],
    "mvsdet_bev_iou_rotated_f32": [_vp, _i, _vp, _i, _vp, _vp],
    "mvsdet_head_targets_workspace_bytes": [_i, _i],
    "mvsdet_head_targets_f32": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "mvsdet_head_loss_workspace_bytes": [_i, _i],
    "mvsdet_head_loss_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _sz, _vp],
    "mvsdet_head_loss_backward_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp,
                                      _vp],
    "mvsdet_head_targets_rotated_f32": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "mvsdet_head_loss_rotated_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _sz,
                                     _vp],
    "mvsdet_head_loss_rotated_backward_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp,
                                              _vp, _vp, _vp],
    "mvsdet_eval_state_bytes": [_i, _i, _i],
    "mvsdet_eval_workspace_bytes": [_i, _i, _i, _i],
    "mvsdet_eval_reset": [_vp, _sz, _i, _i, _i, _vp],
    "mvsdet_eval_match_f32": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp],
    "mvsdet_eval_compute": [_vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_float), _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                            _vp],
    "mvsdet_eval_iou_f32": [_vp, _i, _vp, _i, _vp, _vp],
    "mvsdet_nvs_workspace_bytes": [_i, _i, _i, _i],
    "mvsdet_nvs_reset": [_vp, _vp],
    "mvsdet_nvs_score_f32": [_vp, _vp, _i64p, _vp, _i64p, _vp, _i64p, _vp, _i64p, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "mvsdet_homo_warp_pixel_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "mvsdet_homo_warp_pixel_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_variance_pixel_packed_f32": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_pixel_bwd_workspace_bytes": [_i, _i, _i, _i],
    "mvsdet_plane_sweep_variance_pixel_bwd_packed_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_groupcorr_packed_f32": [_vp, _vp, _vp, _vp, _i64p, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_plane_sweep_groupcorr_bwd_packed_f32": [_vp, _vp, _vp, _vp, _i64p, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp],
    "mvsdet_pixel_form_blocking": [_i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp],
}
_RESTYPE = {"mvsdet_last_error": ctypes.c_char_p, "mvsdet_conv3d_k3_bf16x3_stats_parts": ctypes.c_size_t, "mvsdet_convT3d_k3_s2_bf16x3_stats_parts": ctypes.c_size_t, "mvsdet_gemm_split_weight_bytes": ctypes.c_size_t, "mvsdet_neck_gemm_dw_partial_bytes": ctypes.c_size_t, "mvsdet_scl_bytes": ctypes.c_size_t, "mvsdet_pscl_bytes": ctypes.c_size_t,
            "mvsdet_split_conv_weight_bytes": ctypes.c_size_t, "mvsdet_packed_bytes": ctypes.c_size_t,
            "mvsdet_split_conv_weight_mx_bytes": ctypes.c_size_t, "mvsdet_detect_workspace_bytes": ctypes.c_size_t,
            "mvsdet_detect_rotated_workspace_bytes": ctypes.c_size_t,
            "mvsdet_head_targets_workspace_bytes": ctypes.c_size_t, "mvsdet_head_loss_workspace_bytes": ctypes.c_size_t,
            "mvsdet_plane_sweep_scratch_bytes": ctypes.c_size_t, "mvsdet_plane_sweep_workspace_bytes": ctypes.c_size_t,
            "mvsdet_plane_sweep_bwd_workspace_bytes": ctypes.c_size_t,
            "mvsdet_plane_sweep_pixel_bwd_workspace_bytes": ctypes.c_size_t,
            "mvsdet_conv3d_k3_dw_partial_bytes": ctypes.c_size_t,
            "mvsdet_conv3d_k3_bf16x3_workspace_bytes": ctypes.c_size_t,
            "mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes": ctypes.c_size_t,
            "mvsdet_depth_diagnostics_workspace_bytes": ctypes.c_size_t,
            "mvsdet_depth_loss_workspace_bytes": ctypes.c_size_t,
            "mvsdet_photo_loss_workspace_bytes": ctypes.c_size_t, "mvsdet_photo_select_workspace_bytes": ctypes.c_size_t,
            "mvsdet_splat_workspace_bytes": ctypes.c_size_t, "mvsdet_gshead_partial_bytes": ctypes.c_size_t,
            "mvsdet_eval_state_bytes": ctypes.c_size_t, "mvsdet_eval_workspace_bytes": ctypes.c_size_t,
            "mvsdet_nvs_workspace_bytes": ctypes.c_size_t,
            "mvsdet_fpn_dw_workspace_bytes": ctypes.c_size_t, "mvsdet_resnet_dw_s2_workspace_bytes": ctypes.c_size_t,
            "mvsdet_conv3d_k3_mfma_workspace_bytes": ctypes.c_size_t, "mvsdet_bn3d_workspace_bytes": ctypes.c_size_t}


def build(verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 every kernel into mvsdet_amd/libmvsdet_hip.so (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def load():
    """Load the HIP library; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C mvsdet_amd/csrc`). mvsdet_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = _RESTYPE.get(name, ctypes.c_int)
    _lib = lib
    return lib


def set_option(name: str, value: int):
    """Schedule-only tuning option of the library (include/mvsdet_hip.h: mvsdet_set_option)."""
    check(load().mvsdet_set_option(name.encode(), int(value)), f"set_option({name})")


def get_option(name: str) -> int:
    v = ctypes.c_int(0)
    check(load().mvsdet_get_option(name.encode(), ctypes.byref(v)), f"get_option({name})")
    return int(v.value)


def check(rc: int, what: str):
    if rc != 0:
        msg = load().mvsdet_last_error().decode("utf-8", "replace")
        kinds = {1: ValueError, 2: RuntimeError, 3: RuntimeError}
        raise kinds.get(rc, RuntimeError)(f"{what} failed (code {rc}): {msg}")


def strides(t, n=None) -> ctypes.Array:
    """HOST int64[n] with the first n element strides of a tensor (n None: all of them)."""
    values = t.stride() if n is None else t.stride()[:n]
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def strides4(t) -> ctypes.Array:
    """HOST int64[4] with the element strides of a 4-D tensor."""
    assert t.dim() == 4
    return strides(t)


def strides3(t) -> ctypes.Array:
    """HOST int64[3] with the element strides of a 3-D tensor."""
    return strides(t)


def strides4_of5(t) -> ctypes.Array:
    """HOST int64[4] with the element strides of n, c, d, h of a 5-D tensor (the kernels want w stride 1)."""
    assert t.dim() == 5
    return (ctypes.c_int64 * 4)(*t.stride()[:4])


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream(device) -> ctypes.c_void_p:
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def sweep_tile_shape(K: int, D: int, H: int, W: int):
    """(tile_w, tile_h, box_texels) the sweep uses for this problem (mvsdet_plane_sweep_tile_shape)."""
    tw, th, cap = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(load().mvsdet_plane_sweep_tile_shape(K, D, H, W, ctypes.byref(tw), ctypes.byref(th), ctypes.byref(cap)), "sweep_tile_shape")
    return tw.value, th.value, cap.value


def pixel_form_blocking(N: int, C: int, G: int, D: int, H: int, W: int, backward: bool = False):
    """(units, xcd_parts, d_per_block) of a launch of the per-pixel form under the options in force (mvsdet_pixel_form_blocking);
    G = 0: variance / compatibility warp, G > 0: group correlation with G groups."""
    u, parts, dpb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(load().mvsdet_pixel_form_blocking(N, C, G, D, H, W, int(bool(backward)), ctypes.byref(u), ctypes.byref(parts), ctypes.byref(dpb)),
          "pixel_form_blocking")
    return u.value, parts.value, dpb.value
