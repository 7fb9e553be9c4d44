"""Level 0 of the 2-D feature pyramid in front of the sweep (csrc/fpn.hip): the four lateral 1x1 convolutions with the top-down
nearest-neighbour sum in their epilogue and the one live 3x3 output convolution, which can write the packed maps the sweep reads.

The module is mmdet.models.necks.FPN as shipped (in_channels=[256,512,1024,2048], out_channels=256, num_outs=4, start_level=0, no
add_extra_convs, no norm, no activation, upsample_cfg=dict(mode='nearest')); mmdet is not part of this tree, the reading of it is
stated in include/mvsdet_hip.h.  Forward only: gradients stay on torch (`mvsdet_amd.fpn.FPNLevel0`'s torch route).

The names live in this module only (`ops.fpn.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ._common import _lib, req, stream
from .costnet import _check_wsplit

ROW_BLOCK = 128      # output channels per block of both kernels (mvsdet_gemm_split_weight's M % 128 == 0)
K_STEP = 32          # input channels per K step (K % 32 == 0)
CONV3X3_TILE = (8, 16)   # rows x columns of the 3x3 kernel's pixel tile (csrc/fpn.hip: kFcTH, kFcTW)


def check_shapes(stages: Sequence[Tensor], lateral_weights: Sequence[Tensor], lateral_biases: Sequence[Tensor], out_weight: Tensor,
                 out_bias: Tensor) -> Tuple[int, int]:
    """Every refusal of level 0 that needs no device: ValueError / TypeError -> (N, Cout).  `stages` = the backbone maps, finest
    first; lateral_weights[i] (Cout, C_i, 1, 1) or (Cout, C_i); out_weight (Cout, Cout, 3, 3).  Runs before anything is launched (and
    before the tensors' devices are looked at, so it can be exercised without a GPU)."""
    n_levels = len(lateral_weights)
    if len(stages) != n_levels or len(lateral_biases) != n_levels:
        raise ValueError(f"fpn: {len(stages)} stages for {n_levels} lateral convolutions ({len(lateral_biases)} biases)")
    if n_levels < 1:
        raise ValueError("fpn: no levels")
    for i, s in enumerate(stages):
        if not isinstance(s, Tensor) or s.dim() != 4:
            raise ValueError(f"fpn: stage {i} must be an (N,C,H,W) tensor")
        if s.dtype != torch.float32:
            raise TypeError(f"fpn: stage {i} must be torch.float32 (got {s.dtype})")
    N = stages[0].shape[0]
    if tuple(out_weight.shape[2:]) != (3, 3) or out_weight.dim() != 4 or out_weight.shape[0] != out_weight.shape[1]:
        raise ValueError(f"fpn: the output convolution's weight {tuple(out_weight.shape)} must be (Cout,Cout,3,3)")
    cout = int(out_weight.shape[0])
    if cout % ROW_BLOCK:
        raise ValueError(f"fpn: Cout = {cout} output channels are not divisible by {ROW_BLOCK}")
    if tuple(out_bias.shape) != (cout,):
        raise ValueError(f"fpn: the output convolution's bias {tuple(out_bias.shape)} must be ({cout},)")
    for i, (s, w, b) in enumerate(zip(stages, lateral_weights, lateral_biases)):
        if s.shape[0] != N:
            raise ValueError(f"fpn: stage {i} has batch size {s.shape[0]}, stage 0 has {N}")
        c, h, wd = int(s.shape[1]), int(s.shape[2]), int(s.shape[3])
        if N < 1 or h < 1 or wd < 1:
            raise ValueError(f"fpn: stage {i} {tuple(s.shape)} is empty")
        if c % K_STEP:
            raise ValueError(f"fpn: stage {i} has {c} channels, not divisible by {K_STEP}")
        if tuple(w.shape) not in ((cout, c, 1, 1), (cout, c)):
            raise ValueError(f"fpn: lateral weight {i} {tuple(w.shape)} must be ({cout},{c},1,1)")
        if tuple(b.shape) != (cout,):
            raise ValueError(f"fpn: lateral bias {i} {tuple(b.shape)} must be ({cout},)")
        if i > 0 and (h > stages[i - 1].shape[2] or wd > stages[i - 1].shape[3]):
            raise ValueError(f"fpn: top level {i} ({h} x {wd}) is larger than the level below it "
                             f"({stages[i - 1].shape[2]} x {stages[i - 1].shape[3]})")
        if N * h * wd >= 2 ** 31 - 64:
            raise ValueError(f"fpn: stage {i}: N H W = {N * h * wd} columns exceed 2^31")
    if N > 65535:
        raise ValueError(f"fpn: {N} views (at most 65535)")
    return N, cout


def conv3x3_matrix(weight: Tensor) -> Tensor:
    """(Cout,Cin,3,3) -> the (Cout, 9 Cin) tap-major matrix of the implicit GEMM: column k = Cin (3 dy + dx) + c."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"conv3x3_matrix: weight {tuple(weight.shape)} must be (Cout,Cin,3,3)")
    return weight.detach().permute(0, 2, 3, 1).reshape(weight.shape[0], 9 * weight.shape[1]).contiguous()


def lateral(x: Tensor, wsplit: Tensor, bias: Tensor, top: Optional[Tensor] = None) -> Tensor:
    """x (N,Cin,H,W), wsplit = gemm_split_weight of the (Cout,Cin) matrix, bias (Cout), top (N,Cout,Ht,Wt) or None ->
    W x + bias [+ F.interpolate(top, size=(H,W), mode='nearest')] as (N,Cout,H,W).  One launch."""
    req(x, "x", dim=4)
    req(bias, "bias", dim=1)
    N, Cin, H, W = x.shape
    cout = int(bias.numel())
    Ht = Wt = 0
    if top is not None:
        req(top, "top", dim=4)
        if tuple(top.shape[:2]) != (N, cout) or not (1 <= top.shape[2] <= H and 1 <= top.shape[3] <= W):
            raise ValueError(f"fpn.lateral: top {tuple(top.shape)} must be ({N},{cout},Ht,Wt) with Ht <= {H}, Wt <= {W}")
        top = top.contiguous()
        Ht, Wt = int(top.shape[2]), int(top.shape[3])
    if Cin % K_STEP or cout % ROW_BLOCK:
        raise ValueError(f"fpn.lateral: Cin = {Cin} must be divisible by {K_STEP} and Cout = {cout} by {ROW_BLOCK}")
    _check_wsplit("fpn.lateral", wsplit, cout, Cin, x)
    x = x.contiguous()
    out = torch.empty((N, cout, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_fpn_lateral_bf16x3(_lib.ptr(x), _lib.ptr(wsplit), _lib.ptr(bias.contiguous()), _lib.ptr(top), _lib.ptr(out),
                                                         N, Cin, cout, H, W, Ht, Wt, stream(x)), "fpn.lateral")
    return out


def conv3x3(x: Tensor, wsplit: Tensor, bias: Tensor, want_nchw: bool = True, want_packed: bool = False):
    """x (N,Cin,H,W), wsplit = gemm_split_weight(conv3x3_matrix(weight)), bias (Cout) -> conv3x3(x) + bias (zero padding 1) as the
    (N,Cout,H,W) tensor, as the packed maps `ops.pack_features` would make of it (flat float32), or as the pair (nchw, packed).  One
    launch."""
    req(x, "x", dim=4)
    req(bias, "bias", dim=1)
    if not (want_nchw or want_packed):
        raise ValueError("fpn.conv3x3: at least one of want_nchw and want_packed")
    N, Cin, H, W = x.shape
    cout = int(bias.numel())
    if Cin % K_STEP or cout % ROW_BLOCK:
        raise ValueError(f"fpn.conv3x3: Cin = {Cin} must be divisible by {K_STEP} and Cout = {cout} by {ROW_BLOCK}")
    _check_wsplit("fpn.conv3x3", wsplit, cout, 9 * Cin, x)
    x = x.contiguous()
    lib = _lib.load()
    out = torch.empty((N, cout, H, W), dtype=torch.float32, device=x.device) if want_nchw else None
    packed = torch.empty(lib.mvsdet_packed_bytes(N, cout, H, W) // 4, dtype=torch.float32, device=x.device) if want_packed else None
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_fpn_conv3x3_bf16x3(_lib.ptr(x), _lib.ptr(wsplit), _lib.ptr(bias.contiguous()), _lib.ptr(out), _lib.ptr(packed), N,
                                                 Cin, cout, H, W, stream(x)), "fpn.conv3x3")
    if want_nchw and want_packed:
        return out, packed
    return out if want_nchw else packed
