"""Level 0 of the 2-D feature pyramid in front of the sweep (csrc/fpn.hip): the four lateral 1x1 convolutions with the top-down
nearest-neighbour sum in their epilogue and the one live 3x3 output convolution, which can write the packed maps the sweep reads.

The module is mmdet.models.necks.FPN as shipped (in_channels=[256,512,1024,2048], out_channels=256, num_outs=4, start_level=0, no
add_extra_convs, no norm, no activation, upsample_cfg=dict(mode='nearest')); mmdet is not part of this tree, the reading of it is
stated in include/mvsdet_hip.h.  The gradients (csrc/fpn_bwd.hip) are here as well: `weight_grad` (one bf16x3 kernel for the 1x1 and the
3x3 form, the pixels as the reduction, split K summed in a fixed order), `bias_grad`, `top_down_grad` (the adjoint of the nearest
gather) and the two input gradients, which are the forward kernels on transposed weights.  `mvsdet_amd.fpn.FPNLevel0` chains them
under autograd where its `autograd_route` is "hip".

The names live in this module only (`ops.fpn.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ._common import _lib, req, stream
from .costnet import _check_wsplit, gemm_split_weight

ROW_BLOCK = 128      # output channels per block of both kernels (mvsdet_gemm_split_weight's M % 128 == 0)
K_STEP = 32          # input channels per K step (K % 32 == 0)
CONV3X3_TILE = (8, 16)   # rows x columns of the 3x3 kernel's pixel tile (csrc/fpn.hip: kFcTH, kFcTW)
DW_TILE = (2, 16)        # rows x columns of the weight gradient's pixel tile (csrc/fpn_bwd.hip: kDwTH, kDwTW); one tap: 32 consecutive pixels
DW_COL_BLOCK = 32        # input channels per block of the weight gradient (kDwBC): its channel rule is C % 32 == 0
DW_SPLIT_BLOCKS = 512    # the weight gradient splits K until about this many blocks run (kDwSplitBlocks)


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


# --------------------------------------------------------------------------------------------------------- gradients
def weight_grad_plan(taps: int, N: int, C: int, cout: int, H: int, W: int) -> Tuple[int, int, int]:
    """(tiles, tiles per split, splits) of `weight_grad`, restated from csrc/fpn_bwd.hip's dw_plan (the kernel's own answer is
    `mvsdet_fpn_dw_splits`; tests/test_fpn_grad_host.py pins the two to each other).  Pure arithmetic."""
    th, tw = DW_TILE
    per_view = -(-W // tw) * -(-H // th) if taps == 9 else -(-(H * W) // (th * tw))
    tiles = N * per_view
    want = max(1, min(-(-DW_SPLIT_BLOCKS // ((C // DW_COL_BLOCK) * (cout // ROW_BLOCK))), tiles, 65535))
    per_split = -(-tiles // want)
    return tiles, per_split, -(-tiles // per_split)


def check_grad_shapes(stages: Sequence[Tensor], lateral_weights: Sequence[Tensor], lateral_biases: Sequence[Tensor], out_weight: Tensor,
                      out_bias: Tensor) -> Tuple[int, int]:
    """`check_shapes` plus what the HIP autograd route adds: a stage's input gradient is the lateral GEMM on W_i^T, whose ROWS are the
    stage's channels, so C_i % 128 == 0.  ValueError / TypeError before any device is looked at -> (N, Cout)."""
    N, cout = check_shapes(stages, lateral_weights, lateral_biases, out_weight, out_bias)
    for i, s in enumerate(stages):
        if int(s.shape[1]) % ROW_BLOCK:
            raise ValueError(f"fpn (autograd_route='hip'): stage {i} has {int(s.shape[1])} channels, not divisible by {ROW_BLOCK} "
                             f"(its input gradient is a GEMM whose rows are the stage's channels)")
    for t in list(lateral_weights) + list(lateral_biases) + [out_weight, out_bias]:
        if t.dtype != torch.float32:
            raise TypeError(f"fpn (autograd_route='hip'): parameters must be torch.float32 (got {t.dtype})")
    return N, cout


def weight_grad(gy: Tensor, x: Tensor, taps: int) -> Tensor:
    """gy (N,Cout,H,W), x (N,C,H,W) -> the weight gradient of the 1x1 (taps = 1) or the 3x3 padding-1 (taps = 9) convolution
    y = conv(x, w): dW (Cout,C,1,1) or (Cout,C,3,3).  bf16x3, split K through a workspace, the splits added in ascending order: the same
    bits on every run.  C % 32 == 0, Cout % 128 == 0.  Two launches."""
    if taps not in (1, 9):
        raise ValueError(f"fpn.weight_grad: taps = {taps} must be 1 or 9")
    if gy.dim() != 4 or x.dim() != 4:
        raise ValueError("fpn.weight_grad: gy and x must be (N,C,H,W) tensors")
    N, cout, H, W = gy.shape
    C = int(x.shape[1])
    if (x.shape[0], x.shape[2], x.shape[3]) != (N, H, W):
        raise ValueError(f"fpn.weight_grad: x {tuple(x.shape)} and gy {tuple(gy.shape)} must share N, H and W")
    if C % DW_COL_BLOCK or cout % ROW_BLOCK:
        raise ValueError(f"fpn.weight_grad: C = {C} must be divisible by {DW_COL_BLOCK} and Cout = {cout} by {ROW_BLOCK}")
    req(gy, "gy", dim=4)
    req(x, "x", dim=4)
    if x.device != gy.device:
        raise ValueError("fpn.weight_grad: gy and x must live on one device")
    lib = _lib.load()
    nbytes = lib.mvsdet_fpn_dw_workspace_bytes(taps, N, C, cout, H, W)
    if nbytes == 0:
        raise ValueError("fpn.weight_grad: " + lib.mvsdet_last_error().decode())
    k = 3 if taps == 9 else 1
    gy, x = gy.contiguous(), x.contiguous()
    dw = torch.empty((cout, C, k, k), dtype=torch.float32, device=x.device)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_fpn_dw_bf16x3(_lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(ws), nbytes, taps, N, C, cout, H, W, stream(x)),
                   "fpn.weight_grad")
    return dw


def bias_grad(g: Tensor) -> Tensor:
    """g (N,C,H,W) -> (C): the sum over views and pixels, in a fixed order.  One launch."""
    req(g, "g", dim=4)
    N, C, H, W = g.shape
    g = g.contiguous()
    db = torch.empty((C,), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _lib.check(_lib.load().mvsdet_fpn_bias_grad_f32(_lib.ptr(g), _lib.ptr(db), N, C, H, W, stream(g)), "fpn.bias_grad")
    return db


def top_down_grad(g: Tensor, size: Sequence[int]) -> Tensor:
    """g (N,C,H,W), size = (Ht, Wt) of the level above -> (N,C,Ht,Wt): the adjoint of F.interpolate(top, size=(H,W), mode='nearest'),
    every element the sum of its pre-image, rows ascending, then columns ascending.  One launch."""
    if g.dim() != 4:
        raise ValueError("fpn.top_down_grad: g must be an (N,C,H,W) tensor")
    N, C, H, W = g.shape
    Ht, Wt = int(size[0]), int(size[1])
    if not (1 <= Ht <= H and 1 <= Wt <= W):
        raise ValueError(f"fpn.top_down_grad: size {(Ht, Wt)} must lie within 1 x 1 .. {H} x {W}")
    req(g, "g", dim=4)
    g = g.contiguous()
    gt = torch.empty((N, C, Ht, Wt), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _lib.check(_lib.load().mvsdet_fpn_top_down_grad_f32(_lib.ptr(g), _lib.ptr(gt), N, C, H, W, Ht, Wt, stream(g)), "fpn.top_down_grad")
    return gt


def lateral_input_grad(g: Tensor, weight: Tensor) -> Tensor:
    """g (N,Cout,H,W), weight (Cout,C[,1,1]) of the lateral -> dx (N,C,H,W) = W^T g: the lateral kernel on the split of W^T with a zero
    bias and no top (C % 128 == 0, Cout % 32 == 0).  The pieces are cut per call."""
    cout, C = int(weight.shape[0]), int(weight.shape[1])
    if g.dim() != 4 or weight.dim() not in (2, 4) or weight.numel() != cout * C or g.shape[1] != cout:
        raise ValueError(f"fpn.lateral_input_grad: weight {tuple(weight.shape)} must be ({int(g.shape[1])},C,1,1)")
    if C % ROW_BLOCK or cout % K_STEP:
        raise ValueError(f"fpn.lateral_input_grad: C = {C} must be divisible by {ROW_BLOCK} and Cout = {cout} by {K_STEP}")
    req(g, "g", dim=4)
    wt = weight.detach().reshape(cout, C).t().contiguous()
    return lateral(g, gemm_split_weight(wt), torch.zeros(C, dtype=torch.float32, device=g.device))


def conv3x3_input_grad(g: Tensor, weight: Tensor) -> Tensor:
    """g (N,Cout,H,W), weight (Cout,C,3,3) -> dx (N,C,H,W) = conv3x3(g, w'), w'[c,o,dy,dx] = w[o,c,2-dy,2-dx], padding 1: the 3x3 kernel
    on the flipped, transposed weight with a zero bias (C % 128 == 0, Cout % 32 == 0).  The pieces are cut per call."""
    if g.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or g.shape[1] != weight.shape[0]:
        raise ValueError(f"fpn.conv3x3_input_grad: weight {tuple(weight.shape)} must be ({int(g.shape[1])},C,3,3)")
    cout, C = int(weight.shape[0]), int(weight.shape[1])
    if C % ROW_BLOCK or cout % K_STEP:
        raise ValueError(f"fpn.conv3x3_input_grad: C = {C} must be divisible by {ROW_BLOCK} and Cout = {cout} by {K_STEP}")
    req(g, "g", dim=4)
    wt = weight.detach().flip(2, 3).transpose(0, 1)
    return conv3x3(g, gemm_split_weight(conv3x3_matrix(wt)), torch.zeros(C, dtype=torch.float32, device=g.device))
