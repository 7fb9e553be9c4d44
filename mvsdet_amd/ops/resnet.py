"""The bottleneck layers of the 2-D backbone (csrc/resnet.hip): 1x1 and 3x3 convolutions of stride 1 or 2 with the frozen BatchNorm
as a per-channel affine, an optional residual and an optional ReLU in the epilogue.

    conv1x1: out = [relu]( (W' x[.., s y, s x] + shift) [+ residual] )
    conv3x3: out = [relu]( conv3x3(x, stride s, zero padding 1) + shift )

`W'` is the weight with the BatchNorm's `scale` folded into its rows (`fold`), split by `ops.gemm_split_weight`; `shift` is the
kernel's addend.  ReLU keeps a NaN (torch.relu's rule).  The reading of ResNet v1.5 these serve is stated in include/mvsdet_hip.h;
`mvsdet_amd.resnet.ResNetStages` chains them.

The names live in this module only (`ops.resnet.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from ._common import _lib, req, stream
from .costnet import _check_wsplit

ROW_BLOCK = 128      # matrix rows per block of both kernels: the matrix has ceil(Cout / 128) * 128 rows, those from Cout on zero
ROW_TILE = 32        # a wave's rows: Cout % 32 == 0
K_STEP = 32          # input channels per K step (Cin % 32 == 0)
CONV3X3_TILE = (8, 16)      # rows x columns of OUTPUT pixels of the stride-1 3x3 kernel's tile (csrc/resnet.hip: RnTile<1>)
CONV3X3_S2_TILE = (4, 16)   # the stride-2 kernel's (RnTile<2>): a 9 x 33 halo of input pixels
STRIDES = (1, 2)


def ceil128(cout: int) -> int:
    return -(-int(cout) // ROW_BLOCK) * ROW_BLOCK


def out_size(h: int, stride: int) -> int:
    """The output size of a strided layer: the 1x1 without padding and the 3x3 with padding 1 agree on it."""
    return (int(h) - 1) // int(stride) + 1


def fold(weight: Tensor, scale: Tensor) -> Tensor:
    """(Cout,Cin,k,k), k = 1 or 3, and the BatchNorm's scale (Cout) -> the (ceil128(Cout), k k Cin) fp32 matrix of the GEMM: the rows
    times `scale`, tap-major for a 3x3 (column Cin (3 dy + dx) + c), zero rows appended."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or int(weight.shape[2]) not in (1, 3) or tuple(scale.shape) != (weight.shape[0],):
        raise ValueError(f"resnet.fold: weight {tuple(weight.shape)} must be (Cout,Cin,1,1) or (Cout,Cin,3,3) and scale {tuple(scale.shape)} (Cout,)")
    cout = int(weight.shape[0])
    return torch.nn.functional.pad((weight.detach() * scale.detach().view(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(cout, -1),
                                   (0, 0, 0, ceil128(cout) - cout)).contiguous()


def check_shapes(x: Tensor, cin_taps: int, cout: int, shift: Tensor, stride: int = 1, residual: Optional[Tensor] = None,
                 taps: int = 1) -> Tuple[int, int, int, int]:
    """Every refusal of one layer that needs no device: ValueError / TypeError -> (N, Cin, Ho, Wo).  `cin_taps` = the matrix's
    columns (Cin for the 1x1, 9 Cin for the 3x3, `taps` = 1 | 9).  Runs before anything is launched and before the tensors' devices
    are looked at."""
    name = "resnet.conv3x3" if taps == 9 else "resnet.conv1x1"
    if taps not in (1, 9):
        raise ValueError(f"resnet: taps = {taps} must be 1 or 9")
    if stride not in STRIDES:
        raise ValueError(f"{name}: stride = {stride} must be one of {STRIDES}")
    if not isinstance(x, Tensor) or x.dim() != 4:
        raise ValueError(f"{name}: x must be an (N,C,H,W) tensor")
    for t, what in ((x, "x"), (shift, "shift"), (residual, "residual")):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{name}: {what} must be torch.float32 (got {t.dtype})")
    N, cin, H, W = (int(v) for v in x.shape)
    if N < 1 or H < 1 or W < 1:
        raise ValueError(f"{name}: x {tuple(x.shape)} is empty")
    if cin < 1 or cin % K_STEP:
        raise ValueError(f"{name}: Cin = {cin} input channels are not divisible by {K_STEP}")
    if cout < 1 or cout % ROW_TILE:
        raise ValueError(f"{name}: Cout = {cout} output channels are not divisible by {ROW_TILE}")
    if cin_taps != taps * cin:
        raise ValueError(f"{name}: the matrix has {cin_taps} columns, x has {cin} channels ({taps * cin} wanted)")
    if tuple(shift.shape) != (cout,):
        raise ValueError(f"{name}: shift {tuple(shift.shape)} must be ({cout},)")
    ho, wo = out_size(H, stride), out_size(W, stride)
    if residual is not None:
        if taps == 9:
            raise ValueError("resnet.conv3x3: takes no residual")
        if tuple(residual.shape) != (N, cout, ho, wo):
            raise ValueError(f"{name}: residual {tuple(residual.shape)} must be {(N, cout, ho, wo)}")
    if taps == 9 and N > 65535:
        raise ValueError(f"{name}: {N} views (at most 65535)")
    if H * W >= 2 ** 31 - 1:
        raise ValueError(f"{name}: map {H} x {W} too large")
    if N * ho * wo >= 2 ** 31 - 64:
        raise ValueError(f"{name}: N Ho Wo = {N * ho * wo} output pixels exceed 2^31")
    return N, cin, ho, wo


def conv1x1(x: Tensor, wsplit: Tensor, shift: Tensor, cout: int, stride: int = 1, residual: Optional[Tensor] = None,
            relu: bool = True) -> Tensor:
    """x (N,Cin,H,W), wsplit = gemm_split_weight(fold(weight, scale)), shift (Cout) -> (N,Cout,Ho,Wo).  One launch."""
    cout = int(cout)
    N, cin, ho, wo = check_shapes(x, int(x.shape[1]) if isinstance(x, Tensor) and x.dim() == 4 else 0, cout, shift, stride, residual, 1)
    req(x, "x", dim=4)
    req(shift, "shift", dim=1)
    if residual is not None:
        req(residual, "residual", dim=4)
        residual = residual.contiguous()
    _check_wsplit("resnet.conv1x1", wsplit, ceil128(cout), cin, x)
    x = x.contiguous()
    out = torch.empty((N, cout, ho, wo), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_resnet_conv1x1_bf16x3(_lib.ptr(x), _lib.ptr(wsplit), _lib.ptr(shift.contiguous()), _lib.ptr(residual),
                                                            _lib.ptr(out), N, cin, cout, int(x.shape[2]), int(x.shape[3]), int(stride),
                                                            int(bool(relu)), stream(x)), "resnet.conv1x1")
    return out


def conv3x3(x: Tensor, wsplit: Tensor, shift: Tensor, cout: int, stride: int = 1, relu: bool = True) -> Tensor:
    """x (N,Cin,H,W), wsplit = gemm_split_weight(fold(weight, scale)) of the (Cout,Cin,3,3) weight, shift (Cout) -> (N,Cout,Ho,Wo),
    zero padding 1.  One launch."""
    cout = int(cout)
    N, cin, ho, wo = check_shapes(x, 9 * int(x.shape[1]) if isinstance(x, Tensor) and x.dim() == 4 else 0, cout, shift, stride, None, 9)
    req(x, "x", dim=4)
    req(shift, "shift", dim=1)
    _check_wsplit("resnet.conv3x3", wsplit, ceil128(cout), 9 * cin, x)
    x = x.contiguous()
    out = torch.empty((N, cout, ho, wo), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_resnet_conv3x3_bf16x3(_lib.ptr(x), _lib.ptr(wsplit), _lib.ptr(shift.contiguous()), _lib.ptr(out), N, cin,
                                                            cout, int(x.shape[2]), int(x.shape[3]), int(stride), int(bool(relu)), stream(x)),
                   "resnet.conv3x3")
    return out
