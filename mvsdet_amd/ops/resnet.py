"""The bottleneck layers of the 2-D backbone (csrc/resnet.hip): 1x1 and 3x3 convolutions of stride 1 or 2 with the frozen BatchNorm
as a per-channel affine, an optional residual and an optional ReLU in the epilogue.

    conv1x1: out = [relu]( (W' x[.., s y, s x] + shift) [+ residual] )
    conv3x3: out = [relu]( conv3x3(x, stride s, zero padding 1) + shift )

`W'` is the weight with the BatchNorm's `scale` folded into its rows (`fold`), split by `ops.gemm_split_weight`; `shift` is the
kernel's addend.  ReLU keeps a NaN (torch.relu's rule).  The reading of ResNet v1.5 these serve is stated in include/mvsdet_hip.h;
`mvsdet_amd.resnet.ResNetStages` chains them.

The gradients (csrc/resnet_bwd.hip) are here as well, one bottleneck's chain with g = dL/dout:

    gz = relu_gate(g, out);  dW3 = scale3 (.) weight_grad(gz, b, 1, 1);  gb = conv1x1_input_grad(gz, W3, scale3, gate=b)
    dW2 = scale2 (.) weight_grad(gb, a, 9, s);  ga = conv3x3_input_grad(gb, W2, scale2, a's size, s, gate=a)
    dW1 = scale1 (.) weight_grad(ga, x, 1, 1);  dx = conv1x1_input_grad(ga, W1, scale1, residual=gz | Wd'^T gz, spread=1 | s)
    dWd = scaled (.) weight_grad(gz, x, 1, s)

`relu_gate(v, y)` = `y <= 0 ? 0 : v` on the saved OUTPUT of the ReLU (ATen's threshold_backward: +0.0 where y is 0.0, -0.0 or negative,
v where y is positive, inf or NaN); the input-gradient kernels apply it in their epilogues (`gate=`).  The additions inside dx have a
fixed order: the GEMM's accumulator, then + the residual, then the gate.  The transposed / flipped weight pieces are cut per call (the
weights move every step).  No atomics: the same bits on every run.  `mvsdet_amd.resnet.ResNetStages(autograd_route="hip")` chains them.

The names live in this module only (`ops.resnet.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ._common import _lib, req, stream
from . import fpn as _fpn
from .costnet import _check_wsplit, gemm_split_weight

ROW_BLOCK = 128      # matrix rows per block of both kernels: the matrix has ceil(Cout / 128) * 128 rows, those from Cout on zero
ROW_TILE = 32        # a wave's rows: Cout % 32 == 0
K_STEP = 32          # input channels per K step (Cin % 32 == 0)
CONV3X3_TILE = (8, 16)      # rows x columns of OUTPUT pixels of the stride-1 3x3 kernel's tile (csrc/resnet.hip: RnTile<1>)
CONV3X3_S2_TILE = (4, 16)   # the stride-2 kernel's (RnTile<2>): a 9 x 33 halo of input pixels
STRIDES = (1, 2)
DW_ROW_BLOCK = 128          # the weight gradients' channel rule: Cout % 128 == 0 (a block's output channels) ...
DW_COL_BLOCK = 32           # ... and C % 32 == 0 (its input channels), at both strides
DW_S2_TILE = (2, 16)        # rows x columns of OUTPUT pixels of the stride-2 weight gradient's tile (csrc/resnet_bwd.hip: kD2TH, kD2TW)
DW_SPLIT_BLOCKS = 512       # it splits K until about this many blocks run (kD2SplitBlocks)


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


# --------------------------------------------------------------------------------------------------------- gradients
def _folded(weight: Tensor, scale: Tensor) -> Tensor:
    """W' = the weight rows times the BatchNorm's scale: the fp32 values `fold` lays out for the forward."""
    return weight.detach() * scale.detach().view(-1, 1, 1, 1)


def _pad_rows(m: Tensor) -> Tensor:
    return torch.nn.functional.pad(m, (0, 0, 0, ceil128(m.shape[0]) - m.shape[0])).contiguous()


def transposed_matrix(weight: Tensor, scale: Tensor) -> Tensor:
    """(Cout,C,1,1) -> the (ceil128(C), Cout) fp32 matrix W'^T of the 1x1 input gradient, zero rows appended."""
    wf = _folded(weight, scale)
    return _pad_rows(wf.reshape(wf.shape[0], wf.shape[1]).t())


def flipped_matrix(weight: Tensor, scale: Tensor) -> Tensor:
    """(Cout,C,3,3) -> the (ceil128(C), 9 Cout) tap-major matrix of w'[c,o,dy,dx] = W'[o,c,2-dy,2-dx]: the stride-1 3x3 input gradient is
    the forward 3x3 on it."""
    wt = _folded(weight, scale).flip(2, 3).transpose(0, 1)
    return _pad_rows(wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1))


def parity_taps(parity: int) -> Tuple[int, ...]:
    """The taps dy that reach an input coordinate of this parity under stride 2, padding 1 (y + 1 - dy even), ascending."""
    return (0, 2) if parity else (1,)


def class_matrices(weight: Tensor, scale: Tensor) -> Sequence[Tensor]:
    """(Cout,C,3,3) -> the four (ceil128(C), taps Cout) matrices of the stride-2 3x3 input gradient, classes (py, px) = (0,0), (0,1),
    (1,0), (1,1): column (tap index) Cout + o holds W'[o,c,dy,dx], the class's taps ordered dy ascending, then dx ascending."""
    wf = _folded(weight, scale)
    out = []
    for py in (0, 1):
        for px in (0, 1):
            cols = [wf[:, :, dy, dx].t() for dy in parity_taps(py) for dx in parity_taps(px)]
            out.append(_pad_rows(torch.cat(cols, dim=1)))
    return out


def weight_grad_plan(taps: int, N: int, C: int, cout: int, H: int, W: int) -> Tuple[int, int, int]:
    """(tiles, tiles per split, splits) of the stride-2 `weight_grad` on an (H, W) input, restated from csrc/resnet_bwd.hip's dw2_plan (the
    kernel's own answer is `mvsdet_resnet_dw_s2_splits`).  Pure arithmetic."""
    th, tw = DW_S2_TILE
    tiles = N * -(-out_size(W, 2) // tw) * -(-out_size(H, 2) // th)
    want = max(1, min(-(-DW_SPLIT_BLOCKS // ((C // DW_COL_BLOCK) * (cout // DW_ROW_BLOCK))), tiles, 65535))
    per_split = -(-tiles // want)
    return tiles, per_split, -(-tiles // per_split)


def check_grad_shapes(x: Tensor, w1: Tensor, w2: Tensor, w3: Tensor, wd: Optional[Tensor] = None, stride: int = 1,
                      weight_grads: Sequence[bool] = (True, True, True, True)) -> Tuple[int, int, int]:
    """Every refusal of one bottleneck's backward that needs no device: ValueError / TypeError -> (N, Ho, Wo).  x (N,C,H,W) = the block's
    input; w1 (p,C,1,1), w2 (p,p,3,3), w3 (Cout,p,1,1), wd (Cout,C,1,1) or None = its weights; weight_grads = which of (w1, w2, w3, wd)
    get a gradient.  The input gradients take any channel counts divisible by 32; a weight gradient needs Cout % 128 == 0 and
    C % 32 == 0 of its own layer."""
    name = "resnet (autograd_route='hip')"
    if stride not in STRIDES:
        raise ValueError(f"{name}: stride = {stride} must be one of {STRIDES}")
    if not isinstance(x, Tensor) or x.dim() != 4:
        raise ValueError(f"{name}: x must be an (N,C,H,W) tensor")
    for t, what in ((x, "x"), (w1, "conv1's weight"), (w2, "conv2's weight"), (w3, "conv3's weight"), (wd, "the downsample weight")):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{name}: {what} must be torch.float32 (got {t.dtype})")
    N, cin, H, W = (int(v) for v in x.shape)
    if N < 1 or cin < 1 or H < 1 or W < 1:
        raise ValueError(f"{name}: x {tuple(x.shape)} is empty")
    p, cout = int(w1.shape[0]), int(w3.shape[0])
    if tuple(w1.shape) != (p, cin, 1, 1) or tuple(w2.shape) != (p, p, 3, 3) or tuple(w3.shape) != (cout, p, 1, 1) or p < 1 or cout < 1:
        raise ValueError(f"{name}: weights {tuple(w1.shape)}, {tuple(w2.shape)}, {tuple(w3.shape)} are not a bottleneck on {cin} channels")
    if wd is None:
        if stride != 1 or cin != cout:
            raise ValueError(f"{name}: a block without a downsample branch keeps the map ({cin} -> {cout} channels, stride {stride})")
    elif tuple(wd.shape) != (cout, cin, 1, 1):
        raise ValueError(f"{name}: the downsample weight {tuple(wd.shape)} must be {(cout, cin, 1, 1)}")
    for c in (cin, p, cout):
        if c % K_STEP:
            raise ValueError(f"{name}: {c} channels are not divisible by {K_STEP}")
    layers = (("conv1", p, cin), ("conv2", p, p), ("conv3", cout, p), ("downsample", cout, cin))
    for want, (what, o, c) in zip(weight_grads, layers):
        if want and (what != "downsample" or wd is not None) and (o % DW_ROW_BLOCK or c % DW_COL_BLOCK):
            raise ValueError(f"{name}: {what}'s weight gradient needs Cout = {o} divisible by {DW_ROW_BLOCK} and C = {c} by {DW_COL_BLOCK}")
    if N > 65535:
        raise ValueError(f"{name}: {N} views (at most 65535)")
    ho, wo = out_size(H, stride), out_size(W, stride)
    if H * W >= 2 ** 31 - 1:
        raise ValueError(f"{name}: map {H} x {W} too large")
    if N * H * W >= 2 ** 31 - 64:
        raise ValueError(f"{name}: N H W = {N * H * W} pixels exceed 2^31")
    return N, ho, wo


def relu_gate(g: Tensor, y: Tensor) -> Tensor:
    """g and y = the ReLU's saved OUTPUT, of one shape -> `y <= 0 ? 0 : g` (torch.relu's gradient rule).  One launch."""
    req(g, "g")
    req(y, "y")
    if g.shape != y.shape or g.device != y.device or g.numel() < 1:
        raise ValueError(f"resnet.relu_gate: g {tuple(g.shape)} and y {tuple(y.shape)} must share one non-empty shape and device")
    g, y = g.contiguous(), y.contiguous()
    out = torch.empty_like(g)
    with torch.cuda.device(g.device):
        _lib.check(_lib.load().mvsdet_resnet_relu_gate_f32(_lib.ptr(g), _lib.ptr(y), _lib.ptr(out), g.numel(), stream(g)), "resnet.relu_gate")
    return out


def _grad_operands(name: str, g: Tensor, weight: Tensor, scale: Tensor, k: int) -> Tuple[int, int]:
    if not isinstance(g, Tensor) or g.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (k, k) or g.shape[1] != weight.shape[0]:
        raise ValueError(f"{name}: weight {tuple(weight.shape)} must be ({int(g.shape[1]) if isinstance(g, Tensor) and g.dim() == 4 else '?'},C,{k},{k})")
    cout, C = int(weight.shape[0]), int(weight.shape[1])
    if tuple(scale.shape) != (cout,):
        raise ValueError(f"{name}: scale {tuple(scale.shape)} must be ({cout},)")
    if C % ROW_TILE or cout % K_STEP:
        raise ValueError(f"{name}: C = {C} must be divisible by {ROW_TILE} and Cout = {cout} by {K_STEP}")
    req(g, "g", dim=4)
    req(weight, "weight", dim=4)
    req(scale, "scale", dim=1)
    return cout, C


def conv1x1_input_grad(g: Tensor, weight: Tensor, scale: Tensor, gate: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                       spread: int = 1) -> Tensor:
    """g (N,Cout,H,W), weight (Cout,C,1,1), scale (Cout) -> (N,C,H,W) = gate( (W'^T g) [+ residual], gate ).  residual: (N,C,H,W) with
    spread = 1, or the half-resolution (N,C,(H-1)//2+1,(W-1)//2+1) map with spread = 2, added at (y // 2, x // 2) where y and x are both
    even.  gate = the gate map (N,C,H,W) or None.  One launch behind the cut of W'^T."""
    cout, C = _grad_operands("resnet.conv1x1_input_grad", g, weight, scale, 1)
    if spread not in STRIDES:
        raise ValueError(f"resnet.conv1x1_input_grad: spread = {spread} must be one of {STRIDES}")
    N, _, H, W = (int(v) for v in g.shape)
    if gate is not None:
        req(gate, "gate", dim=4)
        if tuple(gate.shape) != (N, C, H, W):
            raise ValueError(f"resnet.conv1x1_input_grad: gate {tuple(gate.shape)} must be {(N, C, H, W)}")
        gate = gate.contiguous()
    if residual is not None:
        req(residual, "residual", dim=4)
        want = (N, C, out_size(H, spread), out_size(W, spread))
        if tuple(residual.shape) != want:
            raise ValueError(f"resnet.conv1x1_input_grad: residual {tuple(residual.shape)} must be {want}")
        residual = residual.contiguous()
    g = g.contiguous()
    wq = gemm_split_weight(transposed_matrix(weight, scale))
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _lib.check(_lib.load().mvsdet_resnet_conv1x1_dx_bf16x3(_lib.ptr(g), _lib.ptr(wq), _lib.ptr(residual), _lib.ptr(gate), _lib.ptr(out), N, C,
                                                               cout, H, W, int(spread), stream(g)), "resnet.conv1x1_input_grad")
    return out


def conv3x3_input_grad(g: Tensor, weight: Tensor, scale: Tensor, size: Sequence[int], stride: int = 1, gate: Optional[Tensor] = None) -> Tensor:
    """g (N,Cout,Ho,Wo), weight (Cout,C,3,3), scale (Cout), size = (H, W) of the convolution's input -> (N,C,H,W) = gate( convT3x3_s(g; W'),
    gate ).  Stride 1: the forward 3x3 on the flipped, transposed weight, one launch.  Stride 2: one GEMM per parity class of the input
    pixels over that class's 1, 2, 2 or 4 taps (no inserted zeros are multiplied), four launches."""
    cout, C = _grad_operands("resnet.conv3x3_input_grad", g, weight, scale, 3)
    if stride not in STRIDES:
        raise ValueError(f"resnet.conv3x3_input_grad: stride = {stride} must be one of {STRIDES}")
    N, H, W = int(g.shape[0]), int(size[0]), int(size[1])
    if H < 1 or W < 1 or (int(g.shape[2]), int(g.shape[3])) != (out_size(H, stride), out_size(W, stride)):
        raise ValueError(f"resnet.conv3x3_input_grad: g {tuple(g.shape)} is not the stride-{stride} output of an {H} x {W} map")
    if gate is not None:
        req(gate, "gate", dim=4)
        if tuple(gate.shape) != (N, C, H, W):
            raise ValueError(f"resnet.conv3x3_input_grad: gate {tuple(gate.shape)} must be {(N, C, H, W)}")
        gate = gate.contiguous()
    g = g.contiguous()
    if stride == 1:
        wq = gemm_split_weight(flipped_matrix(weight, scale))
    else:
        wq = torch.cat([gemm_split_weight(m) for m in class_matrices(weight, scale)])
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _lib.check(_lib.load().mvsdet_resnet_conv3x3_dx_bf16x3(_lib.ptr(g), _lib.ptr(wq), _lib.ptr(gate), _lib.ptr(out), N, C, cout, H, W,
                                                               int(stride), stream(g)), "resnet.conv3x3_input_grad")
    return out


def weight_grad(gy: Tensor, x: Tensor, taps: int, stride: int = 1) -> Tensor:
    """gy (N,Cout,Ho,Wo), x (N,C,H,W) -> the weight gradient of the 1x1 (taps = 1) or the 3x3 padding-1 (taps = 9) convolution of this
    stride: dW (Cout,C,1,1) or (Cout,C,3,3), dW[o,c,dy,dx] = sum gy[n,o,yo,xo] x[n,c,s yo+dy-1,s xo+dx-1].  Stride 1 is `ops.fpn.weight_grad`;
    stride 2 its own kernel of the same contract: bf16x3, split K through a workspace, the splits added in ascending order.
    C % 32 == 0, Cout % 128 == 0.  Two launches."""
    if stride not in STRIDES:
        raise ValueError(f"resnet.weight_grad: stride = {stride} must be one of {STRIDES}")
    if stride == 1:
        return _fpn.weight_grad(gy, x, taps)
    if taps not in (1, 9):
        raise ValueError(f"resnet.weight_grad: taps = {taps} must be 1 or 9")
    if not isinstance(gy, Tensor) or not isinstance(x, Tensor) or gy.dim() != 4 or x.dim() != 4:
        raise ValueError("resnet.weight_grad: gy and x must be (N,C,H,W) tensors")
    N, cout = int(gy.shape[0]), int(gy.shape[1])
    C, H, W = int(x.shape[1]), int(x.shape[2]), int(x.shape[3])
    if x.shape[0] != N or H < 1 or W < 1 or (int(gy.shape[2]), int(gy.shape[3])) != (out_size(H, 2), out_size(W, 2)):
        raise ValueError(f"resnet.weight_grad: gy {tuple(gy.shape)} is not the stride-2 output of x {tuple(x.shape)}")
    if C % DW_COL_BLOCK or cout % DW_ROW_BLOCK:
        raise ValueError(f"resnet.weight_grad: C = {C} must be divisible by {DW_COL_BLOCK} and Cout = {cout} by {DW_ROW_BLOCK}")
    req(gy, "gy", dim=4)
    req(x, "x", dim=4)
    if x.device != gy.device:
        raise ValueError("resnet.weight_grad: gy and x must live on one device")
    lib = _lib.load()
    nbytes = lib.mvsdet_resnet_dw_s2_workspace_bytes(taps, N, C, cout, H, W)
    if nbytes == 0:
        raise ValueError("resnet.weight_grad: " + lib.mvsdet_last_error().decode())
    k = 3 if taps == 9 else 1
    gy, x = gy.contiguous(), x.contiguous()
    dw = torch.empty((cout, C, k, k), dtype=torch.float32, device=x.device)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_resnet_dw_s2_bf16x3(_lib.ptr(gy), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(ws), nbytes, taps, N, C, cout, H, W, stream(x)),
                   "resnet.weight_grad")
    return dw
