"""The 3-D neck that consumes the hot path's voxel volume: `IndoorImVoxelNeck` of
mmdet3d/models/necks/imvoxel_neck.py:70-231 -- a three-level 3-D FPN of residual blocks over the (C,40,40,16) volume,
~0.49 TFLOP per scene with the shipped configuration (in_channels=256, out_channels=128, n_blocks=[1,1,1]).

The module is plain PyTorch with the reference's parameter names (mmcv's ConvModule registers its layers as `conv`
and `bn`, so `down_layer_1.0.conv0.conv.weight`, `down_layer_1.0.downsample.bn.running_mean`, `up_block_2.0.weight`,
`out_block_0.1.bias` ... load from a reference checkpoint's `neck_3d.*` entries with `load_state_dict`).  In eval mode
without autograd, on a ROCm device, every 3x3x3 convolution runs on the bf16x3 MFMA kernels of csrc/costreg_bf16.hip
(three bf16 products per fp32-equivalent product, fp32 accumulation: DESIGN 4.3; `matrix_precision = "fp32"` keeps the
fp32-MFMA kernels of csrc/costreg_conv0.hip) with eval-mode BatchNorm, ReLU and the residual addition folded into the
epilogue; the small levels split their input channels until ~768 blocks run.  The 1x1x1 stride-2 shortcut and the
kernel-2 stride-2 transposed convolutions are one GEMM each on csrc/neck_gemm.hip (a kernel-2 stride-2 transposed
convolution is 8 independent single-tap classes; bias, ReLU and the 2x2x2 interleave in the epilogue; no rocBLAS call).
Training, CPU tensors and other shapes take the framework's layers -- unless `autograd_route` is "hip" (below) --, each such
layer call counted with its reason in `layers.framework_calls`.

Training on the HIP kernels (opt-in: `IndoorImVoxelNeck.autograd_route` / `NerfDetHeadConvs.autograd_route`, initial value from the
environment variable MVSDET_DETECTOR_AUTOGRAD, "aten" by default).  With "hip", a neck in training mode on CUDA fp32 tensors runs every
layer on our kernels, with autograd on or off (off: the running statistics still update): the 3x3x3 convolutions on the bf16x3
forward / input-gradient / weight-gradient kernels of the cost network (`layers.ConvK3S1`, `ConvK3S2`; BatchNorm statistics from
the convolution's epilogue where the grid is not split over input channels), the 1x1x1 stride-2 shortcut and the kernel-2 stride-2
transposed layer on csrc/neck_gemm.hip (forward, input gradient, weight gradient), BatchNorm on csrc/costreg_bn.hip -- the ResModule's
`relu(bn(conv1) + identity)` with the residual inside the ReLU.  A neck in eval mode with autograd on stays on the framework's layers
(whatever the route), as does everything with "aten".  Shapes the HIP route cannot take raise instead of falling back.
"""
from __future__ import annotations

import os
import sys
from typing import List, Sequence

import torch
from torch import Tensor, nn

from . import _lib, layers, ops
from .layers import (ConvK3S1, ConvK3S2, DerivedTensorsMixin, autograd_route_from_env, await_made, bn_affine, bn_train,
                     check_route, fp32_under_autocast, mark_made, relu_hooked)
# the names of this module's earlier layout, for code written against them; modules pickled whole store their load hook as
# neck._drop_after_load
from .layers import _drop_after_load, drop_derived_tensors  # noqa: F401
sys.modules[__name__].__class__ = layers.ForwardedToggles   # neck.RELU_MASKS sets the one in `layers`
_bn_affine = bn_affine


class _ConvModule(nn.Module):
    """mmcv.cnn.ConvModule(conv_cfg=Conv3d, norm_cfg=BN3d, act_cfg=ReLU|None) as used by imvoxel_neck.py:196-217:
    Conv3d without bias -> BatchNorm3d [-> ReLU], sub-modules named `conv` and `bn` as mmcv names them."""

    def __init__(self, cin: int, cout: int, kernel: int, stride: int = 1, padding: int = 0, act: bool = True):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, kernel, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm3d(cout)
        self.with_act = act

    def forward(self, x):
        x = self.bn(self.conv(x))
        return relu_hooked(self, x) if self.with_act else x


def _block_route(x: Tensor, block: nn.Module, conv: nn.Module) -> str:   # by the block's own `training`: it is a module of its own
    return layers.decide(layers.call_facts(x, block), conv.out_channels % 64 == 0, other=False, keyed="training")


# Stride-1 3x3x3 convolutions on volumes of at least this many voxels go to the bf16 matrix cores with three-term split
# operands (csrc/costreg_bf16.hip; outputs within ~1e-5 of the fp32 sums' scale).  The 20x20x8 and 10x10x4 levels are a
# handful of tiles (padded 1.9x): there the kernel splits the 512 / 1024 input channels over blocks and a second kernel
# adds the partial sums (neck 4.05 -> 3.10 ms).  0 disables the bf16 route.
BF16X3_MIN_VOXELS = 256
# stride-1 layers with this many output channels or more (four blocks of 64 per tile) on volumes of at least PACK_INPUT_MIN_VOXELS
# voxels (grids that are not split over the input channels) read a packed SCL copy of their input by DMA; 0 = never
PACK_INPUT_FROM_COUT = int(os.environ.get("MVSDET_NECK_PACK_COUT", "256"))
PACK_INPUT_MIN_VOXELS = 16384
# the two stride-2 layers on the bf16x3 stride-2 kernel (its 3x16x8 tiles fit their outputs: neck 2.77 -> 2.58 ms; on 4x8x16 tiles
# it lost to the fp32 kernel, 0.72 against 0.64 ms)
S2_BF16X3 = True


def _split_weight(conv: nn.Module, order: int | None = None) -> Tensor:
    """The weight cut into bf16 pieces in the bf16x3 kernel's layout (tap order of the layer's stride; `order` 2 = a
    ConvTranspose3d weight), kept on the module (the neck's weights are 300 MB: not re-split per call) until the weight tensor
    changes or `drop_derived_tensors` runs."""
    w = conv.weight
    if order is None:
        order = 1 if conv.stride[0] == 2 else 0
    key = (w.data_ptr(), w._version, w.device, order)
    cached = conv.__dict__.get("_mvs_wsplit")
    if cached is None or cached[0] != key:
        cached = (key, ops.split_conv_weight(w, order=order))
        mark_made(cached[1])
        conv.__dict__["_mvs_wsplit"] = cached
    await_made(cached[1])
    return cached[1]


def _gemm_weight(conv: nn.Module, bn: nn.BatchNorm3d, split: bool = False):
    """The 1x1x1 convolution (Cout x Cin) or the ConvTranspose3d(k=2, s=2) (8*Cout x Cin) as ONE matrix with the eval-mode
    BatchNorm's scale folded in, and the matching bias; kept on the module like the split weights (three tiny kernels per layer
    and call otherwise).  split=False: (wmat fp32 with rows (p, q, r, o), bias column (1, 8 Cout, 1)) for torch.baddbmm;
    split=True: (the bf16 pieces of the matrix with rows 8 o + 4 p + 2 q + r in the GEMM kernel's fragment order, bias (Cout,))."""
    w = conv.weight
    key = (w.data_ptr(), w._version, w.device, bool(split)) + tuple((t.data_ptr(), t._version) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    cached = conv.__dict__.get("_mvs_wmat")
    if cached is None or cached[0] != key:
        scale, shift = bn_affine(bn)
        with torch.no_grad():
            if isinstance(conv, nn.ConvTranspose3d):
                cout = conv.out_channels
                ws = w.detach() * scale.view(1, -1, 1, 1, 1)
                if split:
                    wmat, bias = ws.permute(1, 2, 3, 4, 0).reshape(8 * cout, w.shape[0]).contiguous(), shift.contiguous()
                else:
                    wmat, bias = ws.permute(2, 3, 4, 1, 0).reshape(8 * cout, w.shape[0]).contiguous(), shift.repeat(8).view(1, -1, 1).contiguous()
            else:
                wmat = (w.detach().reshape(conv.out_channels, -1) * scale[:, None]).contiguous()
                bias = shift.contiguous() if split else shift.view(1, -1, 1).contiguous()
            if split:
                wmat = ops.gemm_split_weight(wmat)
        cached = (key, wmat, bias)
        mark_made(wmat, bias)
        conv.__dict__["_mvs_wmat"] = cached
    await_made(cached[1], cached[2])
    return cached[1], cached[2]


def _conv_k3(x: Tensor, conv: nn.Conv3d, bn: nn.BatchNorm3d, relu: bool, residual: Tensor | None = None) -> Tensor:
    """Conv3d(k=3, p=1, stride 1|2) + BN(eval) [+ residual] [+ ReLU] in one MFMA kernel."""
    scale, shift = bn_affine(bn)
    if conv.stride[0] == 1 and BF16X3_MIN_VOXELS and x[0, 0].numel() >= BF16X3_MIN_VOXELS and conv.out_channels % 64 == 0:
        src = x
        if PACK_INPUT_FROM_COUT and conv.out_channels >= PACK_INPUT_FROM_COUT and x[0, 0].numel() >= PACK_INPUT_MIN_VOXELS:
            # four blocks of output channels per tile would each cut the same fp32 values into bf16 pieces: one packing pass
            # (26 MB at the 40x40x16 level) and the DMA-fed form instead; the copy is this call's own (from the caching allocator,
            # the packing kernel writes its zero border): nothing kept on the module, nothing tied to a stream
            src = ops.scl_pack(x)
        return ops.conv3d_k3_bf16x3(src, _split_weight(conv), scale, shift, relu, residual)
    if S2_BF16X3 and conv.stride[0] == 2 and residual is None and conv.out_channels % 64 == 0:
        return ops.conv3d_k3_s2_bf16x3(x, _split_weight(conv), scale, shift, relu)
    return ops.conv3d_k3_mfma(x, ops.permute_conv_weight(conv.weight), scale, shift, relu, conv.stride[0], residual)


class ResModule(nn.Module):
    """imvoxel_neck.py:183-231."""

    def __init__(self, cin: int, cout: int, stride: int = 1):
        super().__init__()
        self.conv0 = _ConvModule(cin, cout, 3, stride, 1, act=True)
        self.conv1 = _ConvModule(cout, cout, 3, 1, 1, act=False)
        if stride != 1:
            self.downsample = _ConvModule(cin, cout, 1, stride, 0, act=False)
        self.stride = stride

    def forward(self, x):
        route = layers.record(self, _block_route(x, self, self.conv0.conv), "conv0", "conv1")
        if route == "eval":
            identity = x
            if self.stride != 1:   # 1x1x1 stride-2 convolution + BN: one GEMM on the sub-sampled volume
                ds = self.downsample
                gemm = (self.stride == 2 and ops.gemm_layer_ok(ds.conv.out_channels, ds.conv.in_channels)
                        and not any(v % 2 for v in x.shape[2:]))
                if layers.record(self, "eval" if gemm else "shape", "downsample") == "eval":
                    wq, bias = _gemm_weight(ds.conv, ds.bn, split=True)      # the sub-sampling is the kernel's gather
                    identity = ops.conv3d_k1_s2_bf16x3(x, wq, bias, ds.conv.out_channels)
                else:   # a shape the GEMM kernel refuses (odd extents, channel counts outside `gemm_layer_ok`): torch.baddbmm
                    xs = x[:, :, ::self.stride, ::self.stride, ::self.stride]
                    n, c, d, h, w = xs.shape
                    wmat, bias = _gemm_weight(ds.conv, ds.bn)
                    identity = torch.baddbmm(bias, wmat.unsqueeze(0).expand(n, -1, -1), xs.reshape(n, c, -1))
                    identity = identity.view(n, -1, d, h, w)
            h0 = _conv_k3(x, self.conv0.conv, self.conv0.bn, True)
            return _conv_k3(h0, self.conv1.conv, self.conv1.bn, True, identity)   # relu(bn(conv1) + identity)
        identity = x
        x = self.conv1(self.conv0(x))
        if self.stride != 1:
            layers.record(self, route, "downsample")
            identity = self.downsample(identity)
        return relu_hooked(self, x + identity)

    def _train_hip(self, x):
        """The training step of the block on the HIP kernels (autograd_route "hip"): relu(bn1(conv1(relu(bn0(conv0 x)))) + identity),
        identity = x or bn_ds(downsample x); in the stride-2 block conv0 and the shortcut are one autograd node (`_DownS2`) whose
        input gradient is conv0's with the shortcut's accumulated into its even positions."""
        c0, c1 = self.conv0, self.conv1
        if self.stride == 1:
            identity = x
            y0, parts, pivot = _conv3_train(c0.conv, x, c0.bn)
        else:
            layers.count_hip(2)   # conv0 and the shortcut
            y0, yd = _DownS2.apply(x, c0.conv.weight, self.downsample.conv.weight)
            identity = bn_train(self.downsample.bn, yd, None)
            parts = pivot = None
        h = bn_train(c0.bn, y0, c0, parts, pivot)
        y1, parts, pivot = _conv3_train(c1.conv, h, c1.bn)
        return bn_train(c1.bn, y1, self, parts, pivot, residual=identity)


class _UpBlock(nn.Sequential):
    """imvoxel_neck.py:166-180: ConvTranspose3d(k=2, s=2) BN ReLU Conv3d(k=3) BN ReLU, Sequential indices as the reference's."""

    def __init__(self, cin: int, cout: int):
        super().__init__(nn.ConvTranspose3d(cin, cout, 2, 2, bias=False), nn.BatchNorm3d(cout), nn.ReLU(inplace=True),
                         nn.Conv3d(cout, cout, 3, 1, 1, bias=False), nn.BatchNorm3d(cout), nn.ReLU(inplace=True))

    def forward(self, x):
        route = layers.record(self, _block_route(x, self, self[3]), "3")
        if route == "eval":
            deconv, bn = self[0], self[1]
            n, cin, d, h, w = x.shape
            cout = deconv.out_channels
            # out[:, o, 2i+p, 2j+q, 2k+r] = sum_c x[:, c, i, j, k] * W[c, o, p, q, r]: one (8*Cout x Cin) GEMM with the BatchNorm's
            # shift as its bias; the ReLU writes the interleaved (N, Cout, 2D, 2H, 2W) tensor directly (one pass, no copy)
            if layers.record(self, "eval" if ops.gemm_layer_ok(8 * cout, cin) else "shape", "0") == "eval":
                wq, bias = _gemm_weight(deconv, bn, split=True)      # bias, ReLU and the 2x2x2 interleave in the GEMM's epilogue
                return _conv_k3(ops.convT3d_k2_s2_bf16x3(x, wq, bias, cout, True), self[3], self[4], True)
            # channel counts the GEMM kernel refuses (`gemm_layer_ok` false): torch.baddbmm, then the ReLU interleaves
            wmat, bias = _gemm_weight(deconv, bn)
            y = torch.baddbmm(bias, wmat.unsqueeze(0).expand(n, -1, -1), x.reshape(n, cin, -1)).view(n, 2, 2, 2, cout, d, h, w)
            out = torch.empty((n, cout, 2 * d, 2 * h, 2 * w), dtype=x.dtype, device=x.device)
            torch.clamp_min(y.permute(0, 4, 5, 1, 6, 2, 7, 3), 0.0, out=out.view(n, cout, d, 2, h, 2, w, 2))
            return _conv_k3(out, self[3], self[4], True)
        layers.record(self, route, "0")
        return super().forward(x) if layers.RELU_MASKS is None else _seq_hooked(self, x)

    def _train_hip(self, x):
        layers.count_hip()
        y = _ConvT2S2.apply(x, self[0].weight)
        h = bn_train(self[1], y, self[2])
        y, parts, pivot = _conv3_train(self[3], h, self[4])
        return bn_train(self[4], y, self[5], parts, pivot)


class _OutBlock(nn.Sequential):
    """imvoxel_neck.py:152-163: Conv3d(k=3) BN ReLU."""

    def __init__(self, cin: int, cout: int):
        super().__init__(nn.Conv3d(cin, cout, 3, 1, 1, bias=False), nn.BatchNorm3d(cout), nn.ReLU(inplace=True))

    def forward(self, x):
        if layers.record(self, _block_route(x, self, self[0]), "0") == "eval":
            return _conv_k3(x, self[0], self[1], True)
        return super().forward(x) if layers.RELU_MASKS is None else _seq_hooked(self, x)

    def _train_hip(self, x):
        y, parts, pivot = _conv3_train(self[0], x, self[1])
        return bn_train(self[1], y, self[2], parts, pivot)


class IndoorImVoxelNeck(DerivedTensorsMixin, nn.Module):
    """imvoxel_neck.py:70-131: x (N, C_in, Nx, Ny, Nz) -> list of n_scales tensors (N, C_out, Nx/2^i, Ny/2^i, Nz/2^i)."""

    def __init__(self, in_channels: int, out_channels: int, n_blocks: Sequence[int]):
        super().__init__()
        self._init_derived_hooks()
        # training route: "aten" (the framework's layers) or "hip" (our kernels in training mode on CUDA fp32; module docstring)
        self.autograd_route = autograd_route_from_env()
        self.n_scales = len(n_blocks)
        n_channels = in_channels
        for i, nb in enumerate(n_blocks):
            stride = 1 if i == 0 else 2
            blocks = []
            for b in range(nb):   # imvoxel_neck.py:133-149
                if b == 0 and stride != 1:
                    blocks.append(ResModule(n_channels, n_channels * 2, stride))
                    n_channels = n_channels * 2
                else:
                    blocks.append(ResModule(n_channels, n_channels))
            setattr(self, f"down_layer_{i}", nn.Sequential(*blocks))
            if i > 0:
                setattr(self, f"up_block_{i}", _UpBlock(n_channels, n_channels // 2))
            setattr(self, f"out_block_{i}", _OutBlock(n_channels, out_channels))

    @fp32_under_autocast
    def forward(self, x: Tensor) -> List[Tensor]:
        # the training kernels: keyed on the neck's `training`, whatever autograd is (`layers.decide`)
        hip = layers.decide(layers.call_facts(x, self), other=check_route(self) == "hip", keyed="training") == "grad"
        if hip:
            self._check_hip_train(x)

        def run(m, t):
            return m._train_hip(t) if hip else m(t)

        down_outs = []
        for i in range(self.n_scales):
            layer = getattr(self, f"down_layer_{i}")
            if hip:
                for blk in layer:
                    x = blk._train_hip(x)
            else:
                x = layer(x)
            down_outs.append(x)
        outs = []
        for i in range(self.n_scales - 1, -1, -1):
            if i < self.n_scales - 1:
                x = run(getattr(self, f"up_block_{i + 1}"), x)
                x = down_outs[i] + x
            outs.append(run(getattr(self, f"out_block_{i}"), x))
        return outs[::-1]

    def _check_hip_train(self, x: Tensor) -> None:
        """The HIP training route's shape limits, checked before anything runs (no silent fall-back to the framework)."""
        if any(s % (1 << self.n_scales) for s in x.shape[2:]):
            raise ValueError(f"IndoorImVoxelNeck (autograd_route='hip'): the grid {tuple(x.shape[2:])} must be divisible by "
                             f"{1 << self.n_scales}")
        for m in self.modules():
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)) and (m.in_channels % 64 or m.out_channels % 64):
                raise ValueError(f"IndoorImVoxelNeck (autograd_route='hip'): {m} needs channel counts that are multiples of 64")
            if isinstance(m, ResModule) and m.stride != 1:
                cin, cout = m.downsample.conv.in_channels, m.downsample.conv.out_channels
                if m.stride != 2 or not (ops.gemm_layer_ok(cout, cin) and ops.gemm_layer_ok(cin, cout)):
                    raise ValueError(f"IndoorImVoxelNeck (autograd_route='hip'): stride-2 shortcut {cin} -> {cout} not supported")
            if isinstance(m, _UpBlock):
                cin, cout = m[0].in_channels, m[0].out_channels
                if not (ops.gemm_layer_ok(8 * cout, cin) and ops.gemm_layer_ok(cin, 8 * cout)):
                    raise ValueError(f"IndoorImVoxelNeck (autograd_route='hip'): up block {cin} -> {cout} not supported")

    @staticmethod
    def flops(n: int, grid: Sequence[int], in_channels: int = 256, out_channels: int = 128, n_scales: int = 3) -> float:
        """2 x multiply-adds of one forward pass with n_blocks = [1]*n_scales (for the MFMA roofline)."""
        total, c = 0.0, in_channels
        v = [n * (grid[0] >> i) * (grid[1] >> i) * (grid[2] >> i) for i in range(n_scales)]
        for i in range(n_scales):
            if i == 0:
                total += 2 * 54 * c * c * v[0]
            else:
                total += 54 * c * 2 * c * v[i] + 54 * (2 * c) ** 2 * v[i] + 2 * c * 2 * c * v[i]
                c *= 2
            total += 54 * c * out_channels * v[i]
            if i > 0:
                total += 2 * c * (c // 2) * v[i - 1] + 54 * (c // 2) ** 2 * v[i - 1]
        return total


def _seq_hooked(seq: nn.Sequential, x: Tensor) -> Tensor:
    """nn.Sequential.forward with its ReLU modules through the hook."""
    for m in seq:
        x = relu_hooked(m, x) if isinstance(m, nn.ReLU) else m(x)
    return x


# ------------------------------------------------------------------------------------------ training on the HIP kernels
def _conv3_train(conv: nn.Conv3d, x: Tensor, bn: nn.BatchNorm3d):
    """A 3x3x3 convolution (stride 1 or 2, padding 1, no bias) under autograd on the bf16x3 kernels -> (y, parts, pivot): the
    BatchNorm statistics' partial sums from the epilogue (around the running mean) where the stride-1 kernel may give them
    (`layers.fused_stats_ok`) and its grid is not split over the input channels (the 20x20x8 and 10x10x4 levels are; the epilogue
    form would run them unsplit), else (y, None, None)."""
    layers.count_hip()
    if conv.stride[0] == 2:
        return ConvK3S2.apply(x, conv.weight, True), None, None
    n, _, d, h, w = x.shape
    if layers.fused_stats_ok(x) and int(_lib.load().mvsdet_conv3d_k3_bf16x3_workspace_bytes(n, conv.in_channels, conv.out_channels, d, h, w)) == 0:
        pivot = bn.running_mean.detach() if bn.running_mean is not None else None
        y, parts = ConvK3S1.apply(x, conv.weight, True, True, pivot)
        return y, parts, pivot
    return ConvK3S1.apply(x, conv.weight, True), None, None


class _DownS2(torch.autograd.Function):
    """conv0 (3x3x3 stride 2) and the 1x1x1 stride-2 shortcut of a down-sampling ResModule, which read the same input, as one node:
    forward on `ops.conv3d_k3_s2_bf16x3` and `ops.conv3d_k1_s2_bf16x3`; the input gradient is conv0's (the transposed convolution of its
    grad_out, `ops.convT3d_k3_s2_bf16x3`) with the shortcut's accumulated into its even positions (`ops.conv3d_k1_s2_dx_bf16x3`: no
    full-resolution zero tensor, no extra pass); weight gradients `ops.conv3d_k3_dw(stride 2)` and `ops.neck_gemm_dw_bf16x3`.  The
    split weights are cut per call (the weights change every step)."""

    @staticmethod
    def forward(ctx, x, w0, wds):
        ctx.save_for_backward(x, w0, wds)
        cout, cin = wds.shape[:2]
        y0 = ops.conv3d_k3_s2_bf16x3(x, ops.split_conv_weight(w0, 1), None, None, False)
        yd = ops.conv3d_k1_s2_bf16x3(x, ops.gemm_split_weight(wds.detach().reshape(cout, cin)), x.new_zeros(cout), cout, False)
        return y0, yd

    @staticmethod
    def backward(ctx, gy0, gyd):
        x, w0, wds = ctx.saved_tensors
        cout, cin = wds.shape[:2]
        gy0, gyd = gy0.contiguous(), gyd.contiguous()
        gx = gw0 = gwd = None
        if ctx.needs_input_grad[0]:
            gx = ops.convT3d_k3_s2_bf16x3(gy0, ops.split_conv_weight(w0.detach(), 2), None, None, None, False)
            ops.conv3d_k1_s2_dx_bf16x3(gyd, ops.gemm_split_weight(wds.detach().reshape(cout, cin).t().contiguous()), gx)
        if ctx.needs_input_grad[1]:
            gw0 = ops.conv3d_k3_dw(x, gy0, 0, 2, x.shape[-1] % 8 == 0)
        if ctx.needs_input_grad[2]:
            gwd = ops.neck_gemm_dw_bf16x3(x, gyd, False)
        return gx, gw0, gwd


class _ConvT2S2(torch.autograd.Function):
    """ConvTranspose3d(kernel 2, stride 2, no bias) of an up block under autograd: forward `ops.convT3d_k2_s2_bf16x3` (zero bias, no
    ReLU: the training BatchNorm follows), input gradient `ops.convT3d_k2_s2_dx_bf16x3`, weight gradient `ops.neck_gemm_dw_bf16x3`."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        cin, cout = w.shape[:2]
        wq = ops.gemm_split_weight(w.detach().permute(1, 2, 3, 4, 0).reshape(8 * cout, cin).contiguous())
        return ops.convT3d_k2_s2_bf16x3(x, wq, x.new_zeros(cout), cout, False)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        cin, cout = w.shape[:2]
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = ops.convT3d_k2_s2_dx_bf16x3(gy, ops.gemm_split_weight(w.detach().reshape(cin, 8 * cout)), cin)
        if ctx.needs_input_grad[1]:
            gw = ops.neck_gemm_dw_bf16x3(x, gy, True)
        return gx, gw
