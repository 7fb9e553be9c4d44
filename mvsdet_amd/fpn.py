"""Level 0 of the 2-D feature pyramid in front of the sweep: what MVSDet keeps of its `neck` (mvsdet.py:374-376: `x = self.neck(x)[0]`).

The module is mmdet.models.necks.FPN in the shipped configuration: in_channels=[256,512,1024,2048], out_channels=256, num_outs=4,
start_level=0, no add_extra_convs, no norm, no activation, upsample_cfg=dict(mode='nearest').  mmdet is not part of this tree; the
definition below is the builder's reading of that module:

    L3 = lat3(c5)                                  lat_i: 1x1 convolution with bias
    L2 = lat2(c4) + up(L3 -> size of c4)           up: F.interpolate(size=..., mode='nearest')
    L1 = lat1(c3) + up(L2 -> size of c3)
    L0 = lat0(c2) + up(L1 -> size of c2)
    out0 = conv3x3(L0), padding 1, with bias       == FPN(inputs)[0]

The stock module also runs the 3x3 output convolutions of levels 1-3, whose results MVSDet drops; `FPNLevel0` does not.  On CUDA
float32 maps without autograd it runs on csrc/fpn.hip (bf16 matrix cores, three-term split operands: fp32-equivalent; four lateral
launches with the top-down sum in their epilogue, one 3x3 launch that can also write the packed maps the sweep reads); anything else
-- CPU tensors, a grad-enabled call with trainable parameters or inputs -- takes the same function on torch's layers, which is
differentiable.

Training on the HIP kernels is opt-in: `FPNLevel0(..., autograd_route="hip")`.  A grad-enabled call on CUDA float32 tensors where a
stage or a parameter requires grad then runs the same HIP forward under one autograd node, whose backward is csrc/fpn_bwd.hip:

    g   = dL/dout0
    gL0 = conv3x3(g, w3'), w3'[c,o,dy,dx] = w3[o,c,2-dy,2-dx]     the 3x3 kernel on the flipped, transposed weight
    gL1 = up^T(gL0), gL2 = up^T(gL1), gL3 = up^T(gL2)             adjoint of the nearest gather
    dx_i = W_i^T gL_i                                             the lateral kernel on W_i^T (so C_i % 128 == 0)
    dW_i = sum gL_i x_i^T, db_i = sum gL_i;  dW3 = the nine shifted sums of g L0^T, db3 = sum g

Out of scope here: double backward, fp16 / bf16 stage maps, start_level != 0, extra levels, normalised or activated ConvModules,
scale_factor up-sampling.
"""
from __future__ import annotations

from typing import Mapping, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import ops

ROUTES = ("auto", "torch", "hip")
AUTOGRAD_ROUTES = ("torch", "hip")


def _forward_hip(stages, lateral_weights, lateral_biases, out_weight, out_bias, packed, want_l0=False):
    """Four lateral launches, coarsest first, each adding the level above in its epilogue; one 3x3 launch.  The bf16 pieces of the
    weights are cut here, per call."""
    top = None
    for i in range(len(stages) - 1, -1, -1):
        w = lateral_weights[i].detach()
        wq = ops.gemm_split_weight(w.reshape(w.shape[0], w.shape[1]))
        top = ops.fpn.lateral(stages[i].detach(), wq, lateral_biases[i].detach(), top)
    wq = ops.gemm_split_weight(ops.fpn.conv3x3_matrix(out_weight))
    out = ops.fpn.conv3x3(top, wq, out_bias.detach(), want_nchw=True, want_packed=packed)
    return (out, top) if want_l0 else out


class _Level0Function(torch.autograd.Function):
    """Level 0 as ONE autograd node: forward = the HIP forward, backward = the chain of the module's docstring on ops.fpn's gradient
    kernels.  Saves the stages and L0.  Arguments: n_levels, packed, then the stages, the lateral weights, the lateral biases, the
    output weight and bias.  Returns the feature map and, with packed, the packed maps (not differentiable)."""

    @staticmethod
    def forward(ctx, n, packed, *t):
        stages, lw, lb, ow, ob = t[:n], t[n:2 * n], t[2 * n:3 * n], t[3 * n], t[3 * n + 1]
        out, l0 = _forward_hip(stages, lw, lb, ow, ob, packed, want_l0=True)
        ctx.n = n
        ctx.save_for_backward(l0, *stages, *lw, ow)
        if not packed:
            return out
        ctx.mark_non_differentiable(out[1])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        n = ctx.n
        saved = ctx.saved_tensors
        l0, stages, lw, ow = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n], saved[1 + 2 * n]
        need = ctx.needs_input_grad[2:]
        need_x, need_w, need_b, need_ow, need_ob = need[:n], need[n:2 * n], need[2 * n:3 * n], need[3 * n], need[3 * n + 1]
        g = g.contiguous()
        d_ow = ops.fpn.weight_grad(g, l0, 9) if need_ow else None
        d_ob = ops.fpn.bias_grad(g) if need_ob else None
        dx, dw, db = [None] * n, [None] * n, [None] * n
        # the coarsest level that still needs gL_i: nothing above it is computed
        last = max([i for i in range(n) if need_x[i] or need_w[i] or need_b[i]], default=-1)
        gl = ops.fpn.conv3x3_input_grad(g, ow) if last >= 0 else None
        for i in range(last + 1):
            if i > 0:
                gl = ops.fpn.top_down_grad(gl, stages[i].shape[2:])
            if need_x[i]:
                dx[i] = ops.fpn.lateral_input_grad(gl, lw[i])
            if need_w[i]:
                dw[i] = ops.fpn.weight_grad(gl, stages[i], 1).view(lw[i].shape)
            if need_b[i]:
                db[i] = ops.fpn.bias_grad(gl)
        return (None, None, *dx, *dw, *db, d_ow, d_ob)


class FPNLevel0(nn.Module):
    """forward(stages, packed=False): stages = the backbone maps (N,C_i,H_i,W_i), finest first -> feature (N,Cout,H_0,W_0); with
    packed=True -> (feature, packed), packed = what `ops.pack_features(feature)` gives (on the HIP route written by the 3x3 kernel's
    epilogue: no packing launch).

    route: "auto" (HIP where it can run, else torch), "torch", or "hip" (raises where it cannot run).

    autograd_route: "torch" (default: a grad-enabled call where something requires grad takes torch's layers; route "hip" raises) or
    "hip": such a call on CUDA float32 tensors, under route "auto" or "hip", runs the HIP kernels forward AND backward (one autograd
    node, once differentiable; csrc/fpn_bwd.hip).  What that route cannot run -- a stage whose channels are not divisible by 128 --
    raises ValueError from `ops.fpn.check_grad_shapes`; there is no silent fall-back.

    The bf16 pieces of the five weight matrices are cut on EVERY call (five splits and the copy that lays the 3x3 weight out
    tap-major: six small launches, 13 MB of traffic), not kept per parameter `_version` as neck.py / costreg.py keep theirs: an
    in-place update through `.data` does not move `_version`, and kept pieces measured no faster.  So any in-place
    update of a weight is seen by the next call."""

    def __init__(self, lateral_weights: Sequence[Tensor], lateral_biases: Sequence[Tensor], out_weight: Tensor, out_bias: Tensor,
                 route: str = "auto", autograd_route: str = "torch"):
        super().__init__()
        if route not in ROUTES:
            raise ValueError(f"FPNLevel0: route {route!r} is not one of {ROUTES}")
        if autograd_route not in AUTOGRAD_ROUTES:
            raise ValueError(f"FPNLevel0: autograd_route {autograd_route!r} is not one of {AUTOGRAD_ROUTES}")
        if len(lateral_weights) != len(lateral_biases) or len(lateral_weights) < 1:
            raise ValueError("FPNLevel0: one bias per lateral weight")

        def param(t):
            return t if isinstance(t, nn.Parameter) else nn.Parameter(t.detach().clone())

        self.lateral_weights = nn.ParameterList([param(w) for w in lateral_weights])
        self.lateral_biases = nn.ParameterList([param(b) for b in lateral_biases])
        self.out_weight = param(out_weight)
        self.out_bias = param(out_bias)
        self.route = route
        self.autograd_route = autograd_route

    # ------------------------------------------------------------------------------------------------- constructors
    @classmethod
    def from_module(cls, fpn, route: str = "auto", autograd_route: str = "torch") -> "FPNLevel0":
        """From an object laid out as mmdet's FPN (duck-typed): `fpn.lateral_convs[i].conv.{weight,bias}` and
        `fpn.fpn_convs[0].conv.{weight,bias}`.  The parameters are SHARED with `fpn`, not copied."""
        lats = [m.conv for m in fpn.lateral_convs]
        out = fpn.fpn_convs[0].conv
        for i, c in enumerate(lats + [out]):
            if getattr(c, "bias", None) is None:
                raise ValueError(f"FPNLevel0.from_module: convolution {i} has no bias (a normalised ConvModule is out of scope)")
        return cls([c.weight for c in lats], [c.bias for c in lats], out.weight, out.bias, route=route, autograd_route=autograd_route)

    @classmethod
    def from_state_dict(cls, sd: Mapping[str, Tensor], prefix: str = "neck.", route: str = "auto",
                        autograd_route: str = "torch") -> "FPNLevel0":
        """From a checkpoint with mmdet's keys `{prefix}lateral_convs.{i}.conv.weight|bias` and `{prefix}fpn_convs.0.conv.weight|bias`
        (copies).  The keys of the unused `fpn_convs.1..` are accepted and ignored; a missing lateral raises KeyError."""
        def key(name):
            k = prefix + name
            if k not in sd:
                raise KeyError(f"FPNLevel0.from_state_dict: {k!r} is missing")
            return sd[k]

        # as many levels as the highest lateral index says: a hole below it (laterals 0, 1, 3) is a missing key
        head = prefix + "lateral_convs."
        idx = [int(k[len(head):].split(".")[0]) for k in sd if k.startswith(head)]
        if not idx:
            raise KeyError(f"FPNLevel0.from_state_dict: no {head}* keys")
        n = max(idx) + 1
        lw = [key(f"lateral_convs.{i}.conv.weight") for i in range(n)]
        lb = [key(f"lateral_convs.{i}.conv.bias") for i in range(n)]
        return cls(lw, lb, key("fpn_convs.0.conv.weight"), key("fpn_convs.0.conv.bias"), route=route, autograd_route=autograd_route)

    # ------------------------------------------------------------------------------------------------- routes
    def _hip_refusal(self, stages: Sequence[Tensor]) -> Optional[str]:
        """Why this call cannot take the HIP route (None: it can)."""
        tensors = list(stages) + list(self.parameters())
        if not all(isinstance(s, Tensor) and s.is_cuda for s in tensors):
            return "stages and parameters must live on a ROCm device"
        if any(s.dtype != torch.float32 for s in tensors):
            return "stages and parameters must be float32"
        if self.autograd_route != "hip" and self._wants_grad(stages):
            return "autograd is on and a stage or a parameter requires grad (the HIP route is forward only unless autograd_route='hip')"
        return None

    def _wants_grad(self, stages: Sequence[Tensor]) -> bool:
        return torch.is_grad_enabled() and any(t.requires_grad for t in list(stages) + list(self.parameters()))

    def forward_torch(self, stages: Sequence[Tensor], packed: bool = False):
        """The five F.conv2d and three F.interpolate of level 0 on torch's layers (differentiable)."""
        top = None
        for i in range(len(stages) - 1, -1, -1):
            w = self.lateral_weights[i]
            lat = F.conv2d(stages[i], w.reshape(w.shape[0], w.shape[1], 1, 1), self.lateral_biases[i])
            top = lat if top is None else lat + F.interpolate(top, size=lat.shape[2:], mode="nearest")
        feature = F.conv2d(top, self.out_weight, self.out_bias, padding=1)
        if not packed:
            return feature
        return feature, ops.pack_features(feature.detach())

    def forward_hip(self, stages: Sequence[Tensor], packed: bool = False):
        """Four lateral launches, coarsest first, each adding the level above in its epilogue; one 3x3 launch."""
        return _forward_hip(stages, list(self.lateral_weights), list(self.lateral_biases), self.out_weight, self.out_bias, packed)

    def forward_hip_autograd(self, stages: Sequence[Tensor], packed: bool = False):
        """`forward_hip` under one autograd node whose backward runs on csrc/fpn_bwd.hip (autograd_route "hip")."""
        ops.fpn.check_grad_shapes(stages, list(self.lateral_weights), list(self.lateral_biases), self.out_weight, self.out_bias)
        out = _Level0Function.apply(len(stages), bool(packed), *stages, *self.lateral_weights, *self.lateral_biases, self.out_weight,
                                    self.out_bias)
        return tuple(out) if packed else out

    def forward(self, stages: Sequence[Tensor], packed: bool = False):
        stages = list(stages)
        ops.fpn.check_shapes(stages, list(self.lateral_weights), list(self.lateral_biases), self.out_weight, self.out_bias)
        if self.route not in ROUTES:
            raise ValueError(f"FPNLevel0: route {self.route!r} is not one of {ROUTES}")
        if self.autograd_route not in AUTOGRAD_ROUTES:
            raise ValueError(f"FPNLevel0: autograd_route {self.autograd_route!r} is not one of {AUTOGRAD_ROUTES}")
        if self.route != "torch":
            why = self._hip_refusal(stages)
            if why is None:
                if self._wants_grad(stages):
                    return self.forward_hip_autograd(stages, packed)
                return self.forward_hip(stages, packed)
            if self.route == "hip":
                raise RuntimeError(f"FPNLevel0 (route='hip'): {why}")
        return self.forward_torch(stages, packed)
