"""Layer code shared by the cost network (costreg.py), the 3-D neck (neck.py) and the detection head (head.py): the caches of
tensors derived from parameters and their stream ordering, the `--amp` wrapper, the training route option, the facts that decide
whether a layer call runs on our kernels or on the framework's with the counters of both outcomes (`route_stats`,
`framework_calls`), the 3x3x3 autograd functions on our convolution kernels, and training-mode BatchNorm with its ReLU-decision test
hook.  None of those three modules imports another; each imports from here.

Tests toggle `RELU_MASKS` and `FUSED_BN_STATS` on this module: read them through the module object at call time.  `costreg` and
`neck` forward their attributes of those names here (`ForwardedToggles`).
"""
from __future__ import annotations

import collections
import functools
import os
import types
import weakref

import torch
from torch import Tensor, nn
from torch.nn import functional as F

from . import ops


def fp32_under_autocast(forward):
    """`--amp` (tools/train.py:24-28): under torch.autocast a module of this package still computes in float32 (bf16x3 on the
    matrix cores is fp32-equivalent; the framework's layers it falls back to would otherwise run float16 convolutions beside
    it): low-precision inputs are cast up and autocast is off for the call.  Outside autocast the call is untouched."""
    def _up(v):
        if isinstance(v, Tensor):
            return v.float() if v.is_floating_point() and v.dtype != torch.float32 else v
        if isinstance(v, (list, tuple)):
            return type(v)(_up(t) for t in v)
        return v

    @functools.wraps(forward)
    def wrapped(self, x, *args, **kwargs):
        if torch.is_autocast_enabled("cuda"):
            with torch.autocast("cuda", enabled=False):
                return forward(self, _up(x), *args, **kwargs)
        return forward(self, x, *args, **kwargs)
    return wrapped


# ------------------------------------------------------------------------------------------ tensors derived from parameters
_DERIVED = ("_mvs_affine", "_fused", "_mvs_wsplit", "_mvs_wmat", "_mvs_sclbuf")   # tensors computed from parameters and kept on a module


def drop_derived_tensors(root: nn.Module) -> None:
    """Forget every tensor this package derived from `root`'s parameters (BatchNorm affines, fused / permuted / split
    weights).  The caches key on (data_ptr, _version), which an in-place update through `.data` does not bump (mmengine's
    EMAHook swaps parameters that way) -- so they are also dropped on every train()/eval() switch and after
    load_state_dict (`DerivedTensorsMixin`); call this by hand after any other out-of-band `.data` write."""
    for m in root.modules():
        for name in _DERIVED:
            if m.__dict__.get(name) is not None:
                m.__dict__[name] = None


def _drop_after_load(module: nn.Module, incompatible_keys) -> None:
    # module-level (not a lambda or a closure): the hook is stored on the module and must pickle with it
    # (torch.save(model), mp.spawn)
    drop_derived_tensors(module)


class DerivedTensorsMixin:
    """nn.Module mixin of the modules that own derived-tensor caches: mode switches and state-dict loads drop them."""

    def _init_derived_hooks(self):
        self.register_load_state_dict_post_hook(_drop_after_load)

    def train(self, mode: bool = True):
        drop_derived_tensors(self)
        return super().train(mode)


# Derived tensors are computed by whichever stream first needs them and kept on the module; a call on ANOTHER stream shortly
# afterwards (the two halves of CostRegNet3DGS.view_streams; a detector moved to a side stream) must not read them before the
# kernels that fill them ran.  Every derived tensor is therefore registered with the event recorded behind its computation, and every
# use makes the using stream wait for it while it is pending.  Kept outside the modules (events do not pickle), by the tensor.
_PENDING: dict = {}   # id(tensor) -> (weak reference to it, event); by identity: tensors compare element-wise


def mark_made(*tensors: Tensor) -> None:
    ts = [t for t in tensors if isinstance(t, Tensor) and t.is_cuda]
    if ts:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(ts[0].device))
        for t in ts:
            _PENDING[id(t)] = (weakref.ref(t), ev)
        if len(_PENDING) > 4096:   # entries of tensors that died before anyone asked again
            for k in [k for k, (r, e) in _PENDING.items() if r() is None or e.query()]:
                _PENDING.pop(k, None)


def await_made(*tensors: Tensor) -> None:
    for t in tensors:
        ent = _PENDING.get(id(t)) if isinstance(t, Tensor) else None
        if ent is not None and ent[0]() is t:
            if ent[1].query():
                _PENDING.pop(id(t), None)
            else:
                torch.cuda.current_stream(t.device).wait_event(ent[1])


def bn_affine(bn: nn.BatchNorm3d):
    """Eval-mode BatchNorm as a per-channel affine; kept on the module until one of its four tensors changes (five tiny
    kernels per layer otherwise: a twentieth of the neck's time at one scene) or `drop_derived_tensors` runs."""
    key = tuple((t.data_ptr(), t._version) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    cached = getattr(bn, "_mvs_affine", None)
    if cached is None or cached[0] != key:
        with torch.no_grad():
            scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
            cached = (key, scale, bn.bias - bn.running_mean * scale)
        mark_made(cached[1], cached[2])
        bn._mvs_affine = cached
    await_made(cached[1], cached[2])
    return cached[1], cached[2]


# ------------------------------------------------------------------------------------------ training route of neck and head
AUTOGRAD_ROUTES = ("aten", "hip")


def autograd_route_from_env() -> str:
    """The initial `autograd_route` of the neck and the head: MVSDET_DETECTOR_AUTOGRAD, "aten" when unset."""
    route = os.environ.get("MVSDET_DETECTOR_AUTOGRAD", "aten")
    if route not in AUTOGRAD_ROUTES:
        raise ValueError(f"MVSDET_DETECTOR_AUTOGRAD must be one of {AUTOGRAD_ROUTES}, got {route!r}")
    return route


def check_route(module: nn.Module) -> str:
    route = getattr(module, "autograd_route", "aten")
    if route not in AUTOGRAD_ROUTES:
        raise ValueError(f"{type(module).__name__}.autograd_route must be one of {AUTOGRAD_ROUTES}, got {route!r}")
    return route


# ------------------------------------------------------------------------------------------ which route a layer call takes
# A layer of costreg / neck / head runs on this library's eval kernels, on its second family of kernels (autograd / training), or
# on the framework's own layers (ATen / MIOpen).  The facts of a call that decide between them are the same for every layer of one
# forward pass: a module's forward reads them once (`call_facts`) and hands them to its layers; each layer adds only its own rule
# (channel multiples, stride, `ops.gemm_layer_ok`, the module's options) and `decide` is the one table both the route and, for the
# framework, the reason come from.  They read only x.is_cuda, x.dtype, module.training and torch.is_grad_enabled().
def hip_tensor(x) -> bool:
    """A tensor our kernels take: on a ROCm device, float32."""
    return x.is_cuda and x.dtype == torch.float32


Call = collections.namedtuple("Call", "tensor grad training")   # hip_tensor(x), autograd is on, the module's mode


def call_facts(x, module: nn.Module) -> Call:
    return Call(hip_tensor(x), torch.is_grad_enabled(), module.training)


def decide(call: Call, fits: bool = True, other=None, other_fits: bool = True, keyed: str = "grad", any_mode: bool = False) -> str:
    """The route of a layer call: "eval" = our eval kernels, "grad" = our other kernels, else why the framework runs it.
    eval kernels: a `hip_tensor`, autograd off, the module not training, and `fits` (the layer's shape rule).  `any_mode`: `training`
        is not looked at (the cost network's head convolution, which has no BatchNorm behind it).
    other kernels: `other` is None where the site has none, else the option that enables them (`hip_backward`, `autograd_route ==
        "hip"`).  They run when the fact named by `keyed` is set, WHATEVER THE OTHER FACT IS, and `fits and other_fits`.  The modules
        differ here, on purpose: the cost network and the head key on "grad" (autograd on, in .train() or .eval(): a cost network in
        .train() under no_grad has no kernel route at all, and in .eval() under autograd its convolutions run here while its
        BatchNorms, on running statistics, go to the framework: `bn_relu_framework`); the neck keys on "training" (the neck's
        training kernels run with autograd on or off; a block of it called in training mode is on the framework by that option).
    reasons, the first that applies: "tensor" (not a `hip_tensor`), "option" (the kernels for this call exist and the module's option
        chose the framework), "mode" (an autograd / training combination the site has no kernels for), "shape" (the layer's own rule:
        a channel multiple, a stride, `ops.gemm_layer_ok`, odd extents, a BatchNorm without affine parameters)."""
    if not call.tensor:
        return "tensor"
    if other is not None and (call.grad if keyed == "grad" else call.training):
        return "option" if not other else "grad" if fits and other_fits else "shape"
    if call.grad or (call.training and not any_mode):
        return "mode"
    return "eval" if fits else "shape"


# Which way each layer call went.  The unit is one layer of the reference module -- a convolution with the BatchNorm and ReLU behind
# it, a shortcut, the head's fused convolution of a level -- counted once per call, whichever of our kernels run it; a BatchNorm that
# goes to the framework beside a convolution of ours is one "framework" call of its own.  Host-side dict increments: no tensor
# operation, no synchronisation, no warning (a CPU run takes the framework everywhere, legitimately).  Under a captured graph they
# count at capture time only, not per replay.  A choice between two kernels of ours (bf16x3 / fp32 MFMA / fp16 + MX, packed or plain
# input) is not a route and is not counted.
route_stats = {"hip": 0, "framework": 0}   # layer calls on a kernel of this library | on the framework's layer, GEMM or BatchNorm
framework_calls: dict = {}                 # (site, reason) -> count; site = "<owner's class>.<layer attribute>"


def reset_route_stats() -> None:
    route_stats.update(hip=0, framework=0)
    framework_calls.clear()


def count_hip(n: int = 1) -> None:
    route_stats["hip"] += n


def count_framework(owner: nn.Module, reason: str, *path) -> None:
    """One layer call handed to the framework.  path: the sub-module of `owner` that ran, or its attribute name (then, for a part of
    a layer, the sub-module of that one): the site is the owner's class and those names, "CostRegNet3DGS.conv0", "_UpBlock.3",
    "CostRegNet3DGS.conv9.1"."""
    names, parent = [type(owner).__name__], owner
    for child in path:
        names.append(child if isinstance(child, str) else next(k for k, m in parent._modules.items() if m is child))
        parent = child
    key = (".".join(names), reason)
    route_stats["framework"] += 1
    framework_calls[key] = framework_calls.get(key, 0) + 1


def record(owner: nn.Module, route: str, *sublayers) -> str:
    """Count the call of each of `owner`'s layers `sublayers` (sub-modules or their attribute names) by the route their site decided
    (`decide`) and hand the route back."""
    if route == "eval" or route == "grad":
        route_stats["hip"] += len(sublayers)
    else:
        for layer in sublayers:
            count_framework(owner, route, layer)
    return route


def bn_relu_framework(owner: nn.Module, layer: nn.Module, bn: nn.BatchNorm3d, y: Tensor) -> Tensor:
    """relu(bn(y)) on the framework's BatchNorm behind an autograd convolution of ours (`layer`'s), counted: it runs on running
    statistics ("mode") or has no affine parameters ("shape"), and the training kernels take neither."""
    count_framework(owner, "shape" if bn.training else "mode", layer, bn)
    return torch.relu_(bn(y))


# ------------------------------------------------------------------------------------------ 3x3x3 convolutions under autograd
class ConvK3S1(torch.autograd.Function):
    """Conv3d(kernel 3, stride 1, padding 1, no bias) with all three passes on the fp32 matrix cores: forward and input
    gradient through `ops.conv3d_k3_mfma` (the input gradient is the same convolution of grad_out with the weights
    transposed and flipped), weight gradient through `ops.conv3d_k3_dw`.  MIOpen needs 34 + 42 + 360 ms for conv0 at the
    reference-true shape, these kernels 15 + 15 + 22 ms."""

    @staticmethod
    def forward(ctx, x, weight, bf16x3=False, stats=False, pivot=None):
        """stats (bf16x3 only): also return the per-channel partial sums of the output and of its squares from the kernel's
        epilogue (`ops.conv3d_k3_bf16x3_stats`, sums of value - pivot_c), for the training-mode BatchNorm behind the layer."""
        ctx.save_for_backward(x, weight)
        ctx.bf16x3 = bool(bf16x3)
        if ctx.bf16x3 and stats:
            y, parts = ops.conv3d_k3_bf16x3_stats(x, ops.split_conv_weight(weight), pivot)
            ctx.mark_non_differentiable(parts)
            return y, parts
        if ctx.bf16x3:   # forward and input gradient on the bf16 matrix cores, three-term split (csrc/costreg_bf16.hip)
            return ops.conv3d_k3_bf16x3(x, ops.split_conv_weight(weight), None, None, False)
        return ops.conv3d_k3_mfma(x, ops.permute_conv_weight(weight), None, None, False)

    @staticmethod
    def backward(ctx, gy, gparts=None):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            wflip = weight.detach().transpose(0, 1).flip(2, 3, 4).contiguous()      # (Cin, Cout, 3,3,3)
            if ctx.bf16x3 and wflip.shape[0] % 64 == 0:
                src = gy
                if wflip.shape[0] >= 256:
                    # four or more blocks of output channels per tile would each cut the same grad_out values into bf16 pieces:
                    # one packing pass and the DMA-fed form instead (conv0: 4.78 -> 4.65 ms, the same bits).  The SCL copy
                    # (larger than grad_out itself) lives for this one convolution: it comes from the caching allocator and goes
                    # back to it when `src` dies below -- the packing kernel writes the zero border itself, nothing is kept
                    src = ops.scl_pack(gy)
                gx = ops.conv3d_k3_bf16x3(src, ops.split_conv_weight(wflip), None, None, False)
                del src
            else:
                gx = ops.conv3d_k3_mfma(gy, ops.permute_conv_weight(wflip), None, None, False)
        if ctx.needs_input_grad[1]:   # bf16x3: csrc/costreg_dw_bf16.hip (rows read as float4)
            gw = ops.conv3d_k3_dw(x, gy, 0, 1, ctx.bf16x3 and x.shape[-1] % 4 == 0)
        return gx, gw, None, None, None


class ConvK3S2(torch.autograd.Function):
    """Conv3d(kernel 3, stride 2, padding 1, no bias) of conv1 / conv3 (mvsnet.py:77,80) under autograd: forward on
    `ops.conv3d_k3_mfma(stride=2)`; the input gradient is the transposed convolution of grad_out with the same weight
    (`ops.convT3d_k3_s2_mfma`: the (Cout,Cin,3,3,3) tensor read as a ConvTranspose3d weight), the weight gradient
    `ops.conv3d_k3_dw(stride=2)`.  D, H, W even (the network asks for multiples of 4)."""

    @staticmethod
    def forward(ctx, x, weight, bf16x3=False, split_skip=False):
        """split_skip: also return x itself as a second output, for the skip connection that reads it (mvsnet.py:109-111).  The
        input then has this one consumer, both gradients arrive here together, and the skip's is added in the epilogue of the
        input-gradient kernel instead of by a pass of autograd's own over the full-resolution tensor."""
        ctx.save_for_backward(x, weight)
        ctx.bf16x3 = bool(bf16x3)
        ctx.set_materialize_grads(False)
        if ctx.bf16x3:
            y = ops.conv3d_k3_s2_bf16x3(x, ops.split_conv_weight(weight, 1), None, None, False)
        else:
            y = ops.conv3d_k3_mfma(x, ops.permute_conv_weight(weight), None, None, False, 2)
        return (y, x.view_as(x)) if split_skip else y

    @staticmethod
    def backward(ctx, gy, gskip=None):
        x, weight = ctx.saved_tensors
        gx = gw = None
        if gy is None:   # only the skip branch reached the loss
            return gskip, None, None, None
        gy = gy.contiguous()
        if ctx.needs_input_grad[0]:
            res = None if gskip is None else gskip.contiguous()
            if ctx.bf16x3 and weight.shape[1] % 64 == 0:   # the (Cout,Cin,3,3,3) tensor read as a ConvTranspose3d weight
                gx = ops.convT3d_k3_s2_bf16x3(gy, ops.split_conv_weight(weight.detach(), 2), None, None, res, False)
            else:
                gx = ops.convT3d_k3_s2_mfma(gy, ops.permute_convT_weight(weight.detach()), None, None, res, False)
        if ctx.needs_input_grad[1]:
            gw = ops.conv3d_k3_dw(x, gy, 0, 2, ctx.bf16x3 and x.shape[-1] % 8 == 0)
        return gx, gw, None, None


class ConvT3S2(torch.autograd.Function):
    """ConvTranspose3d(kernel 3, stride 2, padding 1, output_padding 1, no bias) of conv9 / conv11 (mvsnet.py:92-100) under
    autograd, the mirror image of `ConvK3S2`: forward on `ops.convT3d_k3_s2_mfma`, input gradient = the stride-2
    convolution of grad_out with the (Cin,Cout,3,3,3) weight read as a Conv3d weight, weight gradient = the stride-2
    weight-gradient kernel with the two tensors exchanged."""

    @staticmethod
    def forward(ctx, x, weight, bf16x3=False, stats=False, pivot=None):
        """stats (bf16x3 only): also return the partial sums of the output's BatchNorm statistics from the kernel's epilogue
        (`ops.convT3d_k3_s2_bf16x3_stats`); an empty tensor where the shape has no such form."""
        ctx.save_for_backward(x, weight)
        ctx.bf16x3 = bool(bf16x3)
        if ctx.bf16x3 and stats:
            got = ops.convT3d_k3_s2_bf16x3_stats(x, ops.split_conv_weight(weight, 2), pivot)
            if got is None:
                y, parts = ops.convT3d_k3_s2_bf16x3(x, ops.split_conv_weight(weight, 2), None, None, None, False), x.new_empty(0, dtype=torch.float64)
            else:
                y, parts = got
            ctx.mark_non_differentiable(parts)
            return y, parts
        if ctx.bf16x3:
            return ops.convT3d_k3_s2_bf16x3(x, ops.split_conv_weight(weight, 2), None, None, None, False)
        return ops.convT3d_k3_s2_mfma(x, ops.permute_convT_weight(weight), None, None, None, False)

    @staticmethod
    def backward(ctx, gy, gparts=None):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            if ctx.bf16x3 and weight.shape[0] % 64 == 0:   # the (Cin,Cout,3,3,3) tensor read as a Conv3d weight
                gx = ops.conv3d_k3_s2_bf16x3(gy, ops.split_conv_weight(weight.detach(), 1), None, None, False)
            else:
                gx = ops.conv3d_k3_mfma(gy, ops.permute_conv_weight(weight.detach()), None, None, False, 2)
        if ctx.needs_input_grad[1]:
            gw = ops.conv3d_k3_dw(gy, x, 0, 2, ctx.bf16x3 and gy.shape[-1] % 8 == 0)
        return gx, gw, None, None, None


# training: the statistics of a BatchNorm behind a stride-1 bf16x3 convolution come from that convolution's epilogue (partial sums
# per block, finished in a fixed order) instead of a pass of their own over the tensor; MVSDET_FUSED_BN_STATS=0: the separate pass
FUSED_BN_STATS = os.environ.get("MVSDET_FUSED_BN_STATS", "1") != "0"


def fused_stats_ok(x: Tensor) -> bool:
    """Whether a stride-1 bf16x3 convolution of x may hand its BatchNorm the statistics from its epilogue: FUSED_BN_STATS, more
    than one output voxel.  Callers add their own conditions (the neck refuses grids split over the input channels; the cost network does not)."""
    n, _, d, h, w = x.shape
    return FUSED_BN_STATS and n * d * h * w > 1


# ------------------------------------------------------------------------------------------ training BatchNorm and its test hook
# Test hook (tests/test_gpu_parity.py, tests/test_f3_goldens.py G12c, tests/test_g14_neck_head_train.py): the ReLU DECISIONS of a
# training pass recorded or imposed.  None (always, outside those tests) | ("record", {}) -- filled with {key: mask of the ReLU's
# positive side} -- | ("apply", {key: bool mask}): the layer multiplies by the mask instead of taking the ReLU.  With the decisions of
# ONE pass imposed on two routes (or the reference's on ours) no activation can fall on the other side of zero, and gradients can be
# compared element-wise instead of by direction.  Keys: the cost network's BatchNorm modules; in the neck the `_ConvModule` with an
# activation (conv0 of a ResModule), the ResModule (its output ReLU) and the nn.ReLU modules of the up / out blocks.
RELU_MASKS = None


def relu_hooked(key: nn.Module, t: Tensor) -> Tensor:
    """The framework's in-place ReLU through the hook (the neck's ATen route)."""
    hook = RELU_MASKS
    if hook is None:
        return F.relu(t, inplace=True)
    if hook[0] == "record":
        t = F.relu(t, inplace=True)
        hook[1][key] = t.detach() > 0
        return t
    return t * hook[1][key].to(t.dtype)


def update_running_stats(bn: nn.BatchNorm3d, x: Tensor, mean: Tensor, invstd: Tensor) -> None:
    """The running statistics of a training-mode BatchNorm from the batch's mean and 1/sqrt(biased var + eps), as
    torch.nn.BatchNorm3d updates them (momentum or the cumulative average, unbiased variance, num_batches_tracked)."""
    if bn.track_running_stats and bn.running_mean is not None:
        with torch.no_grad():
            m = x.numel() // x.shape[1]
            bn.num_batches_tracked += 1
            mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            var = (1.0 / (invstd * invstd) - bn.eps).clamp_min_(0.0) * (m / max(m - 1, 1))
            bn.running_mean.mul_(1.0 - mom).add_(mean, alpha=mom)
            bn.running_var.mul_(1.0 - mom).add_(var, alpha=mom)


def bn_train(bn: nn.BatchNorm3d, x: Tensor, key, parts: Tensor | None = None, pivot: Tensor | None = None,
             residual: Tensor | None = None, skip: Tensor | None = None) -> Tensor:
    """Training-mode BatchNorm with batch statistics on the streaming kernels of csrc/costreg_bn.hip -- [relu](bn(x) [+ residual])
    [+ skip] -- and the running statistics updated the way torch.nn.BatchNorm3d does.  key: the hook's key of the ReLU, None = no
    activation; residual: added inside the ReLU (the neck's ResModule); skip: added after it (the cost network's up layers,
    mvsnet.py:109-111); parts / pivot: the statistics' partial sums from the producing convolution's epilogue (no pass over x for
    them) and the vector they are taken around."""
    hook = RELU_MASKS if key is not None else None
    act = key is not None and (hook is None or hook[0] == "record")
    if residual is not None:
        out, mean, invstd = ops.bn3d_res_relu_train(x, bn.weight, bn.bias, residual, bn.eps, act, parts, pivot)
    else:   # without the hook the skip is added in the kernel's second pass
        out, mean, invstd = ops.bn3d_relu_train(x, bn.weight, bn.bias, bn.eps, act, skip if hook is None else None, parts, pivot)
    if hook is not None:
        if hook[0] == "record":
            hook[1][key] = out.detach() > 0
        else:
            out = out * hook[1][key].to(out.dtype)
        if skip is not None:
            out = out + skip
    update_running_stats(bn, x, mean, invstd)
    return out


class ForwardedToggles(types.ModuleType):
    """The module type of `costreg` and `neck`: their RELU_MASKS and FUSED_BN_STATS attributes read and write this module's, so
    code written when each model kept its own copy (costreg.RELU_MASKS, costreg.FUSED_BN_STATS, neck.RELU_MASKS) still sets the
    one hook and the one option."""


for _name in ("RELU_MASKS", "FUSED_BN_STATS"):
    setattr(ForwardedToggles, _name, property(lambda _m, n=_name: globals()[n], lambda _m, v, n=_name: globals().__setitem__(n, v)))
del _name
