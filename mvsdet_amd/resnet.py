"""The 2-D backbone in front of the pyramid: the stages C2..C5 of a bottleneck ResNet with frozen BatchNorm.

The shipped configs use ResNet(depth=50, style='pytorch', norm_eval=True, norm_cfg=dict(type='BN', requires_grad=False)): every
BatchNorm is a fixed per-channel affine in training and in evaluation alike, and no convolution has a bias.  mmdet is not part of this
tree; the definition below is the builder's reading of ResNet v1.5 (what `torchvision://resnet50` with style='pytorch' means):

    stem(img)  = maxpool(3, stride 2, pad 1)( relu( bn1( conv 7x7, stride 2, pad 3, 3 -> 64 (img) ) ) )
    bottleneck(x; planes p, stride s, downsample?):
        a   = relu(bn1(conv1x1(x)))                       C  -> p
        b   = relu(bn2(conv3x3(a, stride s, pad 1)))      p  -> p      the stride sits on the 3x3
        c   = bn3(conv1x1(b))                             p  -> 4p
        id  = bn_d(conv1x1(x, stride s)) if downsample else x
        out = relu(c + id)
    layer1..4: (3, 4, 6, 3) blocks, planes (64, 128, 256, 512), strides (1, 2, 2, 2); the first block of each has the downsample branch
    bn(y) = y * scale + shift, scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale
    C2..C5 = the outputs of layer1..layer4

On CUDA float32 images without autograd the layers run on csrc/resnet.hip (bf16 matrix cores, three-term split operands:
fp32-equivalent; one launch per convolution, the affine, the residual sum and the ReLU in its epilogue: 52 launches for ResNet-50);
anything else -- CPU tensors, a grad-enabled call where something requires grad -- takes the same function on F.conv2d, which is
differentiable.  The stem stays on torch's layers on both routes.

Training on the HIP kernels is opt-in: `ResNetStages(..., autograd_route="hip")`.  A grad-enabled call on CUDA float32 tensors where
something requires grad then runs the stem on torch and every bottleneck whose input or convolution weights require grad as the SAME
HIP forward under its own once-differentiable autograd node (a bottleneck where nothing does -- all of layer 1 under the shipped
frozen_stages=1 -- runs the plain forward with no node).  The node saves x, a, b, out; its backward is csrc/resnet_bwd.hip, g = dL/dout:

    gz  = gate(g, out)                       gate(v, y) = y <= 0 ? 0 : v on the saved OUTPUT y: torch.relu's gradient rule
    dW3 = scale3 (.) (gz b^T)                gb = gate(W3'^T gz, b)
    dW2 = scale2 (.) dw3x3_s(gb, a)          ga = gate(convT3x3_s(gb; W2'), a)
    dW1 = scale1 (.) (ga x^T)                dx = (W1'^T ga) + ( gz | spread_s(Wd'^T gz) )      the GEMM first, then + the residual
    dWd = scaled (.) (gz x[.., s y, s x]^T)

gz is one elementwise launch (the gradient arriving at `out` is autograd's sum over the next block and the pyramid, so no producer of
ours has it in an epilogue); gb's and ga's gates are their producers' epilogues.  With every gradient wanted an identity block's
backward is 10 gradient launches (the gate, gb, ga, dx, three weight gradients of two launches each), a stride-2 block with the branch
16 (ga is four, one per parity class; the branch adds Wd'^T gz and dWd), behind the torch expressions and the splits that cut the
transposed weights per call and the three or four elementwise products that scale the rows of dW.  What that
route cannot run raises ValueError: a BatchNorm weight or bias that requires grad (the config's norm_cfg=dict(requires_grad=False)), a
trainable convolution whose layer breaks the weight-gradient channel rule Cout % 128 == 0, C % 32 == 0 (layer 1's 64-row layers: the
config's frozen_stages=1), double backward.  There is no silent fall-back.  `freeze_()` sets what the shipped configs set.

Out of scope here: the stem on HIP, BatchNorm parameters' gradients, trainable layers with Cout % 128 != 0, double backward, activation
recomputation (with_cp), fp16 / bf16 images and an autocast rule, style='caffe', dilations, avg_down, deep stems, DCN, plugins,
BasicBlock nets.
"""
from __future__ import annotations

from typing import List, Mapping, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import ops
from .layers import DerivedTensorsMixin, await_made, drop_derived_tensors, mark_made

ROUTES = ("auto", "torch", "hip")
AUTOGRAD_ROUTES = ("torch", "hip")
# What "auto" resolves to on CUDA float32 tensors without autograd: the measured choice of profiles/resnet_timing.txt.
AUTO_ON_CUDA = "hip"
_BN_TENSORS = ("weight", "bias", "running_mean", "running_var")


def _affine(bn) -> Tuple[Tensor, Tensor]:
    """The frozen BatchNorm as (scale, shift); differentiable in bn.weight and bn.bias."""
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias - bn.running_mean * scale


def _derived(conv, bn) -> Tuple[Tensor, Tensor]:
    """(the bf16 pieces of the folded matrix in the GEMM's fragment order, shift), kept on the convolution until its weight or one of
    the BatchNorm's four tensors changes (`data_ptr`, `_version`) or `drop_derived_tensors` runs -- the neck's rule: an update through
    `.data` does not move `_version` and needs `drop_derived_tensors`."""
    w = conv.weight
    key = (w.data_ptr(), w._version, w.device) + tuple((t.data_ptr(), t._version) for t in (getattr(bn, n) for n in _BN_TENSORS))
    cached = conv.__dict__.get("_mvs_wmat")
    if cached is None or cached[0] != key:
        with torch.no_grad():
            scale, shift = _affine(bn)
            wsplit = ops.gemm_split_weight(ops.resnet.fold(w, scale))
            shift = shift.contiguous()
        cached = (key, wsplit, shift)
        mark_made(wsplit, shift)
        conv.__dict__["_mvs_wmat"] = cached
    await_made(cached[1], cached[2])
    return cached[1], cached[2]


def _stride(conv) -> int:
    s = conv.stride
    s = tuple(s) if isinstance(s, (tuple, list)) else (s, s)
    if s[0] != s[1]:
        raise ValueError(f"ResNetStages: a convolution with stride {s}")
    return int(s[0])


class _Bottleneck(nn.Module):
    """One block's eight modules, by reference (whoever built them owns them), and its static facts."""

    def __init__(self, conv1, bn1, conv2, bn2, conv3, bn3, down_conv=None, down_bn=None, name="block"):
        super().__init__()
        self.conv1, self.bn1, self.conv2, self.bn2, self.conv3, self.bn3 = conv1, bn1, conv2, bn2, conv3, bn3
        self.down_conv, self.down_bn = down_conv, down_bn
        self.stride = _stride(conv2)
        p, cin, cout = int(conv1.weight.shape[0]), int(conv1.weight.shape[1]), int(conv3.weight.shape[0])
        if tuple(conv1.weight.shape[2:]) != (1, 1) or tuple(conv2.weight.shape) != (p, p, 3, 3) or tuple(conv3.weight.shape[1:]) != (p, 1, 1):
            raise ValueError(f"ResNetStages: {name} is not a bottleneck: conv1 {tuple(conv1.weight.shape)}, conv2 "
                             f"{tuple(conv2.weight.shape)}, conv3 {tuple(conv3.weight.shape)}")
        if self.stride not in ops.resnet.STRIDES or _stride(conv1) != 1 or _stride(conv3) != 1:
            raise ValueError(f"ResNetStages: {name}: the stride must sit on the 3x3 (style='pytorch') and be 1 or 2")
        if down_conv is None:
            if self.stride != 1 or cin != cout:
                raise ValueError(f"ResNetStages: {name} changes the map ({cin} -> {cout} channels, stride {self.stride}) without a "
                                 "downsample branch")
        elif tuple(down_conv.weight.shape) != (cout, cin, 1, 1) or _stride(down_conv) != self.stride:
            raise ValueError(f"ResNetStages: {name}: downsample weight {tuple(down_conv.weight.shape)} with stride {_stride(down_conv)} "
                             f"must be {(cout, cin, 1, 1)} with stride {self.stride}")
        for c in (cin, p, cout):
            if c % ops.resnet.K_STEP:
                raise ValueError(f"ResNetStages: {name} has {c} channels, not divisible by {ops.resnet.K_STEP}")
        for conv in (conv1, conv2, conv3, down_conv):
            if conv is not None and getattr(conv, "bias", None) is not None:
                raise ValueError(f"ResNetStages: {name}: a convolution with a bias")
        self.cin, self.planes, self.cout = cin, p, cout


def _conv_bn_torch(x, conv, bn, stride, padding):
    scale, shift = _affine(bn)
    return F.conv2d(x, conv.weight, None, stride, padding) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)


def _block_torch(x: Tensor, b: _Bottleneck) -> Tensor:
    a = torch.relu(_conv_bn_torch(x, b.conv1, b.bn1, 1, 0))
    a = torch.relu(_conv_bn_torch(a, b.conv2, b.bn2, b.stride, 1))
    c = _conv_bn_torch(a, b.conv3, b.bn3, 1, 0)
    identity = x if b.down_conv is None else _conv_bn_torch(x, b.down_conv, b.down_bn, b.stride, 0)
    return torch.relu(c + identity)


def _block_hip(x: Tensor, b: _Bottleneck, want_inner: bool = False):
    """Three launches, four with the downsample branch; the sum and the last ReLU are the third 1x1's epilogue.  want_inner: (out, a, b),
    the two inner activations as well (what the backward's gates and weight gradients read)."""
    identity = x
    if b.down_conv is not None:
        identity = ops.resnet.conv1x1(x, *_derived(b.down_conv, b.down_bn), b.cout, stride=b.stride, relu=False)
    a = ops.resnet.conv1x1(x, *_derived(b.conv1, b.bn1), b.planes)
    c = ops.resnet.conv3x3(a, *_derived(b.conv2, b.bn2), b.planes, stride=b.stride)
    out = ops.resnet.conv1x1(c, *_derived(b.conv3, b.bn3), b.cout, residual=identity)
    return (out, a, c) if want_inner else out


def _scale(bn) -> Tensor:
    with torch.no_grad():
        return _affine(bn)[0].contiguous()


def _block_backward(ctx, g):
    """The chain of the module's docstring on ops.resnet's gradient kernels.  A GEMM whose result nobody needs is not launched."""
    b = ctx.block
    n_w = 4 if b.down_conv is not None else 3
    saved = ctx.saved_tensors
    x, a, c, out = saved[:4]
    w1, w2, w3 = saved[4:7]
    wd = saved[7] if n_w == 4 else None
    # the frozen affines' scales, made here: the forward's launches are the no_grad route's and no more
    s1, s2, s3 = _scale(b.bn1), _scale(b.bn2), _scale(b.bn3)
    sd = _scale(b.down_bn) if n_w == 4 else None
    need_x, need_w1, need_w2, need_w3 = ctx.needs_input_grad[1:5]
    need_wd = n_w == 4 and ctx.needs_input_grad[5]
    R = ops.resnet

    def rows(dw, scale):
        return dw * scale.view(-1, 1, 1, 1)

    gz = R.relu_gate(g.contiguous(), out)
    d1 = d2 = d3 = dd = dx = None
    if need_w3:
        d3 = rows(R.weight_grad(gz, c, 1, 1), s3)
    need_ga = need_w1 or need_x
    if need_w2 or need_ga:
        gb = R.conv1x1_input_grad(gz, w3, s3, gate=c)
        if need_w2:
            d2 = rows(R.weight_grad(gb, a, 9, b.stride), s2)
        if need_ga:
            ga = R.conv3x3_input_grad(gb, w2, s2, a.shape[2:], b.stride, gate=a)
            if need_w1:
                d1 = rows(R.weight_grad(ga, x, 1, 1), s1)
            if need_x:
                if wd is None:
                    dx = R.conv1x1_input_grad(ga, w1, s1, residual=gz)
                else:
                    dx = R.conv1x1_input_grad(ga, w1, s1, residual=R.conv1x1_input_grad(gz, wd, sd), spread=b.stride)
    if need_wd:
        dd = rows(R.weight_grad(gz, x, 1, b.stride), sd)
    return (None, dx, d1, d2, d3) + ((dd,) if n_w == 4 else ())


class _BottleneckFunction(torch.autograd.Function):
    """One bottleneck as ONE autograd node: forward = `_block_hip` (the bits of the no_grad route), backward = csrc/resnet_bwd.hip.
    Saves x, a, b, out and the convolution weights; the BatchNorm scales are read in the backward (a frozen affine: whoever changes a
    BatchNorm's tensors between a forward and its backward gets the new scale in dW and in W').  Arguments: the block, x, conv1's,
    conv2's and conv3's weight and, with the branch, the downsample convolution's."""

    @staticmethod
    def forward(ctx, block, x, *weights):
        out, a, c = _block_hip(x.detach(), block, want_inner=True)
        ctx.block = block
        ctx.save_for_backward(x, a, c, out, *weights)
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise ValueError("ResNetStages (autograd_route='hip'): double backward (create_graph=True) is not supported: the node is once "
                             "differentiable")
        return _once(ctx, g)


_once = once_differentiable(_block_backward)


def _block_hip_autograd(x: Tensor, b: _Bottleneck, name: str) -> Tensor:
    """`_block_hip` under its own autograd node where the block's input or one of its convolution weights requires grad; the plain
    forward with no node where nothing does.  Refuses (ValueError) what the backward cannot run."""
    convs = [b.conv1, b.conv2, b.conv3] + ([b.down_conv] if b.down_conv is not None else [])
    weights = [m.weight for m in convs]
    wants = [w.requires_grad for w in weights]
    for bn_name in ("bn1", "bn2", "bn3", "down_bn"):
        bn = getattr(b, bn_name)
        if bn is not None and any(p is not None and p.requires_grad for p in (bn.weight, bn.bias)):
            raise ValueError(f"ResNetStages (autograd_route='hip'): {name}.{bn_name} has a trainable weight or bias; the HIP backward treats "
                             "every BatchNorm as a fixed affine and computes no gradient for it: build the backbone with the config's "
                             "norm_cfg=dict(type='BN', requires_grad=False), or call freeze_()")
    if not (x.requires_grad or any(wants)):
        return _block_hip(x, b)
    for m, want, what in zip(convs, wants, ("conv1", "conv2", "conv3", "downsample")):
        o, c = int(m.weight.shape[0]), int(m.weight.shape[1])
        if want and (o % ops.resnet.DW_ROW_BLOCK or c % ops.resnet.DW_COL_BLOCK):
            raise ValueError(f"ResNetStages (autograd_route='hip'): {name}.{what} is trainable with Cout = {o}, C = {c}; the weight-gradient "
                             f"kernel needs Cout % {ops.resnet.DW_ROW_BLOCK} == 0 and C % {ops.resnet.DW_COL_BLOCK} == 0: freeze the layer "
                             "(the config's frozen_stages=1 freezes ResNet-50's 64-row layer 1; freeze_(frozen_stages=...))")
    ops.resnet.check_grad_shapes(x, *weights[:3], weights[3] if len(weights) == 4 else None, b.stride, wants + [False] * (4 - len(wants)))
    return _BottleneckFunction.apply(b, x, *weights)


class ResNetStages(DerivedTensorsMixin, nn.Module):
    """forward(img (N,3,H,W) float32) -> (c2, c3, c4, c5), the outputs of layer1..layer4; forward_from_stem(s) the same from the
    (N,64,H/4,W/4) map behind the max-pool.

    route: "auto" (HIP where it can run, else torch), "torch", or "hip" (raises where it cannot run).

    autograd_route: "torch" (default: the HIP route is forward only; a grad-enabled call where the image or a parameter requires grad
    takes torch's layers, route "hip" raises) or "hip": such a call on CUDA float32 tensors, under route "auto" or "hip", runs the HIP
    kernels forward AND backward, one autograd node per bottleneck that needs one (the module's docstring has the chain and the
    refusals).  The forward's bits are the no_grad HIP route's.  The transposed / flipped weight pieces of the backward are cut per
    call; the forward's kept pieces follow the optimizer's in-place updates through `_version`.

    The module's definition is the frozen affine.  A BatchNorm that is in training mode at call time raises ValueError (the config's
    `norm_eval=True` is what this module implements) on every route; batch statistics are never used.  `train()` / `eval()` on this
    module do not touch the BatchNorm layers' mode: they belong to whoever built them.

    The folded, split weight matrices and the shifts are kept per convolution (94 MB of pieces for ResNet-50) under the key
    (data_ptr, _version) of the weight and the BatchNorm's four tensors, so `with torch.no_grad(): w.mul_(2)` is seen by the next
    call.  A write through `.data` does not move `_version`: call `mvsdet_amd.layers.drop_derived_tensors(module)` after one (mode
    switches and load_state_dict do)."""

    def __init__(self, stem_conv, stem_bn, layers: Sequence[Sequence[_Bottleneck]], route: str = "auto", autograd_route: str = "torch"):
        super().__init__()
        if route not in ROUTES:
            raise ValueError(f"ResNetStages: route {route!r} is not one of {ROUTES}")
        if autograd_route not in AUTOGRAD_ROUTES:
            raise ValueError(f"ResNetStages: autograd_route {autograd_route!r} is not one of {AUTOGRAD_ROUTES}")
        if not layers or any(len(blocks) < 1 for blocks in layers):
            raise ValueError("ResNetStages: every layer needs at least one block")
        self.stem_conv, self.stem_bn = stem_conv, stem_bn
        self.layers = nn.ModuleList([nn.ModuleList(blocks) for blocks in layers])
        c = int(stem_conv.weight.shape[0]) if stem_conv is not None else None
        for li, blocks in enumerate(self.layers):
            for bi, b in enumerate(blocks):
                if c is not None and b.cin != c:
                    raise ValueError(f"ResNetStages: layer{li + 1}.{bi} takes {b.cin} channels, the map before it has {c}")
                c = b.cout
        self.route = route
        self.autograd_route = autograd_route
        self._init_derived_hooks()

    def train(self, mode: bool = True):
        drop_derived_tensors(self)
        self.training = mode
        return self

    # ------------------------------------------------------------------------------------------------- constructors
    @classmethod
    def from_module(cls, backbone, route: str = "auto", autograd_route: str = "torch") -> "ResNetStages":
        """From an object laid out as torchvision's or mmdet's ResNet (duck-typed): `conv1`, `bn1`,
        `layer1..4[i].conv1|bn1|conv2|bn2|conv3|bn3|downsample[0]|downsample[1]`.  Depths, planes and strides are read from what is
        there.  Parameters and buffers are SHARED with `backbone`, not copied."""
        layers = []
        for li in range(1, 5):
            layer = getattr(backbone, f"layer{li}", None)
            if layer is None:
                break
            blocks = []
            for bi, m in enumerate(layer):
                down = getattr(m, "downsample", None)
                blocks.append(_Bottleneck(m.conv1, m.bn1, m.conv2, m.bn2, m.conv3, m.bn3, None if down is None else down[0],
                                          None if down is None else down[1], name=f"layer{li}.{bi}"))
            layers.append(blocks)
        if not layers:
            raise ValueError("ResNetStages.from_module: no `layer1`")
        return cls(backbone.conv1, backbone.bn1, layers, route=route, autograd_route=autograd_route)

    @classmethod
    def from_state_dict(cls, sd: Mapping[str, Tensor], prefix: str = "backbone.", route: str = "auto",
                        strides: Sequence[int] = (1, 2, 2, 2), eps: float = 1e-5, autograd_route: str = "torch") -> "ResNetStages":
        """From a checkpoint with torchvision's keys under `prefix` (copies).  Depths and planes are read from the keys; a state-dict
        holds no strides, so `strides` gives each layer's (the first block's 3x3 and downsample carry it).  `*.num_batches_tracked`
        and `fc.*` are accepted and ignored; a missing key raises KeyError naming it.  Every tensor becomes an nn.Parameter that
        requires grad: `freeze_()` makes of it what the shipped configs train."""
        def key(name):
            k = prefix + name
            if k not in sd:
                raise KeyError(f"ResNetStages.from_state_dict: {k!r} is missing")
            return sd[k].detach().clone().float()

        def conv(name, stride, padding):
            w = key(name + ".weight")
            m = nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], stride=stride, padding=padding, bias=False)
            m.weight = nn.Parameter(w)
            return m

        def bn(name):
            t = {n: key(f"{name}.{n}") for n in _BN_TENSORS}
            m = nn.BatchNorm2d(t["weight"].numel(), eps=eps)
            m.weight, m.bias = nn.Parameter(t["weight"]), nn.Parameter(t["bias"])
            m.running_mean, m.running_var = t["running_mean"], t["running_var"]
            return m.eval()

        layers = []
        for li in range(1, 5):
            if not any(k.startswith(f"{prefix}layer{li}.") for k in sd):
                break
            if li > len(strides):
                raise ValueError(f"ResNetStages.from_state_dict: layer{li} has no entry in strides = {tuple(strides)}")
            blocks, bi = [], 0
            while bi == 0 or any(k.startswith(f"{prefix}layer{li}.{bi}.") for k in sd):
                b, s = f"layer{li}.{bi}", (int(strides[li - 1]) if bi == 0 else 1)
                has_down = any(k.startswith(f"{prefix}{b}.downsample.") for k in sd)
                blocks.append(_Bottleneck(conv(b + ".conv1", 1, 0), bn(b + ".bn1"), conv(b + ".conv2", s, 1), bn(b + ".bn2"),
                                          conv(b + ".conv3", 1, 0), bn(b + ".bn3"), conv(b + ".downsample.0", s, 0) if has_down else None,
                                          bn(b + ".downsample.1") if has_down else None, name=b))
                bi += 1
            layers.append(blocks)
        if not layers:
            raise KeyError(f"ResNetStages.from_state_dict: {prefix + 'layer1.0.conv1.weight'!r} is missing")
        return cls(conv("conv1", 2, 3), bn("bn1"), layers, route=route, autograd_route=autograd_route)

    def freeze_(self, frozen_stages: int = 1, norm: bool = True) -> "ResNetStages":
        """mmdet's ResNet._freeze_stages, in place: frozen_stages >= 0 freezes the stem (its BatchNorm in eval(), requires_grad=False
        on its parameters), frozen_stages = k the layers 1..k as well.  norm=True adds requires_grad=False on the weight and bias of
        EVERY BatchNorm, the config's norm_cfg=dict(type='BN', requires_grad=False).  The defaults are the shipped configs'."""
        frozen_stages = int(frozen_stages)
        if frozen_stages > len(self.layers):
            raise ValueError(f"ResNetStages.freeze_: frozen_stages = {frozen_stages} of {len(self.layers)} layers")
        if frozen_stages >= 0 and self.stem_conv is not None:
            self.stem_bn.eval()
            for m in (self.stem_conv, self.stem_bn):
                for p in m.parameters():
                    p.requires_grad_(False)
        for li in range(max(frozen_stages, 0)):
            for b in self.layers[li]:
                for m in (b.conv1, b.bn1, b.conv2, b.bn2, b.conv3, b.bn3, b.down_conv, b.down_bn):
                    if m is None:
                        continue
                    if isinstance(m, nn.modules.batchnorm._BatchNorm):
                        m.eval()
                    for p in m.parameters():
                        p.requires_grad_(False)
        if norm:
            for _, bn in self._batchnorms():
                for p in bn.parameters():
                    p.requires_grad_(False)
        return self

    # ------------------------------------------------------------------------------------------------- routes
    def _batchnorms(self):
        if self.stem_bn is not None:
            yield "bn1", self.stem_bn
        for li, blocks in enumerate(self.layers):
            for bi, b in enumerate(blocks):
                for name in ("bn1", "bn2", "bn3", "down_bn"):
                    m = getattr(b, name)
                    if m is not None:
                        yield f"layer{li + 1}.{bi}.{name}", m

    def _check_frozen(self):
        for name, m in self._batchnorms():
            if getattr(m, "training", False):
                raise ValueError(f"ResNetStages: {name} is in training mode; this module is the config's norm_eval=True (frozen "
                                 "BatchNorm as a per-channel affine) and never uses batch statistics: put the BatchNorm layers in eval()")

    def _tensors(self) -> List[Tensor]:
        return list(self.parameters()) + list(self.buffers())

    def _wants_grad(self, x: Tensor) -> bool:
        return torch.is_grad_enabled() and any(t.requires_grad for t in [x] + list(self.parameters()))

    def _hip_refusal(self, x: Tensor) -> Optional[str]:
        """Why this call cannot take the HIP route (None: it can)."""
        tensors = [x] + [t for t in self._tensors() if t.is_floating_point()]
        if not all(isinstance(t, Tensor) and t.is_cuda for t in tensors):
            return "the input, the parameters and the buffers must live on a ROCm device"
        if any(t.dtype != torch.float32 for t in tensors):
            return "the input, the parameters and the buffers must be float32"
        if self.autograd_route != "hip" and self._wants_grad(x):
            return "autograd is on and the input or a parameter requires grad (the HIP route is forward only unless autograd_route='hip')"
        return None

    def resolve_route(self, x: Tensor) -> str:
        """"hip" or "torch" for this call; route "hip" raises where the HIP route cannot run."""
        if self.route not in ROUTES:
            raise ValueError(f"ResNetStages: route {self.route!r} is not one of {ROUTES}")
        if self.autograd_route not in AUTOGRAD_ROUTES:
            raise ValueError(f"ResNetStages: autograd_route {self.autograd_route!r} is not one of {AUTOGRAD_ROUTES}")
        if self.route == "torch":
            return "torch"
        why = self._hip_refusal(x)
        if why is None:
            return "hip" if self.route == "hip" else AUTO_ON_CUDA
        if self.route == "hip":
            raise RuntimeError(f"ResNetStages (route='hip'): {why}")
        return "torch"

    # ------------------------------------------------------------------------------------------------- forward
    def stem(self, img: Tensor) -> Tensor:
        """conv 7x7 / affine / ReLU / max-pool on torch's layers (both routes)."""
        if self.stem_conv is None:
            raise ValueError("ResNetStages: built without a stem")
        conv = self.stem_conv
        y = _conv_bn_torch(img, conv, self.stem_bn, conv.stride, conv.padding)
        return F.max_pool2d(torch.relu(y), kernel_size=3, stride=2, padding=1)

    def _check_input(self, x: Tensor, channels: int, what: str):
        if not isinstance(x, Tensor) or x.dim() != 4 or x.shape[1] != channels:
            raise ValueError(f"ResNetStages: {what} must be an (N,{channels},H,W) tensor")
        if x.dtype != torch.float32:
            raise TypeError(f"ResNetStages: {what} must be torch.float32 (got {x.dtype})")
        if min(x.shape) < 1:
            raise ValueError(f"ResNetStages: {what} {tuple(x.shape)} is empty")

    def _stages(self, s: Tensor, route: str, autograd: bool = False) -> Tuple[Tensor, ...]:
        """autograd (route "hip" alone): every block whose input or convolution weights require grad under its own autograd node."""
        block = _block_hip if route == "hip" else _block_torch
        outs = []
        for li, blocks in enumerate(self.layers):
            for bi, b in enumerate(blocks):
                s = _block_hip_autograd(s, b, f"layer{li + 1}.{bi}") if autograd else block(s, b)
            outs.append(s)
        return tuple(outs)

    def forward_from_stem(self, s: Tensor) -> Tuple[Tensor, ...]:
        self._check_input(s, self.layers[0][0].cin, "the stem's map")
        self._check_frozen()
        route = self.resolve_route(s)
        return self._stages(s, route, autograd=route == "hip" and self._wants_grad(s))

    def forward(self, img: Tensor) -> Tuple[Tensor, ...]:
        if self.stem_conv is None:
            raise ValueError("ResNetStages: built without a stem")
        self._check_input(img, int(self.stem_conv.weight.shape[1]), "img")
        self._check_frozen()
        route = self.resolve_route(img)
        if route == "hip" and self._wants_grad(img):                    # autograd_route "hip": the stem is torch's graph in front of the nodes
            return self._stages(self.stem(img), route, autograd=True)
        if route == "hip":
            with torch.no_grad():
                return self._stages(self.stem(img), route)
        return self._stages(self.stem(img), route)
