"""Gaussian head (csrc/gshead.hip): `to_gaussians` = nn.Sequential(ReLU, Linear) of the novel-view branch (mvsdet.py:210-216) on the
rows extract_feat concatenates per source pixel (:561-569) and the quarter-size image of process_rgb_raw (:319-333), read in place.

The names live in this module only (`ops.gshead.<name>`); they are not re-exported by the package.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from ._common import _NS, _lib, req, stream, to_device


def _unit_w(t: Tensor) -> Tensor:
    """The tensor itself where the kernels can walk it (unit stride along the last axis, no negative stride), else a copy."""
    return t if t.stride(-1) == 1 and min(t.stride()) >= 0 else t.contiguous()


def _depth_map(depth_coding: Tensor) -> Tensor:
    return depth_coding[:, 0] if depth_coding.dim() == 4 else depth_coding


def check_shapes(name: str, feature: Tensor, depth_coding: Tensor, n_ids: int, weight: Tensor, bias: Optional[Tensor], h: int, w: int,
                 rgb_raw: Optional[Tensor], images: Optional[Tensor], num_surfaces: int = 1) -> Tuple[int, int, int, int, int, int]:
    """Every refusal that needs no device: ValueError -> (N, V, C, K, M, R).  Runs before anything is launched (and before the
    tensors' devices are looked at, so it can be exercised without a GPU)."""
    if feature.dim() != 4:
        raise ValueError(f"{name}: feature {tuple(feature.shape)} must be (N,C,Hf,Wf)")
    N, C, Hf, Wf = feature.shape
    h, w, V = int(h), int(w), int(n_ids)
    if not (1 <= h <= Hf and 1 <= w <= Wf):
        raise ValueError(f"{name}: the map {h} x {w} must lie inside the feature map {Hf} x {Wf}")
    if tuple(depth_coding.shape) not in ((N, 1, h, w), (N, h, w)):
        raise ValueError(f"{name}: depth_coding {tuple(depth_coding.shape)} must be {(N, 1, h, w)} or {(N, h, w)}")
    if not 1 <= V <= 65535:
        raise ValueError(f"{name}: {V} source views (1 .. 65535)")
    if rgb_raw is not None and images is not None:
        raise ValueError(f"{name}: rgb comes as rows (rgb_raw) or as images (denorm_images), not both")
    if weight.dim() != 2 or (bias is not None and tuple(bias.shape) != (weight.shape[0],)):
        raise ValueError(f"{name}: weight {tuple(weight.shape)} and bias {None if bias is None else tuple(bias.shape)} must be (M,K) and (M)")
    M, K = weight.shape
    want = C + (1 if rgb_raw is None and images is None else 4)
    if K != want:
        raise ValueError(f"{name}: K = {K} columns of weight, but the rows have C + {want - C} = {want} entries "
                         f"({C} feature channels, depth_coding{'' if want == C + 1 else ', rgb'})")
    if int(num_surfaces) < 1 or M % int(num_surfaces):
        raise ValueError(f"{name}: M = {M} outputs are not divisible by num_surfaces = {num_surfaces}")
    R = h * w
    if rgb_raw is not None and tuple(rgb_raw.shape) not in ((V, R, 3), (1, V, R, 3)):
        raise ValueError(f"{name}: rgb_raw {tuple(rgb_raw.shape)} must be {(V, R, 3)} or {(1, V, R, 3)}")
    if images is not None:
        if images.dim() != 4 or images.shape[0] != N or images.shape[1] != 3 or images.shape[2] < 4 * h - 1 or images.shape[3] < 4 * w - 1:
            raise ValueError(f"{name}: denorm_images {tuple(images.shape)} must be ({N},3,Hi,Wi) with Hi >= {4 * h - 1}, Wi >= {4 * w - 1} "
                             "(only ratio 4)")
    if V * R * M >= 2 ** 40:
        raise ValueError(f"{name}: V R M = {V * R * M} outputs exceed 2^40")
    return N, V, C, K, M, R


def device_ids(name: str, ids: Union[Tensor, Sequence[int]], N: int, dev) -> Tensor:
    """ids as an int64 device tensor.  Host data (a sequence or a CPU tensor, what `render_source_ids` returns) is checked here:
    inside [0, N) and unique -> ValueError.  A device tensor is taken as it is (no synchronisation): the kernels never use an id
    outside [0, N) as an address; such a view's output is NaN."""
    if isinstance(ids, Tensor) and ids.is_cuda:
        if ids.dtype != torch.int64 or ids.dim() != 1:
            raise TypeError(f"{name}: ids must be a 1-D int64 tensor (got {ids.dtype}, shape {tuple(ids.shape)})")
        return ids.contiguous()
    host = torch.as_tensor(ids).reshape(-1)
    if host.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"{name}: ids must be integers (got {host.dtype})")
    host = host.to(torch.int64)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= N):
        raise ValueError(f"{name}: ids {host.tolist()} outside [0, {N})")
    if torch.unique(host).numel() != host.numel():
        raise ValueError(f"{name}: ids {host.tolist()} are not unique")
    return to_device(host, dev)


def _prepare(name: str, feature: Tensor, depth_coding: Tensor, ids: Tensor, weight: Tensor, bias: Optional[Tensor], h: int, w: int,
             rgb_raw: Optional[Tensor], images: Optional[Tensor]):
    N, V, C, K, M, R = check_shapes(name, feature, depth_coding, ids.numel(), weight, bias, h, w, rgb_raw, images)
    req(feature, "feature", dim=4)
    req(depth_coding, "depth_coding")
    req(ids, "ids", dtype=torch.int64, dim=1)
    req(weight, "weight", dim=2)
    if bias is not None:
        req(bias, "bias", dim=1)
    if rgb_raw is not None:
        req(rgb_raw, "rgb_raw")
        rgb_raw = rgb_raw.contiguous()
    if images is not None:
        req(images, "denorm_images", dim=4)
        images = _unit_w(images)
    feature, depth = _unit_w(feature), _unit_w(_depth_map(depth_coding))
    return (N, V, C, K, M, R), feature, depth, ids.contiguous(), weight.contiguous(), None if bias is None else bias.contiguous(), rgb_raw, images


def _image_args(images: Optional[Tensor]):
    if images is None:
        return None, None, 0, 0
    return _lib.ptr(images), _lib.strides(images, 3), int(images.shape[2]), int(images.shape[3])


def forward_into(feature: Tensor, depth_coding: Tensor, ids: Tensor, weight: Tensor, bias: Tensor, h: int, w: int, raw: Tensor,
                 rgb_raw: Optional[Tensor] = None, images: Optional[Tensor] = None) -> None:
    """The forward launch into the caller's contiguous raw (V,R,M) (or (V,R,S,M/S)): what `gaussian_head` does after allocating it."""
    (N, V, C, K, M, R), feature, depth, ids, weight, bias, rgb_raw, images = _prepare("gaussian_head", feature, depth_coding, ids, weight, bias,
                                                                                      h, w, rgb_raw, images)
    req(raw, "raw")
    if raw.numel() != V * R * M or not raw.is_contiguous():
        raise ValueError(f"gaussian_head: raw {tuple(raw.shape)} must be contiguous with {V * R * M} floats")
    img, img_strides, Hi, Wi = _image_args(images)
    with torch.cuda.device(feature.device):
        _lib.check(_lib.load().mvsdet_gshead_forward_f32(
            _lib.ptr(feature), _lib.strides(feature, 3), _lib.ptr(depth), _lib.strides(depth, 2), _lib.ptr(rgb_raw), img, img_strides,
            ids.data_ptr(), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(raw), N, V, C, K, M, int(h), int(w), int(feature.shape[2]),
            int(feature.shape[3]), Hi, Wi, stream(feature)), "gaussian_head")


def partial_floats(V: int, R: int, M: int, K: int, chunk_pixels: int = 0) -> int:
    """Floats of the weight gradient's chunk sums (mvsdet_gshead_partial_bytes)."""
    nbytes = int(_lib.load().mvsdet_gshead_partial_bytes(int(V), int(R), int(M), int(K), int(chunk_pixels)))
    if nbytes == 0:
        raise ValueError(f"gaussian_head_backward: no partial size for V={V} R={R} M={M} K={K} chunk_pixels={chunk_pixels}")
    return nbytes // 4


def backward_into(feature: Tensor, depth_coding: Tensor, ids: Tensor, weight: Tensor, g: Tensor, h: int, w: int,
                  g_feature: Optional[Tensor], g_depth_coding: Optional[Tensor], g_weight: Optional[Tensor], g_bias: Optional[Tensor],
                  rgb_raw: Optional[Tensor] = None, images: Optional[Tensor] = None, chunk_pixels: int = 0,
                  partial: Optional[Tensor] = None) -> None:
    """The backward launches into the caller's buffers.  g (V,R,M) or (V,R,S,M/S).  g_feature (in feature's shape) and g_depth_coding
    (in depth_coding's shape), both or neither, unit stride along w: the selected views' cropped pixels are written, NOTHING else
    (the caller zeroes them).  g_weight (M,K) and g_bias (M), contiguous, both or neither; partial: `partial_floats` floats (allocated
    here if None)."""
    (N, V, C, K, M, R), feature, depth, ids, weight, _, rgb_raw, images = _prepare("gaussian_head_backward", feature, depth_coding, ids, weight,
                                                                                   None, h, w, rgb_raw, images)
    req(g, "g")
    if g.numel() != V * R * M or tuple(g.shape[:2]) != (V, R):
        raise ValueError(f"gaussian_head_backward: g {tuple(g.shape)} must be ({V},{R},{M}) or ({V},{R},S,{M}/S)")
    g = g.contiguous()
    if (g_feature is None) != (g_depth_coding is None) or (g_weight is None) != (g_bias is None):
        raise ValueError("gaussian_head_backward: g_feature and g_depth_coding come as a pair, and so do g_weight and g_bias")
    lib = _lib.load()
    with torch.cuda.device(feature.device):
        if g_feature is not None:
            req(g_feature, "g_feature", dim=4)
            req(g_depth_coding, "g_depth_coding")
            gd = _depth_map(g_depth_coding)
            if (tuple(g_feature.shape) != tuple(feature.shape) or tuple(g_depth_coding.shape) != tuple(depth_coding.shape)
                    or _unit_w(g_feature) is not g_feature or _unit_w(gd) is not gd):
                raise ValueError(f"gaussian_head_backward: g_feature {tuple(g_feature.shape)} / g_depth_coding {tuple(g_depth_coding.shape)} "
                                 "must have the inputs' shapes and unit stride along w")
            _lib.check(lib.mvsdet_gshead_backward_input_f32(
                _lib.ptr(feature), _lib.strides(feature, 3), _lib.ptr(depth), _lib.strides(depth, 2), ids.data_ptr(), _lib.ptr(weight),
                _lib.ptr(g), _lib.ptr(g_feature), _lib.strides(g_feature, 3), _lib.ptr(gd), _lib.strides(gd, 2), N, V, C, K, M, int(h),
                int(w), int(feature.shape[2]), int(feature.shape[3]), stream(feature)), "gaussian_head_backward")
        if g_weight is not None:
            req(g_weight, "g_weight", dim=2)
            req(g_bias, "g_bias", dim=1)
            if tuple(g_weight.shape) != (M, K) or tuple(g_bias.shape) != (M,) or not g_weight.is_contiguous() or not g_bias.is_contiguous():
                raise ValueError(f"gaussian_head_backward: g_weight {tuple(g_weight.shape)} and g_bias {tuple(g_bias.shape)} must be contiguous "
                                 f"({M},{K}) and ({M})")
            need = partial_floats(V, R, M, K, chunk_pixels)
            if partial is None:
                partial = torch.empty(need, dtype=torch.float32, device=feature.device)
            req(partial, "partial")
            if not partial.is_contiguous():
                raise ValueError("gaussian_head_backward: partial must be contiguous")
            img, img_strides, Hi, Wi = _image_args(images)
            _lib.check(lib.mvsdet_gshead_backward_weight_f32(
                _lib.ptr(feature), _lib.strides(feature, 3), _lib.ptr(depth), _lib.strides(depth, 2), _lib.ptr(rgb_raw), img, img_strides,
                ids.data_ptr(), _lib.ptr(g), _lib.ptr(g_weight), _lib.ptr(g_bias), _lib.ptr(partial), partial.numel() * 4, int(chunk_pixels),
                N, V, C, K, M, int(h), int(w), int(feature.shape[2]), int(feature.shape[3]), Hi, Wi, stream(feature)),
                "gaussian_head_backward")


# ------------------------------------------------------------------------------------------- the operator
@torch.library.custom_op(f"{_NS}::gshead_forward", mutates_args=(), device_types="cuda")
def _gshead_forward(feature: Tensor, depth_coding: Tensor, ids: Tensor, weight: Tensor, bias: Tensor, h: int, w: int,
                    rgb_raw: Optional[Tensor], images: Optional[Tensor], chunk_pixels: int) -> Tensor:
    raw = torch.empty((ids.numel(), h * w, weight.shape[0]), dtype=torch.float32, device=feature.device)
    forward_into(feature, depth_coding, ids, weight, bias, h, w, raw, rgb_raw, images)
    return raw


@_gshead_forward.register_fake
def _(feature, depth_coding, ids, weight, bias, h, w, rgb_raw, images, chunk_pixels):
    return feature.new_empty((ids.shape[0], h * w, weight.shape[0]))


@torch.library.custom_op(f"{_NS}::gshead_backward", mutates_args=(), device_types="cuda")
def gaussian_head_backward(feature: Tensor, depth_coding: Tensor, ids: Tensor, weight: Tensor, g: Tensor, h: int, w: int,
                           rgb_raw: Optional[Tensor], images: Optional[Tensor], chunk_pixels: int, need_input: bool,
                           need_weight: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Gradients of `gaussian_head` from g (V,R,M) -> (g_feature, g_depth_coding, g_weight (M,K), g_bias (M)); g_feature and
    g_depth_coding in the inputs' shapes, exactly zero outside the selected views' cropped pixels.  A pair that is not needed comes back
    as empty tensors.  Three launches (input gradient; weight gradient and the fixed-order sum of its chunks) and the zero fill."""
    dev = feature.device
    g_feature = torch.zeros(tuple(feature.shape) if need_input else (0,), dtype=torch.float32, device=dev)
    g_depth = torch.zeros(tuple(depth_coding.shape) if need_input else (0,), dtype=torch.float32, device=dev)
    g_weight = torch.empty(tuple(weight.shape) if need_weight else (0,), dtype=torch.float32, device=dev)
    g_bias = torch.empty((weight.shape[0] if need_weight else 0,), dtype=torch.float32, device=dev)
    backward_into(feature, depth_coding, ids, weight, g, h, w, g_feature if need_input else None, g_depth if need_input else None,
                  g_weight if need_weight else None, g_bias if need_weight else None, rgb_raw, images, chunk_pixels)
    return g_feature, g_depth, g_weight, g_bias


@gaussian_head_backward.register_fake
def _(feature, depth_coding, ids, weight, g, h, w, rgb_raw, images, chunk_pixels, need_input, need_weight):
    return (feature.new_empty(tuple(feature.shape) if need_input else (0,)), feature.new_empty(tuple(depth_coding.shape) if need_input else (0,)),
            feature.new_empty(tuple(weight.shape) if need_weight else (0,)), feature.new_empty((weight.shape[0] if need_weight else 0,)))


def _gh_setup(ctx, inputs, output):
    feature, depth_coding, ids, weight, bias, h, w, rgb_raw, images, chunk_pixels = inputs
    for t, name in ((rgb_raw, "rgb_raw"), (images, "denorm_images")):
        if t is not None and t.requires_grad:
            raise RuntimeError(f"gaussian_head: {name} carries no gradient here; detach it")
    ctx.save_for_backward(feature, depth_coding, ids, weight, rgb_raw, images)
    ctx.args = (h, w, chunk_pixels)


def _gh_bwd(ctx, g):
    feature, depth_coding, ids, weight, rgb_raw, images = ctx.saved_tensors
    h, w, chunk_pixels = ctx.args
    need_input = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    need_weight = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
    if g is None or not (need_input or need_weight):
        return (None,) * 10
    gf, gd, gw, gb = gaussian_head_backward(feature, depth_coding, ids, weight, g, h, w, rgb_raw, images, chunk_pixels, need_input, need_weight)
    return (gf if need_input else None, gd if need_input else None, None, gw if need_weight else None, gb if need_weight else None,
            None, None, None, None, None)


_gshead_forward.register_autograd(_gh_bwd, setup_context=_gh_setup)
_gshead_forward.register_autocast("cuda", torch.float32)


def gaussian_head(feature: Tensor, depth_coding: Tensor, ids: Union[Tensor, Sequence[int]], weight: Tensor, bias: Tensor, h: int, w: int,
                  num_surfaces: int = 1, rgb_raw: Optional[Tensor] = None, images: Optional[Tensor] = None,
                  chunk_pixels: int = 0) -> Tensor:
    """feature (N,C,Hf,Wf) (any strides with unit stride along w), depth_coding (N,1,h,w) or (N,h,w), ids (V) the chosen views (host
    data is checked: inside [0, N), unique; a device tensor is trusted), weight (M,K) and bias (M) of the nn.Linear, the map size
    h <= Hf, w <= Wf; rgb either as rows rgb_raw (V,R,3) or as denormalised images (N,3,Hi,Wi) of four times the map's size (K = C + 4)
    or not at all (K = C + 1) -> raw (V, R = h w, S, M / S): bias + weight relu(row), what `ops.adapter.pixel_gaussians` takes.  One
    launch, and three for the backward; no row matrix, no atomics, no host synchronisation.  Differentiable in feature, depth_coding,
    weight and bias; the rgb inputs carry no gradient.  chunk_pixels: pixels per partial sum of the weight gradient (0: 256)."""
    N = feature.shape[0] if feature.dim() == 4 else 0
    n_ids = ids.numel() if isinstance(ids, Tensor) else len(ids)
    check_shapes("gaussian_head", feature, depth_coding, n_ids, weight, bias, h, w, rgb_raw, images, num_surfaces)
    ids = device_ids("gaussian_head", ids, N, feature.device)
    if rgb_raw is not None and rgb_raw.dim() == 4:
        rgb_raw = rgb_raw[0]
    raw = _gshead_forward(feature, depth_coding, ids, weight, bias, int(h), int(w), rgb_raw, images, int(chunk_pixels))
    S = int(num_surfaces)
    return raw.reshape(raw.shape[0], raw.shape[1], S, raw.shape[2] // S)


def process_rgb_raw_rows(images: Tensor, ids: Union[Tensor, Sequence[int]], h: int, w: int) -> Tensor:
    """images (N,3,Hi,Wi), Hi >= 4h - 1, Wi >= 4w - 1 -> (V, h w, 3): the quarter-size image of the chosen views cropped to h x w, pixel
    (y, x) = 0.25 ((I[4y+1][4x+1] + I[4y+1][4x+2]) + (I[4y+2][4x+1] + I[4y+2][4x+2])) -- F.interpolate(scale_factor=0.25,
    mode='bilinear') and the crop of process_rgb_raw (mvsdet.py:319-333).  One launch; no gradient."""
    h, w = int(h), int(w)
    if images.dim() != 4 or images.shape[1] != 3 or h < 1 or w < 1 or images.shape[2] < 4 * h - 1 or images.shape[3] < 4 * w - 1:
        raise ValueError(f"process_rgb_raw: images {tuple(images.shape)} must be (N,3,Hi,Wi) with Hi >= {4 * h - 1}, Wi >= {4 * w - 1} "
                         "(only ratio 4)")
    ids = device_ids("process_rgb_raw", ids, images.shape[0], images.device)
    req(images, "images", dim=4)
    images = _unit_w(images.detach())
    rows = torch.empty((ids.numel(), h * w, 3), dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        _lib.check(_lib.load().mvsdet_gshead_rgb_rows_f32(_lib.ptr(images), _lib.strides(images, 3), ids.data_ptr(), _lib.ptr(rows),
                                                          int(images.shape[0]), int(ids.numel()), h, w, int(images.shape[2]),
                                                          int(images.shape[3]), stream(images)), "process_rgb_raw")
    return rows
