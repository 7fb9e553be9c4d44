"""PyTorch-ROCm custom operators over the C ABI (torch.ops.mvsdet_amd.*).

Every operator enqueues hand-written gfx950 kernels of libmvsdet_hip.so on the current HIP stream
through ctypes; torch supplies device memory, streams and autograd plumbing only.  Operators raise if
their inputs are not float32 tensors on a ROCm device -- there is no CPU implementation here.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import _lib

_NS = "mvsdet_amd"


def _req(t: Tensor, name: str, dtype=torch.float32, dim=None):
    if not t.is_cuda:
        raise RuntimeError(f"mvsdet_amd: `{name}` must live on a ROCm device (got {t.device}); "
                           "this package has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"mvsdet_amd: `{name}` must be {dtype} (got {t.dtype})")
    if dim is not None and t.dim() != dim:
        raise ValueError(f"mvsdet_amd: `{name}` must be {dim}-D (got shape {tuple(t.shape)})")


def _stream(t: Tensor):
    return _lib.current_stream(t.device)


# ------------------------------------------------------------------------------------------- pack
@torch.library.custom_op(f"{_NS}::pack_features", mutates_args=(), device_types="cuda")
def pack_features(feat: Tensor) -> Tensor:
    """(N,C,H,W) float32 or float16 (any strides) -> packed channel-last maps, flat float32
    (see include/mvsdet_hip.h; the fp16 -> fp32 conversion is exact)."""
    half = feat.dtype == torch.float16
    _req(feat, "feat", dtype=torch.float16 if half else torch.float32, dim=4)
    N, C, H, W = feat.shape
    lib = _lib.load()
    out = torch.empty(lib.mvsdet_packed_bytes(N, C, H, W) // 4, dtype=torch.float32, device=feat.device)
    fn = lib.mvsdet_pack_features_f16 if half else lib.mvsdet_pack_features_f32
    with torch.cuda.device(feat.device):
        _lib.check(fn(_lib.ptr(feat), _lib.strides4(feat), _lib.ptr(out), N, C, H, W, _stream(feat)), "pack_features")
    return out


@pack_features.register_fake
def _(feat):
    N, C, H, W = feat.shape
    return feat.new_empty(N * H * W * 32 * ((C + 31) // 32), dtype=torch.float32)


# ------------------------------------------------------------------------------------------- a3
@torch.library.custom_op(f"{_NS}::homo_warp", mutates_args=(), device_types="cuda")
def homo_warp(src: Tensor, proj: Tensor, depth: Tensor) -> Tensor:
    """a3 (mvs_models/module.py:105): src (B,C,H,W), proj (B,4,4) = src_proj @ inv(ref_proj), depth (B,D)."""
    _req(src, "src", dim=4)
    _req(proj, "proj", dim=3)
    _req(depth, "depth", dim=2)
    B, C, H, W = src.shape
    D = depth.shape[1]
    if proj.shape != (B, 4, 4) or depth.shape[0] != B:
        raise ValueError(f"homo_warp: proj {tuple(proj.shape)} / depth {tuple(depth.shape)} do not match B={B}")
    src, proj, depth = src.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((B, C, D, H, W), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().mvsdet_homo_warp_f32(_lib.ptr(src), _lib.ptr(proj), _lib.ptr(depth), _lib.ptr(out),
                                                    B, C, D, H, W, _stream(src)), "homo_warp")
    return out


@homo_warp.register_fake
def _(src, proj, depth):
    B, C, H, W = src.shape
    return src.new_empty((B, C, depth.shape[1], H, W))


# ------------------------------------------------------------------------------------------- a3+a4
def _ray_depth_launch(intr: Tensor, est_depth: Optional[Tensor], h: int, w: int):
    """The kernel launch of `ray_depth` -> depth_scale (N,h*w,1), est_ray_depth (N,J,h*w) or None."""
    _req(intr, "intr", dim=2)
    N = intr.shape[0]
    intr = intr.contiguous()
    scale = torch.empty((N, h * w, 1), dtype=torch.float32, device=intr.device)
    ray = None
    J, H, W = 0, h, w
    if est_depth is not None:
        _req(est_depth, "est_depth", dim=4)
        if est_depth.shape[0] != N:
            raise ValueError("ray_depth: est_depth and intr disagree on the number of views")
        est_depth = est_depth.contiguous()
        J, H, W = est_depth.shape[1:]
        ray = torch.empty((N, J, h * w), dtype=torch.float32, device=intr.device)
    with torch.cuda.device(intr.device):
        _lib.check(_lib.load().mvsdet_ray_depth_f32(_lib.ptr(intr), _lib.ptr(est_depth), _lib.ptr(scale), _lib.ptr(ray), N, J, H, W,
                                                    h, w, _stream(intr)), "ray_depth")
    return scale, ray


class _RayDepthGrad(torch.autograd.Function):
    """est_ray_depth under autograd: the forward is the same launch as the no-grad path; the backward is that of the
    reference's `est_depth / (scale + 1e-8)` (mvsdet.py:494): g / (scale + 1e-8) on the cropped (h, w) window of est_depth,
    zero on its padding.  depth_scale depends on the intrinsics alone and carries no gradient."""

    @staticmethod
    def forward(ctx, est_depth, intr, h, w):
        scale, ray = _ray_depth_launch(intr, est_depth, h, w)
        ctx.mark_non_differentiable(scale)
        ctx.save_for_backward(scale)
        ctx.geometry = (tuple(est_depth.shape), h, w)
        return scale, ray

    @staticmethod
    def backward(ctx, g_scale, g_ray):
        (scale,) = ctx.saved_tensors
        (N, J, H, W), h, w = ctx.geometry
        grad = g_ray.new_zeros((N, J, H, W))
        grad[:, :, :h, :w] = (g_ray / (scale.view(N, 1, h * w) + 1e-8)).view(N, J, h, w)
        return grad, None, None, None


def ray_depth(intr: Tensor, est_depth: Optional[Tensor], h: int, w: int):
    """mvsdet.py:1158-1216 + :494: intr (N,5) {fx,fy,cx,cy,skew} at feature level -> depth_scale (N,h*w,1) and, when
    est_depth (N,J,H,W) is given, est_ray_depth (N,h*w,1,J) in the layout extract_feat hands to the Gaussian adapter.
    Differentiable in est_depth only (when it requires grad): d est_ray_depth / d est_depth = 1 / (depth_scale + 1e-8) on
    the (h, w) window, 0 on the padding, as the reference's division; depth_scale and the intrinsics carry no gradient.
    The forward values are those of the no-grad path, bit for bit (the same launch)."""
    if est_depth is not None and est_depth.requires_grad and torch.is_grad_enabled():
        scale, ray = _RayDepthGrad.apply(est_depth, intr, h, w)
    else:
        scale, ray = _ray_depth_launch(intr, est_depth, h, w)
    return scale, (None if ray is None else ray.transpose(2, 1).unsqueeze(2))


def validate_neighbors(nbr: Tensor, n_src: int) -> None:
    """Host check of neighbour view ids (include/mvsdet_hip.h: mvsdet_validate_neighbors): the reference's index gather
    (mvsdet.py:440) raises on an id outside [0, N); the kernels only clamp.  `nbr` must be a CPU tensor."""
    if nbr.device.type != "cpu":
        raise ValueError("validate_neighbors: the ids are checked on their host copy")
    t = nbr.to(torch.int64).contiguous()
    m, k = (t.shape[0], t.shape[1]) if t.dim() == 2 else (t.numel(), 1)
    p = ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int64)) if t.numel() else None
    _lib.check(_lib.load().mvsdet_validate_neighbors(p, int(m), int(k), int(n_src)), "validate_neighbors")


def _check_sweep(feat, nbr, proj, depth):
    _req(feat, "feat", dim=4)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    _req(proj, "proj", dim=4)
    _req(depth, "depth", dim=2)
    N, C, H, W = feat.shape
    K = nbr.shape[1]
    if nbr.shape[0] != N or proj.shape != (N, K, 4, 4) or depth.shape[0] != N:
        raise ValueError(f"plane_sweep_variance: nbr {tuple(nbr.shape)}, proj {tuple(proj.shape)}, depth "
                         f"{tuple(depth.shape)} do not match N={N}")
    return N, K, C, depth.shape[1], H, W


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_packed", mutates_args=(), device_types="cuda")
def plane_sweep_variance_packed(packed: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, C: int, H: int,
                                W: int) -> Tensor:
    """a3+a4 on already packed maps (mvsdet.py:439-467) -> (N,C,D,H,W)."""
    _req(packed, "packed", dim=1)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    _req(proj, "proj", dim=4)
    _req(depth, "depth", dim=2)
    N, K = nbr.shape
    D = depth.shape[1]
    lib = _lib.load()
    if packed.numel() * 4 != lib.mvsdet_packed_bytes(N, C, H, W):
        raise ValueError("plane_sweep_variance_packed: packed buffer does not match (N,C,H,W)")
    if proj.shape != (N, K, 4, 4) or depth.shape[0] != N:
        raise ValueError("plane_sweep_variance_packed: proj/depth shape mismatch")
    nbr, proj, depth = nbr.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=packed.device)
    # channel-independent sampling table (8 B per view, neighbour, plane, pixel), built by the op's first kernel
    sbytes = lib.mvsdet_plane_sweep_scratch_bytes(N, K, D, H, W)
    scratch = torch.empty(max(sbytes // 4, 4), dtype=torch.float32, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(lib.mvsdet_plane_sweep_variance_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj),
                                                              _lib.ptr(depth), _lib.ptr(out), _lib.ptr(scratch), sbytes,
                                                              N, K, C, D, H, W, _stream(packed)),
                   "plane_sweep_variance_packed")
    return out


@plane_sweep_variance_packed.register_fake
def _(packed, nbr, proj, depth, C, H, W):
    return packed.new_empty((nbr.shape[0], C, depth.shape[1], H, W))


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_shard", mutates_args=(), device_types="cuda")
def plane_sweep_variance_shard(packed: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, n_src: int, ref_first: int,
                               C: int, H: int, W: int, half_out: bool = False) -> Tensor:
    """a3+a4 for the reference views ref_first .. ref_first+M-1 of a scene whose n_src views are all in `packed`
    (intra-scene view sharding).  nbr (M,K) holds global view ids -> (M,C,D,H,W), bit-identical to the
    same rows of plane_sweep_variance_packed.  half_out=True stores the same fp32 result rounded to float16
    (BASELINE configs[4]).  Forward only."""
    _req(packed, "packed", dim=1)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    _req(proj, "proj", dim=4)
    _req(depth, "depth", dim=2)
    M, K = nbr.shape
    D = depth.shape[1]
    lib = _lib.load()
    if packed.numel() * 4 != lib.mvsdet_packed_bytes(n_src, C, H, W):
        raise ValueError("plane_sweep_variance_shard: packed buffer does not match (n_src,C,H,W)")
    if proj.shape != (M, K, 4, 4) or depth.shape[0] != M:
        raise ValueError("plane_sweep_variance_shard: proj/depth shape mismatch")
    if M < 1 or ref_first < 0 or ref_first + M > n_src:
        raise ValueError(f"plane_sweep_variance_shard: views [{ref_first},{ref_first + M}) outside the {n_src} packed views")
    nbr, proj, depth = nbr.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((M, C, D, H, W), dtype=torch.float16 if half_out else torch.float32, device=packed.device)
    sbytes = lib.mvsdet_plane_sweep_scratch_bytes(M, K, D, H, W)
    scratch = torch.empty(max(sbytes // 4, 4), dtype=torch.float32, device=packed.device)
    fn = lib.mvsdet_plane_sweep_variance_shard_f16 if half_out else lib.mvsdet_plane_sweep_variance_shard_f32
    with torch.cuda.device(packed.device):
        _lib.check(fn(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj),
                      _lib.ptr(depth), _lib.ptr(out), _lib.ptr(scratch), sbytes,
                      n_src, ref_first, M, K, C, D, H, W, _stream(packed)),
                   "plane_sweep_variance_shard")
    return out


@plane_sweep_variance_shard.register_fake
def _(packed, nbr, proj, depth, n_src, ref_first, C, H, W, half_out=False):
    return packed.new_empty((nbr.shape[0], C, depth.shape[1], H, W), dtype=torch.float16 if half_out else torch.float32)


@torch.library.custom_op(f"{_NS}::plane_sweep_table", mutates_args=(), device_types="cuda")
def plane_sweep_table(proj: Tensor, depth: Tensor, H: int, W: int) -> Tensor:
    """Channel-independent sampling table of a scene (8 B per view, neighbour, plane, pixel): proj (N,K,4,4),
    depth (N,D) -> opaque flat buffer for plane_sweep_variance_tabled."""
    _req(proj, "proj", dim=4)
    _req(depth, "depth", dim=2)
    N, K = proj.shape[:2]
    D = depth.shape[1]
    lib = _lib.load()
    sbytes = lib.mvsdet_plane_sweep_scratch_bytes(N, K, D, H, W)
    table = torch.empty(max(sbytes // 4, 4), dtype=torch.float32, device=proj.device)
    proj, depth = proj.contiguous(), depth.contiguous()
    with torch.cuda.device(proj.device):
        _lib.check(lib.mvsdet_plane_sweep_table_f32(_lib.ptr(proj), _lib.ptr(depth), _lib.ptr(table), sbytes, N, K, D, H, W,
                                                    _stream(proj)), "plane_sweep_table")
    return table


@plane_sweep_table.register_fake
def _(proj, depth, H, W):
    # same size as the real op: the scratch-size query is a host-only function of the shape
    sbytes = _lib.load().mvsdet_plane_sweep_scratch_bytes(proj.shape[0], proj.shape[1], depth.shape[1], H, W)
    return proj.new_empty(max(sbytes // 4, 4))


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_tabled", mutates_args=(), device_types="cuda")
def plane_sweep_variance_tabled(packed: Tensor, nbr: Tensor, table: Tensor, C: int, D: int, H: int, W: int) -> Tensor:
    """The per-channel half of the sweep on a table from plane_sweep_table -> (N,C,D,H,W)."""
    _req(packed, "packed", dim=1)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    _req(table, "table", dim=1)
    N, K = nbr.shape
    nbr = nbr.contiguous()
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(_lib.load().mvsdet_plane_sweep_variance_tabled_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(table),
                                                                      table.numel() * 4, _lib.ptr(out), N, K, C, D, H, W,
                                                                      _stream(packed)), "plane_sweep_variance_tabled")
    return out


@plane_sweep_variance_tabled.register_fake
def _(packed, nbr, table, C, D, H, W):
    return packed.new_empty((nbr.shape[0], C, D, H, W))


def plane_sweep_variance_tabled_f16(packed: Tensor, nbr: Tensor, table: Tensor, C: int, D: int, H: int, W: int) -> Tensor:
    """plane_sweep_variance_tabled with fp16 storage: the fp32 result rounded to nearest-even at the store -> (N,C,D,H,W) float16.
    Forward only."""
    _req(packed, "packed", dim=1)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    _req(table, "table", dim=1)
    N, K = nbr.shape
    nbr = nbr.contiguous()
    out = torch.empty((N, C, D, H, W), dtype=torch.float16, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(_lib.load().mvsdet_plane_sweep_variance_tabled_f16(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(table),
                                                                      table.numel() * 4, _lib.ptr(out), N, K, C, D, H, W,
                                                                      _stream(packed)), "plane_sweep_variance_tabled_f16")
    return out


def sweep_flags(table: Tensor, N: int, K: int, D: int, H: int, W: int) -> Tensor:
    """The flags words of a geometry table (plane_sweep_table / plane_sweep_table_pitched / plane_sweep_table_pooled) as an (N, tiles, D) int64 tensor:
    one nibble per neighbour -- 1 live, 2 staged, 4 refill, 8 inside (csrc/sweep_kernel.h).  Layout of the table: header int4
    {magic, tile width | box capacity << 8, W, D << 8 | K}, boxes [N*tiles*D*K] int4, then the flags."""
    words = table.view(torch.int32)
    hd = [int(v) for v in words[:4].cpu()]
    if hd[0] not in (0x4d565347, 0x4d565350) or hd[2] != W or hd[3] != ((D << 8) | K):
        raise ValueError("sweep_flags: not a geometry table of this (K, D, W)")
    tw = hd[1] & 0xff
    tiles = ((W + tw - 1) // tw) * ((H + 128 // tw - 1) // (128 // tw))
    first = 4 + N * tiles * D * K * 4
    return (words[first:first + N * tiles * D].to(torch.int64) & 0xffff).view(N, tiles, D)


def sweep_inside_count(table: Tensor, N: int, K: int, D: int, H: int, W: int) -> Tuple[int, int]:
    """(live, lean) of a geometry table: the (tile, plane, pass) triples whose pass has a visible neighbour, and how many of
    them the geometry kernel flagged for the slab kernel's lean decode -- every visible neighbour of the pass carries
    kFlagInside.  What the table says, whatever "sweep_inside" is set to."""
    fl = sweep_flags(table, N, K, D, H, W)
    live = lean = 0
    for p in range((K + 1) // 2):
        fp = (fl >> (8 * p)) & 0xff
        vis = fp & 0x11                      # kFlagLive of the pass's two neighbours
        live += int((vis != 0).sum())
        lean += int(((vis != 0) & ((vis & ~(fp >> 3)) == 0)).sum())
    return live, lean


def sweep_stall_events(table: Tensor, N: int, K: int, D: int, H: int, W: int) -> Tuple[int, int]:
    """(events, blocks) of a geometry table: the planes of a (view, tile) block on which at least one neighbour refills its
    footprint box (one block-wide stall of the slab kernel each, for a block that sweeps all planes), and the number of blocks."""
    fl = sweep_flags(table, N, K, D, H, W)
    refill = 0
    for j in range(K):
        nib = fl >> (4 * j)
        refill = refill | (((nib & 2) != 0) & ((nib & 4) != 0))
    return int(refill.sum()), int(fl.shape[0] * fl.shape[1])


def sweep_row_pitch(W: int) -> int:
    """Row pitch (elements) of a cost volume whose rows start on 128-byte lines: W rounded up to a multiple of 32."""
    return (int(W) + 31) // 32 * 32


def plane_sweep_table_pitched(proj: Tensor, depth: Tensor, H: int, W: int, w_pitch: int) -> Tensor:
    """plane_sweep_table for a cost volume with row pitch `w_pitch` (plane_sweep_variance_tabled_pitched)."""
    _req(proj, "proj", dim=4)
    _req(depth, "depth", dim=2)
    N, K = proj.shape[:2]
    D = depth.shape[1]
    lib = _lib.load()
    sbytes = lib.mvsdet_plane_sweep_scratch_bytes(N, K, D, H, W)
    table = torch.empty(max(sbytes // 4, 4), dtype=torch.float32, device=proj.device)
    proj, depth = proj.contiguous(), depth.contiguous()
    with torch.cuda.device(proj.device):
        _lib.check(lib.mvsdet_plane_sweep_table_pitched_f32(_lib.ptr(proj), _lib.ptr(depth), _lib.ptr(table), sbytes, N, K, D, H,
                                                            W, int(w_pitch), _stream(proj)), "plane_sweep_table_pitched")
    return table


@torch.library.custom_op(f"{_NS}::plane_sweep_table_pooled", mutates_args=(), device_types="cuda")
def plane_sweep_table_pooled(proj: Tensor, depth: Tensor, H: int, W: int, w_pitch: int = 0) -> Tensor:
    """plane_sweep_table / plane_sweep_table_pitched (w_pitch: 0 or W = contiguous) under the pooled run policy: with two
    neighbours and 32x4 tiles a footprint box may take the other neighbour's idle LDS slot (csrc/sweep_kernel.h).  For the
    FORWARD sweep only (plane_sweep_variance_tabled / _pitched); the backward refuses such a table (all-NaN gradient).
    Library option "sweep_pool" 0: the unpooled table."""
    _req(proj, "proj", dim=4)
    _req(depth, "depth", dim=2)
    N, K = proj.shape[:2]
    D = depth.shape[1]
    lib = _lib.load()
    sbytes = lib.mvsdet_plane_sweep_scratch_bytes(N, K, D, H, W)
    table = torch.empty(max(sbytes // 4, 4), dtype=torch.float32, device=proj.device)
    proj, depth = proj.contiguous(), depth.contiguous()
    with torch.cuda.device(proj.device):
        _lib.check(lib.mvsdet_plane_sweep_table_pooled_f32(_lib.ptr(proj), _lib.ptr(depth), _lib.ptr(table), sbytes, N, K, D, H,
                                                           W, int(w_pitch), _stream(proj)), "plane_sweep_table_pooled")
    return table


@plane_sweep_table_pooled.register_fake
def _(proj, depth, H, W, w_pitch=0):
    sbytes = _lib.load().mvsdet_plane_sweep_scratch_bytes(proj.shape[0], proj.shape[1], depth.shape[1], H, W)
    return proj.new_empty(max(sbytes // 4, 4))


def plane_sweep_variance_tabled_pitched(packed: Tensor, nbr: Tensor, table: Tensor, C: int, D: int, H: int, W: int,
                                        w_pitch: int) -> Tensor:
    """The per-channel half of the sweep into a row-PITCHED volume: returns the (N,C,D,H,W) view of an (N,C,D,H,w_pitch)
    buffer -- the values of plane_sweep_variance_tabled bit for bit, rows `w_pitch` elements apart (every row on a 128-byte
    line when w_pitch % 32 == 0: whole-line stores from 32x4 tiles for the 80-wide maps of the shipped configs).
    Forward only; the pad columns are never written."""
    _req(packed, "packed", dim=1)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    _req(table, "table", dim=1)
    if w_pitch < W:
        raise ValueError(f"plane_sweep_variance_tabled_pitched: pitch {w_pitch} < W={W}")
    N, K = nbr.shape
    nbr = nbr.contiguous()
    buf = torch.empty((N, C, D, H, int(w_pitch)), dtype=torch.float32, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(_lib.load().mvsdet_plane_sweep_variance_tabled_pitched_f32(
            _lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(table), table.numel() * 4, _lib.ptr(buf), N, K, C, D, H, W, int(w_pitch),
            _stream(packed)), "plane_sweep_variance_tabled_pitched")
    return buf[..., :W]


@torch.library.custom_op(f"{_NS}::plane_sweep_variance", mutates_args=(), device_types="cuda")
def plane_sweep_variance(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor) -> Tensor:
    """a3+a4 (mvsdet.py:439-467): feat (N,C,H,W), nbr (N,K) int64, proj (N,K,4,4), depth (N,D) -> (N,C,D,H,W)."""
    N, K, C, D, H, W = _check_sweep(feat, nbr, proj, depth)
    packed = pack_features(feat)
    return plane_sweep_variance_packed(packed, nbr, proj, depth, C, H, W)


@plane_sweep_variance.register_fake
def _(feat, nbr, proj, depth):
    N, C, H, W = feat.shape
    return feat.new_empty((N, C, depth.shape[1], H, W))


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_backward", mutates_args=(), device_types="cuda")
def plane_sweep_variance_backward(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, grad: Tensor) -> Tensor:
    N, K, C, D, H, W = _check_sweep(feat, nbr, proj, depth)
    _req(grad, "grad", dim=5)
    if grad.shape != (N, C, D, H, W):
        raise ValueError("plane_sweep_variance_backward: grad shape mismatch")
    feat, nbr, proj, depth, grad = feat.contiguous(), nbr.contiguous(), proj.contiguous(), depth.contiguous(), grad.contiguous()
    lib = _lib.load()
    wbytes = lib.mvsdet_plane_sweep_bwd_workspace_bytes(N, K, C, D, H, W)
    ws = torch.empty(wbytes // 4, dtype=torch.float32, device=feat.device)
    gfeat = torch.empty_like(feat)
    with torch.cuda.device(feat.device):
        _lib.check(lib.mvsdet_plane_sweep_variance_bwd_f32(_lib.ptr(feat), _lib.ptr(nbr), _lib.ptr(proj), _lib.ptr(depth),
                                                           _lib.ptr(grad), _lib.ptr(gfeat), _lib.ptr(ws), wbytes, N, K, C,
                                                           D, H, W, _stream(feat)), "plane_sweep_variance_backward")
    return gfeat


@plane_sweep_variance_backward.register_fake
def _(feat, nbr, proj, depth, grad):
    return torch.empty_like(feat)


def _sweep_setup(ctx, inputs, output):
    feat, nbr, proj, depth = inputs
    ctx.save_for_backward(feat, nbr, proj, depth)


def _sweep_bwd(ctx, grad):
    feat, nbr, proj, depth = ctx.saved_tensors
    return plane_sweep_variance_backward(feat, nbr, proj, depth, grad), None, None, None


plane_sweep_variance.register_autograd(_sweep_bwd, setup_context=_sweep_setup)


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_keep", mutates_args=(), device_types="cuda")
def plane_sweep_variance_keep(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """a3+a4 for a TRAINING step: (variance (N,C,D,H,W), the packed maps, the sweep geometry) -- what the forward pass makes on its
    way is handed out instead of dropped: the lifting reads the packed maps, and the backward pass takes both
    (`plane_sweep_variance_backward_packed`) instead of packing the features and building the geometry a second time."""
    N, K, C, D, H, W = _check_sweep(feat, nbr, proj, depth)
    packed = pack_features(feat)
    nbr, proj, depth = nbr.contiguous(), proj.contiguous(), depth.contiguous()
    lib = _lib.load()
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=feat.device)
    sbytes = lib.mvsdet_plane_sweep_scratch_bytes(N, K, D, H, W)
    table = torch.empty(max(sbytes // 4, 4), dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        _lib.check(lib.mvsdet_plane_sweep_variance_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj), _lib.ptr(depth),
                                                              _lib.ptr(out), _lib.ptr(table), sbytes, N, K, C, D, H, W,
                                                              _stream(feat)), "plane_sweep_variance_keep")
    return out, packed, table


@plane_sweep_variance_keep.register_fake
def _(feat, nbr, proj, depth):
    N, C, H, W = feat.shape
    sbytes = int(_lib.load().mvsdet_plane_sweep_scratch_bytes(N, nbr.shape[1], depth.shape[1], H, W))   # a host-side size function
    return (feat.new_empty((N, C, depth.shape[1], H, W)), feat.new_empty((N * ((C + 31) // 32) * H * W * 32,)),
            feat.new_empty((max(sbytes // 4, 4),)))


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_backward_packed", mutates_args=(), device_types="cuda")
def plane_sweep_variance_backward_packed(packed: Tensor, nbr: Tensor, table: Tensor, grad: Tensor) -> Tensor:
    """dL/dfeat (N,C,H,W) from dL/dvar (N,C,D,H,W), the packed maps and the sweep geometry of the forward pass."""
    _req(grad, "grad", dim=5)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    N, C, D, H, W = grad.shape
    K = nbr.shape[1]
    lib = _lib.load()
    if nbr.shape[0] != N or packed.numel() * 4 != lib.mvsdet_packed_bytes(N, C, H, W):
        raise ValueError("plane_sweep_variance_backward_packed: packed maps / neighbour ids do not match the gradient")
    grad, nbr = grad.contiguous(), nbr.contiguous()
    pb = (int(lib.mvsdet_packed_bytes(N, C, H, W)) + 255) // 256 * 256
    ws = torch.empty(pb // 4, dtype=torch.float32, device=grad.device)
    gfeat = torch.empty((N, C, H, W), dtype=torch.float32, device=grad.device)
    with torch.cuda.device(grad.device):
        _lib.check(lib.mvsdet_plane_sweep_variance_bwd_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(table), table.numel() * 4,
                                                                  _lib.ptr(grad), _lib.ptr(gfeat), _lib.ptr(ws), pb, N, K, C, D, H, W,
                                                                  _stream(grad)), "plane_sweep_variance_backward_packed")
    return gfeat


@plane_sweep_variance_backward_packed.register_fake
def _(packed, nbr, table, grad):
    N, C, D, H, W = grad.shape
    return grad.new_empty((N, C, H, W))


def _sweep_keep_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1], inputs[1], output[2])
    ctx.mark_non_differentiable(output[1], output[2])


def _sweep_keep_bwd(ctx, grad, g_packed, g_table):
    packed, nbr, table = ctx.saved_tensors
    return plane_sweep_variance_backward_packed(packed, nbr, table, grad), None, None, None


plane_sweep_variance_keep.register_autograd(_sweep_keep_bwd, setup_context=_sweep_keep_setup)


# ------------------------------------------------------------------------------------------- a3 / a3+a4, per-pixel depths
# homo_warping's depth_values (B,D,H,W) form (mvs_models/module.py:130-133): every reference pixel carries its own D
# hypotheses.  Kernels of their own (csrc/planesweep_pixel.hip); the plane operators above still refuse a 4-D depth.
def _check_depth_pixel(name, depth, B, H, W):
    _req(depth, "depth", dim=4)
    if depth.shape[0] != B or tuple(depth.shape[2:]) != (H, W):
        raise ValueError(f"{name}: depth {tuple(depth.shape)} is not (B={B}, D, H={H}, W={W})")
    return depth.shape[1]


@torch.library.custom_op(f"{_NS}::homo_warp_pixel", mutates_args=(), device_types="cuda")
def homo_warp_pixel(src: Tensor, proj: Tensor, depth: Tensor) -> Tensor:
    """a3 at per-pixel depths: src (B,C,H,W), proj (B,4,4) = src_proj @ inv(ref_proj), depth (B,D,H,W) -> (B,C,D,H,W).
    Differentiable in src."""
    _req(src, "src", dim=4)
    _req(proj, "proj", dim=3)
    B, C, H, W = src.shape
    D = _check_depth_pixel("homo_warp_pixel", depth, B, H, W)
    if proj.shape != (B, 4, 4):
        raise ValueError(f"homo_warp_pixel: proj {tuple(proj.shape)} does not match B={B}")
    src, proj, depth = src.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((B, C, D, H, W), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().mvsdet_homo_warp_pixel_f32(_lib.ptr(src), _lib.ptr(proj), _lib.ptr(depth), _lib.ptr(out),
                                                          B, C, D, H, W, _stream(src)), "homo_warp_pixel")
    return out


@homo_warp_pixel.register_fake
def _(src, proj, depth):
    B, C, H, W = src.shape
    return src.new_empty((B, C, depth.shape[1], H, W))


@torch.library.custom_op(f"{_NS}::homo_warp_pixel_backward", mutates_args=(), device_types="cuda")
def homo_warp_pixel_backward(proj: Tensor, depth: Tensor, grad: Tensor) -> Tensor:
    """dL/dsrc (B,C,H,W) from dL/dwarped (B,C,D,H,W): bilinear scatter with float atomics (last bits depend on arrival order)."""
    _req(grad, "grad", dim=5)
    _req(proj, "proj", dim=3)
    B, C, D, H, W = grad.shape
    if _check_depth_pixel("homo_warp_pixel_backward", depth, B, H, W) != D or proj.shape != (B, 4, 4):
        raise ValueError("homo_warp_pixel_backward: proj / depth do not match the gradient")
    proj, depth, grad = proj.contiguous(), depth.contiguous(), grad.contiguous()
    lib = _lib.load()
    wbytes = int(lib.mvsdet_plane_sweep_pixel_bwd_workspace_bytes(B, C, H, W))
    ws = torch.empty(wbytes // 4, dtype=torch.float32, device=grad.device)
    gsrc = torch.empty((B, C, H, W), dtype=torch.float32, device=grad.device)
    with torch.cuda.device(grad.device):
        _lib.check(lib.mvsdet_homo_warp_pixel_bwd_f32(_lib.ptr(proj), _lib.ptr(depth), _lib.ptr(grad), _lib.ptr(gsrc), _lib.ptr(ws),
                                                      wbytes, B, C, D, H, W, _stream(grad)), "homo_warp_pixel_backward")
    return gsrc


@homo_warp_pixel_backward.register_fake
def _(proj, depth, grad):
    B, C, D, H, W = grad.shape
    return grad.new_empty((B, C, H, W))


def _warp_pixel_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1], inputs[2])


def _warp_pixel_bwd(ctx, grad):
    proj, depth = ctx.saved_tensors
    return homo_warp_pixel_backward(proj, depth, grad), None, None


homo_warp_pixel.register_autograd(_warp_pixel_bwd, setup_context=_warp_pixel_setup)


def _check_sweep_pixel(feat, nbr, proj, depth):
    _req(feat, "feat", dim=4)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    _req(proj, "proj", dim=4)
    N, C, H, W = feat.shape
    D = _check_depth_pixel("plane_sweep_variance_pixel", depth, N, H, W)
    K = nbr.shape[1]
    if nbr.shape[0] != N or proj.shape != (N, K, 4, 4):
        raise ValueError(f"plane_sweep_variance_pixel: nbr {tuple(nbr.shape)}, proj {tuple(proj.shape)} do not match N={N}")
    return N, K, C, D, H, W


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_pixel_packed", mutates_args=(), device_types="cuda")
def plane_sweep_variance_pixel_packed(packed: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, C: int) -> Tensor:
    """a3+a4 at per-pixel depths on already packed maps: depth (N,D,H,W) -> variance (N,C,D,H,W)."""
    _req(packed, "packed", dim=1)
    _req(nbr, "nbr", dtype=torch.int64, dim=2)
    _req(proj, "proj", dim=4)
    _req(depth, "depth", dim=4)
    N, K = nbr.shape
    D, H, W = depth.shape[1:]
    lib = _lib.load()
    if packed.numel() * 4 != lib.mvsdet_packed_bytes(N, C, H, W):
        raise ValueError("plane_sweep_variance_pixel_packed: packed buffer does not match (N,C,H,W)")
    if proj.shape != (N, K, 4, 4) or depth.shape[0] != N:
        raise ValueError("plane_sweep_variance_pixel_packed: proj/depth shape mismatch")
    nbr, proj, depth = nbr.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(lib.mvsdet_plane_sweep_variance_pixel_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj), _lib.ptr(depth),
                                                                    _lib.ptr(out), N, K, C, D, H, W, _stream(packed)),
                   "plane_sweep_variance_pixel_packed")
    return out


@plane_sweep_variance_pixel_packed.register_fake
def _(packed, nbr, proj, depth, C):
    N, D, H, W = depth.shape
    return packed.new_empty((N, C, D, H, W))


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_pixel", mutates_args=(), device_types="cuda")
def plane_sweep_variance_pixel(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor) -> Tensor:
    """a3+a4 at per-pixel depths: feat (N,C,H,W), nbr (N,K) int64, proj (N,K,4,4), depth (N,D,H,W) -> (N,C,D,H,W).
    Differentiable in feat (the backward packs the features again)."""
    N, K, C, D, H, W = _check_sweep_pixel(feat, nbr, proj, depth)
    return plane_sweep_variance_pixel_packed(pack_features(feat), nbr, proj, depth, C)


@plane_sweep_variance_pixel.register_fake
def _(feat, nbr, proj, depth):
    N, C, H, W = feat.shape
    return feat.new_empty((N, C, depth.shape[1], H, W))


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_pixel_backward", mutates_args=(), device_types="cuda")
def plane_sweep_variance_pixel_backward(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, grad: Tensor) -> Tensor:
    N, K, C, D, H, W = _check_sweep_pixel(feat, nbr, proj, depth)
    _req(grad, "grad", dim=5)
    if grad.shape != (N, C, D, H, W):
        raise ValueError("plane_sweep_variance_pixel_backward: grad shape mismatch")
    packed = pack_features(feat)
    nbr, proj, depth, grad = nbr.contiguous(), proj.contiguous(), depth.contiguous(), grad.contiguous()
    lib = _lib.load()
    wbytes = int(lib.mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W))
    ws = torch.empty(wbytes // 4, dtype=torch.float32, device=feat.device)
    gfeat = torch.empty((N, C, H, W), dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        _lib.check(lib.mvsdet_plane_sweep_variance_pixel_bwd_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj), _lib.ptr(depth),
                                                                        _lib.ptr(grad), _lib.ptr(gfeat), _lib.ptr(ws), wbytes, N, K, C,
                                                                        D, H, W, _stream(feat)), "plane_sweep_variance_pixel_backward")
    return gfeat


@plane_sweep_variance_pixel_backward.register_fake
def _(feat, nbr, proj, depth, grad):
    return torch.empty_like(feat)


def _sweep_pixel_bwd(ctx, grad):
    feat, nbr, proj, depth = ctx.saved_tensors
    return plane_sweep_variance_pixel_backward(feat, nbr, proj, depth, grad), None, None, None


plane_sweep_variance_pixel.register_autograd(_sweep_pixel_bwd, setup_context=_sweep_setup)


# ------------------------------------------------------------------------------------------- a5-a7
@torch.library.custom_op(f"{_NS}::depth_prob_topk", mutates_args=(), device_types="cuda")
def depth_prob_topk(cost_reg: Tensor, off_logit: Tensor, near: float, interval: float,
                    topk: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """a5-a7 (mvsdet.py:470-475, 266-283, 298-317) -> prob, off (N,D,H,W); est_depth, est_dens (N,topk,H,W);
    est_idx (N,topk,H,W) int32; avg_depth (N,H,W)."""
    _req(cost_reg, "cost_reg", dim=4)
    _req(off_logit, "off_logit", dim=4)
    if cost_reg.shape != off_logit.shape:
        raise ValueError("depth_prob_topk: cost_reg / off_logit shape mismatch")
    N, D, H, W = cost_reg.shape
    # the slices of one (N, 2, D, H, W) tensor (the network's output) are read in place: dense (D, H, W) blocks, one stride
    # between the views; anything else is made contiguous first
    dense = (W * H * D, W * H, W, 1)
    if not (cost_reg.stride()[1:] == dense[1:] == off_logit.stride()[1:] and cost_reg.stride(0) == off_logit.stride(0) >= dense[0]):
        cost_reg, off_logit = cost_reg.contiguous(), off_logit.contiguous()
    view_stride = cost_reg.stride(0) if N > 1 else dense[0]
    dev = cost_reg.device
    prob = torch.empty((N, D, H, W), dtype=torch.float32, device=dev)
    off = torch.empty((N, D, H, W), dtype=torch.float32, device=dev)
    est_depth = torch.empty((N, topk, H, W), dtype=torch.float32, device=dev)
    est_dens = torch.empty((N, topk, H, W), dtype=torch.float32, device=dev)
    est_idx = torch.empty((N, topk, H, W), dtype=torch.int32, device=dev)
    avg = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_depth_prob_topk_strided_f32(_lib.ptr(cost_reg), _lib.ptr(off_logit), view_stride,
                                                                  _lib.ptr(prob), _lib.ptr(off), _lib.ptr(est_depth),
                                                                  _lib.ptr(est_dens), _lib.ptr(est_idx), _lib.ptr(avg), N, D, H,
                                                                  W, topk, near, interval, _stream(cost_reg)), "depth_prob_topk")
    return prob, off, est_depth, est_dens, est_idx, avg


@depth_prob_topk.register_fake
def _(cost_reg, off_logit, near, interval, topk):
    N, D, H, W = cost_reg.shape
    e = cost_reg.new_empty
    return (e((N, D, H, W)), e((N, D, H, W)), e((N, topk, H, W)), e((N, topk, H, W)),
            cost_reg.new_empty((N, topk, H, W), dtype=torch.int32), e((N, H, W)))


@torch.library.custom_op(f"{_NS}::sample_depth_prob", mutates_args=(), device_types="cuda")
def sample_depth_prob(prob: Tensor, off: Tensor, near: float, interval: float,
                      topk: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """a6+a7 on ready-made probabilities (mvsdet.py:266-283, 298-317) -> est_depth, est_dens (N,topk,H,W),
    est_idx int32, avg_depth (N,H,W)."""
    _req(prob, "prob", dim=4)
    _req(off, "off", dim=4)
    if prob.shape != off.shape:
        raise ValueError("sample_depth_prob: prob / off shape mismatch")
    N, D, H, W = prob.shape
    prob, off = prob.contiguous(), off.contiguous()
    dev = prob.device
    est_depth = torch.empty((N, topk, H, W), dtype=torch.float32, device=dev)
    est_dens = torch.empty((N, topk, H, W), dtype=torch.float32, device=dev)
    est_idx = torch.empty((N, topk, H, W), dtype=torch.int32, device=dev)
    avg = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_sample_depth_prob_f32(_lib.ptr(prob), _lib.ptr(off), _lib.ptr(est_depth),
                                                            _lib.ptr(est_dens), _lib.ptr(est_idx), _lib.ptr(avg), N, D, H,
                                                            W, topk, near, interval, _stream(prob)), "sample_depth_prob")
    return est_depth, est_dens, est_idx, avg


@sample_depth_prob.register_fake
def _(prob, off, near, interval, topk):
    N, D, H, W = prob.shape
    e = prob.new_empty
    return e((N, topk, H, W)), e((N, topk, H, W)), prob.new_empty((N, topk, H, W), dtype=torch.int32), e((N, H, W))


def _sdp_setup(ctx, inputs, output):
    prob, off, near, interval, topk = inputs
    ctx.save_for_backward(prob, off, output[2])
    ctx.near, ctx.interval = near, interval


def _sdp_bwd(ctx, g_depth, g_dens, g_idx, g_avg):
    # gradients w.r.t. prob and off directly (no softmax / sigmoid Jacobian), in plain tensor ops:
    # est_dens = prob[idx]; est_depth = idx*iv + near + off[idx]*iv; avg = sum_d prob_d * depth_d
    prob, off, est_idx = ctx.saved_tensors
    iv, near = ctx.interval, ctx.near
    idx = est_idx.long()
    gp = torch.zeros_like(prob)
    go = torch.zeros_like(prob)
    if g_dens is not None:
        gp.scatter_add_(1, idx, g_dens)
    if g_depth is not None:
        go.scatter_add_(1, idx, g_depth * iv)
    if g_avg is not None:
        d = torch.arange(prob.shape[1], device=prob.device, dtype=torch.float32).view(1, -1, 1, 1)
        gp += g_avg.unsqueeze(1) * ((d * iv + near) + off * iv)
        go += g_avg.unsqueeze(1) * prob * iv
    return gp, go, None, None, None


sample_depth_prob.register_autograd(_sdp_bwd, setup_context=_sdp_setup)


@torch.library.custom_op(f"{_NS}::depth_prob_topk_backward", mutates_args=(), device_types="cuda")
def depth_prob_topk_backward(prob: Tensor, off: Tensor, est_idx: Tensor, g_prob: Tensor, g_depth: Tensor,
                             g_dens: Tensor, g_avg: Tensor, near: float, interval: float) -> Tuple[Tensor, Tensor]:
    N, D, H, W = prob.shape
    topk = est_idx.shape[1]
    g_cost = torch.empty_like(prob)
    g_off = torch.empty_like(prob)
    g_prob, g_depth, g_dens, g_avg = g_prob.contiguous(), g_depth.contiguous(), g_dens.contiguous(), g_avg.contiguous()
    with torch.cuda.device(prob.device):
        _lib.check(_lib.load().mvsdet_depth_prob_topk_bwd_f32(
            _lib.ptr(prob), _lib.ptr(off), _lib.ptr(est_idx), _lib.ptr(g_prob), _lib.ptr(g_depth), _lib.ptr(g_dens),
            _lib.ptr(g_avg), _lib.ptr(g_cost), _lib.ptr(g_off), N, D, H, W, topk, near, interval, _stream(prob)),
            "depth_prob_topk_backward")
    return g_cost, g_off


@depth_prob_topk_backward.register_fake
def _(prob, off, est_idx, g_prob, g_depth, g_dens, g_avg, near, interval):
    return torch.empty_like(prob), torch.empty_like(prob)


def _dp_setup(ctx, inputs, output):
    cost_reg, off_logit, near, interval, topk = inputs
    prob, off, est_depth, est_dens, est_idx, avg = output
    ctx.save_for_backward(prob, off, est_idx)
    ctx.near, ctx.interval = near, interval


def _dp_bwd(ctx, g_prob, g_off, g_depth, g_dens, g_idx, g_avg):
    prob, off, est_idx = ctx.saved_tensors

    def z(g, like_shape):
        return torch.zeros(like_shape, dtype=torch.float32, device=prob.device) if g is None else g

    N, D, H, W = prob.shape
    k = est_idx.shape[1]
    g_cost, g_offl = depth_prob_topk_backward(prob, off, est_idx, z(g_prob, prob.shape), z(g_depth, (N, k, H, W)),
                                              z(g_dens, (N, k, H, W)), z(g_avg, (N, H, W)), ctx.near, ctx.interval)
    if g_off is not None:  # direct gradient on the sigmoid output
        g_offl = g_offl + g_off * off * (1.0 - off)
    return g_cost, g_offl, None, None, None


depth_prob_topk.register_autograd(_dp_bwd, setup_context=_dp_setup)


# ------------------------------------------------------------------------------------------- a9
def _check_stage3(features, points, projection, est_depth, est_dens):
    _req(features, "features", dim=4)
    _req(points, "points")
    _req(projection, "projection", dim=3)
    _req(est_depth, "est_depth", dim=4)
    _req(est_dens, "est_dens", dim=4)
    N, C, h, w = features.shape
    if points.shape[0] != 3:
        raise ValueError("backproject_weigh: points must be (3, ...)")
    V = points.numel() // 3
    J = est_depth.shape[1]
    if projection.shape != (N, 3, 4):
        raise ValueError(f"backproject_weigh: projection {tuple(projection.shape)} != ({N},3,4)")
    if est_depth.shape != (N, J, h, w) or est_dens.shape != (N, J, h, w):
        raise ValueError(f"backproject_weigh: est_depth/est_dens must be ({N},J,{h},{w}), got "
                         f"{tuple(est_depth.shape)} / {tuple(est_dens.shape)}")
    if est_depth.stride() != est_dens.stride():
        est_dens = est_dens.contiguous()
        est_depth = est_depth.contiguous()
    return N, C, h, w, V, J, est_depth, est_dens


@torch.library.custom_op(f"{_NS}::backproject_weigh", mutates_args=(), device_types="cuda")
def backproject_weigh(features: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor, est_dens: Tensor,
                      vz: float) -> Tuple[Tensor, Tensor]:
    """a9 (mvsdet.py:1372): features (N,C,h,w) any strides; points (3,X,Y,Z); projection (N,3,4);
    est_depth/est_dens (N,J,h,w) any strides -> volume (N,C,V) fp32, valid (N,V) bool."""
    N, C, h, w, V, J, est_depth, est_dens = _check_stage3(features, points, projection, est_depth, est_dens)
    points, projection = points.contiguous(), projection.contiguous()
    dev = features.device
    volume = torch.empty((N, C, V), dtype=torch.float32, device=dev)
    valid = torch.empty((N, V), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_backproject_weigh_f32(
            _lib.ptr(features), _lib.strides4(features), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth),
            _lib.ptr(est_dens), _lib.strides4(est_depth), _lib.ptr(volume), _lib.ptr(valid), None, None,
            N, C, h, w, V, J, vz, _stream(features)), "backproject_weigh")
    return volume, valid.bool()


@backproject_weigh.register_fake
def _(features, points, projection, est_depth, est_dens, vz):
    N, C = features.shape[:2]
    V = points.numel() // 3
    return features.new_empty((N, C, V)), features.new_empty((N, V), dtype=torch.bool)


@torch.library.custom_op(f"{_NS}::backproject_weigh_backward", mutates_args=(), device_types="cuda")
def backproject_weigh_backward(features: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor,
                               est_dens: Tensor, vz: float, grad: Tensor) -> Tuple[Tensor, Tensor]:
    N, C, h, w, V, J, est_depth, est_dens = _check_stage3(features, points, projection, est_depth, est_dens)
    points, projection, grad = points.contiguous(), projection.contiguous(), grad.contiguous()
    dev = features.device
    gfeat = torch.empty((N, C, h, w), dtype=torch.float32, device=dev)
    gdens = torch.empty((N, J, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_backproject_weigh_bwd_f32(
            _lib.ptr(features), _lib.strides4(features), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth),
            _lib.ptr(est_dens), _lib.strides4(est_depth), _lib.ptr(grad), _lib.ptr(gfeat), _lib.ptr(gdens),
            N, C, h, w, V, J, vz, _stream(features)), "backproject_weigh_backward")
    return gfeat, gdens


@backproject_weigh_backward.register_fake
def _(features, points, projection, est_depth, est_dens, vz, grad):
    N, C, h, w = features.shape
    return features.new_empty((N, C, h, w)), features.new_empty((N, est_depth.shape[1], h, w))


def _bp_setup(ctx, inputs, output):
    features, points, projection, est_depth, est_dens, vz = inputs
    ctx.save_for_backward(features, points, projection, est_depth, est_dens)
    ctx.vz = vz


def _bp_bwd(ctx, g_volume, g_valid):
    features, points, projection, est_depth, est_dens = ctx.saved_tensors
    gfeat, gdens = backproject_weigh_backward(features, points, projection, est_depth, est_dens, ctx.vz, g_volume)
    return gfeat, None, None, None, gdens, None


backproject_weigh.register_autograd(_bp_bwd, setup_context=_bp_setup)


# ------------------------------------------------------------------------------------------- a9 against ground-truth depth
def _strides3(t: Tensor) -> ctypes.Array:
    """HOST int64[3] with the element strides of a 3-D tensor."""
    return (ctypes.c_int64 * 3)(*[int(v) for v in t.stride()])


@torch.library.custom_op(f"{_NS}::depth_diagnostics", mutates_args=(), device_types="cuda")
def depth_diagnostics(points: Tensor, projection: Tensor, est_depth: Tensor, est_dens: Tensor, depth_mean: Tensor,
                      gt_depth: Tensor, vz: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The gt_depth branch of backproject_Weigh (mvsdet.py:1435-1484): points (3,X,Y,Z); projection (N,3,4); est_depth / est_dens
    (N,J,h,w) any strides; depth_mean (N,h,w) any strides (the cropped depth expectation); gt_depth (N,Hg,Wg) any strides, any size
    -> scalars (2) {gap_all ("weight_gap"), rmse ("src_rmse")}, per_view (N,4) {gap_i, orig_gap, new_gap, n_reduce}, sums (N,6)
    float64 (include/mvsdet_hip.h), gt_resized (N,h,w).  Three launches on the current stream, no host synchronisation; no autograd
    (the reference runs the branch under no_grad).  gap_all is NaN when no view keeps a voxel (the reference raises there)."""
    _req(points, "points")
    _req(projection, "projection", dim=3)
    _req(est_depth, "est_depth", dim=4)
    _req(est_dens, "est_dens", dim=4)
    _req(depth_mean, "depth_mean", dim=3)
    _req(gt_depth, "gt_depth", dim=3)
    N, J, h, w = est_depth.shape
    if points.shape[0] != 3:
        raise ValueError("depth_diagnostics: points must be (3, ...)")
    V = points.numel() // 3
    if projection.shape != (N, 3, 4) or est_dens.shape != (N, J, h, w):
        raise ValueError(f"depth_diagnostics: projection {tuple(projection.shape)} / est_dens {tuple(est_dens.shape)} do not match "
                         f"est_depth {tuple(est_depth.shape)}")
    if depth_mean.shape != (N, h, w) or gt_depth.shape[0] != N:
        raise ValueError(f"depth_diagnostics: depth_mean {tuple(depth_mean.shape)} must be ({N},{h},{w}) and gt_depth "
                         f"{tuple(gt_depth.shape)} ({N},Hg,Wg)")
    if est_depth.stride() != est_dens.stride():
        est_depth, est_dens = est_depth.contiguous(), est_dens.contiguous()
    points, projection = points.contiguous(), projection.contiguous()
    Hg, Wg = int(gt_depth.shape[1]), int(gt_depth.shape[2])
    dev = est_depth.device
    lib = _lib.load()
    scalars = torch.empty((2,), dtype=torch.float32, device=dev)
    per_view = torch.empty((N, 4), dtype=torch.float32, device=dev)
    sums = torch.empty((N, 6), dtype=torch.float64, device=dev)
    gt_resized = torch.empty((N, h, w), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.mvsdet_depth_diagnostics_workspace_bytes(N, h, w, V))
    workspace = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_depth_diagnostics_f32(
            _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth), _lib.ptr(est_dens), _lib.strides4(est_depth),
            _lib.ptr(depth_mean), _strides3(depth_mean), _lib.ptr(gt_depth), _strides3(gt_depth), _lib.ptr(scalars),
            _lib.ptr(per_view), _lib.ptr(sums), _lib.ptr(gt_resized), _lib.ptr(workspace), ws_bytes, N, h, w, V, J, Hg, Wg, vz,
            _stream(est_depth)), "depth_diagnostics")
    return scalars, per_view, sums, gt_resized


@depth_diagnostics.register_fake
def _(points, projection, est_depth, est_dens, depth_mean, gt_depth, vz):
    N, _, h, w = est_depth.shape
    return (est_depth.new_empty((2,)), est_depth.new_empty((N, 4)), est_depth.new_empty((N, 6), dtype=torch.float64),
            est_depth.new_empty((N, h, w)))


# ------------------------------------------------------------------------------------------- a9+a10
@torch.library.custom_op(f"{_NS}::backproject_weigh_mean", mutates_args=(), device_types="cuda")
def backproject_weigh_mean(features: Tensor, packed: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor,
                           est_dens: Tensor, H: int, W: int, vz: float) -> Tuple[Tensor, Tensor]:
    """a9+a10 fused (mvsdet.py:1372 + 511-515).  `features` is the (N,C,h,w) crop view (used for shapes and by
    the backward pass), `packed` = pack_features(full (N,C,H,W) maps).  -> mean (C,V) fp32, count (V) int32."""
    N, C, h, w, V, J, est_depth, est_dens = _check_stage3(features, points, projection, est_depth, est_dens)
    _req(packed, "packed", dim=1)
    lib = _lib.load()
    if packed.numel() * 4 != lib.mvsdet_packed_bytes(N, C, H, W):
        raise ValueError("backproject_weigh_mean: packed buffer does not match (N,C,H,W)")
    points, projection = points.contiguous(), projection.contiguous()
    dev = features.device
    mean = torch.empty((C, V), dtype=torch.float32, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_backproject_weigh_mean_packed_f32(
            _lib.ptr(packed), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth), _lib.ptr(est_dens),
            _lib.strides4(est_depth), _lib.ptr(mean), _lib.ptr(count), N, C, H, W, h, w, V, J, vz, _stream(features)),
            "backproject_weigh_mean")
    return mean, count


@backproject_weigh_mean.register_fake
def _(features, packed, points, projection, est_depth, est_dens, H, W, vz):
    C = features.shape[1]
    V = points.numel() // 3
    return features.new_empty((C, V)), features.new_empty((V,), dtype=torch.int32)


@torch.library.custom_op(f"{_NS}::backproject_weigh_sum_shard", mutates_args=(), device_types="cuda")
def backproject_weigh_sum_shard(packed: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor, est_dens: Tensor,
                                n_src: int, ref_first: int, C: int, H: int, W: int, vz: float) -> Tuple[Tensor, Tensor]:
    """a9 summed over the M views ref_first .. ref_first+M-1 only, NOT divided (the a10 division happens after the
    ranks' sums and counts are all-reduced).  projection (M,3,4), est_depth / est_dens (M,J,h,w) are the shard's;
    `packed` holds all n_src views.  -> sum (C,V) fp32, count (V) int32.  Forward only."""
    _req(packed, "packed", dim=1)
    _req(points, "points")
    _req(projection, "projection", dim=3)
    _req(est_depth, "est_depth", dim=4)
    _req(est_dens, "est_dens", dim=4)
    M, J, h, w = est_depth.shape
    V = points.numel() // 3
    lib = _lib.load()
    if packed.numel() * 4 != lib.mvsdet_packed_bytes(n_src, C, H, W):
        raise ValueError("backproject_weigh_sum_shard: packed buffer does not match (n_src,C,H,W)")
    if points.shape[0] != 3 or projection.shape != (M, 3, 4) or est_dens.shape != est_depth.shape:
        raise ValueError("backproject_weigh_sum_shard: points / projection / est_dens shape mismatch")
    if M < 1 or ref_first < 0 or ref_first + M > n_src:
        raise ValueError(f"backproject_weigh_sum_shard: views [{ref_first},{ref_first + M}) outside the {n_src} packed views")
    if est_depth.stride() != est_dens.stride():
        est_depth, est_dens = est_depth.contiguous(), est_dens.contiguous()
    points, projection = points.contiguous(), projection.contiguous()
    dev = packed.device
    total = torch.empty((C, V), dtype=torch.float32, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    view_floats = lib.mvsdet_packed_bytes(1, C, H, W) // 4
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_backproject_weigh_sum_packed_f32(
            _lib.ptr(packed[view_floats * ref_first:]), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth),
            _lib.ptr(est_dens), _lib.strides4(est_depth), _lib.ptr(total), _lib.ptr(count), M, C, H, W, h, w, V, J, vz,
            _stream(packed)), "backproject_weigh_sum_shard")
    return total, count


@backproject_weigh_sum_shard.register_fake
def _(packed, points, projection, est_depth, est_dens, n_src, ref_first, C, H, W, vz):
    V = points.numel() // 3
    return packed.new_empty((C, V)), packed.new_empty((V,), dtype=torch.int32)


@torch.library.custom_op(f"{_NS}::backproject_weigh_mean_backward", mutates_args=(), device_types="cuda")
def backproject_weigh_mean_backward(features: Tensor, points: Tensor, projection: Tensor, est_depth: Tensor,
                                    est_dens: Tensor, count: Tensor, vz: float, grad: Tensor) -> Tuple[Tensor, Tensor]:
    N, C, h, w, V, J, est_depth, est_dens = _check_stage3(features, points, projection, est_depth, est_dens)
    points, projection, grad = points.contiguous(), projection.contiguous(), grad.contiguous()
    dev = features.device
    gfeat = torch.empty((N, C, h, w), dtype=torch.float32, device=dev)
    gdens = torch.empty((N, J, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_backproject_weigh_mean_bwd_f32(
            _lib.ptr(features), _lib.strides4(features), _lib.ptr(points), _lib.ptr(projection), _lib.ptr(est_depth),
            _lib.ptr(est_dens), _lib.strides4(est_depth), _lib.ptr(count), _lib.ptr(grad), _lib.ptr(gfeat),
            _lib.ptr(gdens), N, C, h, w, V, J, vz, _stream(features)), "backproject_weigh_mean_backward")
    return gfeat, gdens


@backproject_weigh_mean_backward.register_fake
def _(features, points, projection, est_depth, est_dens, count, vz, grad):
    N, C, h, w = features.shape
    return features.new_empty((N, C, h, w)), features.new_empty((N, est_depth.shape[1], h, w))


def _bpm_setup(ctx, inputs, output):
    features, packed, points, projection, est_depth, est_dens, H, W, vz = inputs
    mean, count = output
    ctx.save_for_backward(features, points, projection, est_depth, est_dens, count)
    ctx.vz = vz


def _bpm_bwd(ctx, g_mean, g_count):
    features, points, projection, est_depth, est_dens, count = ctx.saved_tensors
    gfeat, gdens = backproject_weigh_mean_backward(features, points, projection, est_depth, est_dens, count, ctx.vz,
                                                   g_mean)
    return gfeat, None, None, None, None, gdens, None, None, None


backproject_weigh_mean.register_autograd(_bpm_bwd, setup_context=_bpm_setup)


# ------------------------------------------------------------------------------------------- cost network on bf16x3 (f-1)
def split_bf16(t: Tensor):
    """fp32 -> (hi, mid) bfloat16 pieces: hi = bf16(t), mid = bf16(t - hi), both round-to-nearest-even; t - hi is exact."""
    hi = t.to(torch.bfloat16)
    mid = (t - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, mid


def _tap_table(order: int):
    """The 3x3x3 tap of each half of the 14 tap pairs (-1 = empty), as csrc/costreg_bf16.hip:tap_table builds it."""
    if order == 0:
        return [i if i < 27 else -1 for i in range(28)]
    t = []
    for pi in range(8):
        pd, ph, pw = pi >> 2, (pi >> 1) & 1, pi & 1
        nt = 1 << (pd + ph + pw)
        for j in range(nt):
            bits, jw, jh, jd = j, 0, 0, 0
            if pw:
                jw, bits = bits & 1, bits >> 1
            if ph:
                jh, bits = bits & 1, bits >> 1
            if pd:
                jd = bits & 1
            t.append(((2 * jd if pd else 1) * 3 + (2 * jh if ph else 1)) * 3 + (2 * jw if pw else 1))
        if nt == 1:
            t.append(-1)
    return t


# MFMA row m of a row group carries output channel ROW_CHANNEL[m] (csrc/costreg_bf16.hip: bf_mfma_row_channel): a lane's
# accumulator registers 8q..8q+7 are then eight consecutive channels, i.e. one 16-byte unit of the SCL form
ROW_CHANNEL = [8 * ((m >> 4) * 2 + ((m >> 2) & 1)) + (m & 3) + 4 * ((m >> 3) & 1) for m in range(32)]


def get_option(name: str) -> int:
    """A tuning option of the library (mvsdet_get_option)."""
    v = ctypes.c_int(0)
    _lib.check(_lib.load().mvsdet_get_option(name.encode(), ctypes.byref(v)), "get_option")
    return int(v.value)


def split_conv_weight(weight: Tensor, order: int = 0) -> Tensor:
    """Conv3d weight (Cout = 64*m, Cin, 3,3,3) fp32 -> the layout the bf16x3 kernels stream into LDS (include/mvsdet_hip.h):
    [Cout/64][ceil(Cin/8)][14 tap pairs][2 row groups][2 pieces][64 lanes][8 channels] bf16, lane = 32*(half of the pair) +
    MFMA row m (which carries output ROW_CHANNEL[m] of its group of 32); empty halves and the channels beyond Cin are zero.
    order 0: stride-1 convolution, the same bytes as [7 k-steps][4 row groups of 16][2 pieces][64 lanes][8 channels], lane =
    16*(tap of the k-step) + MFMA row (the 16x16x32 instruction's fragments);
    1: stride-2 convolution (pairs grouped by the parity class of the input voxel); 2: `weight` is a ConvTranspose3d weight
    (Cin, Cout = 64*m, 3,3,3), pairs grouped by the parity class of the output voxel.  On a ROCm device this is ONE small
    kernel (run per call: in-place weight updates are always seen); on the CPU the same layout from torch ops (tests)."""
    if order == 2:
        cin, cout = weight.shape[:2]
    else:
        cout, cin = weight.shape[:2]
    if cout % 64 or tuple(weight.shape[2:]) != (3, 3, 3) or order not in (0, 1, 2):
        raise ValueError(f"split_conv_weight: weight {tuple(weight.shape)} (order {order}) has no 64*m output channels / 3x3x3 taps")
    c8 = (cin + 7) // 8
    if weight.is_cuda:
        w = weight.detach().to(torch.float32).contiguous()
        out = torch.empty((cout // 64, c8, 14, 2, 2, 64, 8), dtype=torch.bfloat16, device=w.device)
        with torch.cuda.device(w.device):
            _lib.check(_lib.load().mvsdet_split_conv_weight_ordered(_lib.ptr(w), _lib.ptr(out), cout, cin, order, _stream(w)),
                       "split_conv_weight")
        return out
    w = weight.detach().to(torch.float32)
    w = (w.transpose(0, 1) if order == 2 else w).reshape(cout, cin, 27)
    taps = torch.tensor(_tap_table(order))
    w = torch.where(taps.view(1, 1, 28) >= 0, w[:, :, taps.clamp(min=0)], torch.zeros(()))   # (Cout, Cin, 28) in pair order
    w = torch.nn.functional.pad(w, (0, 0, 0, c8 * 8 - cin))                                  # channels -> 8*c8
    pieces = torch.stack(split_bf16(w), 0)                                                  # (piece, Cout, C, 28)
    if order == 0:
        # channel = ob*64 + 32q + 8mh + 4b + ml (row group rg = 2q + b, row m = 4mh + ml), tap = 4ks + kg
        # (piece, ob, q, mh, b, ml, c8, j, ks, kg) -> (ob, c8, ks, q, b, piece, kg, mh, ml, j)
        pieces = pieces.reshape(2, cout // 64, 2, 4, 2, 4, c8, 8, 7, 4).permute(1, 6, 8, 2, 4, 0, 9, 3, 5, 7)
        return pieces.contiguous().reshape(cout // 64, c8, 14, 2, 2, 64, 8)
    # (piece, ob, a, m, c8, j, p, h) with row m <- channel ROW_CHANNEL[m]  -> (ob, c8, p, a, piece, h, m, j)
    pieces = pieces.reshape(2, cout // 64, 2, 32, c8, 8, 14, 2)[:, :, :, torch.tensor(ROW_CHANNEL)].permute(1, 4, 6, 2, 0, 7, 3, 5)
    return pieces.contiguous().reshape(cout // 64, c8, 14, 2, 2, 64, 8)


def split_conv_weights(items) -> list:
    """`split_conv_weight` of several (weight, order) pairs in ONE launch (up to 8 per launch): a network's layers, cut anew on
    every forward call so that an in-place weight update -- also one through `.data`, which bumps no version counter -- is seen."""
    items = list(items)
    outs = []
    lib = _lib.load()
    for lo in range(0, len(items), 8):
        chunk = items[lo:lo + 8]
        ws, cins, couts, orders, res = [], [], [], [], []
        for weight, order in chunk:
            cin, cout = (weight.shape[:2] if order == 2 else weight.shape[1::-1])
            if cout % 64 or tuple(weight.shape[2:]) != (3, 3, 3) or order not in (0, 1, 2) or not weight.is_cuda:
                raise ValueError(f"split_conv_weights: weight {tuple(weight.shape)} (order {order})")
            ws.append(weight.detach().to(torch.float32).contiguous())
            res.append(torch.empty((cout // 64, (cin + 7) // 8, 14, 2, 2, 64, 8), dtype=torch.bfloat16, device=weight.device))
            cins.append(int(cin)); couts.append(int(cout)); orders.append(int(order))
        n = len(chunk)
        wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
        op = (ctypes.c_void_p * n)(*[r.data_ptr() for r in res])
        ia = lambda v: (ctypes.c_int * n)(*v)   # noqa: E731
        with torch.cuda.device(ws[0].device):
            _lib.check(lib.mvsdet_split_conv_weights_batched(wp, op, ia(couts), ia(cins), ia(orders), n, _stream(ws[0])),
                       "split_conv_weights_batched")
        outs.extend(res)
    return outs


class SclTensor:
    """An activation in the split channel-last form the bf16x3 convolutions read (include/mvsdet_hip.h): `data` is the
    flat bfloat16 buffer [2][N][ceil(C/8)][Dp][Hp][Wp][8] with a zero border; `shape` the logical (N,C,D,H,W)."""

    def __init__(self, data: Tensor, shape, padded):
        self.data, self.shape, self.padded = data, tuple(int(v) for v in shape), tuple(int(v) for v in padded)

    def pieces(self):
        """(hi, mid) as (N, C8*8, D, H, W) bfloat16 tensors (interior only) -- for tests."""
        n, c, d, h, w = self.shape
        c8 = (c + 7) // 8
        dp, hp, wp = self.padded
        v = self.data.view(2, n, c8, dp, hp, wp, 8)[:, :, :, 1:d + 1, 1:h + 1, 1:w + 1]
        v = v.permute(0, 1, 2, 6, 3, 4, 5).reshape(2, n, c8 * 8, d, h, w)
        return v[0], v[1]

    def border_is_zero(self) -> bool:
        """Everything outside the interior voxels (tests: a producing kernel must not write there)."""
        n, c, d, h, w = self.shape
        dp, hp, wp = self.padded
        v = self.data.view(2, n, (c + 7) // 8, dp, hp, wp, 8).clone()
        v[:, :, :, 1:d + 1, 1:h + 1, 1:w + 1] = 0
        return not bool(v.view(torch.int16).any())


class PsclTensor:
    """The parity-split SCL form (include/mvsdet_hip.h): flat bfloat16 buffer [2][8 classes][N][ceil(C/8)][cDp][cHp][cWp][8];
    class = 4*(d&1) + 2*(h&1) + (w&1), voxel (d,h,w) at index (d//2 + 1, h//2 + 1, w//2 + 1) of its class."""

    def __init__(self, data: Tensor, shape, padded):
        self.data, self.shape, self.padded = data, tuple(int(v) for v in shape), tuple(int(v) for v in padded)

    def pieces(self):
        """(hi, mid) as (N, C8*8, D, H, W) bfloat16 tensors, and whether everything else in the buffer is zero -- for tests."""
        n, c, d, h, w = self.shape
        c8 = (c + 7) // 8
        dp, hp, wp = self.padded
        v = self.data.view(2, 8, n, c8, dp, hp, wp, 8)
        out = torch.zeros((2, n, c8, d, h, w, 8), dtype=torch.bfloat16, device=self.data.device)
        rest = v.clone()
        for cls in range(8):
            pd, ph, pw = cls >> 2, (cls >> 1) & 1, cls & 1
            nd, nh, nw = (d - pd + 1) // 2, (h - ph + 1) // 2, (w - pw + 1) // 2
            out[:, :, :, pd::2, ph::2, pw::2] = v[:, cls, :, :, 1:nd + 1, 1:nh + 1, 1:nw + 1]
            rest[:, cls, :, :, 1:nd + 1, 1:nh + 1, 1:nw + 1] = 0
        out = out.permute(0, 1, 2, 6, 3, 4, 5).reshape(2, n, c8 * 8, d, h, w)
        return out[0], out[1], not bool(rest.view(torch.int16).any())


def scl_geometry(N: int, C: int, D: int, H: int, W: int):
    """(bytes, (Dp, Hp, Wp)) of the SCL form of an (N,C,D,H,W) activation."""
    dp, hp, wp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    nbytes = _lib.load().mvsdet_scl_bytes(N, C, D, H, W, ctypes.byref(dp), ctypes.byref(hp), ctypes.byref(wp))
    return int(nbytes), (dp.value, hp.value, wp.value)


def pscl_geometry(N: int, C: int, D: int, H: int, W: int):
    """(bytes, (cDp, cHp, cWp)) of the parity-split SCL form of an (N,C,D,H,W) activation."""
    dp, hp, wp = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    nbytes = _lib.load().mvsdet_pscl_bytes(N, C, D, H, W, ctypes.byref(dp), ctypes.byref(hp), ctypes.byref(wp))
    return int(nbytes), (dp.value, hp.value, wp.value)


def scl_empty(shape, device) -> SclTensor:
    """A zeroed SCL buffer for an (N,C,D,H,W) result: a producing convolution fills the interior, the border stays zero."""
    nbytes, padded = scl_geometry(*[int(v) for v in shape])
    return SclTensor(torch.zeros((nbytes // 2,), dtype=torch.bfloat16, device=device), shape, padded)


def pscl_empty(shape, device) -> PsclTensor:
    nbytes, padded = pscl_geometry(*[int(v) for v in shape])
    return PsclTensor(torch.zeros((nbytes // 2,), dtype=torch.bfloat16, device=device), shape, padded)


def pscl_from_tensor(x: Tensor) -> PsclTensor:
    """(N,C,D,H,W) fp32 -> PsclTensor with torch operators (tests and tools: in the product the form is written by the
    producing convolution's epilogue)."""
    n, c, d, h, w = x.shape
    c8 = (c + 7) // 8
    out = pscl_empty(x.shape, x.device)
    dp, hp, wp = out.padded
    v = out.data.view(2, 8, n, c8, dp, hp, wp, 8)
    xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, 0, 0, c8 * 8 - c))
    for piece, t in enumerate(split_bf16(xp)):
        t = t.view(n, c8, 8, d, h, w).permute(0, 1, 3, 4, 5, 2)           # (n, c8, d, h, w, 8)
        for cls in range(8):
            pd, ph, pw = cls >> 2, (cls >> 1) & 1, cls & 1
            sub = t[:, :, pd::2, ph::2, pw::2]
            v[piece, cls, :, :, 1:sub.shape[2] + 1, 1:sub.shape[3] + 1, 1:sub.shape[4] + 1] = sub
    return out


def scl_pack(x: Tensor, out: Optional[SclTensor] = None) -> SclTensor:
    """(N,C,D,H,W) fp32 -> SclTensor.  x may be any view whose last dimension has stride 1 (a row-pitched cost volume is
    read in place).  `out`: a buffer of the same shape to refill (its border is already zero); without one the result is a
    new buffer from the caching allocator whose border the packing kernel writes itself (no clearing pass, nothing kept)."""
    _req(x, "x", dim=5)
    if x.stride(4) != 1 or min(x.stride()) < 0:
        x = x.contiguous()
    N, C, D, H, W = x.shape
    nbytes, padded = scl_geometry(N, C, D, H, W)
    fresh = out is None or out.shape != tuple(x.shape) or out.data.device != x.device
    if fresh:
        out = SclTensor(torch.empty((nbytes // 2,), dtype=torch.bfloat16, device=x.device), x.shape, padded)
    xstr = (ctypes.c_int64 * 4)(*[int(v) for v in x.stride()[:4]])
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_scl_pack_f32(_lib.ptr(x), xstr, _lib.ptr(out.data), N, C, D, H, W, 2 if fresh else 0, _stream(x)),
                   "scl_pack")
    return out


def gemm_split_weight(wmat: Tensor) -> Tensor:
    """(M, K) fp32 row-major -> the fragment-ordered bf16 pieces the neck's GEMM-shaped layers stream from L2
    ([M/32][K/16][2 pieces][64 lanes][8] bf16; M % 128 == 0, K % 32 == 0: include/mvsdet_hip.h)."""
    _req(wmat, "wmat", dim=2)
    M, K = wmat.shape
    lib = _lib.load()
    nbytes = int(lib.mvsdet_gemm_split_weight_bytes(int(M), int(K)))
    if nbytes == 0:
        raise ValueError(f"gemm_split_weight: ({M}, {K}) is not (128 m, 32 k)")
    w = wmat.detach().contiguous()
    out = torch.empty((nbytes // 2,), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(lib.mvsdet_gemm_split_weight(_lib.ptr(w), _lib.ptr(out), int(M), int(K), _stream(w)), "gemm_split_weight")
    return out


def _check_wsplit(name: str, wsplit: Tensor, rows: int, cin: int, like: Tensor):
    """A split weight is read as [rows/32][cin/16][2][64][8] bf16 with no further check in the kernel: one made for another
    (rows, Cin) would be read out of bounds."""
    need = int(_lib.load().mvsdet_gemm_split_weight_bytes(int(rows), int(cin)))
    if need == 0:
        raise ValueError(f"{name}: ({rows}, {cin}) is not a (128 m, 32 k) layer")
    if not isinstance(wsplit, Tensor) or wsplit.dtype != torch.bfloat16 or not wsplit.is_contiguous() or wsplit.device != like.device:
        raise TypeError(f"{name}: wsplit must be the contiguous bfloat16 tensor gemm_split_weight made, on the input's device")
    if wsplit.numel() * 2 != need:
        raise ValueError(f"{name}: wsplit holds {wsplit.numel() * 2} bytes, a ({rows}, {cin}) layer's split weight {need}")


def gemm_layer_ok(rows: int, cin: int) -> bool:
    """Whether the neck's GEMM kernels take a layer with this many matrix rows (Cout, or 8 Cout for the transposed one) and Cin."""
    return rows % 128 == 0 and cin % 32 == 0


def conv3d_k1_s2_bf16x3(x: Tensor, wsplit: Tensor, bias: Tensor, cout: int, relu: bool = False) -> Tensor:
    """Conv3d(kernel 1, stride 2) + bias [+ ReLU] of an (N,Cin,D,H,W) tensor with even D, H, W: one GEMM over the sub-sampled voxels,
    the sub-sampling in its gather (imvoxel_neck.py:196-217 `downsample` with the eval-mode BatchNorm folded in)."""
    _req(x, "x", dim=5)
    _req(bias, "bias", dim=1)
    x = x.contiguous()
    N, Cin, D, H, W = x.shape
    if D % 2 or H % 2 or W % 2 or bias.numel() != cout:
        raise ValueError("conv3d_k1_s2_bf16x3: D, H, W must be even and bias have Cout elements")
    _check_wsplit("conv3d_k1_s2_bf16x3", wsplit, cout, Cin, x)
    out = torch.empty((N, cout, D // 2, H // 2, W // 2), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_conv3d_k1_s2_bf16x3(_lib.ptr(x), _lib.ptr(wsplit), _lib.ptr(bias.contiguous()), _lib.ptr(out), N, Cin,
                                                          int(cout), D, H, W, int(relu), _stream(x)), "conv3d_k1_s2_bf16x3")
    return out


def convT3d_k2_s2_bf16x3(x: Tensor, wsplit: Tensor, bias: Tensor, cout: int, relu: bool = True) -> Tensor:
    """ConvTranspose3d(kernel 2, stride 2) + bias [+ ReLU]: (N,Cin,D,H,W) -> (N,Cout,2D,2H,2W), the 2x2x2 interleave written by the
    GEMM's epilogue (imvoxel_neck.py:166-180).  `wsplit` = gemm_split_weight of the (8 Cout, Cin) matrix with rows 8 o + 4 p + 2 q + r."""
    _req(x, "x", dim=5)
    _req(bias, "bias", dim=1)
    x = x.contiguous()
    N, Cin, D, H, W = x.shape
    if bias.numel() != cout:
        raise ValueError("convT3d_k2_s2_bf16x3: bias must have Cout elements")
    _check_wsplit("convT3d_k2_s2_bf16x3", wsplit, 8 * cout, Cin, x)
    out = torch.empty((N, cout, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_convT3d_k2_s2_bf16x3(_lib.ptr(x), _lib.ptr(wsplit), _lib.ptr(bias.contiguous()), _lib.ptr(out), N, Cin,
                                                           int(cout), D, H, W, int(relu), _stream(x)), "convT3d_k2_s2_bf16x3")
    return out



# ---- the two GEMM-shaped layers under autograd: input and weight gradients (csrc/neck_gemm.hip MODEs 2 / 3, neck_gemm_dw_bf16x3_kernel)
@torch.library.custom_op(f"{_NS}::conv3d_k1_s2_dx_bf16x3", mutates_args=("grad_x",), device_types="cuda")
def conv3d_k1_s2_dx_bf16x3(grad_out: Tensor, wsplit: Tensor, grad_x: Tensor) -> None:
    """Input gradient of Conv3d(kernel 1, stride 2, no bias) ACCUMULATED into `grad_x` (N,Cin,D,H,W) at its even positions only:
    grad_x[:, c, 2d, 2h, 2w] += sum_o W[o, c] grad_out[:, o, d, h, w].  `wsplit` = gemm_split_weight of the (Cin, Cout) matrix W^T.
    The other positions of grad_x are left as they are (the caller's tensor holds the gradient of the block's other branch)."""
    _req(grad_out, "grad_out", dim=5)
    _req(grad_x, "grad_x", dim=5)
    if not grad_x.is_contiguous():
        raise ValueError("conv3d_k1_s2_dx_bf16x3: grad_x must be contiguous (it is accumulated in place)")
    grad_out = grad_out.contiguous()
    N, Cin, D, H, W = grad_x.shape
    Cout = grad_out.shape[1]
    if D % 2 or H % 2 or W % 2 or tuple(grad_out.shape) != (N, Cout, D // 2, H // 2, W // 2):
        raise ValueError(f"conv3d_k1_s2_dx_bf16x3: grad_out {tuple(grad_out.shape)} does not match grad_x {tuple(grad_x.shape)} at stride 2")
    _check_wsplit("conv3d_k1_s2_dx_bf16x3", wsplit, Cin, Cout, grad_out)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().mvsdet_conv3d_k1_s2_dx_bf16x3(_lib.ptr(grad_out), _lib.ptr(wsplit), _lib.ptr(grad_x), N, Cin, Cout, D, H, W,
                                                             _stream(grad_out)), "conv3d_k1_s2_dx_bf16x3")


@conv3d_k1_s2_dx_bf16x3.register_fake
def _(grad_out, wsplit, grad_x):
    return None


@torch.library.custom_op(f"{_NS}::convT3d_k2_s2_dx_bf16x3", mutates_args=(), device_types="cuda")
def convT3d_k2_s2_dx_bf16x3(grad_out: Tensor, wsplit: Tensor, cin: int) -> Tensor:
    """Input gradient of ConvTranspose3d(kernel 2, stride 2, no bias): grad_out (N,Cout,2D,2H,2W) -> (N,Cin,D,H,W),
    grad_x[:, c, v] = sum_{o,p,q,r} W[c, o, p, q, r] grad_out[:, o, 2v + (p, q, r)].  `wsplit` = gemm_split_weight of W.reshape(Cin, 8 Cout)."""
    _req(grad_out, "grad_out", dim=5)
    grad_out = grad_out.contiguous()
    N, Cout, D2, H2, W2 = grad_out.shape
    if D2 % 2 or H2 % 2 or W2 % 2:
        raise ValueError(f"convT3d_k2_s2_dx_bf16x3: grad_out {tuple(grad_out.shape)} must have even D, H, W")
    _check_wsplit("convT3d_k2_s2_dx_bf16x3", wsplit, int(cin), 8 * Cout, grad_out)
    gx = torch.empty((N, int(cin), D2 // 2, H2 // 2, W2 // 2), dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().mvsdet_convT3d_k2_s2_dx_bf16x3(_lib.ptr(grad_out), _lib.ptr(wsplit), _lib.ptr(gx), N, int(cin), Cout, D2 // 2,
                                                              H2 // 2, W2 // 2, _stream(grad_out)), "convT3d_k2_s2_dx_bf16x3")
    return gx


@convT3d_k2_s2_dx_bf16x3.register_fake
def _(grad_out, wsplit, cin):
    return grad_out.new_empty((grad_out.shape[0], int(cin)) + tuple(s // 2 for s in grad_out.shape[2:]))


def neck_gemm_dw_splits(rows: int, cols: int, voxels: int) -> int:
    """Split-K of the weight-gradient GEMM: enough 64 x 64 tiles x chunks for two blocks per CU of the 256, no chunk under one step."""
    tiles = -(-rows // 64) * -(-cols // 64)
    return max(1, min(-(-512 // tiles), -(-voxels // 32)))


@torch.library.custom_op(f"{_NS}::neck_gemm_dw_bf16x3", mutates_args=(), device_types="cuda")
def neck_gemm_dw_bf16x3(x: Tensor, grad_out: Tensor, transposed: bool, nsplit: int = 0) -> Tensor:
    """Weight gradient of the neck's GEMM-shaped layers on the bf16 matrix cores (three-term split operands, deterministic):
    transposed=False: Conv3d(kernel 1, stride 2), x (N,Cin,D,H,W), grad_out (N,Cout,D/2,H/2,W/2) -> (Cout, Cin, 1, 1, 1);
    transposed=True: ConvTranspose3d(kernel 2, stride 2), x (N,Cin,D,H,W), grad_out (N,Cout,2D,2H,2W) -> (Cin, Cout, 2, 2, 2).
    nsplit: voxel chunks summed separately and added in order (0 = automatic, `neck_gemm_dw_splits`)."""
    _req(x, "x", dim=5)
    _req(grad_out, "grad_out", dim=5)
    x, grad_out = x.contiguous(), grad_out.contiguous()
    N, Cin = x.shape[:2]
    Cout = grad_out.shape[1]
    if transposed:
        ok = tuple(grad_out.shape) == (N, Cout) + tuple(2 * s for s in x.shape[2:])
        coarse = tuple(x.shape[2:])
    else:
        ok = all(s % 2 == 0 for s in x.shape[2:]) and tuple(grad_out.shape) == (N, Cout) + tuple(s // 2 for s in x.shape[2:])
        coarse = tuple(grad_out.shape[2:])
    if not ok:
        raise ValueError(f"neck_gemm_dw_bf16x3: grad_out {tuple(grad_out.shape)} does not match x {tuple(x.shape)} "
                         f"({'transposed ' if transposed else ''}stride 2)")
    D, H, W = coarse
    rows, cols = (Cin, 8 * Cout) if transposed else (Cout, Cin)
    if nsplit <= 0:
        nsplit = neck_gemm_dw_splits(rows, cols, N * D * H * W)
    lib = _lib.load()
    dw = torch.empty((Cin, Cout, 2, 2, 2) if transposed else (Cout, Cin, 1, 1, 1), dtype=torch.float32, device=x.device)
    pbytes = int(lib.mvsdet_neck_gemm_dw_partial_bytes(int(Cin), int(Cout), int(transposed), int(nsplit)))
    partial = torch.empty((pbytes // 4,), dtype=torch.float32, device=x.device) if pbytes else None
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_neck_gemm_dw_bf16x3(_lib.ptr(x), _lib.ptr(grad_out), _lib.ptr(dw), _lib.ptr(partial), pbytes, int(nsplit),
                                                  int(transposed), N, Cin, Cout, D, H, W, _stream(x)), "neck_gemm_dw_bf16x3")
    return dw


@neck_gemm_dw_bf16x3.register_fake
def _(x, grad_out, transposed, nsplit=0):
    cin, cout = x.shape[1], grad_out.shape[1]
    return x.new_empty((cin, cout, 2, 2, 2) if transposed else (cout, cin, 1, 1, 1))


def _conv_input(x, form=()):
    """A convolution's input: an object of the pre-cut `form` (SclTensor / PsclTensor), or the fp32 (N,Cin,D,H,W) tensor itself --
    any view with w stride 1 and no negative stride, else its contiguous copy.
    -> (x, whether it is the pre-cut form, N, Cin, D, H, W, device, HOST strides of n, c, d, h or None for the pre-cut form)."""
    if isinstance(x, form):
        return (x, True, *x.shape, x.data.device, None)
    _req(x, "x", dim=5)
    if x.stride(4) != 1 or min(x.stride()) < 0:
        x = x.contiguous()
    return (x, False, *x.shape, x.device, _lib.strides4_of5(x))


def _check_weight_split(name, weight_split, Cin):
    """Cout of a `split_conv_weight` result cut for Cin input channels."""
    if weight_split.dtype != torch.bfloat16 or weight_split.dim() != 7 or tuple(weight_split.shape[1:]) != ((Cin + 7) // 8, 14, 2, 2, 64, 8):
        raise ValueError(f"{name}: weight_split {tuple(weight_split.shape)} does not match Cin={Cin}")
    return weight_split.shape[0] * 64


def _check_pivot(name, pivot, Cout, dev):
    if pivot is None:
        return None
    if pivot.dtype != torch.float32 or pivot.numel() != Cout or pivot.device != dev:
        raise ValueError(f"{name}: pivot must be {Cout} fp32 values on {dev}")
    return pivot.detach().contiguous()


def _check_affine(name, scale, shift, Cout):
    if (scale is None) != (shift is None):
        raise ValueError(f"{name}: scale and shift come together")
    if scale is not None:
        _req(scale, "scale", dim=1)
        _req(shift, "shift", dim=1)
        if scale.numel() != Cout or shift.numel() != Cout:
            raise ValueError(f"{name}: scale / shift must have {Cout} elements")
        return scale.contiguous(), shift.contiguous()
    return None, None


def _conv_outputs(name, outputs, shape, dev, scl_out, pscl_out, allow_pscl=True):
    """The output buffers a convolution was asked for: `outputs` is a sequence out of "f32", "scl", "pscl" (order = order of
    the returned values); `scl_out` / `pscl_out` are buffers of the same shape to refill (their borders are already zero)."""
    if isinstance(outputs, str):
        outputs = (outputs,)
    bad = [o for o in outputs if o not in ("f32", "scl") + (("pscl",) if allow_pscl else ())]
    if bad or not outputs:
        raise ValueError(f"{name}: outputs {outputs!r}")
    res = {}
    if "f32" in outputs:
        res["f32"] = torch.empty(shape, dtype=torch.float32, device=dev)
    if "scl" in outputs:
        ok = scl_out is not None and scl_out.shape == tuple(shape) and scl_out.data.device == dev
        res["scl"] = scl_out if ok else scl_empty(shape, dev)
    if "pscl" in outputs:
        ok = pscl_out is not None and pscl_out.shape == tuple(shape) and pscl_out.data.device == dev
        res["pscl"] = pscl_out if ok else pscl_empty(shape, dev)
    return outputs, res


def _ret(outputs, res):
    vals = tuple(res[o] for o in outputs)
    return vals[0] if len(vals) == 1 else vals


def conv3d_k3_bf16x3(x, weight_split: Tensor, scale: Optional[Tensor], shift: Optional[Tensor], relu: bool,
                     residual: Optional[Tensor] = None, outputs=("f32",), scl_out: Optional[SclTensor] = None,
                     pscl_out: Optional[PsclTensor] = None):
    """Conv3d(Cin -> Cout = 64*m, kernel 3, stride 1, padding 1, no bias) [+ affine] [+ residual] [+ ReLU] on the bf16
    matrix cores with three-term split operands (csrc/costreg_bf16.hip).
    x: the fp32 (N,Cin,D,H,W) tensor itself (any view with w stride 1: cut into pieces inside the kernel, no extra pass) or
    its SclTensor form (scl_pack, or a producing layer's "scl" output) -- identical results.
    outputs: any of "f32" (the (N,Cout,D,H,W) tensor), "scl" (SclTensor: already cut for a stride-1 / transposed consumer),
    "pscl" (PsclTensor: for a stride-2 consumer); one value or a tuple in that order is returned."""
    x, scl, N, Cin, D, H, W, dev, xstr = _conv_input(x, SclTensor)
    Cout = _check_weight_split("conv3d_k3_bf16x3", weight_split, Cin)
    scale, shift = _check_affine("conv3d_k3_bf16x3", scale, shift, Cout)
    outputs, res = _conv_outputs("conv3d_k3_bf16x3", outputs, (N, Cout, D, H, W), dev, scl_out, pscl_out)
    if residual is not None:
        _req(residual, "residual", dim=5)
        if tuple(residual.shape) != (N, Cout, D, H, W):
            raise ValueError(f"conv3d_k3_bf16x3: residual {tuple(residual.shape)} != output {(N, Cout, D, H, W)}")
        residual = residual.contiguous()
    weight_split = weight_split.contiguous()
    lib = _lib.load()
    # small volumes: partial sums of the input-channel splits (0 bytes: the grid fills the chip unsplit); fp32 output only
    wbytes = lib.mvsdet_conv3d_k3_bf16x3_workspace_bytes(N, Cin, Cout, D, H, W) if tuple(outputs) == ("f32",) else 0
    ws = torch.empty((wbytes // 4,), dtype=torch.float32, device=dev) if wbytes else None
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_conv3d_k3_bf16x3_io(_lib.ptr(x.data) if scl else None, None if scl else _lib.ptr(x), xstr,
                                                  _lib.ptr(weight_split), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(residual),
                                                  _lib.ptr(res.get("f32")), _lib.ptr(res["scl"].data) if "scl" in res else None,
                                                  _lib.ptr(res["pscl"].data) if "pscl" in res else None, _lib.ptr(ws), wbytes,
                                                  N, Cin, Cout, D, H, W, int(relu), _lib.current_stream(dev)), "conv3d_k3_bf16x3")
    return _ret(outputs, res)


def split_conv_weight_mx(weight: Tensor) -> Tensor:
    """(Cout = 64 m, Cin, 3,3,3) fp32 -> the operand image of `conv3d_k3_fp16mx`: per (block of 64 outputs, 8 input channels, sub-stage)
    32 x 64 sixteen-byte units -- fp16 fragments of the weights and block-scaled e2m3 fragments of their fp16 roundings and of the
    remainders (csrc/costreg_mx.h).  A few hundred thousand elements: cut on every call, like the bf16x3 pieces."""
    _req(weight, "weight", dim=5)
    Cout, Cin = weight.shape[:2]
    lib = _lib.load()
    nbytes = int(lib.mvsdet_split_conv_weight_mx_bytes(int(Cout), int(Cin)))
    if nbytes == 0 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError(f"split_conv_weight_mx: weight {tuple(weight.shape)} is not (64 m, Cin, 3, 3, 3)")
    w = weight.detach().contiguous()
    out = torch.empty((Cout // 64, (Cin + 7) // 8, 2, 32, 64, 4), dtype=torch.int32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(lib.mvsdet_split_conv_weight_mx(_lib.ptr(w), _lib.ptr(out), int(Cout), int(Cin), _stream(w)), "split_conv_weight_mx")
    return out


def conv3d_k3_fp16mx_ok(x: Tensor) -> bool:
    """Whether `conv3d_k3_fp16mx` runs this view of x on the fp16 + MX kernel: its 32-bit buffer offsets must cover the view
    (include/mvsdet_hip.h mvsdet_conv3d_k3_fp16mx_ok: a batch element's Cin channels below 4 GiB of span, and with Cin % 8 != 0 no
    channels interleaved with the planes)."""
    copied = x.stride(4) != 1 or min(x.stride()) < 0          # `conv3d_k3_fp16mx` reads a contiguous copy of such a view
    xstr = None if copied else _lib.strides4_of5(x)
    return bool(_lib.load().mvsdet_conv3d_k3_fp16mx_ok(*[int(v) for v in x.shape], xstr))


def conv3d_k3_fp16mx(x: Tensor, weight_split_mx: Tensor, scale: Optional[Tensor], shift: Optional[Tensor], relu: bool,
                     outputs=("f32",), scl_out: Optional[SclTensor] = None, pscl_out: Optional[PsclTensor] = None,
                     weight: Optional[Tensor] = None):
    """Conv3d(Cin -> Cout = 64 m, kernel 3, stride 1, padding 1, no bias) [+ affine] [+ ReLU] of the fp32 (N,Cin,D,H,W) tensor read in
    place (any view with w stride 1), on ONE fp16 and TWO block-scaled FP6 products per fp32-equivalent product (csrc/costreg_mx.h:
    v_mfma_f32_16x16x32_f16 + v_mfma_scale_f32_16x16x128_f8f6f4) instead of bf16x3's three: mvsnet.py:76, the layer that reads the
    variance volume.  weight_split_mx: `split_conv_weight_mx`.  outputs as for `conv3d_k3_bf16x3`.  Error bound: include/mvsdet_hip.h
    (2^-14 of the products' block maxima; ~2^-15 of the output's scale on data of uniform magnitude).
    A view the kernel cannot address (`conv3d_k3_fp16mx_ok` False: 4 GiB or more of span per batch element, or interleaved channels) runs on
    `conv3d_k3_bf16x3` instead, cut from `weight` -- the fp32 (Cout, Cin, 3, 3, 3) weight the split was made from, required then."""
    x, _, N, Cin, D, H, W, dev, xstr = _conv_input(x)
    if not conv3d_k3_fp16mx_ok(x):
        if weight is None:
            raise ValueError(f"conv3d_k3_fp16mx: the view {tuple(x.shape)} / {tuple(x.stride())} is beyond the fp16 + MX kernel's "
                             "addressing (conv3d_k3_fp16mx_ok): pass weight= for the bf16x3 kernel")
        return conv3d_k3_bf16x3(x, split_conv_weight(weight), scale, shift, relu, outputs=outputs, scl_out=scl_out, pscl_out=pscl_out)
    if (weight_split_mx.dtype != torch.int32 or weight_split_mx.dim() != 6 or not weight_split_mx.is_contiguous()
            or tuple(weight_split_mx.shape[1:]) != ((Cin + 7) // 8, 2, 32, 64, 4) or weight_split_mx.device != dev):
        raise ValueError(f"conv3d_k3_fp16mx: weight_split_mx {tuple(weight_split_mx.shape)} {weight_split_mx.dtype} does not match Cin={Cin}")
    Cout = weight_split_mx.shape[0] * 64
    scale, shift = _check_affine("conv3d_k3_fp16mx", scale, shift, Cout)
    outputs, res = _conv_outputs("conv3d_k3_fp16mx", outputs, (N, Cout, D, H, W), dev, scl_out, pscl_out)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_conv3d_k3_fp16mx_f32in(_lib.ptr(x), xstr, _lib.ptr(weight_split_mx), _lib.ptr(scale), _lib.ptr(shift),
                                                             _lib.ptr(res.get("f32")), _lib.ptr(res["scl"].data) if "scl" in res else None,
                                                             _lib.ptr(res["pscl"].data) if "pscl" in res else None, N, Cin, Cout, D, H, W,
                                                             int(relu), _lib.current_stream(dev)), "conv3d_k3_fp16mx")
    return _ret(outputs, res)


def conv3d_k3_bf16x3_stats(x, weight_split: Tensor, pivot: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """`conv3d_k3_bf16x3(x, weight_split, None, None, False)` in front of a training-mode BatchNorm (module.py:26-37): the raw
    fp32 output and, from the kernel's epilogue, the per-channel partial sums of the outputs and of their squares -- a float64
    tensor (Cout, parts, 2), one entry per block of the grid -- that `bn3d_relu_train(..., parts=)` finishes: the BatchNorm then
    reads the tensor once.  pivot (Cout floats, e.g. the BatchNorm's running mean): the sums are those of (value - pivot_c), which
    keeps fp32 lane sums from cancelling when a channel's mean is far from zero; pass the same vector to `bn3d_relu_train`."""
    x, scl, N, Cin, D, H, W, dev, xstr = _conv_input(x, SclTensor)
    Cout = _check_weight_split("conv3d_k3_bf16x3_stats", weight_split, Cin)
    weight_split = weight_split.contiguous()
    pivot = _check_pivot("conv3d_k3_bf16x3_stats", pivot, Cout, dev)
    lib = _lib.load()
    parts = int(lib.mvsdet_conv3d_k3_bf16x3_stats_parts(N, D, H, W, 0 if scl else 1))
    out = torch.empty((N, Cout, D, H, W), dtype=torch.float32, device=dev)
    stats = torch.empty((Cout, parts, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_conv3d_k3_bf16x3_stats(_lib.ptr(x.data) if scl else None, None if scl else _lib.ptr(x), xstr,
                                                     _lib.ptr(weight_split), _lib.ptr(out), _lib.ptr(stats), stats.numel() * 8,
                                                     _lib.ptr(pivot), N, Cin, Cout, D, H, W, _lib.current_stream(dev)),
                   "conv3d_k3_bf16x3_stats")
    return out, stats


def conv3d_k3_s2_bf16x3(x, weight_split: Tensor, scale: Optional[Tensor], shift: Optional[Tensor], relu: bool,
                        outputs=("f32",), scl_out: Optional[SclTensor] = None):
    """Conv3d(Cin -> Cout = 64*m, kernel 3, stride 2, padding 1, no bias) [+ affine] [+ ReLU] (mvsnet.py:77,79) on the bf16
    matrix cores, three-term split: x (N,Cin,D,H,W) fp32 (w stride 1) or its PsclTensor form (a producing layer's "pscl"
    output: the class tiles then arrive by LDS-DMA) -> (N,Cout,(D-1)//2+1,(H-1)//2+1,(W-1)//2+1) as "f32" and / or "scl";
    weight_split = split_conv_weight(weight, order=1)."""
    x, pin, N, Cin, D, H, W, dev, xstr = _conv_input(x, PsclTensor)
    Cout = _check_weight_split("conv3d_k3_s2_bf16x3", weight_split, Cin)
    scale, shift = _check_affine("conv3d_k3_s2_bf16x3", scale, shift, Cout)
    oshape = (N, Cout, (D - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    outputs, res = _conv_outputs("conv3d_k3_s2_bf16x3", outputs, oshape, dev, scl_out, None, allow_pscl=False)
    weight_split = weight_split.contiguous()
    lib = _lib.load()
    wbytes = lib.mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes(N, Cin, Cout, D, H, W) if tuple(outputs) == ("f32",) else 0   # small volumes
    ws = torch.empty((wbytes // 4,), dtype=torch.float32, device=dev) if wbytes else None
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_conv3d_k3_s2_bf16x3_io(None if pin else _lib.ptr(x), xstr, _lib.ptr(x.data) if pin else None,
                                                     _lib.ptr(weight_split), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(res.get("f32")),
                                                     _lib.ptr(res["scl"].data) if "scl" in res else None, _lib.ptr(ws), wbytes, N, Cin,
                                                     Cout, D, H, W, int(relu), _lib.current_stream(dev)), "conv3d_k3_s2_bf16x3")
    return _ret(outputs, res)


def convT3d_k3_s2_bf16x3(x, weight_split: Tensor, scale: Optional[Tensor], shift: Optional[Tensor],
                         residual: Optional[Tensor], relu: bool, outputs=("f32",), scl_out: Optional[SclTensor] = None):
    """ConvTranspose3d(Cin -> Cout = 64*m, kernel 3, stride 2, padding 1, output_padding 1, no bias) [+ affine] [+ ReLU]
    [+ residual, added last] (mvsnet.py:92-100,110-111) on the bf16 matrix cores, three-term split: x (N,Cin,D,H,W) fp32 (or
    its SclTensor) -> (N,Cout,2D,2H,2W) as "f32" and / or "scl"; weight_split = split_conv_weight(weight (Cin,Cout,3,3,3), order=2)."""
    xs = x if isinstance(x, SclTensor) else scl_pack(x)
    N, Cin, D, H, W = xs.shape
    Cout = _check_weight_split("convT3d_k3_s2_bf16x3", weight_split, Cin)
    dev = xs.data.device
    scale, shift = _check_affine("convT3d_k3_s2_bf16x3", scale, shift, Cout)
    oshape = (N, Cout, 2 * D, 2 * H, 2 * W)
    outputs, res = _conv_outputs("convT3d_k3_s2_bf16x3", outputs, oshape, dev, scl_out, None, allow_pscl=False)
    if residual is not None:
        _req(residual, "residual", dim=5)
        if tuple(residual.shape) != oshape:
            raise ValueError(f"convT3d_k3_s2_bf16x3: residual {tuple(residual.shape)} != output {oshape}")
        residual = residual.contiguous()
    weight_split = weight_split.contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_convT3d_k3_s2_bf16x3_io(_lib.ptr(xs.data), _lib.ptr(weight_split), _lib.ptr(scale), _lib.ptr(shift),
                                                              _lib.ptr(residual), _lib.ptr(res.get("f32")),
                                                              _lib.ptr(res["scl"].data) if "scl" in res else None, N, Cin, Cout, D, H, W,
                                                              int(relu), _lib.current_stream(dev)), "convT3d_k3_s2_bf16x3")
    return _ret(outputs, res)


def convT3d_k3_s2_bf16x3_stats(x, weight_split: Tensor, pivot: Optional[Tensor] = None) -> Optional[Tuple[Tensor, Tensor]]:
    """`convT3d_k3_s2_bf16x3(x, weight_split, None, None, None, False)` in front of a training-mode BatchNorm (mvsnet.py:92-100): the
    raw fp32 output and the per-channel partial sums (float64 (Cout, parts, 2), sums of value - pivot_c and of its square) that
    `bn3d_relu_train(..., parts=, pivot=)` finishes.  None where the shape has no statistics form (the plain call applies)."""
    xs = x if isinstance(x, SclTensor) else scl_pack(x)
    N, Cin, D, H, W = xs.shape
    Cout = _check_weight_split("convT3d_k3_s2_bf16x3_stats", weight_split, Cin)
    dev = xs.data.device
    lib = _lib.load()
    parts = int(lib.mvsdet_convT3d_k3_s2_bf16x3_stats_parts(N, D, H, W))
    if parts == 0:
        return None
    pivot = _check_pivot("convT3d_k3_s2_bf16x3_stats", pivot, Cout, dev)
    weight_split = weight_split.contiguous()
    out = torch.empty((N, Cout, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=dev)
    stats = torch.empty((Cout, parts, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mvsdet_convT3d_k3_s2_bf16x3_stats(_lib.ptr(xs.data), _lib.ptr(weight_split), _lib.ptr(out), _lib.ptr(stats),
                                                         stats.numel() * 8, _lib.ptr(pivot), N, Cin, Cout, D, H, W,
                                                         _lib.current_stream(dev)), "convT3d_k3_s2_bf16x3_stats")
    return out, stats


# ------------------------------------------------------------------------------------------- misc
def device_copy(src: Tensor, dst: Tensor):
    """float4 device-to-device copy kernel (bench.py's achievable-HBM yardstick)."""
    _req(src, "src")
    _req(dst, "dst")
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().mvsdet_copy_f32(_lib.ptr(src), _lib.ptr(dst), src.numel(), _stream(src)), "copy")


# ------------------------------------------------------------------------------------------- cost network head (f-1)
def store_pattern_probe(var: Tensor, W: int, tile_w: int, planes_per_block: int = 0) -> None:
    """Overwrites `var` -- an (N,C,D,H,pitch) fp32 or fp16 buffer -- with the sweep's store stream alone (bench.py: the ceiling
    of the output layout on the box at hand)."""
    if var.dtype not in (torch.float32, torch.float16) or not var.is_cuda or not var.is_contiguous() or var.dim() != 5:
        raise ValueError("store_pattern_probe: var must be a contiguous 5-D fp32 or fp16 CUDA tensor")
    N, C, D, H, pitch = var.shape
    lib = _lib.load()
    fn = lib.mvsdet_store_pattern_probe_f32 if var.dtype == torch.float32 else lib.mvsdet_store_pattern_probe_f16
    with torch.cuda.device(var.device):
        _lib.check(fn(_lib.ptr(var), N, C, D, H, int(W), int(pitch), int(tile_w), int(planes_per_block), _stream(var)),
                   "store_pattern_probe")


def conv3d_k3_cout2_sum(x: Tensor, x2: Optional[Tensor], weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """Conv3d(Cin -> 2, kernel 3, padding 1, bias) of mvs_models/mvsnet.py:102,112 on x + x2 (N,Cin,D,H,W) -> (N,2,D,H,W): the
    skip addition of mvsnet.py:111 formed while the head stages its input (forward only; x2 None: x alone)."""
    _req(x, "x", dim=5)
    _req(weight, "weight", dim=5)
    N, Cin, D, H, W = x.shape
    if tuple(weight.shape) != (2, Cin, 3, 3, 3):
        raise ValueError(f"conv3d_k3_cout2_sum: weight {tuple(weight.shape)} != (2,{Cin},3,3,3)")
    if x2 is not None:
        _req(x2, "x2", dim=5)
        if x2.shape != x.shape:
            raise ValueError(f"conv3d_k3_cout2_sum: x2 {tuple(x2.shape)} != x {tuple(x.shape)}")
        if W % 4:
            return conv3d_k3_cout2(x + x2, weight, bias)
        x2 = x2.contiguous()
    if bias is not None:
        _req(bias, "bias", dim=1)
        bias = bias.contiguous()
    x, weight = x.contiguous(), weight.contiguous()
    out = torch.empty((N, 2, D, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_conv3d_k3_cout2_sum_f32(_lib.ptr(x), _lib.ptr(x2), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out),
                                                              N, Cin, D, H, W, _stream(x)), "conv3d_k3_cout2_sum")
    return out


@torch.library.custom_op(f"{_NS}::conv3d_k3_cout2", mutates_args=(), device_types="cuda")
def conv3d_k3_cout2(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """Conv3d(Cin -> 2, kernel 3, stride 1, padding 1) of mvs_models/mvsnet.py:102 on (N,Cin,D,H,W) -> (N,2,D,H,W).
    Forward only: under autograd use torch's convolution (mvsdet_amd.costreg does)."""
    _req(x, "x", dim=5)
    _req(weight, "weight", dim=5)
    N, Cin, D, H, W = x.shape
    if tuple(weight.shape) != (2, Cin, 3, 3, 3):
        raise ValueError(f"conv3d_k3_cout2: weight {tuple(weight.shape)} != (2,{Cin},3,3,3)")
    if bias is not None:
        _req(bias, "bias", dim=1)
        if bias.numel() != 2:
            raise ValueError("conv3d_k3_cout2: bias must have 2 elements")
        bias = bias.contiguous()
    x, weight = x.contiguous(), weight.contiguous()
    out = torch.empty((N, 2, D, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_conv3d_k3_cout2_f32(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out), N, Cin,
                                                          D, H, W, _stream(x)), "conv3d_k3_cout2")
    return out


@conv3d_k3_cout2.register_fake
def _(x, weight, bias):
    return x.new_empty((x.shape[0], 2) + tuple(x.shape[2:]))


def permute_conv_weight(weight: Tensor) -> Tensor:
    """(Cout,Cin,3,3,3) -> the [c][kd][kh][kw][o] layout conv3d_k3_mfma reads (Cin padded to even with zeros)."""
    cout, cin = weight.shape[:2]
    if cout % 64 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError(f"conv3d_k3_mfma: weight {tuple(weight.shape)} != (64*m,Cin,3,3,3)")
    w = weight.detach().permute(1, 2, 3, 4, 0).contiguous()
    if cin % 2:
        w = torch.cat([w, w.new_zeros((1, 3, 3, 3, cout))], 0)
    return w



@torch.library.custom_op(f"{_NS}::conv3d_k3_mfma", mutates_args=(), device_types="cuda")
def conv3d_k3_mfma(x: Tensor, weight_perm: Tensor, scale: Optional[Tensor], shift: Optional[Tensor], relu: bool,
                   stride: int = 1, residual: Optional[Tensor] = None) -> Tensor:
    """Conv3d(Cin -> Cout = 64*m, kernel 3, stride 1 or 2, padding 1, no bias) [+ per-channel affine + ReLU] of
    mvs_models/mvsnet.py:76-82 on the fp32 matrix cores: x (N,Cin,D,H,W), weight_perm = permute_conv_weight(weight)
    -> (N,Cout,D',H',W').  Forward only."""
    _req(x, "x", dim=5)
    _req(weight_perm, "weight_perm", dim=5)
    N, Cin, D, H, W = x.shape
    Cout = weight_perm.shape[4]
    if tuple(weight_perm.shape[:4]) != (Cin + Cin % 2, 3, 3, 3) or Cout % 64:
        raise ValueError(f"conv3d_k3_mfma: weight_perm {tuple(weight_perm.shape)} does not match Cin={Cin}")
    if (scale is None) != (shift is None):
        raise ValueError("conv3d_k3_mfma: scale and shift come together")
    if scale is not None:
        _req(scale, "scale", dim=1)
        _req(shift, "shift", dim=1)
        if scale.numel() != Cout or shift.numel() != Cout:
            raise ValueError(f"conv3d_k3_mfma: scale / shift must have {Cout} elements")
        scale, shift = scale.contiguous(), shift.contiguous()
    if stride not in (1, 2):
        raise ValueError("conv3d_k3_mfma: stride must be 1 or 2")
    x, weight_perm = x.contiguous(), weight_perm.contiguous()
    od, oh, ow = (D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((N, Cout, od, oh, ow), dtype=torch.float32, device=x.device)
    if residual is not None:   # added between the affine and the ReLU (imvoxel_neck.py:227-229); stride 1 only
        _req(residual, "residual", dim=5)
        if stride != 1 or tuple(residual.shape) != tuple(out.shape):
            raise ValueError(f"conv3d_k3_mfma: residual {tuple(residual.shape)} needs stride 1 and the output shape {tuple(out.shape)}")
        residual = residual.contiguous()
    lib = _lib.load()
    # a small volume (the neck at one scene) is split over the input channels: partial sums in a workspace
    wbytes = lib.mvsdet_conv3d_k3_mfma_workspace_bytes(N, Cin, Cout, D, H, W, stride)
    ws = torch.empty((wbytes // 4,), dtype=torch.float32, device=x.device) if wbytes else None
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_conv3d_k3_mfma_ws_f32(_lib.ptr(x), _lib.ptr(weight_perm), _lib.ptr(scale), _lib.ptr(shift),
                                                    _lib.ptr(residual), _lib.ptr(out), _lib.ptr(ws), wbytes, N, Cin, Cout, D, H, W,
                                                    stride, int(relu), _stream(x)), "conv3d_k3_mfma")
    return out


@conv3d_k3_mfma.register_fake
def _(x, weight_perm, scale, shift, relu, stride=1, residual=None):
    return x.new_empty((x.shape[0], weight_perm.shape[4]) + tuple((s - 1) // stride + 1 for s in x.shape[2:]))



def permute_convT_weight(weight: Tensor) -> Tensor:
    """ConvTranspose3d weight (Cin,Cout,3,3,3) -> the [c][kd][kh][kw][o] layout convT3d_k3_s2_mfma reads."""
    cin, cout = weight.shape[:2]
    if cout % 64 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError(f"convT3d_k3_s2_mfma: weight {tuple(weight.shape)} != (Cin,64*m,3,3,3)")
    w = weight.detach().permute(0, 2, 3, 4, 1).contiguous()
    if cin % 2:
        w = torch.cat([w, w.new_zeros((1, 3, 3, 3, cout))], 0)
    return w


@torch.library.custom_op(f"{_NS}::convT3d_k3_s2_mfma", mutates_args=(), device_types="cuda")
def convT3d_k3_s2_mfma(x: Tensor, weight_perm: Tensor, scale: Optional[Tensor], shift: Optional[Tensor],
                       residual: Optional[Tensor], relu: bool) -> Tensor:
    """ConvTranspose3d(kernel 3, stride 2, padding 1, output_padding 1, no bias) [+ affine + ReLU] [+ residual] of
    mvs_models/mvsnet.py:92-100 on the fp32 matrix cores: x (N,Cin,D,H,W) -> (N,Cout,2D,2H,2W).  Forward only."""
    _req(x, "x", dim=5)
    _req(weight_perm, "weight_perm", dim=5)
    N, Cin, D, H, W = x.shape
    Cout = weight_perm.shape[4]
    if tuple(weight_perm.shape[:4]) != (Cin + Cin % 2, 3, 3, 3) or Cout % 64:
        raise ValueError(f"convT3d_k3_s2_mfma: weight_perm {tuple(weight_perm.shape)} does not match Cin={Cin}")
    if (scale is None) != (shift is None):
        raise ValueError("convT3d_k3_s2_mfma: scale and shift come together")
    if scale is not None:
        _req(scale, "scale", dim=1)
        _req(shift, "shift", dim=1)
        if scale.numel() != Cout or shift.numel() != Cout:
            raise ValueError(f"convT3d_k3_s2_mfma: scale / shift must have {Cout} elements")
        scale, shift = scale.contiguous(), shift.contiguous()
    oshape = (N, Cout, 2 * D, 2 * H, 2 * W)
    if residual is not None:
        _req(residual, "residual", dim=5)
        if tuple(residual.shape) != oshape:
            raise ValueError(f"convT3d_k3_s2_mfma: residual {tuple(residual.shape)} != {oshape}")
        residual = residual.contiguous()
    x, weight_perm = x.contiguous(), weight_perm.contiguous()
    out = torch.empty(oshape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_convT3d_k3_s2_mfma_f32(_lib.ptr(x), _lib.ptr(weight_perm), _lib.ptr(scale),
                                                             _lib.ptr(shift), _lib.ptr(residual), _lib.ptr(out), N, Cin, Cout,
                                                             D, H, W, int(relu), _stream(x)), "convT3d_k3_s2_mfma")
    return out


@convT3d_k3_s2_mfma.register_fake
def _(x, weight_perm, scale, shift, residual, relu):
    return x.new_empty((x.shape[0], weight_perm.shape[4]) + tuple(2 * s for s in x.shape[2:]))


@torch.library.custom_op(f"{_NS}::conv3d_k3_dw", mutates_args=(), device_types="cuda")
def conv3d_k3_dw(x: Tensor, grad_out: Tensor, nsplit: int = 0, stride: int = 1, bf16x3: bool = False) -> Tensor:
    """Weight gradient of Conv3d(kernel 3, stride 1 or 2, padding 1): x (N,Cin,D,H,W), grad_out (N,Cout,D/s,H/s,W/s) ->
    (Cout,Cin,3,3,3), on the fp32 matrix cores; `nsplit` voxel splits are accumulated separately and summed
    (0 = automatic: up to 128 splits, fewer when Cin*Cout is large so that the partial sums stay below 256 MB).
    With stride 2 and the tensors exchanged (x = grad of the output, grad_out = the input) this is the weight gradient of
    ConvTranspose3d(kernel 3, stride 2, padding 1, output_padding 1) in its own (Cin,Cout,3,3,3) layout.
    bf16x3: the sum runs on the bf16 matrix cores with three-term split operands (csrc/costreg_dw_bf16.hip; stride 2:
    csrc/costreg_dw_s2_bf16.hip, blocks of 64 grad_out x 16 x channels); rows are read as float4: W a multiple of 4 (stride 2: 8)."""
    _req(x, "x", dim=5)
    _req(grad_out, "grad_out", dim=5)
    if stride not in (1, 2):
        raise ValueError(f"conv3d_k3_dw: stride {stride} not in (1, 2)")
    if bf16x3 and x.shape[-1] % (4 * stride):
        raise ValueError(f"conv3d_k3_dw: the bf16x3 kernel reads rows as float4, W={x.shape[-1]} is not a multiple of {4 * stride}")
    N, Cin, D, H, W = x.shape
    Cout = grad_out.shape[1]
    if any(v % stride for v in (D, H, W)) or tuple(grad_out.shape) != (N, Cout, D // stride, H // stride, W // stride):
        raise ValueError(f"conv3d_k3_dw: grad_out {tuple(grad_out.shape)} does not match x {tuple(x.shape)} at stride {stride}")
    x, grad_out = x.contiguous(), grad_out.contiguous()
    lib = _lib.load()
    if nsplit <= 0:
        nsplit = max(8, min(128, (256 << 20) // (Cout * Cin * 108)))
        if bf16x3:   # one block of 12 waves per CU: 256 / (channel blocks) splits, a multiple of 8 (one split = one XCD)
            cblocks = ((Cin + 31) // 32) * ((Cout + 31) // 32) if stride == 1 else ((Cin + 15) // 16) * ((Cout + 63) // 64)
            nsplit = max(8, min(64, (256 // cblocks) // 8 * 8))
    if bf16x3:       # the kernels keep the columns of a split in a 4096-entry table
        cols = N * ((H + 3) // 4) * ((W + 15) // 16) if stride == 1 else N * ((H // 2 + 3) // 4) * ((W // 2 + 7) // 8)
        nsplit = max(nsplit, -(-cols // 4096))
    pbytes = lib.mvsdet_conv3d_k3_dw_partial_bytes(Cin, Cout, nsplit)
    partial = torch.empty((nsplit, Cout, Cin, 27), dtype=torch.float32, device=x.device)
    fn = lib.mvsdet_conv3d_k3_dw_mfma_f32 if stride == 1 else lib.mvsdet_conv3d_k3_s2_dw_mfma_f32
    if bf16x3:
        fn = lib.mvsdet_conv3d_k3_dw_bf16x3 if stride == 1 else lib.mvsdet_conv3d_k3_s2_dw_bf16x3
    with torch.cuda.device(x.device):
        _lib.check(fn(_lib.ptr(x), _lib.ptr(grad_out), _lib.ptr(partial), pbytes, nsplit, N, Cin, Cout, D, H, W, _stream(x)),
                   "conv3d_k3_dw")
    return partial.sum(0).view(Cout, Cin, 3, 3, 3)


@conv3d_k3_dw.register_fake
def _(x, grad_out, nsplit=0, stride=1, bf16x3=False):
    return x.new_empty((grad_out.shape[1], x.shape[1], 3, 3, 3))


@torch.library.custom_op(f"{_NS}::conv3d_k3_cout2_backward", mutates_args=(), device_types="cuda")
def conv3d_k3_cout2_backward(x: Tensor, weight: Tensor, grad_out: Tensor, nsplit: int = 32,
                             bf16x3: bool = False) -> Tuple[Tensor, Tensor]:
    """Gradients of conv3d_k3_cout2 w.r.t. x (N,Cin,D,H,W) and weight (2,Cin,3,3,3) from grad_out (N,2,D,H,W).
    bf16x3: the weight gradient on the bf16 matrix cores with three-term split operands where its kernel applies
    (Cin in {16, 32, 64}, W % 4 == 0), three blocks per CU; otherwise (and by default) the fp32 kernel with `nsplit` voxel splits."""
    _req(x, "x", dim=5)
    _req(weight, "weight", dim=5)
    _req(grad_out, "grad_out", dim=5)
    N, Cin, D, H, W = x.shape
    if tuple(weight.shape) != (2, Cin, 3, 3, 3) or tuple(grad_out.shape) != (N, 2, D, H, W):
        raise ValueError("conv3d_k3_cout2_backward: shape mismatch")
    x, weight, grad_out = x.contiguous(), weight.contiguous(), grad_out.contiguous()
    lib = _lib.load()
    gx = torch.empty_like(x)
    # the library's own shape gate (channel count, W % 4, the LDS of a row stage: W up to ~470 at Cin = 64); wider maps keep the
    # fp32 kernel instead of raising from the entry point
    on_mfma = (bool(bf16x3) and bool(lib.mvsdet_conv3d_k3_cout2_dw_bf16x3_ok(int(Cin), int(W)))
               and x.data_ptr() % 16 == 0 and grad_out.data_ptr() % 16 == 0)
    if on_mfma:
        nsplit = min(768, N * D * H)   # blocks of four waves, a wave takes whole x rows (n, d, h)
    partial = torch.empty((nsplit, 2, Cin, 27), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_conv3d_k3_cout2_dx_f32(_lib.ptr(grad_out), _lib.ptr(weight), _lib.ptr(gx), N, Cin, D, H, W,
                                                     _stream(x)), "conv3d_k3_cout2_dx")
        fn = lib.mvsdet_conv3d_k3_cout2_dw_bf16x3 if on_mfma else lib.mvsdet_conv3d_k3_cout2_dw_f32
        _lib.check(fn(_lib.ptr(x), _lib.ptr(grad_out), _lib.ptr(partial), partial.numel() * 4, nsplit, N, Cin, D, H, W,
                      _stream(x)), "conv3d_k3_cout2_dw")
    return gx, partial.sum(0).view(2, Cin, 3, 3, 3)


@conv3d_k3_cout2_backward.register_fake
def _(x, weight, grad_out, nsplit=32, bf16x3=False):
    return torch.empty_like(x), torch.empty_like(weight)


def _bn_params(name: str, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], parts: Optional[Tensor],
               pivot: Optional[Tensor]):
    """A training BatchNorm's affine and its statistics from the producing convolution's epilogue, checked against x's channels
    and made contiguous -> (weight, bias, parts, pivot)."""
    C = x.shape[1]
    for t, tname in ((weight, "weight"), (bias, "bias")):
        if t is not None:
            _req(t, tname, dim=1)
            if t.numel() != C:
                raise ValueError(f"{name}: {tname} must have {C} elements")
    if parts is not None:
        if parts.dtype != torch.float64 or parts.dim() != 3 or parts.shape[0] != C or parts.shape[2] != 2 or parts.device != x.device:
            raise ValueError(f"{name}: parts must be float64 ({C}, n, 2) on {x.device}, got {parts.dtype} {tuple(parts.shape)}")
        parts = parts.contiguous()
        if pivot is not None:
            if pivot.dtype != torch.float32 or pivot.numel() != C or pivot.device != x.device:
                raise ValueError(f"{name}: pivot must be {C} fp32 values on {x.device}")
            pivot = pivot.contiguous()
    elif pivot is not None:
        raise ValueError(f"{name}: a pivot belongs to partial sums")
    return (None if weight is None else weight.contiguous(), None if bias is None else bias.contiguous(), parts, pivot)


def _bn_workspace(C: int, device) -> Tuple[Tensor, int]:
    """The BatchNorm kernels' float64 workspace for C channels and its size in bytes."""
    wb = _lib.load().mvsdet_bn3d_workspace_bytes(C)
    return torch.empty(wb // 8, dtype=torch.float64, device=device), wb


@torch.library.custom_op(f"{_NS}::bn3d_relu_train", mutates_args=(), device_types="cuda")
def bn3d_relu_train(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float,
                    relu: bool, residual: Optional[Tensor] = None, parts: Optional[Tensor] = None,
                    pivot: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Training-mode BatchNorm3d [+ ReLU] (mvs_models/module.py:26-37) on the batch statistics of x (N,C,D,H,W) fp32 ->
    (out, batch mean, 1/sqrt(biased batch variance + eps)).  The running statistics are the caller's to update (a custom
    operator with an autograd formula must not mutate its inputs): `layers.update_running_stats` does it from the returned vectors.
    residual (same shape as x): out = [relu](bn(x)) + residual in the same pass (mvsnet.py:109-111, the skip additions).
    parts: float64 (C, n, 2) partial sums of x and of its squares per channel, left by the convolution that produced x
    (`conv3d_k3_bf16x3_stats`): the statistics pass over x is skipped; pivot: the vector that call was given (None = zeros)."""
    _req(x, "x", dim=5)
    if residual is not None:
        _req(residual, "residual", dim=5)
        if residual.shape != x.shape:
            raise ValueError(f"bn3d_relu_train: residual {tuple(residual.shape)} != x {tuple(x.shape)}")
        residual = residual.contiguous()
    weight, bias, parts, pivot = _bn_params("bn3d_relu_train", x, weight, bias, parts, pivot)
    N, C = x.shape[:2]
    vol = x[0, 0].numel()
    x = x.contiguous()
    out = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    lib = _lib.load()
    ws, wb = _bn_workspace(C, x.device)
    with torch.cuda.device(x.device):
        if parts is not None:
            _lib.check(lib.mvsdet_bn3d_relu_train_fwd_parts_f32(_lib.ptr(x), _lib.ptr(parts), int(parts.shape[1]), _lib.ptr(pivot), _lib.ptr(weight), _lib.ptr(bias),
                                                                _lib.ptr(residual), None, None, _lib.ptr(out), _lib.ptr(mean), _lib.ptr(invstd),
                                                                _lib.ptr(ws), wb, N, C, vol, 0.0, float(eps), int(relu), _stream(x)),
                       "bn3d_relu_train")
        else:
            _lib.check(lib.mvsdet_bn3d_relu_train_fwd_res_f32(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(residual), None, None,
                                                              _lib.ptr(out), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(ws), wb, N, C, vol,
                                                              0.0, float(eps), int(relu), _stream(x)), "bn3d_relu_train")
    return out, mean, invstd


@bn3d_relu_train.register_fake
def _(x, weight, bias, eps, relu, residual=None, parts=None, pivot=None):
    return torch.empty_like(x), x.new_empty(x.shape[1]), x.new_empty(x.shape[1])


@torch.library.custom_op(f"{_NS}::bn3d_relu_backward", mutates_args=(), device_types="cuda")
def bn3d_relu_backward(x: Tensor, grad_out: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], save_mean: Tensor,
                       save_invstd: Tensor, relu: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """Backward of bn3d_relu_train -> (grad_x, grad_weight, grad_bias)."""
    _req(x, "x", dim=5)
    _req(grad_out, "grad_out", dim=5)
    if grad_out.shape != x.shape:
        raise ValueError("bn3d_relu_backward: grad_out does not match x")
    N, C = x.shape[:2]
    vol = x[0, 0].numel()
    x, grad_out = x.contiguous(), grad_out.contiguous()
    weight = None if weight is None else weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    gx = torch.empty_like(x)
    gw = torch.empty(C, dtype=torch.float32, device=x.device)
    gb = torch.empty_like(gw)
    lib = _lib.load()
    ws, wb = _bn_workspace(C, x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_bn3d_relu_bwd_f32(_lib.ptr(x), _lib.ptr(grad_out), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(save_mean),
                                                _lib.ptr(save_invstd), _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws), wb, N, C,
                                                vol, int(relu), _stream(x)), "bn3d_relu_backward")
    return gx, gw, gb


@bn3d_relu_backward.register_fake
def _(x, grad_out, weight, bias, save_mean, save_invstd, relu):
    return torch.empty_like(x), x.new_empty(x.shape[1]), x.new_empty(x.shape[1])


def _bn_setup(ctx, inputs, output):
    x, weight, bias, _, relu, residual, _parts, _pivot = inputs
    ctx.save_for_backward(x, weight, bias, output[1], output[2])
    ctx.relu = relu
    ctx.has_residual = residual is not None


def _bn_bwd(ctx, g_out, g_mean, g_invstd):
    x, weight, bias, mean, invstd = ctx.saved_tensors
    gx, gw, gb = bn3d_relu_backward(x, g_out.contiguous(), weight, bias, mean, invstd, ctx.relu)
    # the residual is added after the activation: its gradient is grad_out itself
    return gx, (gw if weight is not None else None), (gb if bias is not None else None), None, None, (g_out if ctx.has_residual else None), None, None


bn3d_relu_train.register_autograd(_bn_bwd, setup_context=_bn_setup)



# ---- training BatchNorm with the residual INSIDE the ReLU (the neck's ResModule: relu(bn(conv1(h)) + identity))
@torch.library.custom_op(f"{_NS}::bn3d_res_relu_train", mutates_args=(), device_types="cuda")
def bn3d_res_relu_train(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], residual: Tensor, eps: float, relu: bool,
                        parts: Optional[Tensor] = None, pivot: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Training-mode BatchNorm3d on the batch statistics of x (N,C,D,H,W) with `residual` added before the activation:
    out = [relu](bn(x) + residual) -> (out, batch mean, invstd).  Running statistics are the caller's to update, as for
    `bn3d_relu_train`; parts / pivot: statistics from the producing convolution's epilogue, as there."""
    _req(x, "x", dim=5)
    _req(residual, "residual", dim=5)
    if residual.shape != x.shape:
        raise ValueError(f"bn3d_res_relu_train: residual {tuple(residual.shape)} != x {tuple(x.shape)}")
    weight, bias, parts, pivot = _bn_params("bn3d_res_relu_train", x, weight, bias, parts, pivot)
    N, C = x.shape[:2]
    vol = x[0, 0].numel()
    x, residual = x.contiguous(), residual.contiguous()
    out = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    lib = _lib.load()
    ws, wb = _bn_workspace(C, x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_bn3d_res_relu_train_fwd_f32(_lib.ptr(x), _lib.ptr(parts), int(parts.shape[1]) if parts is not None else 0,
                                                          _lib.ptr(pivot), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(residual), None, None,
                                                          _lib.ptr(out), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(ws), wb, N, C, vol, 0.0,
                                                          float(eps), int(relu), _stream(x)), "bn3d_res_relu_train")
    return out, mean, invstd


@bn3d_res_relu_train.register_fake
def _(x, weight, bias, residual, eps, relu, parts=None, pivot=None):
    return torch.empty_like(x), x.new_empty(x.shape[1]), x.new_empty(x.shape[1])


@torch.library.custom_op(f"{_NS}::bn3d_res_relu_backward", mutates_args=(), device_types="cuda")
def bn3d_res_relu_backward(x: Tensor, out: Tensor, grad_out: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], save_mean: Tensor,
                           save_invstd: Tensor, relu: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Backward of bn3d_res_relu_train -> (grad_x, grad_weight, grad_bias, grad_residual); the ReLU mask is `out > 0`."""
    _req(x, "x", dim=5)
    _req(out, "out", dim=5)
    _req(grad_out, "grad_out", dim=5)
    if grad_out.shape != x.shape or out.shape != x.shape:
        raise ValueError("bn3d_res_relu_backward: out / grad_out do not match x")
    N, C = x.shape[:2]
    vol = x[0, 0].numel()
    x, out, grad_out = x.contiguous(), out.contiguous(), grad_out.contiguous()
    weight = None if weight is None else weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    gx, gres = torch.empty_like(x), torch.empty_like(x)
    gw = torch.empty(C, dtype=torch.float32, device=x.device)
    gb = torch.empty_like(gw)
    lib = _lib.load()
    ws, wb = _bn_workspace(C, x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.mvsdet_bn3d_res_relu_bwd_f32(_lib.ptr(x), _lib.ptr(out), _lib.ptr(grad_out), _lib.ptr(weight), _lib.ptr(bias),
                                                    _lib.ptr(save_mean), _lib.ptr(save_invstd), _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb),
                                                    _lib.ptr(gres), _lib.ptr(ws), wb, N, C, vol, int(relu), _stream(x)), "bn3d_res_relu_backward")
    return gx, gw, gb, gres


@bn3d_res_relu_backward.register_fake
def _(x, out, grad_out, weight, bias, save_mean, save_invstd, relu):
    return torch.empty_like(x), x.new_empty(x.shape[1]), x.new_empty(x.shape[1]), torch.empty_like(x)


def _bn_res_setup(ctx, inputs, output):
    x, weight, bias, _residual, _eps, relu, _parts, _pivot = inputs
    ctx.save_for_backward(x, output[0], weight, bias, output[1], output[2])
    ctx.relu = relu


def _bn_res_bwd(ctx, g_out, g_mean, g_invstd):
    x, out, weight, bias, mean, invstd = ctx.saved_tensors
    gx, gw, gb, gres = bn3d_res_relu_backward(x, out, g_out.contiguous(), weight, bias, mean, invstd, ctx.relu)
    return gx, (gw if weight is not None else None), (gb if bias is not None else None), gres, None, None, None, None


bn3d_res_relu_train.register_autograd(_bn_res_bwd, setup_context=_bn_res_setup)

# ------------------------------------------------------------------------------------------- --amp (tools/train.py:24-28)
# Under torch.autocast the 2-D backbone hands out float16 / bfloat16 maps.  The hot path computes in float32 -- the rule torch's own
# autocast applies to `grid_sampler`, `softmax` and the reductions the reference runs here -- so these operators CAST low-precision
# floating inputs to float32 while autocast is on (and return float32), instead of raising the TypeError a non-float32 tensor gets
# outside autocast.  The fp16-STORAGE sweep (pack_features on float16 maps, plane_sweep_variance_shard(half_out=True)) is an explicit
# opt-in and keeps its dtypes: it has no autocast rule.
AUTOCAST_FP32_OPS = (homo_warp, plane_sweep_variance, plane_sweep_variance_keep, depth_prob_topk, sample_depth_prob,
                     backproject_weigh, backproject_weigh_mean)
# the evaluation-only diagnostics of the lifting block run under the same rule (no gradient, so not a forward operator of the path)
AUTOCAST_FP32_DIAGNOSTICS = (depth_diagnostics,)
# the per-pixel forms of a3 / a3+a4 (kept apart: AUTOCAST_FP32_OPS lists the operators of the shipped path)
AUTOCAST_FP32_PIXEL_OPS = (homo_warp_pixel, plane_sweep_variance_pixel)
for _op in AUTOCAST_FP32_OPS + AUTOCAST_FP32_PIXEL_OPS + AUTOCAST_FP32_DIAGNOSTICS:
    _op.register_autocast("cuda", torch.float32)
del _op



# ------------------------------------------------------------------------------------------- detection post-processing
# NerfDetHead.predict_by_feat -> _nms -> aligned_3d_nms (nerfdet_head.py:301-420, 564-628) on csrc/detect.hip: head maps -> kept
# boxes in four launches per batch on the current stream, no host synchronisation.
DETECT_MAX_CANDIDATES = 16384   # MVSDET_DETECT_MAX_CANDIDATES: boxes of one scene above score_thr
DETECT_MAX_LEVELS = 4
DETECT_VOXEL_SIZE = (.16, .16, .2)   # NerfDetHead._get_points: tmp_voxel_size, doubled per level


class HeadPrediction(NamedTuple):
    """Padded detections of a batch: boxes (B,Nmax,6) (cx, cy, cz, dx, dy, dz), scores (B,Nmax), labels (B,Nmax) int64 and the
    kept count of every scene (B,) int32 -- a negative count -n: n boxes above score_thr, more than DETECT_MAX_CANDIDATES."""
    boxes: Tensor
    scores: Tensor
    labels: Tensor
    counts: Tensor


def detect_level_geometry(featmap_sizes, origins) -> Tensor:
    """(B, L, 6) host float32: per scene and level the voxel size and get_points' new_origin, from the reference's own torch ops
    (nerfdet_head.py:22-34, 408-419: torch.tensor(featmap_size) / 2. * voxel size, subtracted from the float32 origin)."""
    rows = []
    for origin in origins:
        o = origin if isinstance(origin, Tensor) else torch.tensor(origin)
        if o.dtype != torch.float32:
            raise ValueError(f"detection: lidar2img['origin'] must be float32 (got {o.dtype}); a float64 origin would make the "
                             "reference decode the boxes in float64")
        o = o.cpu().reshape(3)
        per = []
        for i, size in enumerate(featmap_sizes):
            n_voxels = torch.tensor(list(size))
            voxel_size = torch.tensor(DETECT_VOXEL_SIZE) * (2 ** i)
            new_origin = o - n_voxels / 2. * voxel_size
            per.append(torch.cat([voxel_size, new_origin]))
        rows.append(torch.stack(per))
    return torch.stack(rows).float()


def detect_candidates(featmap_sizes, nms_pre: int) -> int:
    """A scene's candidate capacity: per level nms_pre points if the level has more than nms_pre > 0 of them, else all."""
    n = 0
    for s in featmap_sizes:
        v = int(s[0]) * int(s[1]) * int(s[2])
        n += nms_pre if v > nms_pre > 0 else v
    return n


def head_predict(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, origins, nms_pre: int, score_thr: float,
                 iou_thr: float) -> HeadPrediction:
    """The ScanNet head's predict_by_feat up to the boxes, for every scene of the batch, on the current stream without a host sync.
    center_preds / bbox_preds / cls_preds: per level (B,1|6|C,X,Y,Z) float32; valid_pred (B,1,X,Y,Z): the stacked view counts (any
    dtype; taken as float, as the reference's torch.stack(valids).float()); origins: one float32 (3,) origin per scene.
    Kept boxes of a scene in pick order.  Visiting order of the walk: NaN scores first, whatever their sign; -0 and +0 equal; equal
    scores by level, then voxel index.  (The head's scores are >= +0 and a NaN never passes score_thr.)"""
    return _detect_head(center_preds, bbox_preds, cls_preds, valid_pred, origins, nms_pre, score_thr, iou_thr, rotated=False)


def head_predict_rotated(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, origins, nms_pre: int, score_thr: float,
                         iou_thr: float) -> HeadPrediction:
    """ImVoxelHead_ARKit's predict_by_feat up to the boxes (nerfdet_head.py:902-1056, 1190-1243), for every scene of the batch, on
    the current stream without a host sync: as head_predict, with bbox maps of 7 channels.  A top-k point keeps all its class
    scores; per class (ascending) the points with that score > score_thr go through nms3d (ops.nms3d).  HeadPrediction with boxes
    (B,Nmax,7) (x, y, z, dx, dy, dz, heading), Nmax = n_classes * min(candidates, DETECT_MAX_CANDIDATES), class-major rows.
    Visiting order inside a class: its score descending, equal scores by level, then voxel index.  A negative count -n: one class
    of the scene has n boxes above score_thr, more than DETECT_MAX_CANDIDATES."""
    return _detect_head(center_preds, bbox_preds, cls_preds, valid_pred, origins, nms_pre, score_thr, iou_thr, rotated=True)


def _detect_head(center_preds, bbox_preds, cls_preds, valid_pred, origins, nms_pre, score_thr, iou_thr, rotated: bool):
    fname = "head_predict_rotated" if rotated else "head_predict"
    nreg = 7 if rotated else 6
    L = len(center_preds)
    if not (1 <= L <= DETECT_MAX_LEVELS) or len(bbox_preds) != L or len(cls_preds) != L:
        raise ValueError(f"{fname}: 1..{DETECT_MAX_LEVELS} levels of center / bbox / cls maps needed")
    _req(valid_pred, "valid_pred", dtype=valid_pred.dtype, dim=5)
    B = valid_pred.shape[0]
    valid = valid_pred.float().contiguous()
    centers, bboxes, clss, dims = [], [], [], []
    for lvl, (c, r, k) in enumerate(zip(center_preds, bbox_preds, cls_preds)):
        for t, name, ch in ((c, "center", 1), (r, "bbox", nreg), (k, "cls", None)):
            _req(t, f"{name}_preds[{lvl}]", dim=5)
            if t.shape[0] != B or (ch is not None and t.shape[1] != ch) or t.shape[2:] != c.shape[2:]:
                raise ValueError(f"{fname}: {name}_preds[{lvl}] has shape {tuple(t.shape)}")
        if k.shape[1] != cls_preds[0].shape[1]:
            raise ValueError(f"{fname}: every level needs the same class count")
        centers.append(c.contiguous())
        bboxes.append(r.contiguous())
        clss.append(k.contiguous())
        dims += [int(v) for v in c.shape[2:]]
    sizes = [tuple(c.shape[2:]) for c in centers]
    if len(origins) != B:
        raise ValueError(f"{fname}: {len(origins)} origins for {B} scenes")
    dev = valid.device
    geom = detect_level_geometry(sizes, origins).pin_memory().to(dev, non_blocking=True)
    nms_pre = int(nms_pre)
    points = sum(s[0] * s[1] * s[2] for s in sizes)
    ncap = detect_candidates(sizes, nms_pre)
    n_classes = int(clss[0].shape[1])
    lib = _lib.load()
    if rotated:
        nmax = max(1, n_classes * min(ncap, DETECT_MAX_CANDIDATES))
        wsb, entry = lib.mvsdet_detect_rotated_workspace_bytes(B, points, ncap, n_classes), lib.mvsdet_detect_head_rotated_f32
    else:
        nmax = max(1, min(ncap, DETECT_MAX_CANDIDATES))
        wsb, entry = lib.mvsdet_detect_workspace_bytes(B, points, ncap), lib.mvsdet_detect_head_f32
    ws = torch.empty(int(wsb), dtype=torch.uint8, device=dev)
    boxes = torch.empty((B, nmax, nreg), dtype=torch.float32, device=dev)
    scores = torch.empty((B, nmax), dtype=torch.float32, device=dev)
    labels = torch.empty((B, nmax), dtype=torch.int64, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    arr = ctypes.c_void_p * L
    with torch.cuda.device(dev):
        _lib.check(entry(
            arr(*[t.data_ptr() for t in centers]), arr(*[t.data_ptr() for t in bboxes]), arr(*[t.data_ptr() for t in clss]),
            (ctypes.c_int * len(dims))(*dims), _lib.ptr(valid), _lib.ptr(geom), B, L, n_classes, *[int(v) for v in valid.shape[2:]],
            nms_pre, float(score_thr), float(iou_thr), _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(labels), _lib.ptr(counts), nmax,
            _lib.ptr(ws), ws.numel(), _stream(valid)), fname)
    return HeadPrediction(boxes, scores, labels, counts)


def aligned_3d_nms(boxes: Tensor, scores: Tensor, classes: Tensor, thresh: float) -> Tensor:
    """NerfDetHead.aligned_3d_nms (nerfdet_head.py:580-628): boxes (n,6) (x1,y1,z1,x2,y2,z2), scores (n,), classes (n,) ->
    the kept indices in pick order (LongTensor).  CUDA float32 only; n <= DETECT_MAX_CANDIDATES.  Reads the kept count back
    (one host sync, as the reference's loop syncs on every box).  Visiting order: NaN scores first, whatever their sign (the
    reference's argsort puts NaN last and its loop takes from the end); -0 and +0 equal; equal scores by lower index first."""
    _req(boxes, "boxes", dim=2)
    _req(scores, "scores", dim=1)
    if not classes.is_cuda:
        raise RuntimeError(f"mvsdet_amd: `classes` must live on a ROCm device (got {classes.device}); this package has no CPU path")
    n = boxes.shape[0]
    if boxes.shape[1] != 6 or scores.shape[0] != n or classes.numel() != n:
        raise ValueError(f"aligned_3d_nms: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}, classes {tuple(classes.shape)}")
    if n > DETECT_MAX_CANDIDATES:
        raise ValueError(f"aligned_3d_nms: {n} boxes, above the candidate limit {DETECT_MAX_CANDIDATES}")
    b, s, c = boxes.contiguous(), scores.contiguous(), classes.reshape(-1).to(torch.int64).contiguous()
    lib = _lib.load()
    ws = torch.empty(int(lib.mvsdet_detect_workspace_bytes(1, 0, n)), dtype=torch.uint8, device=boxes.device)
    out = torch.empty((max(n, 1),), dtype=torch.int64, device=boxes.device)
    count = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(lib.mvsdet_aligned_3d_nms_f32(_lib.ptr(b), _lib.ptr(s), _lib.ptr(c), n, float(thresh), _lib.ptr(out),
                                                 _lib.ptr(count), _lib.ptr(ws), ws.numel(), _stream(boxes)), "aligned_3d_nms")
    return out[:int(count.item())]


def nms3d(boxes: Tensor, scores: Tensor, iou_threshold: float) -> Tensor:
    """mmcv.ops.nms3d (mmcv 2.1.0) on csrc/detect.hip: boxes (n,7) (x, y, z, dx, dy, dz, heading), scores (n,) -> the kept indices
    in pick order (LongTensor).  Greedy by score; a later box goes when its bird's-eye-view IoU with a kept box is > iou_threshold
    (z and dz unused).  Equal scores by lower index first (mmcv's sort leaves them unordered); NaN scores first.  CUDA float32
    only; n <= DETECT_MAX_CANDIDATES.  Reads the kept count back (one host sync, as mmcv's own op)."""
    _req(boxes, "boxes", dim=2)
    _req(scores, "scores", dim=1)
    n = boxes.shape[0]
    if boxes.shape[1] != 7 or scores.shape[0] != n:
        raise ValueError(f"nms3d: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}")
    if n > DETECT_MAX_CANDIDATES:
        raise ValueError(f"nms3d: {n} boxes, above the candidate limit {DETECT_MAX_CANDIDATES}")
    b, s = boxes.contiguous(), scores.contiguous()
    lib = _lib.load()
    ws = torch.empty(int(lib.mvsdet_detect_rotated_workspace_bytes(1, 0, n, 1)), dtype=torch.uint8, device=boxes.device)
    out = torch.empty((max(n, 1),), dtype=torch.int64, device=boxes.device)
    count = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(lib.mvsdet_nms3d_f32(_lib.ptr(b), _lib.ptr(s), n, float(iou_threshold), _lib.ptr(out), _lib.ptr(count),
                                        _lib.ptr(ws), ws.numel(), _stream(boxes)), "nms3d")
    return out[:int(count.item())]


def bev_iou_rotated(a: Tensor, b: Tensor) -> Tensor:
    """(n, m) bird's-eye-view IoU of the boxes a (n,7) and b (m,7), iou_bev of mmcv's nms3d (the device function the NMS uses,
    a first, early exit included).  CUDA float32 only; no host sync."""
    _req(a, "a", dim=2)
    _req(b, "b", dim=2)
    if a.shape[1] != 7 or b.shape[1] != 7:
        raise ValueError(f"bev_iou_rotated: boxes of 7 values needed, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, m = a.shape[0], b.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=a.device)
    x, y = a.contiguous(), b.contiguous()
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().mvsdet_bev_iou_rotated_f32(_lib.ptr(x), n, _lib.ptr(y), m, _lib.ptr(out), _stream(a)), "bev_iou_rotated")
    return out


# ------------------------------------------------------------------------------------------- head training: targets and losses
# NerfDetHead._get_targets / _loss_by_feat_single (nerfdet_head.py:206-257, 473-562) on csrc/assign.hip: three launches for the
# targets, two for the losses' sums, one for their gradients, on the current stream, no host synchronisation, the same bits from run
# to run.  The `_rotated` functions are ImVoxelHead_ARKit's (:779-846, 1029-1185; RotatedIoU3DLoss) on the same kernels instantiated
# for 7-value boxes.
ASSIGN_MAX_BOXES = 1024   # MVSDET_ASSIGN_MAX_BOXES: ground-truth boxes of one scene (staged in LDS by assign_pick_kernel)


class HeadTargets(NamedTuple):
    """Targets of every point of a batch (P = the levels' points concatenated in order, a level's voxels x-major): labels (B,P)
    int64 (-1: no box), box_index (B,P) int32 (-1), center_targets (B,P), bbox_targets (B,P,6) (x1, y1, z1, x2, y2, z2; zero
    where no box), and geom (B,L,6), the device copy of detect_level_geometry the targets were made with.  From
    head_targets_rotated: bbox_targets (B,P,7) = the chosen ground-truth row (x, y, z, dx, dy, dz, yaw), center_targets -1 where no
    box is assigned."""
    labels: Tensor
    box_index: Tensor
    center_targets: Tensor
    bbox_targets: Tensor
    geom: Tensor


class HeadLossSums(NamedTuple):
    """Unnormalised sums of every scene: center (B,) = the centerness BCE over positive points, bbox (B,) = centerness target *
    (1 - IoU) over positive points, cls (B,) = the focal loss over valid points and classes -- these three carry gradients to the
    nine maps -- and weight_sum (B,) = the positive points' centerness targets, n_pos, n_valid (B,) int32."""
    center: Tensor
    bbox: Tensor
    cls: Tensor
    weight_sum: Tensor
    n_pos: Tensor
    n_valid: Tensor


def _to_device(t: Tensor, dev) -> Tensor:
    """A host tensor through pinned memory (no host synchronisation); a device tensor as it is."""
    return t.to(dev) if t.is_cuda else t.pin_memory().to(dev, non_blocking=True)


def check_box_limit(n_boxes: int) -> None:
    if n_boxes > ASSIGN_MAX_BOXES:
        raise ValueError(f"head_targets: {n_boxes} ground-truth boxes in one scene, above the limit ASSIGN_MAX_BOXES = "
                         f"{ASSIGN_MAX_BOXES} (MVSDET_ASSIGN_MAX_BOXES: the boxes of a scene are staged in LDS)")


def head_targets(featmap_sizes, origins, gt_boxes: Tensor, gt_volumes: Tensor, gt_labels: Tensor, gt_counts: Tensor,
                 pts_assign_threshold: int, pts_center_threshold: int) -> HeadTargets:
    """NerfDetHead._get_targets of every scene of a batch (nerfdet_head.py:473-562).  featmap_sizes: (X, Y, Z) per level; origins:
    one float32 (3,) origin per scene; gt_boxes (B,G,6) = cat(gravity_center, tensor[:, 3:6]), gt_volumes (B,G), gt_labels (B,G)
    int64, padded to the batch's largest G <= ASSIGN_MAX_BOXES (checked on the shape, before any launch); gt_counts (B,) int32 =
    the boxes of every scene.  CUDA tensors only.  Equal volumes: the lowest box index wins (torch.min on the CPU; the reference
    leaves it to the backend).  A scene without boxes gets label -1 everywhere (the reference raises on the empty min).  A box with
    at most pts_center_threshold points inside on its best level keeps them all."""
    return _head_targets(featmap_sizes, origins, gt_boxes, None, gt_volumes, gt_labels, gt_counts, pts_assign_threshold,
                         pts_center_threshold)


def head_targets_rotated(featmap_sizes, origins, gt_boxes: Tensor, gt_rot: Tensor, gt_volumes: Tensor, gt_labels: Tensor,
                         gt_counts: Tensor, pts_assign_threshold: int, pts_center_threshold: int) -> HeadTargets:
    """ImVoxelHead_ARKit._get_targets of every scene of a batch (nerfdet_head.py:1107-1185): as head_targets, with gt_boxes (B,G,7) =
    cat(gravity_center, tensor[:, 3:7]) and gt_rot (B,G,2) = (cos(yaw), sin(yaw)), which the caller computes (torch.cos / torch.sin,
    as rotation_3d_in_axis does) so that no transcendental is evaluated on the way to a label.  Face distances in the box's own
    frame; the top-k takes min(pts_center_threshold + 1, P) values; bbox_targets (B,P,7) are the chosen ground-truth rows,
    center_targets -1 where no box is assigned."""
    return _head_targets(featmap_sizes, origins, gt_boxes, gt_rot, gt_volumes, gt_labels, gt_counts, pts_assign_threshold,
                         pts_center_threshold)


def _head_targets(featmap_sizes, origins, gt_boxes, gt_rot, gt_volumes, gt_labels, gt_counts, pts_assign_threshold,
                  pts_center_threshold):
    rotated = gt_rot is not None
    fname, nbox = ("head_targets_rotated", 7) if rotated else ("head_targets", 6)
    B = len(origins)
    L = len(featmap_sizes)
    if not (1 <= L <= DETECT_MAX_LEVELS):
        raise ValueError(f"{fname}: 1..{DETECT_MAX_LEVELS} levels needed")
    if gt_boxes.dim() != 3:
        raise ValueError(f"{fname}: gt_boxes must be (B, G, {nbox}) (got shape {tuple(gt_boxes.shape)})")
    G = int(gt_boxes.shape[1])
    check_box_limit(G)   # from the shape, before anything else
    _req(gt_boxes, "gt_boxes", dim=3)
    _req(gt_volumes, "gt_volumes", dim=2)
    _req(gt_labels, "gt_labels", dtype=torch.int64, dim=2)
    _req(gt_counts, "gt_counts", dtype=torch.int32, dim=1)
    if rotated:
        _req(gt_rot, "gt_rot", dim=3)
    if gt_boxes.shape != (B, G, nbox) or gt_volumes.shape != (B, G) or gt_labels.shape != (B, G) or gt_counts.shape != (B,) \
            or (rotated and gt_rot.shape != (B, G, 2)):
        raise ValueError(f"{fname}: gt_boxes {tuple(gt_boxes.shape)}, gt_volumes {tuple(gt_volumes.shape)}, gt_labels "
                         f"{tuple(gt_labels.shape)}, gt_counts {tuple(gt_counts.shape)} for {B} scenes")
    dev = gt_boxes.device
    sizes = [tuple(int(v) for v in s) for s in featmap_sizes]
    dims = [v for s in sizes for v in s]
    P = sum(s[0] * s[1] * s[2] for s in sizes)
    geom = _to_device(detect_level_geometry(sizes, origins), dev)
    lib = _lib.load()
    ws = torch.empty(int(lib.mvsdet_head_targets_workspace_bytes(B, G)), dtype=torch.uint8, device=dev)
    labels = torch.empty((B, P), dtype=torch.int64, device=dev)
    box_index = torch.empty((B, P), dtype=torch.int32, device=dev)
    center_t = torch.empty((B, P), dtype=torch.float32, device=dev)
    bbox_t = torch.empty((B, P, nbox), dtype=torch.float32, device=dev)
    boxes, volumes, glabels = gt_boxes.contiguous(), gt_volumes.contiguous(), gt_labels.contiguous()
    gt = [_lib.ptr(boxes) if G else None]
    if rotated:
        rot = gt_rot.contiguous()
        gt.append(_lib.ptr(rot) if G else None)
    entry = lib.mvsdet_head_targets_rotated_f32 if rotated else lib.mvsdet_head_targets_f32
    with torch.cuda.device(dev):
        _lib.check(entry(
            (ctypes.c_int * len(dims))(*dims), _lib.ptr(geom), B, L, *gt, _lib.ptr(volumes) if G else None,
            _lib.ptr(glabels) if G else None, _lib.ptr(gt_counts.contiguous()), G, int(pts_assign_threshold), int(pts_center_threshold),
            _lib.ptr(labels), _lib.ptr(box_index), _lib.ptr(center_t), _lib.ptr(bbox_t), _lib.ptr(ws) if ws.numel() else None,
            ws.numel(), _stream(gt_boxes)), fname)
    return HeadTargets(labels, box_index, center_t, bbox_t, geom)


def _loss_maps(center_preds, bbox_preds, cls_preds, valid_pred, targets: HeadTargets, nreg: int = 6):
    L = len(center_preds)
    if not (1 <= L <= DETECT_MAX_LEVELS) or len(bbox_preds) != L or len(cls_preds) != L:
        raise ValueError(f"head_loss: 1..{DETECT_MAX_LEVELS} levels of center / bbox / cls maps needed")
    _req(valid_pred, "valid_pred", dtype=valid_pred.dtype, dim=5)
    B = valid_pred.shape[0]
    maps = []
    for lvl, (c, r, k) in enumerate(zip(center_preds, bbox_preds, cls_preds)):
        for t, name, ch in ((c, "center", 1), (r, "bbox", nreg), (k, "cls", int(cls_preds[0].shape[1]))):
            _req(t, f"{name}_preds[{lvl}]", dim=5)
            if t.shape[0] != B or t.shape[1] != ch or t.shape[2:] != c.shape[2:]:
                raise ValueError(f"head_loss: {name}_preds[{lvl}] has shape {tuple(t.shape)}")
        maps += [c, r, k]
    P = sum(int(c.shape[2] * c.shape[3] * c.shape[4]) for c in center_preds)
    if targets.labels.shape != (B, P) or targets.geom.shape != (B, L, 6) or targets.bbox_targets.shape != (B, P, nreg):
        raise ValueError(f"head_loss: targets of shape {tuple(targets.labels.shape)} for {B} scenes of {P} points")
    return maps


class _HeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, valid, labels, center_t, bbox_t, geom, gamma, alpha, rotated, *maps):
        L = len(maps) // 3
        maps = [m.contiguous() for m in maps]
        B, C = int(valid.shape[0]), int(maps[2].shape[1])
        dims = [int(v) for l in range(L) for v in maps[3 * l].shape[2:]]
        P = int(labels.shape[1])
        dev = valid.device
        lib = _lib.load()
        ws = torch.empty(int(lib.mvsdet_head_loss_workspace_bytes(B, P)), dtype=torch.uint8, device=dev)
        sums = torch.empty((B, 4), dtype=torch.float32, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
        arr = ctypes.c_void_p * L
        ctx.args = (arr, dims, B, L, C, [int(v) for v in valid.shape[2:]], float(gamma), float(alpha), bool(rotated))
        with torch.cuda.device(dev):
            _lib.check((lib.mvsdet_head_loss_rotated_f32 if rotated else lib.mvsdet_head_loss_f32)(
                arr(*[maps[3 * l].data_ptr() for l in range(L)]), arr(*[maps[3 * l + 1].data_ptr() for l in range(L)]),
                arr(*[maps[3 * l + 2].data_ptr() for l in range(L)]), (ctypes.c_int * len(dims))(*dims), _lib.ptr(valid), _lib.ptr(geom),
                B, L, C, *ctx.args[5], _lib.ptr(labels), _lib.ptr(center_t), _lib.ptr(bbox_t), float(gamma), float(alpha),
                _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _stream(valid)), "head_loss")
        ctx.save_for_backward(valid, labels, center_t, bbox_t, geom, *maps)
        out = (sums[:, 0], sums[:, 1], sums[:, 2], sums[:, 3], counts[:, 0], counts[:, 1])
        ctx.mark_non_differentiable(*out[3:])
        return out

    @staticmethod
    def backward(ctx, g_center, g_bbox, g_cls, *unused):
        valid, labels, center_t, bbox_t, geom, *maps = ctx.saved_tensors
        arr, dims, B, L, C, vdims, gamma, alpha, rotated = ctx.args
        lib = _lib.load()
        coef = torch.stack([g_center, g_bbox, g_cls], dim=1).float().contiguous()
        grads = [torch.empty_like(m) for m in maps]
        with torch.cuda.device(valid.device):
            _lib.check((lib.mvsdet_head_loss_rotated_backward_f32 if rotated else lib.mvsdet_head_loss_backward_f32)(
                arr(*[maps[3 * l].data_ptr() for l in range(L)]), arr(*[maps[3 * l + 1].data_ptr() for l in range(L)]),
                arr(*[maps[3 * l + 2].data_ptr() for l in range(L)]), (ctypes.c_int * len(dims))(*dims), _lib.ptr(valid), _lib.ptr(geom),
                B, L, C, *vdims, _lib.ptr(labels), _lib.ptr(center_t), _lib.ptr(bbox_t), gamma, alpha, _lib.ptr(coef),
                arr(*[grads[3 * l].data_ptr() for l in range(L)]), arr(*[grads[3 * l + 1].data_ptr() for l in range(L)]),
                arr(*[grads[3 * l + 2].data_ptr() for l in range(L)]), _stream(valid)), "head_loss_backward")
        return (None,) * 8 + tuple(grads)


def head_loss(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, targets: HeadTargets, gamma: float = 2.0,
              alpha: float = 0.25) -> HeadLossSums:
    """The sums of NerfDetHead._loss_by_feat_single (nerfdet_head.py:206-257) for every scene of a batch, with gradients to the nine
    maps.  center_preds / bbox_preds / cls_preds: per level (B,1|6|C,X,Y,Z) float32 CUDA maps, read in place; valid_pred
    (B,1,X,Y,Z): the stacked view counts; targets: ops.head_targets of the same level sizes.  Positive = label >= 0 and
    nn.Upsample(trilinear)(valid_pred).round().bool().  The caller divides: center / n_pos', cls / n_pos' with n_pos' =
    max(n_pos, 1) (averaged over the ranks first), bbox / weight_sum (NerfDetHeadConvs.loss_by_feat)."""
    maps = _loss_maps(center_preds, bbox_preds, cls_preds, valid_pred, targets)
    valid = valid_pred.float().contiguous()
    return HeadLossSums(*_HeadLoss.apply(valid, targets.labels, targets.center_targets, targets.bbox_targets, targets.geom,
                                         float(gamma), float(alpha), False, *maps))


def head_loss_rotated(center_preds, bbox_preds, cls_preds, valid_pred: Tensor, targets: HeadTargets, gamma: float = 2.0,
                      alpha: float = 0.25) -> HeadLossSums:
    """The sums of ImVoxelHead_ARKit._loss_by_feat_single (nerfdet_head.py:779-846) for every scene of a batch, with gradients to
    the nine maps: as head_loss, with bbox maps of 7 channels (six distances, heading) and targets of ops.head_targets_rotated.
    bbox (B,) = centerness target * (1 - IoU3D) over positive points, IoU3D the rotated 3-D IoU of RotatedIoU3DLoss between the
    decoded box (_bbox_pred_to_bbox, :1029-1055) and its ground-truth row: the true intersection area of the two rectangles times
    the z overlap over the union of the volumes.  Finite values and gradients at every pair, degenerate ones included (identical
    boxes, shared or touching edges, headings a multiple of pi/2 apart, a target of zero size: csrc/assign.hip's header); the
    targets receive no gradient."""
    maps = _loss_maps(center_preds, bbox_preds, cls_preds, valid_pred, targets, nreg=7)
    valid = valid_pred.float().contiguous()
    return HeadLossSums(*_HeadLoss.apply(valid, targets.labels, targets.center_targets, targets.bbox_targets, targets.geom,
                                         float(gamma), float(alpha), True, *maps))


# ------------------------------------------------------------------------------------------- evaluation: indoor mAP / recall
# mmdet3d's indoor_eval on csrc/evalmap.hip: eval_match appends a batch's detections to an evaluator's device state (two launches),
# eval_compute orders them and returns the per-label values (a key fill, a bitonic sort, a claim and an AP launch), all on the
# current stream without a host synchronisation or a device allocation of the library's.  mvsdet_amd.evaluation builds the
# reference's ret_dict from them.
EVAL_MAX_RECORDS = 1 << 20    # MVSDET_EVAL_MAX_RECORDS
EVAL_MAX_LABELS = 4095        # MVSDET_EVAL_MAX_LABELS
EVAL_MAX_THRESHOLDS = 8       # MVSDET_EVAL_MAX_THRESHOLDS
EVAL_FLAGS = {1: "more detections than `capacity`", 2: "more ground-truth boxes than `gt_capacity`",
              4: "a negative count (the heads' flag for more than DETECT_MAX_CANDIDATES boxes) or a count above the padded size",
              8: "a scene serial below one already fed", 16: "a label outside [0, n_labels)",
              32: "more records than the bound given to eval_compute"}


class EvalState(NamedTuple):
    """An evaluator's device memory: `state` (records, counts; mvsdet_eval_state_bytes) and the `workspace` of eval_compute at full
    capacity, both uint8, and the sizes every call on it repeats."""
    state: Tensor
    workspace: Tensor
    n_labels: int
    capacity: int
    gt_capacity: int
    n_thr: int


class EvalResult(NamedTuple):
    """Device outputs of eval_compute: ap (T,L) float32, recall (T,L) float64, npos, ndet (L) int32, first (L) int64 (where a label
    was first seen; -1 never), tp (T,n_bound) uint8 and order (n_bound) int32 in visiting order, info (4) int32 = records,
    ground-truth slots, flags (EVAL_FLAGS), next scene serial."""
    ap: Tensor
    recall: Tensor
    npos: Tensor
    ndet: Tensor
    first: Tensor
    tp: Tensor
    order: Tensor
    info: Tensor


def _eval_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"mvsdet_amd: the evaluator lives on a ROCm device (got {dev}); this package has no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def eval_state(n_labels: int, capacity: int, gt_capacity: int, n_thr: int, device) -> EvalState:
    """Allocate and clear an evaluator's state for up to `capacity` detections and `gt_capacity` ground-truth boxes in all."""
    dev = _eval_device(device)
    lib = _lib.load()
    n_labels, capacity, gt_capacity, n_thr = int(n_labels), int(capacity), int(gt_capacity), int(n_thr)
    nbytes = int(lib.mvsdet_eval_state_bytes(n_labels, capacity, gt_capacity))
    wbytes = int(lib.mvsdet_eval_workspace_bytes(n_labels, capacity, gt_capacity, n_thr)) if nbytes else 0
    if nbytes == 0 or wbytes == 0:
        raise ValueError(f"eval_state: n_labels={n_labels} (1..{EVAL_MAX_LABELS}), capacity={capacity} (1..{EVAL_MAX_RECORDS}), "
                         f"gt_capacity={gt_capacity} (1..{1 << 24}), {n_thr} thresholds (1..{EVAL_MAX_THRESHOLDS})")
    st = EvalState(torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(wbytes, dtype=torch.uint8, device=dev),
                   n_labels, capacity, gt_capacity, n_thr)
    eval_reset(st)
    return st


def eval_reset(st: EvalState) -> None:
    with torch.cuda.device(st.state.device):
        _lib.check(_lib.load().mvsdet_eval_reset(_lib.ptr(st.state), st.state.numel(), st.n_labels, st.capacity, st.gt_capacity,
                                                 _stream(st.state)), "eval_reset")


def eval_match(st: EvalState, boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, gt_boxes: Tensor, gt_labels: Tensor,
               gt_counts: Tensor, scene0: int) -> None:
    """Append a batch to the state: boxes (B,N,7) and gt_boxes (B,G,7) float32 rows (x, y, BOTTOM z, dx, dy, dz, yaw), scores (B,N),
    labels (B,N) / gt_labels (B,G) int64, counts / gt_counts (B,) int32; scene0: the serial number of the batch's first scene."""
    _req(boxes, "boxes", dim=3)
    _req(scores, "scores", dim=2)
    _req(labels, "labels", dtype=torch.int64, dim=2)
    _req(counts, "counts", dtype=torch.int32, dim=1)
    _req(gt_boxes, "gt_boxes", dim=3)
    _req(gt_labels, "gt_labels", dtype=torch.int64, dim=2)
    _req(gt_counts, "gt_counts", dtype=torch.int32, dim=1)
    B, N, G = int(boxes.shape[0]), int(boxes.shape[1]), int(gt_boxes.shape[1])
    if boxes.shape != (B, N, 7) or scores.shape != (B, N) or labels.shape != (B, N) or counts.shape != (B,) \
            or gt_boxes.shape != (B, G, 7) or gt_labels.shape != (B, G) or gt_counts.shape != (B,):
        raise ValueError(f"eval_match: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}, labels {tuple(labels.shape)}, counts "
                         f"{tuple(counts.shape)}, gt_boxes {tuple(gt_boxes.shape)}, gt_labels {tuple(gt_labels.shape)}, gt_counts "
                         f"{tuple(gt_counts.shape)}: (B,N,7), (B,N), (B,N), (B,), (B,G,7), (B,G), (B,) wanted")
    if boxes.device != st.state.device or gt_boxes.device != st.state.device:
        raise RuntimeError(f"eval_match: inputs on {boxes.device} / {gt_boxes.device}, the evaluator on {st.state.device}")
    t = [x.contiguous() for x in (boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts)]
    with torch.cuda.device(st.state.device):
        _lib.check(_lib.load().mvsdet_eval_match_f32(
            _lib.ptr(st.state), st.n_labels, st.capacity, st.gt_capacity, _lib.ptr(t[0]) if N else None, _lib.ptr(t[1]) if N else None,
            _lib.ptr(t[2]) if N else None, _lib.ptr(t[3]), B, N, _lib.ptr(t[4]) if G else None, _lib.ptr(t[5]) if G else None,
            _lib.ptr(t[6]), G, int(scene0), _stream(st.state)), "eval_match")


def eval_compute(st: EvalState, thresholds, n_bound: int) -> EvalResult:
    """Per-label AP and recall of everything fed so far (the state is left as it is).  n_bound: a host-side upper bound of the
    detections fed (<= capacity), which sizes the sort and the per-record outputs."""
    thr = [float(v) for v in thresholds]
    if len(thr) != st.n_thr:
        raise ValueError(f"eval_compute: {len(thr)} thresholds, the state was made for {st.n_thr}")
    dev, T, L, n = st.state.device, st.n_thr, st.n_labels, int(n_bound)
    ap = torch.empty((T, L), dtype=torch.float32, device=dev)
    recall = torch.empty((T, L), dtype=torch.float64, device=dev)
    npos = torch.empty(L, dtype=torch.int32, device=dev)
    ndet = torch.empty(L, dtype=torch.int32, device=dev)
    first = torch.empty(L, dtype=torch.int64, device=dev)
    tp = torch.empty((T, n), dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_eval_compute(
            _lib.ptr(st.state), L, st.capacity, st.gt_capacity, n, (ctypes.c_float * T)(*thr), T, _lib.ptr(ap), _lib.ptr(recall),
            _lib.ptr(npos), _lib.ptr(ndet), _lib.ptr(first), _lib.ptr(tp) if n else None, _lib.ptr(order) if n else None, _lib.ptr(info),
            _lib.ptr(st.workspace), st.workspace.numel(), _stream(st.state)), "eval_compute")
    return EvalResult(ap, recall, npos, ndet, first, tp, order, info)


def eval_iou(a: Tensor, b: Tensor) -> Tensor:
    """(n, m) IoU of boxes a (n,7) and b (m,7) (x, y, bottom z, dx, dy, dz, yaw) as the evaluator takes it: BaseInstance3DBoxes.overlaps
    as a mathematical function in float32 -- not mmcv's box_iou_rotated rounding, and not iou_bev of bev_iou_rotated."""
    _req(a, "a", dim=2)
    _req(b, "b", dim=2)
    if a.shape[1] != 7 or b.shape[1] != 7:
        raise ValueError(f"eval_iou: boxes of 7 values needed, got {tuple(a.shape)} and {tuple(b.shape)}")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    x, y = a.contiguous(), b.contiguous()
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().mvsdet_eval_iou_f32(_lib.ptr(x), int(a.shape[0]), _lib.ptr(y), int(b.shape[0]), _lib.ptr(out), _stream(a)),
                   "eval_iou")
    return out
