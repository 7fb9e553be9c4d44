"""a3 / a3+a4: packing, the plane sweep in all its forms (csrc/pack.h, planesweep*.hip), the benchmark's two yardsticks for it."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch
from torch import Tensor

from ._common import _NS, _lib, req, stream


@torch.library.custom_op(f"{_NS}::pack_features", mutates_args=(), device_types="cuda")
def pack_features(feat: Tensor) -> Tensor:
    """(N,C,H,W) float32 or float16 (any strides) -> packed channel-last maps, flat float32
    (see include/mvsdet_hip.h; the fp16 -> fp32 conversion is exact)."""
    half = feat.dtype == torch.float16
    req(feat, "feat", dtype=torch.float16 if half else torch.float32, dim=4)
    N, C, H, W = feat.shape
    lib = _lib.load()
    out = torch.empty(lib.mvsdet_packed_bytes(N, C, H, W) // 4, dtype=torch.float32, device=feat.device)
    fn = lib.mvsdet_pack_features_f16 if half else lib.mvsdet_pack_features_f32
    with torch.cuda.device(feat.device):
        _lib.check(fn(_lib.ptr(feat), _lib.strides4(feat), _lib.ptr(out), N, C, H, W, stream(feat)), "pack_features")
    return out


@pack_features.register_fake
def _(feat):
    N, C, H, W = feat.shape
    return feat.new_empty(N * H * W * 32 * ((C + 31) // 32), dtype=torch.float32)


@torch.library.custom_op(f"{_NS}::homo_warp", mutates_args=(), device_types="cuda")
def homo_warp(src: Tensor, proj: Tensor, depth: Tensor) -> Tensor:
    """a3 (mvs_models/module.py:105): src (B,C,H,W), proj (B,4,4) = src_proj @ inv(ref_proj), depth (B,D)."""
    req(src, "src", dim=4)
    req(proj, "proj", dim=3)
    req(depth, "depth", dim=2)
    B, C, H, W = src.shape
    D = depth.shape[1]
    if proj.shape != (B, 4, 4) or depth.shape[0] != B:
        raise ValueError(f"homo_warp: proj {tuple(proj.shape)} / depth {tuple(depth.shape)} do not match B={B}")
    src, proj, depth = src.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((B, C, D, H, W), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().mvsdet_homo_warp_f32(_lib.ptr(src), _lib.ptr(proj), _lib.ptr(depth), _lib.ptr(out),
                                                    B, C, D, H, W, stream(src)), "homo_warp")
    return out


@homo_warp.register_fake
def _fake_warp(src, proj, depth):
    B, C, H, W = src.shape
    return src.new_empty((B, C, depth.shape[1], H, W))


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
    req(feat, "feat", dim=4)
    req(nbr, "nbr", dtype=torch.int64, dim=2)
    req(proj, "proj", dim=4)
    req(depth, "depth", dim=2)
    N, C, H, W = feat.shape
    K = nbr.shape[1]
    if nbr.shape[0] != N or proj.shape != (N, K, 4, 4) or depth.shape[0] != N:
        raise ValueError(f"plane_sweep_variance: nbr {tuple(nbr.shape)}, proj {tuple(proj.shape)}, depth "
                         f"{tuple(depth.shape)} do not match N={N}")
    return N, K, C, depth.shape[1], H, W


def _check_packed(name, packed, nbr, proj, depth, C, H, W, n_src=None, depth_dim=2):
    """The packed buffer holds the (C,H,W) maps of n_src views (None: one per row of nbr); proj is (N,K,4,4) and depth (N, ...)
    of `depth_dim` dimensions for nbr (N,K) -> N, K.  `name`: the operator that was called, for the messages."""
    req(packed, "packed", dim=1)
    req(nbr, "nbr", dtype=torch.int64, dim=2)
    req(proj, "proj", dim=4)
    req(depth, "depth", dim=depth_dim)
    N, K = nbr.shape
    if packed.numel() * 4 != _lib.load().mvsdet_packed_bytes(N if n_src is None else n_src, C, H, W):
        raise ValueError(f"{name}: packed buffer does not match ({'N' if n_src is None else 'n_src'},C,H,W)")
    if proj.shape != (N, K, 4, 4) or depth.shape[0] != N:
        raise ValueError(f"{name}: proj/depth shape mismatch")
    return N, K


def _scratch(N, K, D, H, W, device):
    """A geometry table's buffer in float32 words, real or fake (the size query is a host-only function of the shape), and its bytes."""
    sbytes = int(_lib.load().mvsdet_plane_sweep_scratch_bytes(N, K, D, H, W))
    return torch.empty(max(sbytes // 4, 4), dtype=torch.float32, device=device), sbytes


def _sweep_packed(name, packed, nbr, proj, depth, C, H, W):
    """a3+a4 on packed maps -> (variance (N,C,D,H,W), the geometry table the op's first kernel built)."""
    N, K = _check_packed(name, packed, nbr, proj, depth, C, H, W)
    D = depth.shape[1]
    nbr, proj, depth = nbr.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=packed.device)
    table, sbytes = _scratch(N, K, D, H, W, packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(_lib.load().mvsdet_plane_sweep_variance_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj),
                                                                      _lib.ptr(depth), _lib.ptr(out), _lib.ptr(table), sbytes,
                                                                      N, K, C, D, H, W, stream(packed)), name)
    return out, table


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_packed", mutates_args=(), device_types="cuda")
def plane_sweep_variance_packed(packed: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, C: int, H: int,
                                W: int) -> Tensor:
    """a3+a4 on already packed maps (mvsdet.py:439-467) -> (N,C,D,H,W)."""
    return _sweep_packed("plane_sweep_variance_packed", packed, nbr, proj, depth, C, H, W)[0]


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
    M, K = _check_packed("plane_sweep_variance_shard", packed, nbr, proj, depth, C, H, W, n_src=n_src)
    D = depth.shape[1]
    if M < 1 or ref_first < 0 or ref_first + M > n_src:
        raise ValueError(f"plane_sweep_variance_shard: views [{ref_first},{ref_first + M}) outside the {n_src} packed views")
    nbr, proj, depth = nbr.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((M, C, D, H, W), dtype=torch.float16 if half_out else torch.float32, device=packed.device)
    scratch, sbytes = _scratch(M, K, D, H, W, packed.device)
    lib = _lib.load()
    fn = lib.mvsdet_plane_sweep_variance_shard_f16 if half_out else lib.mvsdet_plane_sweep_variance_shard_f32
    with torch.cuda.device(packed.device):
        _lib.check(fn(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj), _lib.ptr(depth), _lib.ptr(out), _lib.ptr(scratch), sbytes,
                      n_src, ref_first, M, K, C, D, H, W, stream(packed)), "plane_sweep_variance_shard")
    return out


@plane_sweep_variance_shard.register_fake
def _(packed, nbr, proj, depth, n_src, ref_first, C, H, W, half_out=False):
    return packed.new_empty((nbr.shape[0], C, depth.shape[1], H, W), dtype=torch.float16 if half_out else torch.float32)


def _build_table(entry, name, proj, depth, H, W, *pitch):
    """One geometry table: proj (N,K,4,4), depth (N,D) -> the opaque flat buffer `entry` fills (`pitch`: for the entries that take one)."""
    req(proj, "proj", dim=4)
    req(depth, "depth", dim=2)
    N, K = proj.shape[:2]
    D = depth.shape[1]
    table, sbytes = _scratch(N, K, D, H, W, proj.device)
    proj, depth = proj.contiguous(), depth.contiguous()
    with torch.cuda.device(proj.device):
        _lib.check(getattr(_lib.load(), entry)(_lib.ptr(proj), _lib.ptr(depth), _lib.ptr(table), sbytes, N, K, D, H, W,
                                               *(int(v) for v in pitch), stream(proj)), name)
    return table


@torch.library.custom_op(f"{_NS}::plane_sweep_table", mutates_args=(), device_types="cuda")
def plane_sweep_table(proj: Tensor, depth: Tensor, H: int, W: int) -> Tensor:
    """Channel-independent sampling table of a scene (8 B per view, neighbour, plane, pixel): proj (N,K,4,4),
    depth (N,D) -> opaque flat buffer for plane_sweep_variance_tabled."""
    return _build_table("mvsdet_plane_sweep_table_f32", "plane_sweep_table", proj, depth, H, W)


@plane_sweep_table.register_fake
def _fake_table(proj, depth, H, W, w_pitch=0):
    return _scratch(proj.shape[0], proj.shape[1], depth.shape[1], H, W, proj.device)[0]


def plane_sweep_table_pitched(proj: Tensor, depth: Tensor, H: int, W: int, w_pitch: int) -> Tensor:
    """plane_sweep_table for a cost volume with row pitch `w_pitch` (plane_sweep_variance_tabled_pitched)."""
    return _build_table("mvsdet_plane_sweep_table_pitched_f32", "plane_sweep_table_pitched", proj, depth, H, W, w_pitch)


@torch.library.custom_op(f"{_NS}::plane_sweep_table_pooled", mutates_args=(), device_types="cuda")
def plane_sweep_table_pooled(proj: Tensor, depth: Tensor, H: int, W: int, w_pitch: int = 0) -> Tensor:
    """plane_sweep_table / plane_sweep_table_pitched (w_pitch: 0 or W = contiguous) under the pooled run policy: with two
    neighbours and 32x4 tiles a footprint box may take the other neighbour's idle LDS slot (csrc/sweep_kernel.h).  For the
    FORWARD sweep only (plane_sweep_variance_tabled / _pitched); the backward refuses such a table (all-NaN gradient).
    Library option "sweep_pool" 0: the unpooled table."""
    return _build_table("mvsdet_plane_sweep_table_pooled_f32", "plane_sweep_table_pooled", proj, depth, H, W, w_pitch)


plane_sweep_table_pooled.register_fake(_fake_table)


def _run_tabled(entry, name, packed, nbr, table, C, D, H, W, dtype, w_pitch=None):
    """The per-channel half of the sweep through `entry` -> (N,C,D,H,W) of `dtype`; with `w_pitch` the view of an (N,C,D,H,w_pitch) buffer."""
    req(packed, "packed", dim=1)
    req(nbr, "nbr", dtype=torch.int64, dim=2)
    req(table, "table", dim=1)
    if w_pitch is not None and w_pitch < W:
        raise ValueError(f"{name}: pitch {w_pitch} < W={W}")
    N, K = nbr.shape
    nbr = nbr.contiguous()
    pitch = () if w_pitch is None else (int(w_pitch),)
    buf = torch.empty((N, C, D, H, *(pitch or (W,))), dtype=dtype, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(getattr(_lib.load(), entry)(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(table), table.numel() * 4, _lib.ptr(buf),
                                               N, K, C, D, H, W, *pitch, stream(packed)), name)
    return buf if w_pitch is None else buf[..., :W]


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_tabled", mutates_args=(), device_types="cuda")
def plane_sweep_variance_tabled(packed: Tensor, nbr: Tensor, table: Tensor, C: int, D: int, H: int, W: int) -> Tensor:
    """The per-channel half of the sweep on a table from plane_sweep_table -> (N,C,D,H,W)."""
    return _run_tabled("mvsdet_plane_sweep_variance_tabled_f32", "plane_sweep_variance_tabled", packed, nbr, table, C, D, H, W,
                       torch.float32)


@plane_sweep_variance_tabled.register_fake
def _(packed, nbr, table, C, D, H, W):
    return packed.new_empty((nbr.shape[0], C, D, H, W))


def plane_sweep_variance_tabled_f16(packed: Tensor, nbr: Tensor, table: Tensor, C: int, D: int, H: int, W: int) -> Tensor:
    """plane_sweep_variance_tabled with fp16 storage: the fp32 result rounded to nearest-even at the store -> (N,C,D,H,W) float16.
    Forward only."""
    return _run_tabled("mvsdet_plane_sweep_variance_tabled_f16", "plane_sweep_variance_tabled_f16", packed, nbr, table, C, D, H, W,
                       torch.float16)


def plane_sweep_variance_tabled_pitched(packed: Tensor, nbr: Tensor, table: Tensor, C: int, D: int, H: int, W: int,
                                        w_pitch: int) -> Tensor:
    """The per-channel half of the sweep into a row-PITCHED volume: returns the (N,C,D,H,W) view of an (N,C,D,H,w_pitch)
    buffer -- the values of plane_sweep_variance_tabled bit for bit, rows `w_pitch` elements apart (every row on a 128-byte
    line when w_pitch % 32 == 0: whole-line stores from 32x4 tiles for the 80-wide maps of the shipped configs).
    Forward only; the pad columns are never written."""
    return _run_tabled("mvsdet_plane_sweep_variance_tabled_pitched_f32", "plane_sweep_variance_tabled_pitched", packed, nbr, table,
                       C, D, H, W, torch.float32, w_pitch)


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


@torch.library.custom_op(f"{_NS}::plane_sweep_variance", mutates_args=(), device_types="cuda")
def plane_sweep_variance(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor) -> Tensor:
    """a3+a4 (mvsdet.py:439-467): feat (N,C,H,W), nbr (N,K) int64, proj (N,K,4,4), depth (N,D) -> (N,C,D,H,W)."""
    N, K, C, D, H, W = _check_sweep(feat, nbr, proj, depth)
    packed = pack_features(feat)
    return plane_sweep_variance_packed(packed, nbr, proj, depth, C, H, W)


@plane_sweep_variance.register_fake
def _fake_sweep(feat, nbr, proj, depth):
    N, C, H, W = feat.shape
    return feat.new_empty((N, C, depth.shape[1], H, W))


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_backward", mutates_args=(), device_types="cuda")
def plane_sweep_variance_backward(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, grad: Tensor) -> Tensor:
    N, K, C, D, H, W = _check_sweep(feat, nbr, proj, depth)
    req(grad, "grad", dim=5)
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
                                                           D, H, W, stream(feat)), "plane_sweep_variance_backward")
    return gfeat


@plane_sweep_variance_backward.register_fake
def _fake_like_feat(feat, nbr, proj, depth, grad):
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
    out, table = _sweep_packed("plane_sweep_variance_keep", packed, nbr, proj, depth, C, H, W)
    return out, packed, table


@plane_sweep_variance_keep.register_fake
def _(feat, nbr, proj, depth):
    N, C, H, W = feat.shape
    return (feat.new_empty((N, C, depth.shape[1], H, W)), feat.new_empty((N * ((C + 31) // 32) * H * W * 32,)),
            _scratch(N, nbr.shape[1], depth.shape[1], H, W, feat.device)[0])


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_backward_packed", mutates_args=(), device_types="cuda")
def plane_sweep_variance_backward_packed(packed: Tensor, nbr: Tensor, table: Tensor, grad: Tensor) -> Tensor:
    """dL/dfeat (N,C,H,W) from dL/dvar (N,C,D,H,W), the packed maps and the sweep geometry of the forward pass."""
    req(grad, "grad", dim=5)
    req(nbr, "nbr", dtype=torch.int64, dim=2)
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
                                                                  stream(grad)), "plane_sweep_variance_backward_packed")
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
    req(depth, "depth", dim=4)
    if depth.shape[0] != B or tuple(depth.shape[2:]) != (H, W):
        raise ValueError(f"{name}: depth {tuple(depth.shape)} is not (B={B}, D, H={H}, W={W})")
    return depth.shape[1]


@torch.library.custom_op(f"{_NS}::homo_warp_pixel", mutates_args=(), device_types="cuda")
def homo_warp_pixel(src: Tensor, proj: Tensor, depth: Tensor) -> Tensor:
    """a3 at per-pixel depths: src (B,C,H,W), proj (B,4,4) = src_proj @ inv(ref_proj), depth (B,D,H,W) -> (B,C,D,H,W).
    Differentiable in src."""
    req(src, "src", dim=4)
    req(proj, "proj", dim=3)
    B, C, H, W = src.shape
    D = _check_depth_pixel("homo_warp_pixel", depth, B, H, W)
    if proj.shape != (B, 4, 4):
        raise ValueError(f"homo_warp_pixel: proj {tuple(proj.shape)} does not match B={B}")
    src, proj, depth = src.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((B, C, D, H, W), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().mvsdet_homo_warp_pixel_f32(_lib.ptr(src), _lib.ptr(proj), _lib.ptr(depth), _lib.ptr(out),
                                                          B, C, D, H, W, stream(src)), "homo_warp_pixel")
    return out


homo_warp_pixel.register_fake(_fake_warp)


@torch.library.custom_op(f"{_NS}::homo_warp_pixel_backward", mutates_args=(), device_types="cuda")
def homo_warp_pixel_backward(proj: Tensor, depth: Tensor, grad: Tensor) -> Tensor:
    """dL/dsrc (B,C,H,W) from dL/dwarped (B,C,D,H,W): bilinear scatter with float atomics (last bits depend on arrival order)."""
    req(grad, "grad", dim=5)
    req(proj, "proj", dim=3)
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
                                                      wbytes, B, C, D, H, W, stream(grad)), "homo_warp_pixel_backward")
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
    req(feat, "feat", dim=4)
    req(nbr, "nbr", dtype=torch.int64, dim=2)
    req(proj, "proj", dim=4)
    N, C, H, W = feat.shape
    D = _check_depth_pixel("plane_sweep_variance_pixel", depth, N, H, W)
    K = nbr.shape[1]
    if nbr.shape[0] != N or proj.shape != (N, K, 4, 4):
        raise ValueError(f"plane_sweep_variance_pixel: nbr {tuple(nbr.shape)}, proj {tuple(proj.shape)} do not match N={N}")
    return N, K, C, D, H, W


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_pixel_packed", mutates_args=(), device_types="cuda")
def plane_sweep_variance_pixel_packed(packed: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, C: int) -> Tensor:
    """a3+a4 at per-pixel depths on already packed maps: depth (N,D,H,W) -> variance (N,C,D,H,W)."""
    H, W = depth.shape[-2:]
    N, K = _check_packed("plane_sweep_variance_pixel_packed", packed, nbr, proj, depth, C, H, W, depth_dim=4)
    D = depth.shape[1]
    nbr, proj, depth = nbr.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(_lib.load().mvsdet_plane_sweep_variance_pixel_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj),
                                                                            _lib.ptr(depth), _lib.ptr(out), N, K, C, D, H, W,
                                                                            stream(packed)), "plane_sweep_variance_pixel_packed")
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


plane_sweep_variance_pixel.register_fake(_fake_sweep)


@torch.library.custom_op(f"{_NS}::plane_sweep_variance_pixel_backward", mutates_args=(), device_types="cuda")
def plane_sweep_variance_pixel_backward(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, grad: Tensor) -> Tensor:
    N, K, C, D, H, W = _check_sweep_pixel(feat, nbr, proj, depth)
    req(grad, "grad", dim=5)
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
                                                                        D, H, W, stream(feat)), "plane_sweep_variance_pixel_backward")
    return gfeat


plane_sweep_variance_pixel_backward.register_fake(_fake_like_feat)


def _sweep_pixel_bwd(ctx, grad):
    feat, nbr, proj, depth = ctx.saved_tensors
    return plane_sweep_variance_pixel_backward(feat, nbr, proj, depth, grad), None, None, None


plane_sweep_variance_pixel.register_autograd(_sweep_pixel_bwd, setup_context=_sweep_setup)


# ------------------------------------------------------------------------------------------- group-wise correlation
# The second reduction of stage 1 (the reference's mvs_models/lss_fpn.py:499-506): per neighbour the mean over a group's C/G
# channels of reference feature x warped feature, fused with the warp (csrc/groupcorr.hip).  Plane depths (N,D) and per-pixel
# depths (N,D,H,W) run the same kernel: the depth is read through strides, a plane depth with pixel stride 0.
# These operators are names of THIS module (ops.sweep.plane_sweep_groupcorr ...), not re-exported by the package: its recorded
# surface (tests/golden/ops_surface.json) is closed.  functional.groupwise_correlation is the interface callers use.
GROUPCORR_RULE = "C % groups == 0 and C / groups in {4, 8, 16} or a multiple of 32"


def _check_groups(name, C, groups):
    if groups < 1 or C % groups != 0 or not (C // groups in (4, 8, 16) or (C // groups) % 32 == 0):
        raise ValueError(f"{name}: C={C}, groups={groups}: the supported group widths are {GROUPCORR_RULE}")


def _check_groupcorr_depth(name, nbr, proj, depth, N, H, W):
    """nbr (N,K) with K >= 1, proj (N,K,4,4), depth (N,D) or (N,D,H,W) -> K, D."""
    req(nbr, "nbr", dtype=torch.int64, dim=2)
    req(proj, "proj", dim=4)
    if depth.dim() == 4:
        D = _check_depth_pixel(name, depth, N, H, W)
    elif depth.dim() == 2:
        req(depth, "depth", dim=2)
        D = depth.shape[1]
        if depth.shape[0] != N:
            raise ValueError(f"{name}: depth {tuple(depth.shape)} is not (N={N}, D)")
    else:
        raise ValueError(f"{name}: depth must be (N,D) or (N,D,H,W) (got shape {tuple(depth.shape)})")
    K = nbr.shape[1]
    if K < 1:
        raise ValueError(f"{name}: at least one neighbour per view (K={K})")
    if nbr.shape[0] != N or proj.shape != (N, K, 4, 4):
        raise ValueError(f"{name}: nbr {tuple(nbr.shape)}, proj {tuple(proj.shape)} do not match N={N}")
    return K, D


def _depth_strides(depth):
    """depth_strides of the C entries for a contiguous depth: {view, hypothesis, pixel}; pixel stride 0 for plane depths."""
    D = depth.shape[1]
    if depth.dim() == 2:
        return (ctypes.c_int64 * 3)(D, 1, 0)
    HW = depth.shape[2] * depth.shape[3]
    return (ctypes.c_int64 * 3)(D * HW, HW, 1)


@torch.library.custom_op(f"{_NS}::plane_sweep_groupcorr_packed", mutates_args=(), device_types="cuda")
def plane_sweep_groupcorr_packed(packed: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, C: int, groups: int, H: int = 0,
                                 W: int = 0) -> Tensor:
    """Group-wise correlation on already packed maps of (N,C,H,W) features: nbr (N,K), proj (N,K,4,4), depth (N,D) or (N,D,H,W)
    -> (N,K,groups,D,H,W) float32.  H, W: needed with plane depths only, which do not carry the map's shape."""
    name = "plane_sweep_groupcorr_packed"
    req(packed, "packed", dim=1)
    _check_groups(name, C, groups)
    if depth.dim() == 4 and (H, W) == (0, 0):
        H, W = depth.shape[-2:]
    if H < 1 or W < 1:
        raise ValueError(f"{name}: plane depths need the map's H and W")
    N = nbr.shape[0] if nbr.dim() == 2 else -1
    K, D = _check_groupcorr_depth(name, nbr, proj, depth, N, H, W)
    if packed.numel() * 4 != _lib.load().mvsdet_packed_bytes(N, C, H, W):
        raise ValueError(f"{name}: packed buffer does not match (N,C,H,W)")
    nbr, proj, depth = nbr.contiguous(), proj.contiguous(), depth.contiguous()
    out = torch.empty((N, K, groups, D, H, W), dtype=torch.float32, device=packed.device)
    with torch.cuda.device(packed.device):
        _lib.check(_lib.load().mvsdet_plane_sweep_groupcorr_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj), _lib.ptr(depth),
                                                                       _depth_strides(depth), _lib.ptr(out), N, K, C, groups, D, H, W,
                                                                       stream(packed)), name)
    return out


@plane_sweep_groupcorr_packed.register_fake
def _(packed, nbr, proj, depth, C, groups, H=0, W=0):
    if depth.dim() == 4 and (H, W) == (0, 0):
        H, W = depth.shape[-2:]
    return packed.new_empty((nbr.shape[0], nbr.shape[1], groups, depth.shape[1], H, W))


@torch.library.custom_op(f"{_NS}::plane_sweep_groupcorr", mutates_args=(), device_types="cuda")
def plane_sweep_groupcorr(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, groups: int) -> Tensor:
    """Group-wise correlation cost volume: feat (N,C,H,W), nbr (N,K) int64, proj (N,K,4,4), depth (N,D) or (N,D,H,W) ->
    (N,K,groups,D,H,W): out[n,j,g] = mean over the C/groups channels of group g of feat[n] * warp_j(feat[nbr[n,j]]).
    Differentiable in feat (the backward packs the features again)."""
    req(feat, "feat", dim=4)
    N, C, H, W = feat.shape
    _check_groups("plane_sweep_groupcorr", C, groups)
    _check_groupcorr_depth("plane_sweep_groupcorr", nbr, proj, depth, N, H, W)
    return plane_sweep_groupcorr_packed(pack_features(feat), nbr, proj, depth, C, groups, H, W)


@plane_sweep_groupcorr.register_fake
def _(feat, nbr, proj, depth, groups):
    N, C, H, W = feat.shape
    return feat.new_empty((N, nbr.shape[1], groups, depth.shape[1], H, W))


@torch.library.custom_op(f"{_NS}::plane_sweep_groupcorr_backward", mutates_args=(), device_types="cuda")
def plane_sweep_groupcorr_backward(feat: Tensor, nbr: Tensor, proj: Tensor, depth: Tensor, grad: Tensor, groups: int) -> Tensor:
    """dL/dfeat (N,C,H,W) from dL/dcorr (N,K,groups,D,H,W): float atomics, the last bits depend on arrival order."""
    name = "plane_sweep_groupcorr_backward"
    req(feat, "feat", dim=4)
    N, C, H, W = feat.shape
    _check_groups(name, C, groups)
    K, D = _check_groupcorr_depth(name, nbr, proj, depth, N, H, W)
    req(grad, "grad", dim=6)
    if grad.shape != (N, K, groups, D, H, W):
        raise ValueError(f"{name}: grad {tuple(grad.shape)} is not (N,K,groups,D,H,W) = {(N, K, groups, D, H, W)}")
    packed = pack_features(feat)
    nbr, proj, depth, grad = nbr.contiguous(), proj.contiguous(), depth.contiguous(), grad.contiguous()
    lib = _lib.load()
    wbytes = int(lib.mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W))
    ws = torch.empty(wbytes // 4, dtype=torch.float32, device=feat.device)
    gfeat = torch.empty((N, C, H, W), dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        _lib.check(lib.mvsdet_plane_sweep_groupcorr_bwd_packed_f32(_lib.ptr(packed), _lib.ptr(nbr), _lib.ptr(proj), _lib.ptr(depth),
                                                                   _depth_strides(depth), _lib.ptr(grad), _lib.ptr(gfeat), _lib.ptr(ws),
                                                                   wbytes, N, K, C, groups, D, H, W, stream(feat)), name)
    return gfeat


@plane_sweep_groupcorr_backward.register_fake
def _(feat, nbr, proj, depth, grad, groups):
    return torch.empty_like(feat)


def _groupcorr_setup(ctx, inputs, output):
    feat, nbr, proj, depth, groups = inputs
    ctx.save_for_backward(feat, nbr, proj, depth)
    ctx.groups = groups


def _groupcorr_bwd(ctx, grad):
    feat, nbr, proj, depth = ctx.saved_tensors
    return plane_sweep_groupcorr_backward(feat, nbr, proj, depth, grad, ctx.groups), None, None, None, None


plane_sweep_groupcorr.register_autograd(_groupcorr_bwd, setup_context=_groupcorr_setup)
# under torch.autocast low-precision floating inputs are cast to float32, the rule of the package's other forward operators
plane_sweep_groupcorr.register_autocast("cuda", torch.float32)


# ------------------------------------------------------------------------------------------- the benchmark's two yardsticks
def device_copy(src: Tensor, dst: Tensor):
    """float4 device-to-device copy kernel (bench.py's achievable-HBM yardstick)."""
    req(src, "src")
    req(dst, "dst")
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().mvsdet_copy_f32(_lib.ptr(src), _lib.ptr(dst), src.numel(), stream(src)), "copy")


def store_pattern_probe(var: Tensor, W: int, tile_w: int, planes_per_block: int = 0) -> None:
    """Overwrites `var` -- an (N,C,D,H,pitch) fp32 or fp16 buffer -- with the sweep's store stream alone (bench.py: the ceiling
    of the output layout on the box at hand)."""
    if var.dtype not in (torch.float32, torch.float16) or not var.is_cuda or not var.is_contiguous() or var.dim() != 5:
        raise ValueError("store_pattern_probe: var must be a contiguous 5-D fp32 or fp16 CUDA tensor")
    N, C, D, H, pitch = var.shape
    lib = _lib.load()
    fn = lib.mvsdet_store_pattern_probe_f32 if var.dtype == torch.float32 else lib.mvsdet_store_pattern_probe_f16
    with torch.cuda.device(var.device):
        _lib.check(fn(_lib.ptr(var), N, C, D, H, int(W), int(pitch), int(tile_w), int(planes_per_block), stream(var)),
                   "store_pattern_probe")
