"""The cost network (f-1): bf16x3 / fp16 + MX layouts and convolutions, the neck's two GEMM-shaped layers, the fp32 MFMA
convolutions, the weight gradients and training BatchNorm."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch
from torch import Tensor

from ._common import _NS, _lib, req, stream


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
            _lib.check(_lib.load().mvsdet_split_conv_weight_ordered(_lib.ptr(w), _lib.ptr(out), cout, cin, order, stream(w)),
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
            _lib.check(lib.mvsdet_split_conv_weights_batched(wp, op, ia(couts), ia(cins), ia(orders), n, stream(ws[0])),
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
    req(x, "x", dim=5)
    if x.stride(4) != 1 or min(x.stride()) < 0:
        x = x.contiguous()
    N, C, D, H, W = x.shape
    nbytes, padded = scl_geometry(N, C, D, H, W)
    fresh = out is None or out.shape != tuple(x.shape) or out.data.device != x.device
    if fresh:
        out = SclTensor(torch.empty((nbytes // 2,), dtype=torch.bfloat16, device=x.device), x.shape, padded)
    xstr = (ctypes.c_int64 * 4)(*[int(v) for v in x.stride()[:4]])
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_scl_pack_f32(_lib.ptr(x), xstr, _lib.ptr(out.data), N, C, D, H, W, 2 if fresh else 0, stream(x)),
                   "scl_pack")
    return out


def gemm_split_weight(wmat: Tensor) -> Tensor:
    """(M, K) fp32 row-major -> the fragment-ordered bf16 pieces the neck's GEMM-shaped layers stream from L2
    ([M/32][K/16][2 pieces][64 lanes][8] bf16; M % 128 == 0, K % 32 == 0: include/mvsdet_hip.h)."""
    req(wmat, "wmat", dim=2)
    M, K = wmat.shape
    lib = _lib.load()
    nbytes = int(lib.mvsdet_gemm_split_weight_bytes(int(M), int(K)))
    if nbytes == 0:
        raise ValueError(f"gemm_split_weight: ({M}, {K}) is not (128 m, 32 k)")
    w = wmat.detach().contiguous()
    out = torch.empty((nbytes // 2,), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(lib.mvsdet_gemm_split_weight(_lib.ptr(w), _lib.ptr(out), int(M), int(K), stream(w)), "gemm_split_weight")
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
    req(x, "x", dim=5)
    req(bias, "bias", dim=1)
    x = x.contiguous()
    N, Cin, D, H, W = x.shape
    if D % 2 or H % 2 or W % 2 or bias.numel() != cout:
        raise ValueError("conv3d_k1_s2_bf16x3: D, H, W must be even and bias have Cout elements")
    _check_wsplit("conv3d_k1_s2_bf16x3", wsplit, cout, Cin, x)
    out = torch.empty((N, cout, D // 2, H // 2, W // 2), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_conv3d_k1_s2_bf16x3(_lib.ptr(x), _lib.ptr(wsplit), _lib.ptr(bias.contiguous()), _lib.ptr(out), N, Cin,
                                                          int(cout), D, H, W, int(relu), stream(x)), "conv3d_k1_s2_bf16x3")
    return out


def convT3d_k2_s2_bf16x3(x: Tensor, wsplit: Tensor, bias: Tensor, cout: int, relu: bool = True) -> Tensor:
    """ConvTranspose3d(kernel 2, stride 2) + bias [+ ReLU]: (N,Cin,D,H,W) -> (N,Cout,2D,2H,2W), the 2x2x2 interleave written by the
    GEMM's epilogue (imvoxel_neck.py:166-180).  `wsplit` = gemm_split_weight of the (8 Cout, Cin) matrix with rows 8 o + 4 p + 2 q + r."""
    req(x, "x", dim=5)
    req(bias, "bias", dim=1)
    x = x.contiguous()
    N, Cin, D, H, W = x.shape
    if bias.numel() != cout:
        raise ValueError("convT3d_k2_s2_bf16x3: bias must have Cout elements")
    _check_wsplit("convT3d_k2_s2_bf16x3", wsplit, 8 * cout, Cin, x)
    out = torch.empty((N, cout, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_convT3d_k2_s2_bf16x3(_lib.ptr(x), _lib.ptr(wsplit), _lib.ptr(bias.contiguous()), _lib.ptr(out), N, Cin,
                                                           int(cout), D, H, W, int(relu), stream(x)), "convT3d_k2_s2_bf16x3")
    return out


# ---- the two GEMM-shaped layers under autograd: input and weight gradients (csrc/neck_gemm.hip MODEs 2 / 3, neck_gemm_dw_bf16x3_kernel)
@torch.library.custom_op(f"{_NS}::conv3d_k1_s2_dx_bf16x3", mutates_args=("grad_x",), device_types="cuda")
def conv3d_k1_s2_dx_bf16x3(grad_out: Tensor, wsplit: Tensor, grad_x: Tensor) -> None:
    """Input gradient of Conv3d(kernel 1, stride 2, no bias) ACCUMULATED into `grad_x` (N,Cin,D,H,W) at its even positions only:
    grad_x[:, c, 2d, 2h, 2w] += sum_o W[o, c] grad_out[:, o, d, h, w].  `wsplit` = gemm_split_weight of the (Cin, Cout) matrix W^T.
    The other positions of grad_x are left as they are (the caller's tensor holds the gradient of the block's other branch)."""
    req(grad_out, "grad_out", dim=5)
    req(grad_x, "grad_x", dim=5)
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
                                                             stream(grad_out)), "conv3d_k1_s2_dx_bf16x3")


@conv3d_k1_s2_dx_bf16x3.register_fake
def _(grad_out, wsplit, grad_x):
    return None


@torch.library.custom_op(f"{_NS}::convT3d_k2_s2_dx_bf16x3", mutates_args=(), device_types="cuda")
def convT3d_k2_s2_dx_bf16x3(grad_out: Tensor, wsplit: Tensor, cin: int) -> Tensor:
    """Input gradient of ConvTranspose3d(kernel 2, stride 2, no bias): grad_out (N,Cout,2D,2H,2W) -> (N,Cin,D,H,W),
    grad_x[:, c, v] = sum_{o,p,q,r} W[c, o, p, q, r] grad_out[:, o, 2v + (p, q, r)].  `wsplit` = gemm_split_weight of W.reshape(Cin, 8 Cout)."""
    req(grad_out, "grad_out", dim=5)
    grad_out = grad_out.contiguous()
    N, Cout, D2, H2, W2 = grad_out.shape
    if D2 % 2 or H2 % 2 or W2 % 2:
        raise ValueError(f"convT3d_k2_s2_dx_bf16x3: grad_out {tuple(grad_out.shape)} must have even D, H, W")
    _check_wsplit("convT3d_k2_s2_dx_bf16x3", wsplit, int(cin), 8 * Cout, grad_out)
    gx = torch.empty((N, int(cin), D2 // 2, H2 // 2, W2 // 2), dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        _lib.check(_lib.load().mvsdet_convT3d_k2_s2_dx_bf16x3(_lib.ptr(grad_out), _lib.ptr(wsplit), _lib.ptr(gx), N, int(cin), Cout, D2 // 2,
                                                              H2 // 2, W2 // 2, stream(grad_out)), "convT3d_k2_s2_dx_bf16x3")
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
    req(x, "x", dim=5)
    req(grad_out, "grad_out", dim=5)
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
                                                  int(transposed), N, Cin, Cout, D, H, W, stream(x)), "neck_gemm_dw_bf16x3")
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
    req(x, "x", dim=5)
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
        req(scale, "scale", dim=1)
        req(shift, "shift", dim=1)
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
        req(residual, "residual", dim=5)
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
    req(weight, "weight", dim=5)
    Cout, Cin = weight.shape[:2]
    lib = _lib.load()
    nbytes = int(lib.mvsdet_split_conv_weight_mx_bytes(int(Cout), int(Cin)))
    if nbytes == 0 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError(f"split_conv_weight_mx: weight {tuple(weight.shape)} is not (64 m, Cin, 3, 3, 3)")
    w = weight.detach().contiguous()
    out = torch.empty((Cout // 64, (Cin + 7) // 8, 2, 32, 64, 4), dtype=torch.int32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(lib.mvsdet_split_conv_weight_mx(_lib.ptr(w), _lib.ptr(out), int(Cout), int(Cin), stream(w)), "split_conv_weight_mx")
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
        req(residual, "residual", dim=5)
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


# ---- the network's head, the fp32 MFMA convolutions, the weight gradients and training BatchNorm
def conv3d_k3_cout2_sum(x: Tensor, x2: Optional[Tensor], weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """Conv3d(Cin -> 2, kernel 3, padding 1, bias) of mvs_models/mvsnet.py:102,112 on x + x2 (N,Cin,D,H,W) -> (N,2,D,H,W): the
    skip addition of mvsnet.py:111 formed while the head stages its input (forward only; x2 None: x alone)."""
    req(x, "x", dim=5)
    req(weight, "weight", dim=5)
    N, Cin, D, H, W = x.shape
    if tuple(weight.shape) != (2, Cin, 3, 3, 3):
        raise ValueError(f"conv3d_k3_cout2_sum: weight {tuple(weight.shape)} != (2,{Cin},3,3,3)")
    if x2 is not None:
        req(x2, "x2", dim=5)
        if x2.shape != x.shape:
            raise ValueError(f"conv3d_k3_cout2_sum: x2 {tuple(x2.shape)} != x {tuple(x.shape)}")
        if W % 4:
            return conv3d_k3_cout2(x + x2, weight, bias)
        x2 = x2.contiguous()
    if bias is not None:
        req(bias, "bias", dim=1)
        bias = bias.contiguous()
    x, weight = x.contiguous(), weight.contiguous()
    out = torch.empty((N, 2, D, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_conv3d_k3_cout2_sum_f32(_lib.ptr(x), _lib.ptr(x2), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out),
                                                              N, Cin, D, H, W, stream(x)), "conv3d_k3_cout2_sum")
    return out


@torch.library.custom_op(f"{_NS}::conv3d_k3_cout2", mutates_args=(), device_types="cuda")
def conv3d_k3_cout2(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """Conv3d(Cin -> 2, kernel 3, stride 1, padding 1) of mvs_models/mvsnet.py:102 on (N,Cin,D,H,W) -> (N,2,D,H,W).
    Forward only: under autograd use torch's convolution (mvsdet_amd.costreg does)."""
    req(x, "x", dim=5)
    req(weight, "weight", dim=5)
    N, Cin, D, H, W = x.shape
    if tuple(weight.shape) != (2, Cin, 3, 3, 3):
        raise ValueError(f"conv3d_k3_cout2: weight {tuple(weight.shape)} != (2,{Cin},3,3,3)")
    if bias is not None:
        req(bias, "bias", dim=1)
        if bias.numel() != 2:
            raise ValueError("conv3d_k3_cout2: bias must have 2 elements")
        bias = bias.contiguous()
    x, weight = x.contiguous(), weight.contiguous()
    out = torch.empty((N, 2, D, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_conv3d_k3_cout2_f32(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out), N, Cin,
                                                          D, H, W, stream(x)), "conv3d_k3_cout2")
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
    req(x, "x", dim=5)
    req(weight_perm, "weight_perm", dim=5)
    N, Cin, D, H, W = x.shape
    Cout = weight_perm.shape[4]
    if tuple(weight_perm.shape[:4]) != (Cin + Cin % 2, 3, 3, 3) or Cout % 64:
        raise ValueError(f"conv3d_k3_mfma: weight_perm {tuple(weight_perm.shape)} does not match Cin={Cin}")
    scale, shift = _check_affine("conv3d_k3_mfma", scale, shift, Cout)
    if stride not in (1, 2):
        raise ValueError("conv3d_k3_mfma: stride must be 1 or 2")
    x, weight_perm = x.contiguous(), weight_perm.contiguous()
    od, oh, ow = (D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((N, Cout, od, oh, ow), dtype=torch.float32, device=x.device)
    if residual is not None:   # added between the affine and the ReLU (imvoxel_neck.py:227-229); stride 1 only
        req(residual, "residual", dim=5)
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
                                                    stride, int(relu), stream(x)), "conv3d_k3_mfma")
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
    req(x, "x", dim=5)
    req(weight_perm, "weight_perm", dim=5)
    N, Cin, D, H, W = x.shape
    Cout = weight_perm.shape[4]
    if tuple(weight_perm.shape[:4]) != (Cin + Cin % 2, 3, 3, 3) or Cout % 64:
        raise ValueError(f"convT3d_k3_s2_mfma: weight_perm {tuple(weight_perm.shape)} does not match Cin={Cin}")
    scale, shift = _check_affine("convT3d_k3_s2_mfma", scale, shift, Cout)
    oshape = (N, Cout, 2 * D, 2 * H, 2 * W)
    if residual is not None:
        req(residual, "residual", dim=5)
        if tuple(residual.shape) != oshape:
            raise ValueError(f"convT3d_k3_s2_mfma: residual {tuple(residual.shape)} != {oshape}")
        residual = residual.contiguous()
    x, weight_perm = x.contiguous(), weight_perm.contiguous()
    out = torch.empty(oshape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mvsdet_convT3d_k3_s2_mfma_f32(_lib.ptr(x), _lib.ptr(weight_perm), _lib.ptr(scale),
                                                             _lib.ptr(shift), _lib.ptr(residual), _lib.ptr(out), N, Cin, Cout,
                                                             D, H, W, int(relu), stream(x)), "convT3d_k3_s2_mfma")
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
    req(x, "x", dim=5)
    req(grad_out, "grad_out", dim=5)
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
        _lib.check(fn(_lib.ptr(x), _lib.ptr(grad_out), _lib.ptr(partial), pbytes, nsplit, N, Cin, Cout, D, H, W, stream(x)),
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
    req(x, "x", dim=5)
    req(weight, "weight", dim=5)
    req(grad_out, "grad_out", dim=5)
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
                                                     stream(x)), "conv3d_k3_cout2_dx")
        fn = lib.mvsdet_conv3d_k3_cout2_dw_bf16x3 if on_mfma else lib.mvsdet_conv3d_k3_cout2_dw_f32
        _lib.check(fn(_lib.ptr(x), _lib.ptr(grad_out), _lib.ptr(partial), partial.numel() * 4, nsplit, N, Cin, D, H, W,
                      stream(x)), "conv3d_k3_cout2_dw")
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
            req(t, tname, dim=1)
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
    req(x, "x", dim=5)
    if residual is not None:
        req(residual, "residual", dim=5)
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
                                                                _lib.ptr(ws), wb, N, C, vol, 0.0, float(eps), int(relu), stream(x)),
                       "bn3d_relu_train")
        else:
            _lib.check(lib.mvsdet_bn3d_relu_train_fwd_res_f32(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(residual), None, None,
                                                              _lib.ptr(out), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(ws), wb, N, C, vol,
                                                              0.0, float(eps), int(relu), stream(x)), "bn3d_relu_train")
    return out, mean, invstd


@bn3d_relu_train.register_fake
def _(x, weight, bias, eps, relu, residual=None, parts=None, pivot=None):
    return torch.empty_like(x), x.new_empty(x.shape[1]), x.new_empty(x.shape[1])


@torch.library.custom_op(f"{_NS}::bn3d_relu_backward", mutates_args=(), device_types="cuda")
def bn3d_relu_backward(x: Tensor, grad_out: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], save_mean: Tensor,
                       save_invstd: Tensor, relu: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """Backward of bn3d_relu_train -> (grad_x, grad_weight, grad_bias)."""
    req(x, "x", dim=5)
    req(grad_out, "grad_out", dim=5)
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
                                                vol, int(relu), stream(x)), "bn3d_relu_backward")
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
    req(x, "x", dim=5)
    req(residual, "residual", dim=5)
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
                                                          float(eps), int(relu), stream(x)), "bn3d_res_relu_train")
    return out, mean, invstd


@bn3d_res_relu_train.register_fake
def _(x, weight, bias, residual, eps, relu, parts=None, pivot=None):
    return torch.empty_like(x), x.new_empty(x.shape[1]), x.new_empty(x.shape[1])


@torch.library.custom_op(f"{_NS}::bn3d_res_relu_backward", mutates_args=(), device_types="cuda")
def bn3d_res_relu_backward(x: Tensor, out: Tensor, grad_out: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], save_mean: Tensor,
                           save_invstd: Tensor, relu: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Backward of bn3d_res_relu_train -> (grad_x, grad_weight, grad_bias, grad_residual); the ReLU mask is `out > 0`."""
    req(x, "x", dim=5)
    req(out, "out", dim=5)
    req(grad_out, "grad_out", dim=5)
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
                                                    _lib.ptr(gres), _lib.ptr(ws), wb, N, C, vol, int(relu), stream(x)), "bn3d_res_relu_backward")
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
