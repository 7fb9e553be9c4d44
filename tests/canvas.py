"""Guarded device memory for tests that call kernels through the C ABI (shared by test_gpu_conv_edges.py and
test_gpu_hotpath_canvases.py): inputs as strided views inside a NaN canvas, so that a stray read lands in owned memory and shows up
as NaN instead of being hidden by a zero weight or a masked lane; outputs, scratch and workspaces between 1 MiB guards of a fixed
bit pattern, so that a stray write is seen."""
import ctypes

import torch

SENTINEL = 0x5A5A5A5A                 # guard word of the output canvases
GUARD = 1 << 18                       # 1 MiB of 4-byte words on each side of an output


def nan_view(x, dev, pitch=3, plane_gap=5, chan_gap=7, view_gap=11):
    """x (N,C,D,H,W) as a strided view inside a NaN canvas on dev: (canvas, view)."""
    N, C, D, H, W = x.shape
    sH = W + pitch
    sD = H * sH + plane_gap
    sC = D * sD + chan_gap
    sN = C * sC + view_gap
    lead = (sC + 63) // 64 * 64                                  # >= one channel stride, 256-byte aligned
    canvas = torch.full((lead + N * sN + 2 * sC,), float("nan"), dtype=torch.float32, device=dev)
    v = canvas.as_strided((N, C, D, H, W), (sN, sC, sD, sH, 1), lead)
    v.copy_(x.to(dev))
    return canvas, v


def strides(v):
    return (ctypes.c_int64 * 4)(*[int(s) for s in v.stride()[:4]])


class Guarded:
    """nwords 4-byte words in the middle of a sentinel canvas (zeroed: an SCL / PSCL border is zero before a producer writes)."""

    def __init__(self, nwords, dev):
        self.n = int(nwords)
        self.canvas = torch.full((GUARD + (self.n + 3) // 4 * 4 + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.region = self.canvas[GUARD:GUARD + self.n]
        self.region.zero_()

    def ptr(self):
        return ctypes.c_void_p(self.region.data_ptr())

    def guards_intact(self):
        return bool((self.canvas[:GUARD] == SENTINEL).all()) and bool((self.canvas[GUARD + self.n:] == SENTINEL).all())


def guarded_f32(shape, dev):
    g = Guarded(torch.Size(shape).numel(), dev)
    return g, g.region.view(torch.float32).view(shape)


def ok(rc):
    from mvsdet_amd import _lib
    if rc != 0:
        raise AssertionError(_lib.load().mvsdet_last_error().decode())
    torch.cuda.synchronize()
