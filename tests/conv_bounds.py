"""Error bounds shared by the GPU tests of the convolution kernels (a helper module: nothing here is collected)."""
import torch
import torch.nn.functional as F


def mx_bound(x, w, sc, N, Cin, Cout, D, H, W, tile):
    """What the fp16 + MX scheme guarantees element by element (csrc/costreg_mx.h), in terms of each activation block's largest |x|
    (block = a tile's halo x 8 channels: one e8m0 scale per stage) and each weight block's largest |w| (taken over the output
    channel's 8 channels x 27 taps: at least the kernel's 2-tap block).  Per product term x*w the two e2m3 correction terms miss
    at most 2^-15 bmax |w| (Q(xh) * wr, Q(xr) * wh) and 2^-15 wmax |x| (xh * Q(wr), xr * Q(wh)): 2^-14 (bmax |w| + wmax |x|); then fp32
    accumulation (2^-21 of the summed |products|, as test_gpu_bf16's 4e-7) and the epilogue's rounding."""
    td, th, tw = tile
    G = (Cin + 7) // 8
    ax = F.pad(x.double().abs(), (0, 0, 0, 0, 0, 0, 0, 8 * G - Cin)).view(N, G, 8, D, H, W)
    gmax = ax.amax(2)                                                           # (N, G, D, H, W)
    nd, nh, nw = -(-D // td), -(-H // th), -(-W // tw)
    padded = F.pad(gmax, (1, nw * tw - W + 1, 1, nh * th - H + 1, 1, nd * td - D + 1))
    bmax = F.max_pool3d(padded, (td + 2, th + 2, tw + 2), (td, th, tw))         # (N, G, nd, nh, nw): the halo maxima
    bmax = bmax.repeat_interleave(td, 2).repeat_interleave(th, 3).repeat_interleave(tw, 4)[..., :D, :H, :W]
    aw = F.pad(w.double().abs(), (0, 0, 0, 0, 0, 0, 0, 8 * G - Cin)).view(Cout, G, 8, 27)
    wsum, wmax = aw.sum((2, 3)), aw.amax((2, 3))                                # (Cout, G)
    xsum = F.avg_pool3d(F.pad(ax.sum(2), (1, 1, 1, 1, 1, 1)), 3, 1) * 27         # (N, G, D, H, W): sum of |x| over the 27 taps
    mag = F.conv3d(x.double().abs(), w.double().abs(), padding=1)
    b = 2.0 ** -14 * (torch.einsum("og,ngdhw->nodhw", wsum, bmax) + torch.einsum("og,ngdhw->nodhw", wmax, xsum)) + 2.0 ** -21 * mag
    if sc is not None:
        b = b * sc.double().abs().view(1, -1, 1, 1, 1)
    return b
