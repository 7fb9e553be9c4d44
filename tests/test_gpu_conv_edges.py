"""The cost network's convolutions at their memory edges, called through the C ABI with every input and output inside a larger
guarded buffer (a "canvas"):

  * fp32 inputs are strided views inside a NaN canvas -- NaN in the row pitch, between planes, between channels and between views,
    one channel stride of NaN in front and two behind -- so a stray read a plausible addressing bug makes (channel Cin of a ragged
    last channel group, a halo voxel, the next row or view) lands in owned memory and shows up as NaN instead of being hidden by a
    zero weight or a masked lane;
  * SCL / PSCL inputs sit between NaN bf16 patterns;
  * every output (fp32, SCL, PSCL, statistics, split-K partial sums) sits between 1 MiB guards of a fixed bit pattern.

Per case: (a) every guard word unchanged, (b) SCL / PSCL borders still zero, (c) the bits of the same kernel on a clean contiguous
copy (through `mvsdet_amd.ops`), (d) finite and within the kernel's error bound of the float64 convolution.  Shapes from the tile
plans (bf_plan / bf_plan_tile, costreg_bf16.hip): each candidate tile, extents at 1, tile - 1 and tile + 1, channel counts that are
no multiple of 8."""
import ctypes

import pytest
import torch
import torch.nn.functional as F
from canvas import GUARD, SENTINEL, Guarded, guarded_f32, nan_view, ok, strides
from conv_bounds import mx_bound

pytestmark = pytest.mark.gpu

NAN_BF16 = 0x7FC1                     # guard half-word around SCL / PSCL inputs: a bf16 NaN


def guarded_scl(shape, dev, parity=False):
    from mvsdet_amd import ops
    nbytes, padded = (ops.pscl_geometry if parity else ops.scl_geometry)(*shape)
    g = Guarded(nbytes // 4, dev)
    cls = ops.PsclTensor if parity else ops.SclTensor
    return g, cls(g.region.view(torch.bfloat16), shape, padded)


def nan_framed_scl(t, dev):
    """An SCL / PSCL input copied between NaN bf16 guards (its own zero border kept)."""
    n = t.data.numel()
    canvas = torch.full((2 * GUARD + n + 8,), NAN_BF16, dtype=torch.int16, device=dev)
    region = canvas[2 * GUARD:2 * GUARD + n]
    region.copy_(t.data.view(torch.int16))
    return canvas, type(t)(region.view(torch.bfloat16), t.shape, t.padded)


def scl_bits(t):
    return t.data.view(torch.int16)


def variance_like(shape, g, mag=2.0):
    f = torch.randn((3,) + tuple(shape), generator=g)
    return ((f * f).mean(0) - f.mean(0) ** 2) * mag


def affine(Cout, g):
    return torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1


def ref_conv(x, w, sc=None, sh=None, relu=False, res=None, **kw):
    """float64 convolution [+ affine] [+ residual] [+ ReLU] and the summed |products| at the output (scaled like it)."""
    y = F.conv3d(x.double(), w.double(), **kw)
    mag = F.conv3d(x.double().abs(), w.double().abs(), **kw)
    if sc is not None:
        y = y * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1)
        mag = mag * sc.double().abs().view(1, -1, 1, 1, 1)
    if res is not None:
        y = y + res.double()
    return (y.clamp_min(0) if relu else y), mag


def plan_tile(D, H, W, f32in):
    """bf_plan_tile (costreg_bf16.hip): the candidate that pads (D, H, W) least, earlier candidates first at a tie."""
    best, bv = None, None
    for td, th, tw in ((4, 12, 16), (4, 8, 16), (6, 16, 8), (3, 16, 8), (8, 8, 8)):
        if td == 8 and not f32in:
            continue
        v = -(-D // td) * td * -(-H // th) * th * -(-W // tw) * tw
        if bv is None or v < bv:
            best, bv = (td, th, tw), v
    return best


# stride-1 shapes (N, Cin, Cout, D, H, W): every bf_plan_tile candidate, extents at 1 / tile - 1 / tile + 1, Cin in {1, 5, 8, 20, 65}
S1 = [(1, 1, 64, 1, 1, 1), (3, 5, 64, 4, 12, 16), (1, 20, 128, 5, 13, 17), (1, 65, 64, 3, 11, 15), (3, 8, 64, 4, 8, 16),
      (1, 20, 64, 6, 16, 8), (1, 5, 128, 7, 17, 9), (3, 65, 64, 3, 16, 8), (1, 1, 64, 8, 8, 8), (3, 20, 128, 9, 9, 9),
      (1, 8, 64, 7, 7, 7), (1, 5, 64, 2, 15, 17)]


def test_the_shapes_cover_the_tile_plans():
    tiles = {plan_tile(D, H, W, True) for _, _, _, D, H, W in S1}
    assert tiles == {(4, 12, 16), (4, 8, 16), (6, 16, 8), (3, 16, 8), (8, 8, 8)}
    for k in range(3):
        ext = {s[3 + k] for s in S1}
        assert 1 in ext
        for tile in {(4, 12, 16)[k], (4, 8, 16)[k], (6, 16, 8)[k], (8, 8, 8)[k]}:
            assert {tile - 1, tile + 1} <= ext | {0}, (k, tile)
    assert {s[1] for s in S1} == {1, 5, 8, 20, 65} and {s[0] for s in S1} == {1, 3} and {s[2] for s in S1} == {64, 128}


# ----------------------------------------------------------------------------------------------------- conv0 on fp16 + MX FP6
@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 1, 64, 1, 1, 1), (3, 5, 64, 4, 8, 16), (1, 20, 128, 3, 7, 15), (1, 65, 64, 5, 9, 17),
                                               (3, 8, 64, 4, 12, 16), (1, 20, 64, 5, 13, 17), (1, 5, 128, 2, 11, 33)])
def test_conv3d_k3_fp16mx_in_canvases(gpu, N, Cin, Cout, D, H, W):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(1000 * Cin + 10 * D + W)
    x = variance_like((N, Cin, D, H, W), g)
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
    sc, sh = affine(Cout, g)
    wq = ops.split_conv_weight_mx(w.to(gpu))
    _, xv = nan_view(x, gpu)
    was = _lib.get_option("conv_mx_th")
    try:
        for form in (0, 8, 12):
            _lib.set_option("conv_mx_th", form)
            use_affine, relu = form != 8, form != 12
            s, t = (sc.to(gpu), sh.to(gpu)) if use_affine else (None, None)
            gf, out = guarded_f32((N, Cout, D, H, W), gpu)
            gs, scl = guarded_scl((N, Cout, D, H, W), gpu)
            gp, pscl = guarded_scl((N, Cout, D, H, W), gpu, parity=True)
            ok(lib.mvsdet_conv3d_k3_fp16mx_f32in(_lib.ptr(xv), strides(xv), _lib.ptr(wq), _lib.ptr(s), _lib.ptr(t), _lib.ptr(out),
                                                 gs.ptr(), gp.ptr(), N, Cin, Cout, D, H, W, int(relu), _lib.current_stream(gpu)))
            assert gf.guards_intact() and gs.guards_intact() and gp.guards_intact(), form
            assert scl.border_is_zero() and pscl.pieces()[2], form
            c32, cscl, cpscl = ops.conv3d_k3_fp16mx(x.to(gpu), wq, s, t, relu, outputs=("f32", "scl", "pscl"))
            assert torch.equal(out, c32), form
            assert torch.equal(scl_bits(scl), scl_bits(cscl)) and torch.equal(scl_bits(pscl), scl_bits(cpscl)), form
            ref, _ = ref_conv(x, w, sc if use_affine else None, sh if use_affine else None, relu, padding=1)
            tile = (4, 12, 16) if form == 12 and -(-H // 12) * 12 < -(-H // 8) * 8 else (4, 8, 16)
            bound = mx_bound(x, w, sc if use_affine else None, N, Cin, Cout, D, H, W, tile) + 2.0 ** -23 * ref.abs()
            got = out.double().cpu()
            assert bool(torch.isfinite(got).all()), form
            assert bool(((got - ref).abs() <= bound).all()), (form, float(((got - ref).abs() / bound).max()))
            assert float((got - ref).abs().max()) <= 2.0 ** -14 * float(ref.abs().max()) + 1e-30, form   # test_gpu_mx's bound
    finally:
        _lib.set_option("conv_mx_th", was)


# ------------------------------------------------------------------------------------------------------------ bf16x3 stride 1
def b3_check(got, x, w, sc=None, sh=None, relu=False, res=None, **kw):
    """test_gpu_bf16's bound: within 3 * 2^-16 of the largest summed |products| of the float64 convolution."""
    ref, mag = ref_conv(x, w, sc, sh, relu, res, **kw)
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max())
    assert err <= 3 * 2.0 ** -16 * float(mag.max()) + 2.0 ** -22 * float(ref.abs().max()), err


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", S1)
def test_conv3d_k3_bf16x3_in_canvases(gpu, N, Cin, Cout, D, H, W):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(2000 * Cin + 10 * D + W)
    x = variance_like((N, Cin, D, H, W), g)
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
    sc, sh = affine(Cout, g)
    res = torch.randn((N, Cout, D, H, W), generator=g)
    scd, shd, resd = sc.to(gpu), sh.to(gpu), res.to(gpu)
    wq = ops.split_conv_weight(w.to(gpu))
    _, xv = nan_view(x, gpu)
    st = _lib.current_stream(gpu)
    shape = (N, Cout, D, H, W)

    # fp32 input in place, all three outputs, affine + residual + ReLU
    gf, out = guarded_f32(shape, gpu)
    gs, scl = guarded_scl(shape, gpu)
    gp, pscl = guarded_scl(shape, gpu, parity=True)
    ok(lib.mvsdet_conv3d_k3_bf16x3_io(None, _lib.ptr(xv), strides(xv), _lib.ptr(wq), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(resd),
                                      _lib.ptr(out), gs.ptr(), gp.ptr(), None, 0, N, Cin, Cout, D, H, W, 1, st))
    assert gf.guards_intact() and gs.guards_intact() and gp.guards_intact()
    assert scl.border_is_zero() and pscl.pieces()[2]
    c32, cscl, cpscl = ops.conv3d_k3_bf16x3(x.to(gpu), wq, scd, shd, True, resd, outputs=("f32", "scl", "pscl"))
    assert torch.equal(out, c32)
    assert torch.equal(scl_bits(scl), scl_bits(cscl)) and torch.equal(scl_bits(pscl), scl_bits(cpscl))
    b3_check(out, x, w, sc, sh, True, res, padding=1)

    # split over the input channels (fp32 output only): the partial sums in a guarded workspace
    wbytes = int(lib.mvsdet_conv3d_k3_bf16x3_workspace_bytes(N, Cin, Cout, D, H, W))
    gw = Guarded(max(wbytes, 4) // 4, gpu)
    gf2, out2 = guarded_f32(shape, gpu)
    ok(lib.mvsdet_conv3d_k3_bf16x3_io(None, _lib.ptr(xv), strides(xv), _lib.ptr(wq), None, None, None, _lib.ptr(out2), None, None, gw.ptr(),
                                      wbytes, N, Cin, Cout, D, H, W, 0, st))
    assert gf2.guards_intact() and gw.guards_intact()
    assert torch.equal(out2, ops.conv3d_k3_bf16x3(x.to(gpu), wq, None, None, False))
    b3_check(out2, x, w, padding=1)

    # the SCL input between NaN guards, residual, fp32 + SCL outputs
    _, xs = nan_framed_scl(ops.scl_pack(x.to(gpu)), gpu)
    gf3, out3 = guarded_f32(shape, gpu)
    gs3, scl3 = guarded_scl(shape, gpu)
    ok(lib.mvsdet_conv3d_k3_bf16x3_io(_lib.ptr(xs.data), None, None, _lib.ptr(wq), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(resd),
                                      _lib.ptr(out3), gs3.ptr(), None, None, 0, N, Cin, Cout, D, H, W, 1, st))
    assert gf3.guards_intact() and gs3.guards_intact() and scl3.border_is_zero()
    assert torch.equal(out3, c32) and torch.equal(scl_bits(scl3), scl_bits(cscl))   # both input forms: the same bits

    # statistics for a training BatchNorm: output and (Cout, parts) double2 sums guarded
    parts = int(lib.mvsdet_conv3d_k3_bf16x3_stats_parts(N, D, H, W, 1))
    gst = Guarded(Cout * parts * 4, gpu)
    gf4, out4 = guarded_f32(shape, gpu)
    pivot = (torch.randn(Cout, generator=g) * 0.1).to(gpu)
    ok(lib.mvsdet_conv3d_k3_bf16x3_stats(None, _lib.ptr(xv), strides(xv), _lib.ptr(wq), _lib.ptr(out4), gst.ptr(), Cout * parts * 16,
                                         _lib.ptr(pivot), N, Cin, Cout, D, H, W, st))
    assert gf4.guards_intact() and gst.guards_intact()
    c4, cst = ops.conv3d_k3_bf16x3_stats(x.to(gpu), wq, pivot)
    assert torch.equal(out4, c4) and torch.equal(gst.region.view(torch.float64).view(Cout, parts, 2), cst)
    b3_check(out4, x, w, padding=1)


# ------------------------------------------------------------------------------------------------- stride 2 and transposed
@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 5, 64, 2, 2, 2), (3, 20, 64, 8, 16, 32), (1, 65, 128, 9, 17, 33), (1, 8, 64, 7, 23, 15),
                                               (3, 1, 64, 1, 3, 5)])
def test_conv3d_k3_s2_bf16x3_in_canvases(gpu, N, Cin, Cout, D, H, W):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(3000 * Cin + 10 * D + W)
    x = variance_like((N, Cin, D, H, W), g)
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
    sc, sh = affine(Cout, g)
    scd, shd = sc.to(gpu), sh.to(gpu)
    wq = ops.split_conv_weight(w.to(gpu), 1)
    st = _lib.current_stream(gpu)
    oshape = (N, Cout, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2)
    _, xv = nan_view(x, gpu)
    gf, out = guarded_f32(oshape, gpu)
    gs, scl = guarded_scl(oshape, gpu)
    ok(lib.mvsdet_conv3d_k3_s2_bf16x3_io(_lib.ptr(xv), strides(xv), None, _lib.ptr(wq), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(out),
                                         gs.ptr(), None, 0, N, Cin, Cout, D, H, W, 1, st))
    assert gf.guards_intact() and gs.guards_intact() and scl.border_is_zero()
    c32, cscl = ops.conv3d_k3_s2_bf16x3(x.to(gpu), wq, scd, shd, True, outputs=("f32", "scl"))
    assert torch.equal(out, c32) and torch.equal(scl_bits(scl), scl_bits(cscl))
    b3_check(out, x, w, sc, sh, True, stride=2, padding=1)
    # the small-volume form split over the input channels: workspace guarded
    wbytes = int(lib.mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes(N, Cin, Cout, D, H, W))
    gw = Guarded(max(wbytes, 4) // 4, gpu)
    gf2, out2 = guarded_f32(oshape, gpu)
    ok(lib.mvsdet_conv3d_k3_s2_bf16x3_io(_lib.ptr(xv), strides(xv), None, _lib.ptr(wq), None, None, _lib.ptr(out2), None, gw.ptr(),
                                         wbytes, N, Cin, Cout, D, H, W, 0, st))
    assert gf2.guards_intact() and gw.guards_intact()
    assert torch.equal(out2, ops.conv3d_k3_s2_bf16x3(x.to(gpu), wq, None, None, False))
    # the PSCL input between NaN guards
    _, xp = nan_framed_scl(ops.pscl_from_tensor(x.to(gpu)), gpu)
    gf3, out3 = guarded_f32(oshape, gpu)
    ok(lib.mvsdet_conv3d_k3_s2_bf16x3_io(None, None, _lib.ptr(xp.data), _lib.ptr(wq), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(out3),
                                         None, None, 0, N, Cin, Cout, D, H, W, 1, st))
    assert gf3.guards_intact()
    xp_clean = ops.pscl_from_tensor(x.to(gpu))
    clean3 = torch.empty_like(out3)
    ok(lib.mvsdet_conv3d_k3_s2_bf16x3_io(None, None, _lib.ptr(xp_clean.data), _lib.ptr(wq), _lib.ptr(scd), _lib.ptr(shd),
                                         _lib.ptr(clean3), None, None, 0, N, Cin, Cout, D, H, W, 1, st))
    assert torch.equal(out3, clean3)
    b3_check(out3, x, w, sc, sh, True, stride=2, padding=1)


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 8, 64, 1, 1, 1), (3, 64, 64, 2, 4, 8), (1, 128, 128, 3, 5, 9), (1, 256, 128, 3, 15, 20)])
def test_convT3d_k3_s2_bf16x3_in_canvases(gpu, N, Cin, Cout, D, H, W):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(4000 * Cin + 10 * D + W)
    x = torch.randn((N, Cin, D, H, W), generator=g)
    w = torch.randn((Cin, Cout, 3, 3, 3), generator=g) / (27 * Cin / 8) ** 0.5
    sc, sh = affine(Cout, g)
    scd, shd = sc.to(gpu), sh.to(gpu)
    oshape = (N, Cout, 2 * D, 2 * H, 2 * W)
    res = torch.randn(oshape, generator=g)
    resd = res.to(gpu)
    wq = ops.split_conv_weight(w.to(gpu), 2)
    _, xs = nan_framed_scl(ops.scl_pack(x.to(gpu)), gpu)
    gf, out = guarded_f32(oshape, gpu)
    gs, scl = guarded_scl(oshape, gpu)
    ok(lib.mvsdet_convT3d_k3_s2_bf16x3_io(_lib.ptr(xs.data), _lib.ptr(wq), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(resd), _lib.ptr(out),
                                          gs.ptr(), N, Cin, Cout, D, H, W, 1, _lib.current_stream(gpu)))
    assert gf.guards_intact() and gs.guards_intact() and scl.border_is_zero()
    c32, cscl = ops.convT3d_k3_s2_bf16x3(ops.scl_pack(x.to(gpu)), wq, scd, shd, resd, True, outputs=("f32", "scl"))
    assert torch.equal(out, c32) and torch.equal(scl_bits(scl), scl_bits(cscl))
    ref = F.conv_transpose3d(x.double(), w.double(), stride=2, padding=1, output_padding=1)
    mag = F.conv_transpose3d(x.double().abs(), w.double().abs(), stride=2, padding=1, output_padding=1)
    ref = res.double() + torch.relu(ref * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))   # the skip added last
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all())
    assert float((got - ref).abs().max()) <= 3 * 2.0 ** -16 * float((mag * sc.double().view(1, -1, 1, 1, 1)).max()) + 2.0 ** -22 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------------------- packing, head
@pytest.mark.parametrize("zero_border", [0, 1])
@pytest.mark.parametrize("N,C,D,H,W", [(1, 1, 1, 1, 1), (3, 13, 5, 7, 19), (1, 65, 4, 13, 17)])
def test_scl_pack_in_canvases(gpu, N, C, D, H, W, zero_border):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(5000 + C * 10 + W)
    x = torch.randn((N, C, D, H, W), generator=g) * 3.0
    _, xv = nan_view(x, gpu)
    gs, scl = guarded_scl((N, C, D, H, W), gpu)
    if zero_border == 1:
        gs.region.fill_(-1)                                   # the call clears the whole buffer itself
    ok(lib.mvsdet_scl_pack_f32(_lib.ptr(xv), strides(xv), gs.ptr(), N, C, D, H, W, zero_border, _lib.current_stream(gpu)))
    assert gs.guards_intact() and scl.border_is_zero()
    clean = ops.scl_pack(x.to(gpu))
    assert torch.equal(scl_bits(scl), scl_bits(clean))
    hi, mid = scl.pieces()
    eh, em = ops.split_bf16(x)
    assert torch.equal(hi[:, :C].cpu(), eh) and torch.equal(mid[:, :C].cpu(), em)
    assert not bool(hi[:, C:].view(torch.int16).any())


@pytest.mark.parametrize("N,Cin,D,H,W", [(1, 1, 1, 1, 4), (3, 64, 4, 12, 16), (1, 20, 5, 13, 20)])   # a second input: W % 4 == 0
def test_head_cout2_sum_in_canvases(gpu, N, Cin, D, H, W):
    from mvsdet_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(6000 + Cin + W)
    x, x2 = torch.randn((N, Cin, D, H, W), generator=g), torch.randn((N, Cin, D, H, W), generator=g)
    w, b = torch.randn((2, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5, torch.randn(2, generator=g)
    cx, cx2 = torch.full((2 * GUARD + x.numel(),), float("nan"), device=gpu), torch.full((2 * GUARD + x.numel(),), float("nan"), device=gpu)
    xv, x2v = cx[GUARD:GUARD + x.numel()].view(x.shape), cx2[GUARD:GUARD + x.numel()].view(x.shape)
    xv.copy_(x.to(gpu))
    x2v.copy_(x2.to(gpu))
    wd, bd = w.to(gpu), b.to(gpu)
    gf, out = guarded_f32((N, 2, D, H, W), gpu)
    ok(lib.mvsdet_conv3d_k3_cout2_sum_f32(_lib.ptr(xv), _lib.ptr(x2v), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out), N, Cin, D, H, W,
                                          _lib.current_stream(gpu)))
    assert gf.guards_intact()
    clean = torch.empty_like(out)
    xd, x2d = x.to(gpu), x2.to(gpu)
    ok(lib.mvsdet_conv3d_k3_cout2_sum_f32(_lib.ptr(xd), _lib.ptr(x2d), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(clean), N, Cin, D, H, W,
                                          _lib.current_stream(gpu)))
    assert torch.equal(out, clean)
    ref = F.conv3d((x + x2).double(), w.double(), b.double(), padding=1)
    mag = F.conv3d((x + x2).double().abs(), w.double().abs(), padding=1) + b.double().abs().view(1, -1, 1, 1, 1)
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= 1e-5 * mag + 1e-6).all())


def test_split_k_forms_are_exercised():
    """The workspace (split over the input channels) cases above really split for some shapes: their guards check something."""
    from mvsdet_amd import _lib
    lib = _lib.load()
    assert [s for s in S1 if lib.mvsdet_conv3d_k3_bf16x3_workspace_bytes(*s) > 0] == [(1, 65, 64, 3, 11, 15), (3, 65, 64, 3, 16, 8)]
    assert lib.mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes(1, 65, 128, 9, 17, 33) > 0


def test_fp16mx_channels_interleaved_with_planes(gpu):
    """An (N,D,C,H,W) tensor seen as NCDHW: its channel stride is smaller than a channel volume, so the kernel's pad channel Cin
    (Cin % 8 != 0) would be real data of the view -- the next plane's channel 0, here NaN next to a plane of finite values.
    mvsdet_conv3d_k3_fp16mx_ok refuses such a view, the raw entry point returns an error and ops.conv3d_k3_fp16mx runs it on the
    bf16x3 kernel: the bits of bf16x3 on a contiguous copy, finite outside the NaN's receptive field.  With Cin % 8 == 0 (no pad
    channel) the fp16 + MX kernel takes the view and gives the contiguous copy's bits."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(41)
    for Cin in (5, 8):
        N, Cout, D, H, W = 2, 64, 6, 9, 17
        x = variance_like((N, Cin, D, H, W), g)
        x[1, 0, 3, 4, 8] = float("nan")
        w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
        xv = x.permute(0, 2, 1, 3, 4).contiguous().to(gpu).permute(0, 2, 1, 3, 4)       # (N,D,C,H,W) storage
        assert xv.stride(1) == H * W < (D - 1) * xv.stride(2)
        wd = w.to(gpu)
        wq = ops.split_conv_weight_mx(wd)
        out = torch.empty((N, Cout, D, H, W), device=gpu)
        rc = lib.mvsdet_conv3d_k3_fp16mx_f32in(_lib.ptr(xv), strides(xv), _lib.ptr(wq), None, None, _lib.ptr(out), None, None, N, Cin,
                                               Cout, D, H, W, 0, _lib.current_stream(gpu))
        torch.cuda.synchronize()
        got = ops.conv3d_k3_fp16mx(xv, wq, None, None, False, weight=wd)
        if Cin % 8:
            assert rc == 1 and not ops.conv3d_k3_fp16mx_ok(xv)
            want = ops.conv3d_k3_bf16x3(x.to(gpu), ops.split_conv_weight(wd), None, None, False)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))                 # NaN included: bits
        else:
            assert rc == 0 and ops.conv3d_k3_fp16mx_ok(xv)
            clean = ops.conv3d_k3_fp16mx(x.to(gpu), wq, None, None, False)
            assert torch.equal(out.view(torch.int32), clean.view(torch.int32)) and torch.equal(got.view(torch.int32), clean.view(torch.int32))
        field = torch.zeros((N, Cout, D, H, W), dtype=torch.bool)
        field[1, :, 2:5, 3:6, 7:10] = True
        assert bool(torch.isfinite(got.cpu()[~field]).all()) and not bool(torch.isfinite(got.cpu()[field]).any())


# ------------------------------------------------------------------------------------ weight gradients, head backward, BatchNorm
def nan_framed(t, dev):
    """A contiguous fp32 tensor between 1 MiB NaN guards (16-byte aligned)."""
    canvas = torch.full((2 * GUARD + t.numel(),), float("nan"), dtype=torch.float32, device=dev)
    v = canvas[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t.to(dev))
    return canvas, v


@pytest.mark.parametrize("stride,N,Cin,Cout,D,H,W,nsplit", [(1, 2, 5, 64, 3, 7, 16, 4), (1, 1, 65, 128, 4, 9, 20, 7), (1, 3, 8, 70, 1, 1, 4, 1),
                                                            (2, 1, 20, 64, 4, 6, 16, 3), (2, 3, 65, 128, 2, 10, 24, 8), (2, 1, 8, 3, 2, 2, 8, 1)])
def test_conv3d_k3_dw_bf16x3_in_canvases(gpu, stride, N, Cin, Cout, D, H, W, nsplit):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(7000 + 100 * stride + Cin + W)
    x = torch.randn((N, Cin, D, H, W), generator=g)
    gy = torch.randn((N, Cout, D // stride, H // stride, W // stride), generator=g)
    _, xf = nan_framed(x, gpu)
    _, gyf = nan_framed(gy, gpu)
    pbytes = int(lib.mvsdet_conv3d_k3_dw_partial_bytes(Cin, Cout, nsplit))
    gp = Guarded(pbytes // 4, gpu)
    fn = lib.mvsdet_conv3d_k3_dw_bf16x3 if stride == 1 else lib.mvsdet_conv3d_k3_s2_dw_bf16x3
    ok(fn(_lib.ptr(xf), _lib.ptr(gyf), gp.ptr(), pbytes, nsplit, N, Cin, Cout, D, H, W, _lib.current_stream(gpu)))
    assert gp.guards_intact()
    got = gp.region.view(torch.float32).view(nsplit, Cout, Cin, 27).sum(0).view(Cout, Cin, 3, 3, 3)
    assert torch.equal(got, ops.conv3d_k3_dw(x.to(gpu), gy.to(gpu), nsplit, stride, True))
    full = torch.nn.grad.conv3d_weight(x.double(), (Cout, Cin, 3, 3, 3), gy.double(), stride=stride, padding=1)
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    assert float((got - full).abs().max()) <= 1e-4 * float(full.abs().max())          # test_gpu_bf16's bound


@pytest.mark.parametrize("N,Cin,D,H,W,nsplit", [(1, 16, 1, 1, 4, 1), (2, 32, 3, 7, 20, 5), (1, 64, 4, 9, 16, 12)])
def test_head_backward_in_canvases(gpu, N, Cin, D, H, W, nsplit):
    """The head's input gradient (fp32) and weight gradient (bf16x3, partial sums guarded)."""
    from mvsdet_amd import _lib
    lib = _lib.load()
    st = _lib.current_stream(gpu)
    g = torch.Generator().manual_seed(8000 + Cin + W)
    x, gy = torch.randn((N, Cin, D, H, W), generator=g), torch.randn((N, 2, D, H, W), generator=g)
    w = torch.randn((2, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
    _, xf = nan_framed(x, gpu)
    _, gyf = nan_framed(gy, gpu)
    _, wf = nan_framed(w, gpu)
    gx_g, gx = guarded_f32((N, Cin, D, H, W), gpu)
    ok(lib.mvsdet_conv3d_k3_cout2_dx_f32(_lib.ptr(gyf), _lib.ptr(wf), _lib.ptr(gx), N, Cin, D, H, W, st))
    assert gx_g.guards_intact()
    xd, gyd, wd = x.to(gpu), gy.to(gpu), w.to(gpu)
    clean = torch.empty((N, Cin, D, H, W), device=gpu)
    ok(lib.mvsdet_conv3d_k3_cout2_dx_f32(_lib.ptr(gyd), _lib.ptr(wd), _lib.ptr(clean), N, Cin, D, H, W, st))
    assert torch.equal(gx, clean)
    ref = F.conv_transpose3d(gy.double(), w.double(), padding=1)
    mag = F.conv_transpose3d(gy.double().abs(), w.double().abs(), padding=1)
    got = gx.double().cpu()
    assert bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= 1e-5 * mag + 1e-7).all())
    assert lib.mvsdet_conv3d_k3_cout2_dw_bf16x3_ok(Cin, W) == 1
    pbytes = nsplit * 2 * Cin * 27 * 4
    gp = Guarded(pbytes // 4, gpu)
    ok(lib.mvsdet_conv3d_k3_cout2_dw_bf16x3(_lib.ptr(xf), _lib.ptr(gyf), gp.ptr(), pbytes, nsplit, N, Cin, D, H, W, st))
    assert gp.guards_intact()
    part = torch.empty((nsplit, 2, Cin, 27), device=gpu)
    ok(lib.mvsdet_conv3d_k3_cout2_dw_bf16x3(_lib.ptr(xd), _lib.ptr(gyd), _lib.ptr(part), pbytes, nsplit, N, Cin, D, H, W, st))
    assert torch.equal(gp.region.view(torch.float32).view(nsplit, 2, Cin, 27), part)
    full = torch.nn.grad.conv3d_weight(x.double(), (2, Cin, 3, 3, 3), gy.double(), padding=1)
    got = part.sum(0).view(2, Cin, 3, 3, 3).double().cpu()
    assert float((got - full).abs().max()) <= 1e-4 * float(full.abs().max())


@pytest.mark.parametrize("N,C,D,H,W,relu", [(1, 1, 1, 1, 2, 1), (3, 64, 4, 6, 10, 1), (2, 5, 3, 7, 9, 0)])
def test_bn3d_train_in_canvases(gpu, N, C, D, H, W, relu):
    """Training BatchNorm forward and backward: every output vector, the running statistics and the workspace guarded."""
    from mvsdet_amd import _lib
    lib = _lib.load()
    st = _lib.current_stream(gpu)
    g = torch.Generator().manual_seed(9000 + C + W)
    x = torch.randn((N, C, D, H, W), generator=g) * 3 + 1
    gy = torch.randn((N, C, D, H, W), generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    vol, eps, mom = D * H * W, 1e-5, 0.1
    wb = int(lib.mvsdet_bn3d_workspace_bytes(C))

    def run(xp, gyp, gam, bet, outs):
        ok(lib.mvsdet_bn3d_relu_train_fwd_res_f32(_lib.ptr(xp), _lib.ptr(gam), _lib.ptr(bet), None, outs["rm"], outs["rv"], outs["out"],
                                                  outs["mean"], outs["invstd"], outs["ws"], wb, N, C, vol, ctypes.c_float(mom),
                                                  ctypes.c_float(eps), relu, st))
        ok(lib.mvsdet_bn3d_relu_bwd_f32(_lib.ptr(xp), _lib.ptr(gyp), _lib.ptr(gam), _lib.ptr(bet), outs["mean"], outs["invstd"], outs["gx"],
                                        outs["gg"], outs["gb"], outs["ws"], wb, N, C, vol, relu, st))

    sizes = {"rm": C, "rv": C, "out": x.numel(), "mean": C, "invstd": C, "gx": x.numel(), "gg": C, "gb": C, "ws": max(wb, 4) // 4}
    guarded = {k: Guarded(n, gpu) for k, n in sizes.items()}
    guarded["rv"].region.view(torch.float32).fill_(1.0)
    _, xf = nan_framed(x, gpu)
    _, gyf = nan_framed(gy, gpu)
    _, gf = nan_framed(gamma, gpu)
    _, bf = nan_framed(beta, gpu)
    run(xf, gyf, gf, bf, {k: v.ptr() for k, v in guarded.items()})
    assert all(v.guards_intact() for v in guarded.values()), [k for k, v in guarded.items() if not v.guards_intact()]
    clean = {k: torch.zeros(n, dtype=torch.float32, device=gpu) for k, n in sizes.items()}
    clean["rv"].fill_(1.0)
    xd, gyd, gd, bd = x.to(gpu), gy.to(gpu), gamma.to(gpu), beta.to(gpu)
    run(xd, gyd, gd, bd, {k: _lib.ptr(v) for k, v in clean.items()})
    for k in ("rm", "rv", "out", "mean", "invstd", "gx", "gg", "gb"):
        assert torch.equal(guarded[k].region.view(torch.float32), clean[k]), k
    # float64: batch statistics (biased variance), affine, ReLU, and autograd's gradients
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.batch_norm(xr, None, None, gr, br, training=True, eps=eps)
    y = y.clamp_min(0) if relu else y
    y.backward(gy.double())
    out = clean["out"].view(x.shape).double().cpu()
    assert bool(torch.isfinite(out).all()) and float((out - y.detach()).abs().max()) <= 1e-5 * max(1.0, float(y.detach().abs().max()))
    gx = clean["gx"].view(x.shape).double().cpu()
    assert float((gx - xr.grad).abs().max()) <= 1e-4 * max(1.0, float(xr.grad.abs().max()))
    assert float((clean["gg"].double().cpu() - gr.grad).abs().max()) <= 1e-4 * max(1.0, float(gr.grad.abs().max()))
    assert float((clean["gb"].double().cpu() - br.grad).abs().max()) <= 1e-4 * max(1.0, float(br.grad.abs().max()))


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 32, 128, 2, 2, 2), (3, 64, 256, 4, 6, 10), (1, 96, 128, 6, 2, 14)])
def test_neck_gemm_layers_in_canvases(gpu, N, Cin, Cout, D, H, W):
    """The neck's GEMM-shaped layers: Conv3d(kernel 1, stride 2) + bias and ConvTranspose3d(kernel 2, stride 2) + bias + ReLU."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    st = _lib.current_stream(gpu)
    g = torch.Generator().manual_seed(9500 + Cin + W)
    x = torch.randn((N, Cin, D, H, W), generator=g)
    w1 = torch.randn((Cout, Cin), generator=g) / Cin ** 0.5
    b1 = torch.randn(Cout, generator=g) * 0.1
    wt = torch.randn((Cin, Cout, 2, 2, 2), generator=g) / Cin ** 0.5
    bt = torch.randn(Cout, generator=g) * 0.1
    _, xf = nan_framed(x, gpu)
    xd, b1d, btd = x.to(gpu), b1.to(gpu), bt.to(gpu)
    wq1 = ops.gemm_split_weight(w1.to(gpu))
    wqt = ops.gemm_split_weight(wt.permute(1, 2, 3, 4, 0).reshape(8 * Cout, Cin).to(gpu))     # rows 8 o + 4 p + 2 q + r
    go, out = guarded_f32((N, Cout, D // 2, H // 2, W // 2), gpu)
    ok(lib.mvsdet_conv3d_k1_s2_bf16x3(_lib.ptr(xf), _lib.ptr(wq1), _lib.ptr(b1d), _lib.ptr(out), N, Cin, Cout, D, H, W, 0, st))
    assert go.guards_intact()
    assert torch.equal(out, ops.conv3d_k1_s2_bf16x3(xd, wq1, b1d, Cout))
    ref = F.conv3d(x.double(), w1.double().view(Cout, Cin, 1, 1, 1), b1.double(), stride=2)
    mag = F.conv3d(x.double().abs(), w1.double().abs().view(Cout, Cin, 1, 1, 1), stride=2) + b1.double().abs().view(1, -1, 1, 1, 1)
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all()) and float((got - ref).abs().max()) <= 3 * 2.0 ** -16 * float(mag.max())
    gt, outt = guarded_f32((N, Cout, 2 * D, 2 * H, 2 * W), gpu)
    ok(lib.mvsdet_convT3d_k2_s2_bf16x3(_lib.ptr(xf), _lib.ptr(wqt), _lib.ptr(btd), _lib.ptr(outt), N, Cin, Cout, D, H, W, 1, st))
    assert gt.guards_intact()
    assert torch.equal(outt, ops.convT3d_k2_s2_bf16x3(xd, wqt, btd, Cout, True))
    ref = torch.relu(F.conv_transpose3d(x.double(), wt.double(), bt.double(), stride=2))
    mag = F.conv_transpose3d(x.double().abs(), wt.double().abs(), stride=2) + bt.double().abs().view(1, -1, 1, 1, 1)
    got = outt.double().cpu()
    assert bool(torch.isfinite(got).all()) and float((got - ref).abs().max()) <= 3 * 2.0 ** -16 * float(mag.max())
