"""The cost network's convolutions on the bf16 matrix cores with three-term split operands (csrc/costreg_bf16.hip,
SURVEY 8 f-1): the kernels against a float64 evaluation of the SAME three products (so the check is independent of the
split's own truncation: what remains is fp32 accumulation order), and against the plain fp32 convolution within the
truncation the scheme promises (~2^-16 of the products' size).  Reference layers: mvs_models/mvsnet.py:76-82."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def three_term_conv64(x, w, **kw):
    """float64 convolution of the pieces the kernel multiplies: x_hi*w_hi + x_hi*w_mid + x_mid*w_hi."""
    from mvsdet_amd.ops import split_bf16
    xh, xm = (t.double() for t in split_bf16(x))
    wh, wm = (t.double() for t in split_bf16(w))
    return F.conv3d(xh, wh, **kw) + F.conv3d(xh, wm, **kw) + F.conv3d(xm, wh, **kw)


def test_scl_pack_pieces_and_border(gpu):
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 13, 5, 7, 19, generator=g) * 3.0
    x[0, 0, 0, 0, 0] = 0.0
    x[1, 12, 4, 6, 18] = -1e-30
    s = ops.scl_pack(x.to(gpu))
    hi, mid = s.pieces()
    eh, em = ops.split_bf16(x)
    assert torch.equal(hi[:, :13].cpu(), eh) and torch.equal(mid[:, :13].cpu(), em)
    assert float(hi[:, 13:].abs().max()) == 0.0                       # channels beyond C
    n, c, d, h, w = s.shape
    dp, hp, wp = s.padded
    full = s.data.view(2, n, 2, dp, hp, wp, 8).float()
    inner = torch.zeros_like(full, dtype=torch.bool)
    inner[:, :, :, 1:d + 1, 1:h + 1, 1:w + 1] = True
    assert float(full[~inner].abs().max()) == 0.0                     # the zero border
    # refill of the same buffer with other values: border still zero, interior replaced
    s2 = ops.scl_pack((x * 0.5).to(gpu), out=s)
    assert s2 is s and torch.equal(s.pieces()[0][:, :13].cpu(), ops.split_bf16(x * 0.5)[0])
    assert float(s.data.view(2, n, 2, dp, hp, wp, 8).float()[~inner].abs().max()) == 0.0


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 16, 64, 4, 8, 16), (2, 24, 64, 5, 13, 21), (1, 8, 128, 3, 12, 16),
                                               (1, 37, 64, 9, 25, 33), (2, 64, 64, 12, 60, 80), (1, 256, 64, 4, 12, 16),
                                               (1, 5, 64, 1, 1, 1),
                                               # the fp32-input form on its other tiles: 3x16x8 (half / quarter resolution of the
                                               # cost network), 8x8x8 (the neck's 40x40x16-like and 20x20x8 volumes)
                                               (1, 24, 64, 6, 30, 40), (1, 16, 64, 3, 15, 20), (1, 16, 64, 16, 40, 40),
                                               (1, 40, 128, 8, 20, 20)])
def test_conv3d_k3_bf16x3(gpu, N, Cin, Cout, D, H, W):
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g).abs() * 2.0        # variance-like, >= 0
    wgt = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(N, Cout, D, H, W, generator=g)
    xs = ops.scl_pack(x.to(gpu))
    wq = ops.split_conv_weight(wgt.to(gpu))                           # the device kernel ...
    assert torch.equal(wq.cpu().view(torch.int16), ops.split_conv_weight(wgt).view(torch.int16))   # ... == the torch-op layout
    raw = ops.conv3d_k3_bf16x3(xs, wq, None, None, False).cpu()
    direct = ops.conv3d_k3_bf16x3(x.to(gpu), wq, None, None, False).cpu()            # the fp32 tensor itself, cut in the kernel
    assert torch.equal(direct, raw)
    want = three_term_conv64(x, wgt, padding=1)
    mag = float(F.conv3d(x.abs().double(), wgt.abs().double(), padding=1).max())     # size of the summed products
    assert float((raw.double() - want).abs().max()) <= 4e-7 * mag                     # fp32 accumulation of exact products
    ref32 = F.conv3d(x.double(), wgt.double(), padding=1)
    assert float((raw.double() - ref32).abs().max()) <= 3 * 2.0 ** -16 * mag          # the dropped terms, worst case
    # observed truncation is far below the bound: random signs average the dropped terms down
    assert float((raw.double() - ref32).abs().max()) <= 2e-5 * float(ref32.abs().max()) + 1e-6
    full = ops.conv3d_k3_bf16x3(xs, wq, scale.to(gpu), shift.to(gpu), True, res.to(gpu)).cpu()
    pitched = torch.zeros(N, Cin, D, H, W + 11, device=gpu)
    pitched[..., :W] = x.to(gpu)                                                    # a row-pitched input view, read in place
    assert torch.equal(ops.conv3d_k3_bf16x3(pitched[..., :W], wq, scale.to(gpu), shift.to(gpu), True, res.to(gpu)).cpu(), full)
    wantf = torch.relu(torch.addcmul(shift.view(1, -1, 1, 1, 1), raw, scale.view(1, -1, 1, 1, 1)) + res)
    np.testing.assert_allclose(full.numpy(), wantf.numpy(), rtol=0, atol=2e-6 * max(1.0, float(wantf.abs().max())))
    # the layer-to-layer forms: the same values, already cut into the pieces a consumer would cut (bit for bit), nothing
    # written outside the interior of the SCL / PSCL buffers -- from either input form, alone or together with the fp32 tensor
    # (a small grid's fp32-only call is split over the input channels -- other partial sums -- the multi-output call never is)
    from mvsdet_amd import _lib
    was_split = _lib.load().mvsdet_conv3d_k3_bf16x3_workspace_bytes(N, Cin, Cout, D, H, W) > 0
    for inp in (xs, x.to(gpu)):
        f32, scl, pscl = ops.conv3d_k3_bf16x3(inp, wq, scale.to(gpu), shift.to(gpu), True, res.to(gpu), outputs=("f32", "scl", "pscl"))
        if was_split:
            np.testing.assert_allclose(f32.cpu().numpy(), full.numpy(), rtol=0, atol=4e-7 * mag * float(scale.max()))
        else:
            assert torch.equal(f32.cpu(), full)
        eh, em = ops.split_bf16(f32.cpu())
        hi, mid = scl.pieces()
        assert torch.equal(hi.cpu(), eh) and torch.equal(mid.cpu(), em) and scl.border_is_zero()
        hi, mid, clean = pscl.pieces()
        assert torch.equal(hi.cpu(), eh) and torch.equal(mid.cpu(), em) and clean
    only = ops.conv3d_k3_bf16x3(xs, wq, scale.to(gpu), shift.to(gpu), True, res.to(gpu), outputs="scl", scl_out=scl)
    assert only is scl and torch.equal(scl.pieces()[0].cpu(), eh) and scl.border_is_zero()
    # ... and a stride-1 consumer of the SCL output sees what it would have cut from the fp32 tensor
    if Cout == 64 and Cin <= 64:
        w2 = ops.split_conv_weight((torch.randn(64, 64, 3, 3, 3, generator=g) / 40).to(gpu))
        assert torch.equal(ops.conv3d_k3_bf16x3(scl, w2, None, None, False), ops.conv3d_k3_bf16x3(f32, w2, None, None, False))


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(2, 64, 64, 12, 60, 80), (3, 24, 128, 6, 30, 40), (2, 16, 64, 3, 15, 20), (1, 16, 64, 16, 40, 40),
                                               (2, 8, 64, 5, 13, 21), (1, 5, 64, 1, 1, 2)])
def test_conv3d_k3_bf16x3_statistics_for_the_batchnorm_behind_it(gpu, N, Cin, Cout, D, H, W):
    """module.py:26-37 under model.train(): the convolution's epilogue leaves per-channel partial sums of its outputs and of their
    squares (one float64 pair per channel and block) and the BatchNorm finishes them instead of reading the tensor for its
    statistics.  The output tensor is the plain call's bit for bit; the sums are those of that tensor (float64, 1e-6 relative to the
    sum of magnitudes); BatchNorm + ReLU [+ residual] from the partial sums agree with the two-pass operator; the same bits on a
    second run (fixed summation order); a channel far from zero mean keeps its variance when the sums are taken around a pivot
    near its mean (the BatchNorm's running mean in the network)."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 100 + Cin + D)
    x = (torch.randn(N, Cin, D, H, W, generator=g).abs() * 2.0).to(gpu)
    wgt = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    wgt[1] = wgt[1].abs() * 20.0          # a channel whose mean is many times its spread
    wq = ops.split_conv_weight(wgt.to(gpu))
    from mvsdet_amd import _lib
    plain = ops.conv3d_k3_bf16x3(x, wq, None, None, False)
    y, parts = ops.conv3d_k3_bf16x3_stats(x, wq)
    if _lib.load().mvsdet_conv3d_k3_bf16x3_workspace_bytes(N, Cin, Cout, D, H, W) > 0:
        # a small grid's plain call is split over the input channels (other partial sums); the statistics form never is
        assert float((y - plain).abs().max()) <= 4e-6 * float(plain.abs().max())
    else:
        assert torch.equal(y, plain)
    assert parts.dtype == torch.float64 and parts.shape[0] == Cout and parts.shape[2] == 2
    plain = y
    y64 = plain.double()
    # a pivot that is near every channel's mean but not equal to it (the running mean of a BatchNorm a few steps into training)
    pivot = (y64.mean(dim=(0, 2, 3, 4)) * 0.97).float()
    y2, parts2 = ops.conv3d_k3_bf16x3_stats(ops.scl_pack(x), wq, pivot)      # the SCL input form: another tile plan; sums around the pivot
    assert torch.equal(y2, y)
    for pt, pv in ((parts, None), (parts2, pivot)):
        d64 = y64 if pv is None else y64 - pv.double().view(1, -1, 1, 1, 1)
        s, q = pt[:, :, 0].sum(1), pt[:, :, 1].sum(1)
        np.testing.assert_allclose(s.cpu().numpy(), d64.sum(dim=(0, 2, 3, 4)).cpu().numpy(), rtol=0,
                                   atol=1e-6 * float(d64.abs().sum(dim=(0, 2, 3, 4)).max()))
        np.testing.assert_allclose(q.cpu().numpy(), (d64 * d64).sum(dim=(0, 2, 3, 4)).cpu().numpy(), rtol=1e-6)
    assert torch.equal(ops.conv3d_k3_bf16x3_stats(x, wq)[1], parts)   # a fixed summation order
    parts = parts2
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(gpu), (torch.randn(Cout, generator=g) * 0.1).to(gpu)
    res = torch.randn(N, Cout, D, H, W, generator=g).to(gpu)
    for residual in (None, res):
        two = ops.bn3d_relu_train(plain, gamma, beta, 1e-5, True, residual)
        one = ops.bn3d_relu_train(plain, gamma, beta, 1e-5, True, residual, parts, pivot)
        m64 = y64.mean(dim=(0, 2, 3, 4))
        v64 = y64.var(dim=(0, 2, 3, 4), unbiased=False)
        np.testing.assert_allclose(one[1].cpu().numpy(), m64.cpu().numpy(), rtol=1e-6, atol=1e-7 * float(y64.abs().max()))
        np.testing.assert_allclose(one[2].cpu().numpy(), (1.0 / torch.sqrt(v64 + 1e-5)).cpu().numpy(), rtol=2e-6)
        np.testing.assert_allclose(one[2].cpu().numpy(), two[2].cpu().numpy(), rtol=2e-5)
        scale = float((two[0].abs().max()).cpu())
        assert float((one[0] - two[0]).abs().max()) <= 2e-5 * max(1.0, scale)
    # autograd through the partial-sums form: the same backward as the two-pass operator's
    xa, xb = plain.clone().requires_grad_(True), plain.clone().requires_grad_(True)
    ops.bn3d_relu_train(xa, gamma, beta, 1e-5, True, None, parts, pivot)[0].square().mean().backward()
    ops.bn3d_relu_train(xb, gamma, beta, 1e-5, True, None)[0].square().mean().backward()
    assert float((xa.grad - xb.grad).abs().max()) <= 1e-4 * float(xb.grad.abs().max()) + 1e-12


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(2, 128, 64, 6, 30, 40), (3, 64, 128, 3, 15, 20), (1, 16, 64, 5, 13, 7)])
def test_convT3d_k3_s2_bf16x3_statistics_for_the_batchnorm_behind_it(gpu, N, Cin, Cout, D, H, W):
    """mvsnet.py:92-100 under model.train(): the transposed layer's epilogue leaves the partial sums of its BatchNorm's statistics
    (a lane's running sums in LDS slots of its own, added up in a fixed order); same output bits as the plain call, sums of the
    tensor it wrote, the BatchNorm + ReLU + skip from them agrees with the two-pass operator, the same bits on a second run."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 10 + D)
    x = torch.randn(N, Cin, D, H, W, generator=g).to(gpu)
    wq = ops.split_conv_weight((torch.randn(Cin, Cout, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5 * 3.0).to(gpu), 2)
    plain = ops.convT3d_k3_s2_bf16x3(x, wq, None, None, None, False)
    y64 = plain.double()
    pivot = (y64.mean(dim=(0, 2, 3, 4)) * 0.9 + 0.01).float()
    got = ops.convT3d_k3_s2_bf16x3_stats(x, wq, pivot)
    if got is None:      # shapes whose tiles are not 3 x 16 x 8 keep the separate statistics pass
        from mvsdet_amd import _lib
        assert _lib.load().mvsdet_convT3d_k3_s2_bf16x3_stats_parts(N, D, H, W) == 0
        return
    y, parts = got
    assert torch.equal(y, plain)
    d64 = y64 - pivot.double().view(1, -1, 1, 1, 1)
    s, q = parts[:, :, 0].sum(1), parts[:, :, 1].sum(1)
    np.testing.assert_allclose(s.cpu().numpy(), d64.sum(dim=(0, 2, 3, 4)).cpu().numpy(), rtol=0, atol=1e-6 * float(d64.abs().sum(dim=(0, 2, 3, 4)).max()))
    np.testing.assert_allclose(q.cpu().numpy(), (d64 * d64).sum(dim=(0, 2, 3, 4)).cpu().numpy(), rtol=1e-6)
    assert torch.equal(ops.convT3d_k3_s2_bf16x3_stats(x, wq, pivot)[1], parts)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(gpu), (torch.randn(Cout, generator=g) * 0.1).to(gpu)
    skip = torch.randn(plain.shape, generator=g).to(gpu)
    two = ops.bn3d_relu_train(plain, gamma, beta, 1e-5, True, skip)
    one = ops.bn3d_relu_train(plain, gamma, beta, 1e-5, True, skip, parts, pivot)
    np.testing.assert_allclose(one[1].cpu().numpy(), y64.mean(dim=(0, 2, 3, 4)).cpu().numpy(), rtol=1e-6, atol=1e-7 * float(y64.abs().max()))
    np.testing.assert_allclose(one[2].cpu().numpy(), two[2].cpu().numpy(), rtol=2e-5)
    assert float((one[0] - two[0]).abs().max()) <= 2e-5 * max(1.0, float(two[0].abs().max()))


def test_scl_pack_reads_a_pitched_volume_in_place(gpu):
    from mvsdet_amd import ops
    buf = torch.randn(2, 9, 3, 5, 32, device=gpu)
    view = buf[..., :20]                       # rows 32 elements apart, 20 used: a row-pitched cost volume
    a, b = ops.scl_pack(view), ops.scl_pack(view.contiguous())
    assert torch.equal(a.data.view(torch.int16), b.data.view(torch.int16))


@pytest.mark.parametrize("N,Cin,Cout,Di,Hi,Wi", [(1, 16, 64, 8, 16, 32), (2, 24, 64, 5, 13, 21), (1, 8, 128, 6, 30, 40),
                                                  (1, 37, 64, 9, 25, 33), (1, 64, 128, 12, 60, 80), (1, 5, 64, 1, 1, 1),
                                                  (1, 128, 256, 6, 30, 40), (1, 3, 64, 2, 2, 2),
                                                  (1, 512, 128, 8, 20, 20)])   # the last one: split over the input channels
def test_conv3d_k3_s2_bf16x3(gpu, N, Cin, Cout, Di, Hi, Wi):
    """Stride-2 convolution as the sum over the 8 parity classes of its input (conv1 / conv3 of mvsnet.py:77,79)."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + Cin + Wi)
    x = torch.randn(N, Cin, Di, Hi, Wi, generator=g).abs() * 2.0
    wgt = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    wq = ops.split_conv_weight(wgt.to(gpu), 1)
    assert torch.equal(wq.cpu().view(torch.int16), ops.split_conv_weight(wgt, 1).view(torch.int16))
    raw = ops.conv3d_k3_s2_bf16x3(x.to(gpu), wq, None, None, False).cpu()
    want = three_term_conv64(x, wgt, padding=1, stride=2)
    assert raw.shape == want.shape
    mag = float(F.conv3d(x.abs().double(), wgt.abs().double(), padding=1, stride=2).max())
    assert float((raw.double() - want).abs().max()) <= 4e-7 * mag
    ref32 = F.conv3d(x.double(), wgt.double(), padding=1, stride=2)
    assert float((raw.double() - ref32).abs().max()) <= 2e-5 * float(ref32.abs().max()) + 1e-6
    full = ops.conv3d_k3_s2_bf16x3(x.to(gpu), wq, scale.to(gpu), shift.to(gpu), True).cpu()
    wantf = torch.relu(torch.addcmul(shift.view(1, -1, 1, 1, 1), raw, scale.view(1, -1, 1, 1, 1)))
    np.testing.assert_allclose(full.numpy(), wantf.numpy(), rtol=0, atol=2e-6 * max(1.0, float(wantf.abs().max())))
    # the parity-split SCL input (class tiles by LDS-DMA): the same MFMAs on the same pieces.  The fp32 form may have been split
    # over the input channels (small volumes); the unsplit sums are compared at the accumulation-order tolerance then.
    xp = ops.pscl_from_tensor(x.to(gpu))
    hi, mid, clean = xp.pieces()
    assert clean and torch.equal(hi[:, :Cin].cpu(), ops.split_bf16(x)[0])
    f32, scl = ops.conv3d_k3_s2_bf16x3(xp, wq, scale.to(gpu), shift.to(gpu), True, outputs=("f32", "scl"))
    from mvsdet_amd import _lib
    if _lib.load().mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes(N, Cin, Cout, Di, Hi, Wi) == 0:
        assert torch.equal(f32.cpu(), full)
    else:
        np.testing.assert_allclose(f32.cpu().numpy(), full.numpy(), rtol=0, atol=4e-7 * mag)
    eh, em = ops.split_bf16(f32.cpu())
    hi, mid = scl.pieces()
    assert torch.equal(hi.cpu(), eh) and torch.equal(mid.cpu(), em) and scl.border_is_zero()
    # a producing stride-1 layer's PSCL output feeds this layer like the fp32 tensor does
    if Cin % 64 == 0 and Cin <= 128:
        wp = ops.split_conv_weight((torch.randn(Cin, 8, 3, 3, 3, generator=g) / 15).to(gpu))
        pf, pp = ops.conv3d_k3_bf16x3(x[:, :8].contiguous().to(gpu), wp, None, None, True, outputs=("f32", "pscl"))
        assert torch.equal(ops.conv3d_k3_s2_bf16x3(pp, wq, None, None, False, outputs=("f32", "scl"))[0],
                           ops.conv3d_k3_s2_bf16x3(pf, wq, None, None, False, outputs=("f32", "scl"))[0])   # both unsplit


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 16, 64, 4, 8, 16), (2, 24, 64, 3, 7, 11), (1, 256, 128, 3, 15, 20),
                                               (1, 128, 64, 6, 30, 40), (1, 5, 64, 1, 1, 1), (1, 40, 64, 5, 60, 17),
                                               # conv9 / conv11 of the cost network on several views, ragged extents, one voxel
                                               (2, 128, 64, 6, 30, 40), (1, 24, 128, 3, 15, 20), (1, 8, 64, 5, 17, 9),
                                               (3, 128, 64, 6, 30, 40), (2, 256, 128, 3, 15, 20), (3, 128, 64, 5, 13, 21),
                                               (2, 96, 128, 4, 20, 9), (1, 96, 64, 1, 1, 1)])
def test_convT3d_k3_s2_bf16x3(gpu, N, Cin, Cout, D, H, W):
    """Transposed convolution as 8 output parity classes over the coarse input (conv9 / conv11 of mvsnet.py:92-100), with
    the affine, the ReLU and the skip tensor added last (mvsnet.py:110-111)."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + Cin + W)
    x = torch.randn(N, Cin, D, H, W, generator=g).abs() * 2.0
    wgt = torch.randn(Cin, Cout, 3, 3, 3, generator=g) / (27 * Cin / 8) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(N, Cout, 2 * D, 2 * H, 2 * W, generator=g)
    wq = ops.split_conv_weight(wgt.to(gpu), 2)
    assert torch.equal(wq.cpu().view(torch.int16), ops.split_conv_weight(wgt, 2).view(torch.int16))
    raw = ops.convT3d_k3_s2_bf16x3(x.to(gpu), wq, None, None, None, False).cpu()
    kw = dict(stride=2, padding=1, output_padding=1)
    xh, xm = (t.double() for t in ops.split_bf16(x))
    wh, wm = (t.double() for t in ops.split_bf16(wgt))
    want = F.conv_transpose3d(xh, wh, **kw) + F.conv_transpose3d(xh, wm, **kw) + F.conv_transpose3d(xm, wh, **kw)
    assert raw.shape == want.shape
    mag = float(F.conv_transpose3d(x.abs().double(), wgt.abs().double(), **kw).max())
    assert float((raw.double() - want).abs().max()) <= 4e-7 * mag
    ref32 = F.conv_transpose3d(x.double(), wgt.double(), **kw)
    assert float((raw.double() - ref32).abs().max()) <= 2e-5 * float(ref32.abs().max()) + 1e-6
    full = ops.convT3d_k3_s2_bf16x3(x.to(gpu), wq, scale.to(gpu), shift.to(gpu), res.to(gpu), True).cpu()
    wantf = res + torch.relu(torch.addcmul(shift.view(1, -1, 1, 1, 1), raw, scale.view(1, -1, 1, 1, 1)))
    np.testing.assert_allclose(full.numpy(), wantf.numpy(), rtol=0, atol=2e-6 * max(1.0, float(wantf.abs().max())))
    f32, scl = ops.convT3d_k3_s2_bf16x3(x.to(gpu), wq, scale.to(gpu), shift.to(gpu), res.to(gpu), True, outputs=("f32", "scl"))
    assert torch.equal(f32.cpu(), full)
    eh, em = ops.split_bf16(full)
    hi, mid = scl.pieces()
    assert torch.equal(hi.cpu(), eh) and torch.equal(mid.cpu(), em) and scl.border_is_zero()


@pytest.mark.parametrize("N,Cin,D,H,W", [(2, 64, 12, 60, 80), (1, 5, 3, 7, 12), (1, 64, 4, 12, 40), (2, 3, 9, 25, 44)])
def test_head_on_the_sum_of_two_inputs(gpu, N, Cin, D, H, W):
    """mvsnet.py:111-112: the 64 -> 2 head on conv0 + conv11(x) with the addition formed while the halo tiles are staged: the
    same bits as the head on the precomputed sum, and ATen's convolution within fp32 accumulation order."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(Cin + W)
    x, y = torch.randn(N, Cin, D, H, W, generator=g), torch.randn(N, Cin, D, H, W, generator=g)
    wgt, bias = torch.randn(2, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5, torch.randn(2, generator=g)
    got = ops.conv3d_k3_cout2_sum(x.to(gpu), y.to(gpu), wgt.to(gpu), bias.to(gpu))
    one = ops.conv3d_k3_cout2_sum((x + y).to(gpu), None, wgt.to(gpu), bias.to(gpu))
    assert torch.equal(got, one) and torch.equal(one, ops.conv3d_k3_cout2((x + y).to(gpu), wgt.to(gpu), bias.to(gpu)))
    ref = F.conv3d((x + y).double(), wgt.double(), bias.double(), padding=1)
    np.testing.assert_allclose(got.cpu().double().numpy(), ref.numpy(), rtol=0, atol=1e-5 * max(1.0, float(ref.abs().max())))


def test_cost_network_on_two_halves_of_the_views_agrees_bit_for_bit(gpu):
    """`CostRegNet3DGS.view_streams = 2` (eval chain, 8 views or more): the second half of the views on a stream of its own -- the
    same logits as one batch on the caller's stream, for an even and an odd number of views, back to back without a
    synchronisation in between (the halves' buffers are keyed by the stream)."""
    from mvsdet_amd.costreg import CostRegNet3DGS
    torch.manual_seed(5)
    net = CostRegNet3DGS(64).to(gpu).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    assert net.view_streams == 2
    xs = [torch.rand(shape, device=gpu) for shape in ((8, 64, 4, 12, 16), (11, 64, 8, 8, 24), (8, 64, 4, 12, 16))]
    xs.append(torch.rand((9, 64, 4, 12, 48), device=gpu)[..., :16])   # a row-pitched volume (forward_scene's pitched variance): halves of a strided view
    with torch.no_grad():
        two = [net(x) for x in xs]
        net.view_streams = 1
        one = [net(x) for x in xs]
        net.view_streams = 2
    torch.cuda.synchronize(gpu)
    for a, b in zip(one, two):
        assert a.shape == b.shape and torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(two[-1], net(xs[-1].contiguous()))


def test_cost_network_layer_forms_agree_bit_for_bit(gpu):
    """CostRegNet3DGS in eval mode: every layer handing the next one its output already cut into bf16 pieces (SCL / PSCL, the
    default) against fp32 tensors between the layers: the same logits bit for bit, twice in a row (the buffers are reused)."""
    from mvsdet_amd.costreg import CostRegNet3DGS
    torch.manual_seed(3)
    net = CostRegNet3DGS(256).to(gpu).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    from mvsdet_amd import _lib
    lib = _lib.load()
    # these small grids would be split over the input channels on the fp32 route (other partial sums); the 40-view volumes
    # of the shipped configuration never are: the knob keeps both routes unsplit here
    _lib.check(lib.mvsdet_set_option(b"conv_nsplit", 1), "set_option")
    try:
        for shape in ((2, 256, 12, 20, 40), (3, 256, 4, 12, 16), (2, 256, 12, 20, 40)):
            x = torch.rand(shape, device=gpu)
            with torch.no_grad():
                net.layer_forms = "f32"
                ref = net(x)
                net.layer_forms = "scl"
                a = net(x)
                b = net(x * 0.5 + 0.1)
                c = net(x)
            assert torch.equal(a, ref) and torch.equal(c, ref) and not torch.equal(b, ref)
    finally:
        _lib.check(lib.mvsdet_set_option(b"conv_nsplit", 0), "set_option")


def test_conv3d_k3_bf16x3_argument_checks(gpu):
    from mvsdet_amd import ops
    xs = ops.scl_pack(torch.zeros(1, 8, 2, 2, 2, device=gpu))
    wq = ops.split_conv_weight(torch.zeros(64, 8, 3, 3, 3)).to(gpu)
    with pytest.raises(ValueError):
        ops.conv3d_k3_bf16x3(xs, wq[:, :, :13], None, None, False)
    with pytest.raises(ValueError):
        ops.conv3d_k3_bf16x3(xs, wq, torch.ones(64, device=gpu), None, False)
    with pytest.raises(ValueError):
        ops.split_conv_weight(torch.zeros(60, 8, 3, 3, 3))
    assert float(ops.conv3d_k3_bf16x3(xs, wq, None, None, False).abs().max()) == 0.0


@pytest.mark.parametrize("N,Cin,Cout,D,H,W,nsplit", [(2, 32, 64, 3, 8, 16, 4), (1, 40, 70, 2, 5, 20, 3), (2, 5, 3, 1, 1, 4, 2),
                                                     (1, 64, 32, 4, 9, 36, 200), (2, 64, 64, 12, 60, 80, 0),
                                                     (1, 33, 31, 5, 7, 24, 7), (3, 8, 8, 2, 3, 12, 1)])
def test_conv3d_k3_dw_bf16x3(gpu, N, Cin, Cout, D, H, W, nsplit):
    """Weight gradient of the stride-1 layers on the bf16 matrix cores (csrc/costreg_dw_bf16.hip): against the float64 sum
    of the same three piece products, and against ATen's fp32 conv3d_weight within the scheme's truncation."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 100 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    gy = torch.randn(N, Cout, D, H, W, generator=g)
    shape = (Cout, Cin, 3, 3, 3)
    xh, xm = (t.double() for t in ops.split_bf16(x))
    yh, ym = (t.double() for t in ops.split_bf16(gy))
    cw = lambda a, b: torch.nn.grad.conv3d_weight(a, shape, b, padding=1)
    want = cw(xh, yh) + cw(xh, ym) + cw(xm, yh)
    got = ops.conv3d_k3_dw(x.to(gpu), gy.to(gpu), nsplit, 1, True).cpu()
    assert got.shape == want.shape
    scale = float(want.abs().max())
    # fp32 accumulation of N*D*H*W products per element, in splits
    np.testing.assert_allclose(got.double().numpy(), want.numpy(), rtol=0, atol=2e-6 * scale * max(1.0, (N * D * H * W) ** 0.5 / 8))
    full = cw(x.double(), gy.double())
    assert float((got.double() - full).abs().max()) <= 1e-4 * scale
    fp32 = ops.conv3d_k3_dw(x.to(gpu), gy.to(gpu), nsplit).cpu()
    assert float((got - fp32).abs().max()) <= 1e-4 * scale


@pytest.mark.parametrize("N,Cin,Cout,D,H,W,nsplit", [(2, 16, 64, 4, 8, 16, 4), (1, 40, 70, 2, 6, 24, 3), (2, 5, 3, 2, 2, 8, 2),
                                                     (1, 64, 128, 6, 10, 40, 200), (2, 64, 128, 12, 60, 80, 0),
                                                     (1, 33, 31, 6, 14, 24, 7), (3, 8, 130, 2, 4, 16, 1),
                                                     (2, 128, 64, 4, 12, 40, 0)])
def test_conv3d_k3_s2_dw_bf16x3(gpu, N, Cin, Cout, D, H, W, nsplit):
    """Weight gradient of the stride-2 layers (conv1, conv3) and -- the same call with the fine tensor first -- of the transposed
    ones (conv9, conv11) on the bf16 matrix cores (csrc/costreg_dw_s2_bf16.hip): against the float64 sum of the same three
    piece products, against ATen's conv3d_weight in float64 within the scheme's truncation, against the fp32-MFMA kernel,
    and against autograd of conv_transpose3d for the exchanged orientation."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 100 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    gy = torch.randn(N, Cout, D // 2, H // 2, W // 2, generator=g)
    shape = (Cout, Cin, 3, 3, 3)
    xh, xm = (t.double() for t in ops.split_bf16(x))
    yh, ym = (t.double() for t in ops.split_bf16(gy))
    cw = lambda a, b: torch.nn.grad.conv3d_weight(a, shape, b, stride=2, padding=1)
    want = cw(xh, yh) + cw(xh, ym) + cw(xm, yh)
    got = ops.conv3d_k3_dw(x.to(gpu), gy.to(gpu), nsplit, 2, True).cpu()
    assert got.shape == want.shape
    scale = float(want.abs().max())
    nv = N * D * H * W / 8
    np.testing.assert_allclose(got.double().numpy(), want.numpy(), rtol=0, atol=2e-6 * scale * max(1.0, nv ** 0.5 / 8))
    full = cw(x.double(), gy.double())
    assert float((got.double() - full).abs().max()) <= 1e-4 * scale
    fp32 = ops.conv3d_k3_dw(x.to(gpu), gy.to(gpu), nsplit, 2).cpu()
    assert float((got - fp32).abs().max()) <= 1e-4 * scale
    # the transposed layer (Cout -> Cin, input gy-shaped, output x-shaped): its (Cout,Cin,3,3,3) weight gradient is the same sum
    xt = gy.double().requires_grad_(True)
    wt = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv_transpose3d(xt, wt, stride=2, padding=1, output_padding=1).backward(x.double())
    assert float((got.double() - wt.grad).abs().max()) <= 1e-4 * scale


def test_conv3d_k3_s2_dw_bf16x3_needs_rows_of_whole_float4(gpu):
    from mvsdet_amd import ops
    x = torch.zeros(1, 8, 2, 4, 12, device=gpu)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.conv3d_k3_dw(x, torch.zeros(1, 8, 1, 2, 6, device=gpu), 0, 2, True)


def test_conv3d_k3_dw_bf16x3_needs_rows_of_whole_float4(gpu):
    from mvsdet_amd import ops
    x = torch.randn(1, 8, 2, 4, 18, device=gpu)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.conv3d_k3_dw(x, x.clone(), 0, 1, True)


def bf16x3_edge_vector():
    """64 floats at the edges of the fp32 -> (hi, mid) cut: signed zeros and ones, the ties of the first and of the second rounding,
    the carry into the exponent, the last float whose bf16 rounding is finite and the next one, FLT_MAX, tiny normals, two
    subnormals, infinities and a NaN; the remaining slots from the LCG."""
    import os
    import sys
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    from lcg import lcg_uniform
    bits = lambda b: np.array([b], dtype=np.uint32).view(np.float32)[0]
    fmax, fmin = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    head = [0.0, -0.0, 1.0, -1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -16, 1 + 2.0 ** -8 + 3 * 2.0 ** -16,
            float.fromhex("0x1.fep+0"), float.fromhex("0x1.ffp+0"), bits(0x7f7f7fff), bits(0x7f7f8000), fmax, -fmax, 1e-30, -1e-30,
            fmin, -fmin, bits(0x00000001), bits(0x007fffff), np.inf, -np.inf, np.nan]
    v = np.concatenate([np.array(head, dtype=np.float32), lcg_uniform(64 - len(head), 950)]).astype(np.float32)
    assert v.shape == (64,) and v[4] != 1.0 and v[6] != v[4] and v[10] < v[11] < fmax
    return v


def test_the_cut_at_its_edges_in_scl_pack_and_gemm_split_weight(gpu):
    """csrc/mfma.h's cut, through the two kernels that store its pieces as they are: every finite, normal or zero entry of the edge
    vector is cut exactly as ops.split_bf16 cuts it (both pieces, bit for bit), an infinity keeps its sign in hi, a NaN stays one."""
    from mvsdet_amd import ops
    v = torch.from_numpy(bf16x3_edge_vector())
    exact = (torch.isfinite(v) & ((v == 0) | (v.abs() >= float(np.finfo(np.float32).tiny))))
    assert int(exact.sum()) == 64 - 5
    bits = lambda t: t.contiguous().view(torch.int16)

    def check(hi, mid, src):
        eh, em = ops.split_bf16(src)
        ok = exact.view(-1)[torch.arange(src.numel()) % 64].view(src.shape)     # both layouts repeat the vector every 64 elements
        assert torch.equal(bits(hi)[ok], bits(eh)[ok]) and torch.equal(bits(mid)[ok], bits(em)[ok])
        inf = torch.isinf(src)
        assert int(inf.sum()) > 0 and torch.equal(hi.float()[inf], src[inf])
        nan = torch.isnan(src)
        assert int(nan.sum()) > 0 and bool(torch.isnan(hi.float()[nan]).all()) and bool(torch.isnan(mid.float()[nan]).all())

    x = v.view(1, 1, 2, 4, 8).permute(0, 4, 1, 2, 3).contiguous()            # (1, 8, 1, 2, 4): element (c, h, w) = v[8 (4 h + w) + c]
    hi, mid = ops.scl_pack(x.to(gpu)).pieces()
    check(hi.cpu().permute(0, 2, 3, 4, 1), mid.cpu().permute(0, 2, 3, 4, 1), x.permute(0, 2, 3, 4, 1))
    wm = v.repeat(64).view(128, 32)
    got = ops.gemm_split_weight(wm.to(gpu)).cpu().view(4, 2, 2, 2, 32, 8)      # [row tile][k16][piece][k-group][row][8]: lane = 32 (k-group) + row
    src = wm.view(4, 32, 2, 2, 8).permute(0, 2, 3, 1, 4)                       # the same order from the matrix
    eh, em = ops.split_bf16(src)
    okm = exact.repeat(64).view(128, 32).view(4, 32, 2, 2, 8).permute(0, 2, 3, 1, 4)
    assert torch.equal(bits(got[:, :, 0])[okm], bits(eh)[okm]) and torch.equal(bits(got[:, :, 1])[okm], bits(em)[okm])
    inf, nan = torch.isinf(src), torch.isnan(src)
    assert torch.equal(got[:, :, 0].float()[inf], src[inf])
    assert bool(torch.isnan(got[:, :, 0].float()[nan]).all()) and bool(torch.isnan(got[:, :, 1].float()[nan]).all())
