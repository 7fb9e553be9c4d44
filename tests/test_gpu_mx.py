"""conv0 on one fp16 + two block-scaled FP6 products per fp32-equivalent product (csrc/costreg_mx.h).

  * exact data: inputs and weights built so that EVERY piece of the scheme is exact -- xh = fp16(x), Q(xh), xr = x - xh, Q(xr) and
    the same for the weights, under the scales the kernel and the weight split derive -- so the kernel must return the float64 sum
    of the three product terms to fp32 rounding: operand maps, the 6-bit packing, fragment assembly, tap order and scale bytes;
  * random data: within 2^-14 of the output's scale of the float64 convolution (the scheme's own error; bf16x3: 2^-16);
  * the whole network on G8 (the reference module's logits): 1e-4, conv0 on this route;
  * values beyond fp16's range are cut on a block-uniform power of two: no cliff at 65504.
"""
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
from lcg import lcg_fill_state, lcg_uniform  # noqa: E402

pytestmark = pytest.mark.gpu


def _exact_case(N, Cin, Cout, D, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()   # noqa: E731
    # x = 128 k + j / 16, k in 8..15, j in 0..7:  fp16(x) = 128 k (ulp 1 in [1024, 2048)), stage exponent 8 -> Q(xh) = k / 2 exact,
    # xr = j / 16 -> Q(xr * 2^3) = j / 2 exact
    xh = 128.0 * ri(8, 15, (N, Cin, D, H, W))
    xr = ri(0, 7, (N, Cin, D, H, W)) / 16.0
    # w = +-p 2^-5 +- q 2^-16, p in 8..15, q in 0..7: fp16(w) = +-p 2^-5 (ulp 2^-12), Q(wh) = p / 2 and Q(wr) exact under their block scales
    sgn = lambda shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1   # noqa: E731
    wh = sgn((Cout, Cin, 3, 3, 3)) * ri(8, 15, (Cout, Cin, 3, 3, 3)) * 2.0 ** -5
    wr = sgn((Cout, Cin, 3, 3, 3)) * ri(0, 7, (Cout, Cin, 3, 3, 3)) * 2.0 ** -16
    ref = F.conv3d(xh, wh, padding=1) + F.conv3d(xh, wr, padding=1) + F.conv3d(xr, wh, padding=1)
    return (xh + xr).float(), (wh + wr).float(), ref


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 16, 64, 4, 12, 16), (2, 24, 128, 5, 13, 35), (1, 8, 64, 3, 8, 16), (1, 20, 64, 2, 9, 7)])
def test_every_piece_exact(gpu, N, Cin, Cout, D, H, W):
    from mvsdet_amd import ops
    x, w, ref = _exact_case(N, Cin, Cout, D, H, W, seed=Cin + W)
    assert torch.equal((x.double() - x.half().double()), (x.double() - (x.double() / 128).floor() * 128))   # the construction holds
    got = ops.conv3d_k3_fp16mx(x.to(gpu), ops.split_conv_weight_mx(w.to(gpu)), None, None, False)
    err = float((got.double().cpu() - ref).abs().max())
    assert err <= 2e-7 * float(ref.abs().max()) * 8, (err, float(ref.abs().max()))


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(2, 64, 64, 4, 12, 32), (1, 256, 64, 4, 24, 16), (1, 30, 128, 6, 10, 20)])
def test_random_data_against_float64(gpu, N, Cin, Cout, D, H, W, record_property):
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(5)
    f = torch.randn((3, N, Cin, D, H, W), generator=g)
    x = (f * f).mean(0) - f.mean(0) ** 2                                   # variance-like: what the sweep hands conv0
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    ref = torch.relu(F.conv3d(x.double(), w.double(), padding=1) * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))
    xd, wd = x.to(gpu), w.to(gpu)
    got, pscl = ops.conv3d_k3_fp16mx(xd, ops.split_conv_weight_mx(wd), sc.to(gpu), sh.to(gpu), True, outputs=("f32", "pscl"))
    b3 = ops.conv3d_k3_bf16x3(xd, ops.split_conv_weight(wd), sc.to(gpu), sh.to(gpu), True)
    scale = float(ref.abs().max())
    err, err3 = float((got.double().cpu() - ref).abs().max()) / scale, float((b3.double().cpu() - ref).abs().max()) / scale
    record_property("fp16mx_err_of_scale", err)
    print(f"fp16mx {err:.2e} of scale, bf16x3 {err3:.2e}")
    assert err <= 2.0 ** -14, err
    # the parity-split SCL output is the fp32 output cut into bf16 pieces: the same as the bf16x3 kernel's form of the same values
    _, pscl3 = ops.conv3d_k3_bf16x3(got.new_zeros(0) if False else xd, ops.split_conv_weight(wd), sc.to(gpu), sh.to(gpu), True, outputs=("f32", "pscl"))
    assert pscl.data.shape == pscl3.data.shape


def test_strided_view_and_values_beyond_fp16(gpu):
    """A row-pitched view gives the contiguous tensor's bits; values beyond fp16's range (65504) are handled by the block-uniform power
    of two a stage is cut on (costreg_mx.h "fp16"): the result stays within the scheme's error of the float64 convolution, in the
    blocks that meet such values and in all others."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(9)
    big = torch.rand((1, 16, 4, 12, 48), generator=g).to(gpu)
    w = (torch.randn((64, 16, 3, 3, 3), generator=g) * 0.05).to(gpu)
    wq = ops.split_conv_weight_mx(w)
    view = big[..., :32]                                    # a row-pitched volume: w stride 1, h stride 48
    assert torch.equal(ops.conv3d_k3_fp16mx(view, wq, None, None, False), ops.conv3d_k3_fp16mx(view.contiguous(), wq, None, None, False))
    x = view.contiguous().clone()
    x[0, 3, 1, 5, 20] = 7.0e4                               # no fp16 without the stage's power of two
    x[0, 9, 2, 7, 25] = -3.0e9                              # another channel group
    x[0, :, 3, 2:4, 22:26] *= 1.0e5
    got = ops.conv3d_k3_fp16mx(x, wq, None, None, False)
    ref = F.conv3d(x.double().cpu(), w.double().cpu(), padding=1)
    err = (got.double().cpu() - ref).abs()
    assert torch.isfinite(got).all()
    # the blocks that meet the huge values (w >= 16): within the scheme's error of THEIR scale (a stage is cut on one power of two per
    # block: a value 2^-14 below the block's largest loses bits, as any fp16 does) ...
    assert float(err.max()) <= 2.0 ** -13 * float(ref.abs().max())
    # ... the blocks that do not (their halo ends at w = 16): untouched, at their own scale
    assert float(err[..., :12].max()) <= 2.0 ** -14 * float(ref[..., :12].abs().max())
    assert float(ref[..., :12].abs().max()) < 1e3 < float(ref.abs().max())
    with pytest.raises(ValueError):
        ops.conv3d_k3_fp16mx(view, wq[:, :1], None, None, False)


def test_the_three_forms_of_the_kernel_give_the_same_bits(gpu):
    """Library option conv_mx_th: 0 = the wave-specialised kernel (default), 8 / 12 = every wave does everything on 4 x 8 x 16 /
    4 x 12 x 16 tiles: the same sums in the same order."""
    from mvsdet_amd import _lib, ops
    g = torch.Generator().manual_seed(21)
    x = torch.rand((2, 40, 5, 13, 35), generator=g).to(gpu)
    w = (torch.randn((64, 40, 3, 3, 3), generator=g) * 0.05).to(gpu)
    wq = ops.split_conv_weight_mx(w)
    was = _lib.get_option("conv_mx_th")
    try:
        outs = []
        for form in (0, 8, 12):
            _lib.set_option("conv_mx_th", form)
            outs.append(ops.conv3d_k3_fp16mx(x, wq, None, None, True))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and float(outs[0].abs().max()) > 0
    finally:
        _lib.set_option("conv_mx_th", was)


def test_g8_with_conv0_on_the_mixed_format_route(gpu):
    """G8 (the REFERENCE CostRegNet_3DGS's logits, mvs_models/mvsnet.py:73-113) with conv0 on fp16 + MX FP6: 1e-4."""
    from mvsdet_amd.costreg import CostRegNet3DGS
    g = load_golden("g8_cost_regularisation")
    net = CostRegNet3DGS(256, 64).eval()
    with torch.no_grad():
        lcg_fill_state(net, int(g["weight_seed"]))
        shape = tuple(int(v) for v in g["in_shape"])
        x = torch.from_numpy(lcg_uniform(int(np.prod(shape)), int(g["input_seed"]))).reshape(shape).abs().to(gpu)
        net = net.to(gpu)
        assert net.conv0_precision == "fp16mx"            # the default of the eval chain
        y = net(x)
        net.conv0_precision = "bf16x3"
        y3 = net(x)
    e, e3 = float(np.abs(y.cpu().numpy() - g["logits"]).max()), float(np.abs(y3.cpu().numpy() - g["logits"]).max())
    print(f"G8 logits: fp16mx conv0 {e:.2e}, bf16x3 {e3:.2e}")
    assert e <= 1e-4 and not torch.equal(y, y3)


def _hdr_case(N, Cin, Cout, D, H, W, seed, spikes=6):
    """Variance-like input whose per-channel scales span 10^-3 .. 10^3, with isolated spikes 10^4 above their channel."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((3, N, Cin, D, H, W), generator=g)
    x = (f * f).mean(0) - f.mean(0) ** 2
    x = x * (10.0 ** (torch.rand((1, Cin, 1, 1, 1), generator=g) * 6 - 3))
    for _ in range(spikes):
        n, c = int(torch.randint(0, N, (1,), generator=g)), int(torch.randint(0, Cin, (1,), generator=g))
        d, h, w_ = (int(torch.randint(0, s, (1,), generator=g)) for s in (D, H, W))
        x[n, c, d, h, w_] *= 1e4
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
    return x, w


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 64, 64, 4, 16, 32), (2, 20, 128, 5, 13, 17), (1, 256, 64, 4, 8, 16)])
def test_high_dynamic_range_within_the_block_bound(gpu, N, Cin, Cout, D, H, W, record_property):
    """Per-channel scales over six decades and spikes 10^4 above their block: the error of every output stays within what the
    scheme guarantees in terms of each block's largest |x| and the weights' sums (tests/conv_bounds.py mx_bound).  Such data can
    break a bound stated on the output's own summed |products| (tests/fuzz_round6.py's 2^-13): a small value next to a large one
    in its block loses its FP6 correction terms -- how far past that bound it goes is recorded, not asserted."""
    from mvsdet_amd import ops
    from conv_bounds import mx_bound
    x, w = _hdr_case(N, Cin, Cout, D, H, W, seed=Cin + D)
    got = ops.conv3d_k3_fp16mx(x.to(gpu), ops.split_conv_weight_mx(w.to(gpu)), None, None, False).double().cpu()
    ref = F.conv3d(x.double(), w.double(), padding=1)
    mags = F.conv3d(x.double().abs(), w.double().abs(), padding=1)
    bound = mx_bound(x, w, None, N, Cin, Cout, D, H, W, (4, 8, 16)) + 2.0 ** -23 * ref.abs()
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all())
    ratio = float((err / bound).max())
    fuzz = float((err / (2.0 ** -13 * mags)).max())
    record_property("block_bound_used", ratio)
    record_property("summed_products_bound_2m13_used", fuzz)
    record_property("summed_products_bound_failures", int((err > 2.0 ** -13 * mags).sum()))
    print(f"HDR {N}x{Cin}->{Cout} {D}x{H}x{W}: block bound used {ratio:.3f}, 2^-13 summed |products| bound used {fuzz:.3f}")
    assert ratio <= 1.0, ratio


def test_non_finite_inputs_stay_in_their_receptive_field(gpu):
    """A NaN or +-Inf input is non-finite in float64 only inside its 3 x 3 x 3 receptive field.  The stage's block scale
    (costreg_mx.h publish_amax: fmaxf drops NaN, takes Inf) must not carry it further: every output outside the fields is finite
    and within the block bound of the finite data."""
    from mvsdet_amd import ops
    from conv_bounds import mx_bound
    N, Cin, Cout, D, H, W = 1, 20, 64, 8, 16, 32
    g = torch.Generator().manual_seed(77)
    f = torch.randn((3, N, Cin, D, H, W), generator=g)
    x = (f * f).mean(0) - f.mean(0) ** 2
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
    bad = [(0, 3, 1, 4, 5, float("nan")), (0, 12, 6, 11, 20, float("inf")), (0, 17, 2, 9, 28, float("-inf"))]
    xb = x.clone()
    field = torch.zeros((D, H, W), dtype=torch.bool)
    for n, c, d, h, w_, v in bad:
        xb[n, c, d, h, w_] = v
        field[max(d - 1, 0):d + 2, max(h - 1, 0):h + 2, max(w_ - 1, 0):w_ + 2] = True
    got = ops.conv3d_k3_fp16mx(xb.to(gpu), ops.split_conv_weight_mx(w.to(gpu)), None, None, False).double().cpu()
    ref = F.conv3d(x.double(), w.double(), padding=1)
    bound = mx_bound(x, w, None, N, Cin, Cout, D, H, W, (4, 8, 16)) + 2.0 ** -23 * ref.abs()
    outside = ~field.view(1, 1, D, H, W).expand_as(got)
    assert bool(torch.isfinite(got[outside]).all()), int((~torch.isfinite(got[outside])).sum())
    assert bool(((got - ref).abs()[outside] <= bound[outside]).all())
    assert not bool(torch.isfinite(got[~outside]).all())          # and the fields themselves are not finite


def test_views_beyond_32_bit_offsets_run_on_bf16x3(gpu):
    """A view whose channels span more than 4 GiB (8 channels 0.57 GB apart, NaN between them): mvsdet_conv3d_k3_fp16mx_f32in refuses
    it (its buffer offsets are 32 bits), ops.conv3d_k3_fp16mx and the network's conv0 run it on the bf16x3 kernel -- the float64
    convolution within the bf16x3 bound, and the network the same bits as with conv0 on bf16x3 from a contiguous copy."""
    import ctypes
    from mvsdet_amd import _lib, ops
    from mvsdet_amd.costreg import CostRegNet3DGS
    N, Cin, Cout, D, H, W = 1, 8, 64, 16, 24, 40
    vol = D * H * W
    sC = (1 << 32) // (4 * (Cin - 1)) + 64                      # (Cin - 1) * sC * 4 > 2^32: about 4.3 GB in all
    g = torch.Generator().manual_seed(3)
    x = torch.rand((N, Cin, D, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    canvas = torch.full(((Cin - 1) * sC + vol,), float("nan"), device=gpu)
    xv = canvas.as_strided((N, Cin, D, H, W), (Cin * sC, sC, H * W, W, 1))
    xv.copy_(x.to(gpu))
    assert not ops.conv3d_k3_fp16mx_ok(xv) and ops.conv3d_k3_fp16mx_ok(xv[:, :1]) and ops.conv3d_k3_fp16mx_ok(x.to(gpu))
    wd, scd, shd = w.to(gpu), sc.to(gpu), sh.to(gpu)
    wq = ops.split_conv_weight_mx(wd)
    out = torch.empty((N, Cout, D, H, W), device=gpu)
    xs = (ctypes.c_int64 * 4)(*[int(s) for s in xv.stride()[:4]])
    lib = _lib.load()
    assert lib.mvsdet_conv3d_k3_fp16mx_f32in(_lib.ptr(xv), xs, _lib.ptr(wq), None, None, _lib.ptr(out), None, None, N, Cin, Cout, D, H, W,
                                             0, _lib.current_stream(gpu)) == 1
    assert b"4 GiB" in lib.mvsdet_last_error()
    with pytest.raises(ValueError, match="addressing"):
        ops.conv3d_k3_fp16mx(xv, wq, scd, shd, True)
    got = ops.conv3d_k3_fp16mx(xv, wq, scd, shd, True, weight=wd)
    assert torch.equal(got, ops.conv3d_k3_bf16x3(x.to(gpu), ops.split_conv_weight(wd), scd, shd, True))
    ref = torch.relu(F.conv3d(x.double(), w.double(), padding=1) * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))
    mag = F.conv3d(x.double(), w.double().abs(), padding=1) * sc.double().view(1, -1, 1, 1, 1)
    assert float((got.double().cpu() - ref).abs().max()) <= 3 * 2.0 ** -16 * float(mag.max())
    net = CostRegNet3DGS(Cin, 64).eval()
    with torch.no_grad():
        lcg_fill_state(net, 11)
        net = net.to(gpu)
        assert net.conv0_precision == "fp16mx"
        y = net(xv)
        net.conv0_precision = "bf16x3"
        y3 = net(x.to(gpu))
    assert torch.isfinite(y).all() and torch.equal(y, y3)
    del canvas, xv
    torch.cuda.empty_cache()


@pytest.mark.parametrize("seed,hdr", [(0, False), (1, False), (2, True), (3, True)])
def test_network_logits_against_float64_on_swept_scenes(gpu, seed, hdr, record_property):
    """The eval default's gate: CostRegNet3DGS (G8 weights) on the variance volume the HIP sweep makes of a synthetic G13-like scene
    (6 views, C = 256, 12 planes, 60 x 80), against the same module in float64 on the CPU.  hdr: feature channels scaled over three
    decades (the variance over six).  Errors are max |logit - float64| over max(1, max |float64 logit|); fp16mx must keep a 2x margin
    under the project's 1e-4 bar, bf16x3 is recorded beside it."""
    import copy
    from mvsdet_amd import synthetic
    from mvsdet_amd.costreg import CostRegNet3DGS
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 6, 256, 12, (60, 80)
    meta = synthetic.make_img_meta(N, hw, seed=seed)
    feat = synthetic.make_features(N, C, hw, seed=seed)
    if hdr:
        g = torch.Generator().manual_seed(500 + seed)
        feat = feat * 10.0 ** (torch.rand((1, C, 1, 1), generator=g) * 3 - 1.5)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D, topk=3)
    with torch.no_grad():
        out = hp.forward_scene(feat.to(gpu), meta, cost_logits=synthetic.make_cost_logits(N, D, hw, seed=seed).to(gpu))
    var = out["variance"]
    assert tuple(var.shape) == (N, C, D) + hw
    net = CostRegNet3DGS(C, 64).eval()
    lcg_fill_state(net, int(load_golden("g8_cost_regularisation")["weight_seed"]))
    net64 = copy.deepcopy(net).double()
    net = net.to(gpu)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    try:
        with torch.no_grad():
            assert net.conv0_precision == "fp16mx"
            y = net(var).double().cpu()
            net.conv0_precision = "bf16x3"
            y3 = net(var).double().cpu()
            y64 = net64(var.double().cpu())
    finally:
        torch.set_num_threads(threads)
    scale = max(1.0, float(y64.abs().max()))
    e, e3 = float((y - y64).abs().max()) / scale, float((y3 - y64).abs().max()) / scale
    record_property("fp16mx_logit_err", e)
    record_property("bf16x3_logit_err", e3)
    record_property("logit_scale", scale)
    print(f"scene {seed} hdr={hdr}: variance max {float(var.abs().max()):.3g}, logits scale {scale:.3g}: fp16mx {e:.2e}, bf16x3 {e3:.2e}")
    assert bool(torch.isfinite(y).all()) and e3 <= 5e-5
    assert e <= 5e-5, e
