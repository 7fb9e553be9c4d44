"""Level 0 of the 2-D feature pyramid on HIP (csrc/fpn.hip): the lateral kernel, its top-down addition, the 3x3 kernel and its packed
epilogue, their memory edges, the module's chain against the float64 restatement of the FPN (tests/fpn_restated.py) and the hot
path's entry from the backbone stages.

The bounds are the project's (tests/test_gpu_bf16.py), applied per element with mag = conv(|x|, |w|) in float64:
    |kernel - three-term restatement| <= 4e-7 mag      fp32 accumulation of exact products
    |kernel - float64|                <= 3 2^-16 mag   the dropped terms, worst case
The float64 references are computed once per case, on the device (matrix products, `fpn_restated.conv64`)."""
import pytest
import torch
import torch.nn.functional as F

import fpn_restated as R
from canvas import Guarded, guarded_f32, ok

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 8, 16     # the 3x3 kernel's pixel tile: kFcTH x kFcTW of csrc/fpn.hip (ops.fpn.CONV3X3_TILE)


def _within(name, got, want, bound):
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |error| / bound = {ratio:.3e}, max |error| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{name}: max |error| / bound = {ratio}"


def _case(N, Cin, Cout, H, W, k, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).to(gpu)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5).to(gpu)
    b = (torch.randn(Cout, generator=g) * 0.1).to(gpu)
    return x, w, b


def test_tile_constants_are_the_kernels():
    from mvsdet_amd import ops
    assert ops.fpn.CONV3X3_TILE == (TILE_H, TILE_W)


@pytest.mark.parametrize("N,Cin,H,W", [(2, 256, 5, 7), (1, 512, 8, 10), (3, 1024, 15, 20), (1, 2048, 1, 1), (1, 32, 3, 3)])
def test_lateral_alone(gpu, N, Cin, H, W):
    """Column tails (35 pixels: under one block; 80: one block and a tail of 16; 900: views sharing a block), one K step up to 64, one pixel."""
    from mvsdet_amd import ops
    x, w, b = _case(N, Cin, 256, H, W, 1, 100 + Cin, gpu)
    got = ops.fpn.lateral(x, ops.gemm_split_weight(w.view(256, Cin)), b)
    assert got.shape == (N, 256, H, W)
    mag = R.mag64(x, w)
    _within("three-term", got, R.three_term_conv64(x, w) + b.double().view(1, -1, 1, 1), R.ACC * mag)
    _within("float64", got, R.conv64(x, w, b), R.CUT * mag)


@pytest.mark.parametrize("H,W,Ht,Wt", [(15, 20, 8, 10), (7, 5, 4, 3), (60, 80, 30, 40), (44, 46, 26, 14), (82, 3, 2, 1), (3, 3, 1, 1), (4, 4, 4, 4)])
def test_top_down_index_is_exact(gpu, H, W, Ht, Wt):
    """Zero lateral weight and bias, a distinct value per element of `top`: the output IS F.interpolate(top, size, mode='nearest')."""
    from mvsdet_amd import ops
    N, Cin, Cout = 2, 32, 128
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, Cin, H, W, generator=g).to(gpu)
    top = torch.arange(N * Cout * Ht * Wt, dtype=torch.float32).view(N, Cout, Ht, Wt) + 1.0    # < 2^24: exact
    wq = ops.gemm_split_weight(torch.zeros(Cout, Cin, device=gpu))
    got = ops.fpn.lateral(x, wq, torch.zeros(Cout, device=gpu), top.to(gpu)).cpu()
    want = F.interpolate(top, size=(H, W), mode="nearest")
    assert torch.equal(want, R.gather_nearest(top, (H, W)))
    assert torch.equal(got, want)
    assert torch.equal(got, F.interpolate(top.to(gpu), size=(H, W), mode="nearest").cpu())


def test_lateral_with_top(gpu):
    from mvsdet_amd import ops
    x, w, b = _case(2, 512, 256, 15, 20, 1, 21, gpu)
    top = torch.randn(2, 256, 8, 10, generator=torch.Generator().manual_seed(22)).to(gpu)
    got = ops.fpn.lateral(x, ops.gemm_split_weight(w.view(256, 512)), b, top)
    up = R.gather_nearest(top, (15, 20)).double()
    mag = R.mag64(x, w)
    _within("three-term", got, R.three_term_conv64(x, w) + b.double().view(1, -1, 1, 1) + up, R.ACC * mag)
    _within("float64", got, R.conv64(x, w, b) + up, R.CUT * mag)


@pytest.mark.parametrize("N,Cin,Cout,H,W", [(1, 256, 256, 1, 1), (1, 256, 256, 3, 3), (2, 256, 256, 5, 7), (1, 256, 256, 9, 33),
                                            (1, 256, 256, TILE_H, TILE_W), (1, 256, 256, TILE_H + 1, TILE_W + 1),
                                            (1, 256, 256, 60, 80), (1, 32, 128, 9, 33)])
def test_conv3x3_alone(gpu, N, Cin, Cout, H, W):
    """Border taps and tile edges: maps smaller than the tile, the tile itself, one pixel more in each axis, several tiles with ragged
    edges; the smallest channel counts the rules allow."""
    from mvsdet_amd import ops
    x, w, b = _case(N, Cin, Cout, H, W, 3, 300 + H * W + Cin, gpu)
    got = ops.fpn.conv3x3(x, ops.gemm_split_weight(ops.fpn.conv3x3_matrix(w)), b)
    assert got.shape == (N, Cout, H, W)
    mag = R.mag64(x, w, padding=1)
    _within("three-term", got, R.three_term_conv64(x, w, padding=1) + b.double().view(1, -1, 1, 1), R.ACC * mag)
    _within("float64", got, R.conv64(x, w, b, padding=1), R.CUT * mag)


@pytest.mark.parametrize("N,H,W", [(2, 5, 7), (1, TILE_H + 1, TILE_W + 1), (1, 20, 35)])
def test_conv3x3_counts_every_tap_once(gpu, N, H, W):
    """x = 1, w = 2^-12, no bias: every quantity is a power of two times a small integer, so the output equals F.conv2d's exactly and a
    missing or doubled border tap shows as a whole tap (256 2^-12 = 1/16)."""
    from mvsdet_amd import ops
    x = torch.ones(N, 256, H, W)
    w = torch.full((256, 256, 3, 3), 2.0 ** -12)
    got = ops.fpn.conv3x3(x.to(gpu), ops.gemm_split_weight(ops.fpn.conv3x3_matrix(w.to(gpu))), torch.zeros(256, device=gpu)).cpu()
    want = F.conv2d(x, w, padding=1)
    assert float(want[0, 0, 0, 0]) == min(H, 2) * min(W, 2) / 16.0
    assert torch.equal(got, want)


@pytest.mark.parametrize("N,H,W", [(2, 5, 7), (1, 60, 80)])
def test_packed_epilogue(gpu, N, H, W):
    from mvsdet_amd import ops
    x, w, b = _case(N, 256, 256, H, W, 3, 400 + H, gpu)
    wq = ops.gemm_split_weight(ops.fpn.conv3x3_matrix(w))
    nchw, packed = ops.fpn.conv3x3(x, wq, b, want_nchw=True, want_packed=True)
    assert torch.equal(nchw, ops.fpn.conv3x3(x, wq, b))
    assert packed.shape == (N * 256 * H * W,) and torch.equal(packed, ops.pack_features(nchw))
    only = ops.fpn.conv3x3(x, wq, b, want_nchw=False, want_packed=True)
    assert torch.equal(only, packed)
    with pytest.raises(ValueError, match="at least one"):
        ops.fpn.conv3x3(x, wq, b, want_nchw=False, want_packed=False)


def _in_nan_canvas(t, gpu):
    """t as a contiguous tensor in the middle of a NaN canvas: a stray read comes back as NaN."""
    pad = 4096
    canvas = torch.full((pad + t.numel() + pad,), float("nan"), dtype=torch.float32, device=gpu)
    view = canvas[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return canvas, view


def test_memory_edges(gpu):
    """Every output inside a guarded canvas, every input inside a NaN canvas: nothing outside the outputs changes, every output element
    is written (pre-filled with NaN, none left), and no value read from outside an input reaches an output."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    nan = float("nan")
    # lateral with top: (2,512,5,7) <- (3,4)
    x, w, b = _case(2, 512, 256, 5, 7, 1, 51, gpu)
    top = torch.randn(2, 256, 3, 4, generator=torch.Generator().manual_seed(52)).to(gpu)
    wq = ops.gemm_split_weight(w.view(256, 512))
    want = ops.fpn.lateral(x, wq, b, top)
    keep = [_in_nan_canvas(t, gpu) for t in (x, top, b)]
    g, out = guarded_f32((2, 256, 5, 7), gpu)
    out.fill_(nan)
    ok(lib.mvsdet_fpn_lateral_bf16x3(_lib.ptr(keep[0][1]), _lib.ptr(wq), _lib.ptr(keep[2][1]), _lib.ptr(keep[1][1]), g.ptr(), 2, 512, 256, 5, 7,
                                     3, 4, None))
    assert g.guards_intact() and not bool(torch.isnan(out).any()) and torch.equal(out, want)
    # 3x3 with both outputs: (2,256,5,7)
    x, w, b = _case(2, 256, 256, 5, 7, 3, 53, gpu)
    wq = ops.gemm_split_weight(ops.fpn.conv3x3_matrix(w))
    want, want_packed = ops.fpn.conv3x3(x, wq, b, want_nchw=True, want_packed=True)
    keep = [_in_nan_canvas(t, gpu) for t in (x, b)]
    g, out = guarded_f32((2, 256, 5, 7), gpu)
    gp, packed = guarded_f32((lib.mvsdet_packed_bytes(2, 256, 5, 7) // 4,), gpu)
    out.fill_(nan)
    packed.fill_(nan)
    ok(lib.mvsdet_fpn_conv3x3_bf16x3(_lib.ptr(keep[0][1]), _lib.ptr(wq), _lib.ptr(keep[1][1]), g.ptr(), gp.ptr(), 2, 256, 256, 5, 7, None))
    assert g.guards_intact() and gp.guards_intact()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(packed).any())
    assert torch.equal(out, want) and torch.equal(packed, want_packed)


CH, COUT = (32, 64, 96, 128), 128
PYRAMIDS = {"halved": [(12, 16), (6, 8), (3, 4), (2, 2)], "odd": [(15, 20), (8, 10), (4, 5), (2, 3)]}


def _ulp(v):
    """One float32 ulp of |v| at most: 2^-23 |v|."""
    return v.abs() * 2.0 ** -23


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_chain_against_the_restated_fpn(gpu, name):
    """FPNLevel0 on the HIP route against the float64 restatement, the bound propagated: each lateral's own 3 2^-16 mag, summed down
    the pyramid through the exact nearest gather into a per-element bound e0 on L0, then 3 2^-16 mag3 + conv(e0, |w3|) for the
    output, plus one float32 ulp of the result per addition in an epilogue (the bias; the level above)."""
    from mvsdet_amd.fpn import FPNLevel0
    sd = R.make_params(CH, COUT, seed=61)
    stages = R.make_stages(2, CH, PYRAMIDS[name], seed=62)
    fpn = FPNLevel0.from_state_dict(sd, prefix="", route="hip").to(gpu)
    dev_stages = [s.to(gpu) for s in stages]
    with torch.no_grad():
        got, packed = fpn(dev_stages, packed=True)
        again = fpn(dev_stages)
    assert torch.equal(got, again)                                            # the same bits on every run
    from mvsdet_amd import ops
    assert torch.equal(packed, ops.pack_features(got))
    want = R.fpn_full64(stages, sd)[0]
    lat, e = None, None
    for i in range(3, -1, -1):
        w, b = sd[f"lateral_convs.{i}.conv.weight"], sd[f"lateral_convs.{i}.conv.bias"]
        own = R.conv64(stages[i], w, b)
        ei = R.CUT * R.mag64(stages[i], w)
        if lat is None:
            lat, e = own, ei + _ulp(own)
        else:
            lat = own + R.gather_nearest(lat, own.shape[2:])
            e = ei + R.gather_nearest(e, own.shape[2:]) + _ulp(own) + _ulp(lat)
    w3 = sd["fpn_convs.0.conv.weight"]
    torch.testing.assert_close(R.conv64(lat, w3, sd["fpn_convs.0.conv.bias"], padding=1), want, rtol=0, atol=1e-12)
    bound = R.CUT * R.mag64(lat, w3, padding=1) + R.conv64(e, w3.abs(), padding=1) + _ulp(want)
    _within("chain", got.cpu(), want, bound)
    # the torch route on the device: the same function
    fpn.route = "torch"
    with torch.no_grad():
        _within("torch route", fpn(dev_stages).cpu(), want, bound)


def test_chain_sees_an_in_place_weight_update(gpu):
    """weight.data.mul_(2) on the output convolution: the next call's result minus bias doubles exactly (the bf16 pieces, every product
    and every fp32 partial sum double).  The output bias is zero here: fl(2 a + b) is not 2 fl(a + b) - b in float32."""
    from mvsdet_amd.fpn import FPNLevel0
    sd = R.make_params(CH, COUT, seed=71)
    sd["fpn_convs.0.conv.bias"] = torch.zeros(COUT)
    stages = [s.to(gpu) for s in R.make_stages(2, CH, PYRAMIDS["odd"], seed=72)]
    fpn = FPNLevel0.from_state_dict(sd, prefix="", route="hip").to(gpu)
    with torch.no_grad():
        first = fpn(stages)
        fpn.out_weight.data.mul_(2)
        second = fpn(stages)
        assert float(first.abs().max()) > 0 and torch.equal(second, 2 * first)
        fpn.out_weight.mul_(0.5)                                  # ... and an update that bumps `_version` as well
        assert torch.equal(fpn(stages), first)


def test_route_hip_raises_where_it_cannot_run(gpu):
    from mvsdet_amd.fpn import FPNLevel0
    sd = R.make_params(CH, COUT, seed=81)
    stages = [s.to(gpu) for s in R.make_stages(1, CH, PYRAMIDS["halved"], seed=82)]
    fpn = FPNLevel0.from_state_dict(sd, prefix="", route="hip").to(gpu)
    with pytest.raises(RuntimeError, match="requires grad"):
        fpn(stages)                                               # autograd on, trainable parameters
    fpn.route = "auto"
    y = fpn(stages)                                               # ... which the torch route takes
    assert y.requires_grad
    with torch.no_grad():
        fpn.route = "hip"
        with pytest.raises(TypeError, match="float32"):
            fpn([s.half() for s in stages])


def test_hot_path_from_stages(gpu, monkeypatch):
    """forward_scene_from_stages sweeps the packed maps the 3x3 kernel wrote: no pack_features launch, the same variance, volume and
    valid as forward_scene on the module's feature map."""
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.fpn import FPNLevel0
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, D, hw = 3, 4, (12, 16)
    sd = R.make_params(CH, COUT, seed=91)
    stages = [s.to(gpu) for s in R.make_stages(N, CH, PYRAMIDS["halved"], seed=92)]
    hp = MVSDetHotPath([8, 8, 4], [0.4, 0.4, 0.4], [0.2, 5.0], D)
    hp.fpn = FPNLevel0.from_state_dict(sd, prefix="", route="hip").to(gpu)
    meta = synthetic.make_img_meta(N, hw, seed=9)
    logits = synthetic.make_cost_logits(N, D, hw, seed=9).to(gpu)
    calls = []
    real = ops.pack_features
    monkeypatch.setattr(ops, "pack_features", lambda feat: (calls.append(tuple(feat.shape)), real(feat))[1])
    with torch.no_grad():
        a = hp.forward_scene_from_stages(stages, meta, cost_logits=logits)
        assert calls == []
        feature = hp.fpn(stages)
        b = hp.forward_scene(feature, meta, cost_logits=logits)
        assert calls == [(N, COUT, 12, 16)]
    torch.cuda.synchronize()
    assert torch.equal(a["feature"], feature)
    for key in ("variance", "volume", "valid"):
        assert torch.equal(a[key], b[key]), key
    assert float(a["variance"].abs().max()) > 0 and int(a["valid"].sum()) > 0
