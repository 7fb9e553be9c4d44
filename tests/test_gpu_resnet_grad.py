"""The ResNet stages' backward on HIP (csrc/resnet_bwd.hip): the 1x1 and 3x3 input gradients with their gates and residuals, the stride-2
weight gradient, their memory edges and host refusals, one bottleneck and a narrow net under `autograd_route="hip"` against the float64
restatement with the HIP forward's own activations imposed as gates (tests/resnet_grad_restated.py), and the hot path from the images.

The bounds are the project's (tests/fpn_restated.py), per element with mag = the same sum over absolute values in float64:
    |kernel - three-term restatement| <= 4e-7 mag      asserted where the reduction has at most 2304 terms, printed beyond
    |kernel - float64|                <= 3 2^-16 mag   the dropped terms, worst case
A gate passes the bound where it passes the value.  A chain's bound is propagated (`resnet_grad_restated.block_backward64`).

Worst |error| / bound measured on MI355X: see DESIGN 4.23."""
import ctypes

import pytest
import torch

import fpn_restated as FR
import resnet_grad_restated as G
import resnet_restated as R
from canvas import guarded_f32, ok

pytestmark = pytest.mark.gpu

MAPS = [(1, 1), (2, 3), (5, 7), (6, 8), (17, 35)]


def _within(name, got, want, bound, asserted=True):
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |error| / bound = {ratio:.3e}, max |error| = {float(err.max()):.3e}{'' if asserted else ' (printed only)'}")
    if asserted:
        assert bool((err <= bound).all()), f"{name}: max |error| / bound = {ratio}"


def _weights(cout, c, k, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, c, k, k, generator=g) / (k * k * c) ** 0.5).to(gpu)
    scale = (0.5 + torch.rand(cout, generator=g)).to(gpu)
    return w, scale, (w * scale.view(-1, 1, 1, 1))


def _rand(shape, seed, gpu):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(gpu)


def _gate_map(shape, seed, gpu):
    """A saved ReLU output: about half zeros, the rest positive."""
    return torch.relu(_rand(shape, seed, gpu))


# ------------------------------------------------------------------------------------------------- 1x1 input gradient
@pytest.mark.parametrize("C,H,W", [(64, 5, 7), (160, 9, 13), (64, 6, 8)])
def test_conv1x1_input_grad(gpu, C, H, W):
    """Rows 64 (the zero-padding path) and 160, K = 128, columns no multiple of 64; with and without the residual, the spread residual at an
    odd and an even size, with and without the gate."""
    from mvsdet_amd import ops
    N, K = 2, 128
    w, scale, wf = _weights(K, C, 1, 100 + C + H, gpu)
    g = _rand((N, K, H, W), 200 + H, gpu)
    gate = _gate_map((N, C, H, W), 300 + H, gpu)
    full = _rand((N, C, H, W), 400 + H, gpu)
    half = _rand((N, C, G.out_size(H, 2), G.out_size(W, 2)), 500 + H, gpu)
    base, three, mag = G.conv_dx64(g, wf, 1, (H, W)), G.three_term_dx64(g, wf, 1, (H, W)), G.conv_dx64(g.abs(), wf.abs(), 1, (H, W))
    for kind, res, spread in (("none", None, 1), ("full", full, 1), ("spread", half, 2)):
        add = 0 if res is None else G.spread64(res.double(), spread, (H, W))
        m = mag + (0 if res is None else add.abs())
        for gated in (False, True):
            got = ops.resnet.conv1x1_input_grad(g, w, scale, gate=gate if gated else None, residual=res, spread=spread)
            assert got.shape == (N, C, H, W)
            fin = (lambda t: G.gate64(t, gate.double())) if gated else (lambda t: t)
            _within(f"dx1x1 {kind} gate={gated} three-term", got, fin(three + add), FR.ACC * m)
            _within(f"dx1x1 {kind} gate={gated} float64", got, fin(base + add), FR.CUT * m)
            if gated:
                assert bool((got[gate <= 0] == 0).all()) and float(got[gate > 0].abs().max()) > 0


def test_conv1x1_input_grad_gate_table(gpu):
    """The gate map planted with 0.0, -0.0, NaN, inf and negatives: +0.0 where the host table drops the gradient, the ungated result's bits
    where it passes (NaN and inf in the map pass)."""
    from mvsdet_amd import ops
    N, C, K, H, W = 2, 64, 128, 5, 7
    w, scale, _ = _weights(K, C, 1, 7, gpu)
    g = _rand((N, K, H, W), 8, gpu)
    res = _rand((N, C, H, W), 9, gpu)
    gate = _rand((N, C, H, W), 10, gpu)                       # negatives and positives
    flat = gate.view(-1)
    planted = torch.tensor([0.0, -0.0, float("nan"), float("inf"), -1.5, float("-inf")], device=gpu)
    flat[:600] = planted.repeat(100)
    plain = ops.resnet.conv1x1_input_grad(g, w, scale, residual=res)
    got = ops.resnet.conv1x1_input_grad(g, w, scale, gate=gate, residual=res)
    want = G.gate64(plain, gate)                                # the host table, pinned against ATen in test_resnet_grad_host.py
    drop = gate <= 0
    assert int(drop.sum()) > 400 and int(torch.isnan(gate).sum()) == 100
    assert torch.equal(got, want) and not bool(torch.isnan(got).any())
    assert not bool(torch.signbit(got[drop]).any()) and bool((got[drop] == 0).all())
    assert torch.equal(got[~drop], plain[~drop]) and torch.equal(got.view(-1)[2:600:6], plain.view(-1)[2:600:6])   # under the NaNs
    alone = ops.resnet.relu_gate(plain, gate)
    assert torch.equal(alone, want) and not bool(torch.signbit(alone[drop]).any())
    nan_g = plain.clone()
    nan_g.view(-1)[:6] = float("nan")
    assert torch.equal(torch.isnan(ops.resnet.relu_gate(nan_g, gate)).view(-1)[:6].cpu(), torch.tensor([False, False, True, True, False, False]))


# ------------------------------------------------------------------------------------------------- 3x3 input gradient
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,K", [(32, 32), (96, 64)])
@pytest.mark.parametrize("H,W", MAPS)
def test_conv3x3_input_grad_integers(gpu, stride, C, K, H, W):
    """Integer-valued gb and weights (exact in one bf16 piece, sums far below 2^24): bit-exact against the float64 sum that the host loops
    pin, so every parity class and every border tap count is counted exactly once.  K = 64 is two K steps per tap: the stride-2 fetch's
    split of a step into (tap, channels) is pinned exactly, not only within a bound."""
    from mvsdet_amd import ops
    N = 2
    gen = torch.Generator().manual_seed(17 * H + W + stride + K)
    gb = torch.randint(-4, 5, (N, K, G.out_size(H, stride), G.out_size(W, stride)), generator=gen).float().to(gpu)
    w = torch.randint(-3, 4, (K, C, 3, 3), generator=gen).float().to(gpu)
    one = torch.ones(K, device=gpu)
    got = ops.resnet.conv3x3_input_grad(gb, w, one, (H, W), stride)
    want = G.conv_dx64(gb, w, stride, (H, W))
    assert got.shape == (N, C, H, W) and float(want.abs().max()) > 0
    assert torch.equal(got.double(), want)
    if stride == 2 and H <= 6:
        loops, _ = G.convT3x3_s2_loops(gb.cpu(), w.cpu(), H, W)
        assert torch.equal(got.double().cpu(), loops)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,H,W", [(96, 5, 7), (96, 6, 8), (32, 17, 35), (96, 17, 35), (96, 1, 1), (32, 2, 3)])
def test_conv3x3_input_grad(gpu, stride, C, H, W):
    from mvsdet_amd import ops
    N, K = 2, 64
    w, scale, wf = _weights(K, C, 3, 600 + C + H + stride, gpu)
    gb = _rand((N, K, G.out_size(H, stride), G.out_size(W, stride)), 700 + H, gpu)
    gate = _gate_map((N, C, H, W), 800 + H, gpu)
    mag = G.conv_dx64(gb.abs(), wf.abs(), stride, (H, W))
    for gated in (False, True):
        got = ops.resnet.conv3x3_input_grad(gb, w, scale, (H, W), stride, gate=gate if gated else None)
        fin = (lambda t: G.gate64(t, gate.double())) if gated else (lambda t: t)
        _within(f"dx3x3 s{stride} gate={gated} three-term", got, fin(G.three_term_dx64(gb, wf, stride, (H, W))), FR.ACC * mag)
        _within(f"dx3x3 s{stride} gate={gated} float64", got, fin(G.conv_dx64(gb, wf, stride, (H, W))), FR.CUT * mag)
        if gated:
            assert bool((got[gate <= 0] == 0).all())


# ------------------------------------------------------------------------------------------------- stride-2 weight gradient
@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("C,H,W", [(32, 1, 1), (64, 2, 3), (32, 5, 7), (64, 6, 8), (32, 17, 35), (64, 17, 35)])
def test_weight_grad_stride2(gpu, taps, C, H, W):
    """gy = 1, x = 1 gives the exact tap counts; random operands go against both bounds (the reduction is N Ho Wo <= 486 terms)."""
    from mvsdet_amd import ops
    N, cout, k = 3, 128, 3 if taps == 9 else 1
    ho, wo = G.out_size(H, 2), G.out_size(W, 2)
    ones = ops.resnet.weight_grad(torch.ones(N, cout, ho, wo, device=gpu), torch.ones(N, C, H, W, device=gpu), taps, 2)
    counts = G.conv_dw64(torch.ones(N, cout, ho, wo), torch.ones(N, C, H, W), k, 2)
    assert ones.shape == (cout, C, k, k) and torch.equal(ones.double().cpu(), counts)
    assert float(counts[0, 0, k // 2, k // 2]) == N * ho * wo
    gy, x = _rand((N, cout, ho, wo), 900 + H + taps, gpu), _rand((N, C, H, W), 950 + H, gpu)
    got = ops.resnet.weight_grad(gy, x, taps, 2)
    mag = G.conv_dw64(gy.abs(), x.abs(), k, 2)
    assert N * ho * wo <= 2304
    _within(f"dw s2 taps={taps} three-term", got, G.three_term_dw64(gy, x, k, 2), FR.ACC * mag)
    _within(f"dw s2 taps={taps} float64", got, G.conv_dw64(gy, x, k, 2), FR.CUT * mag)
    assert torch.equal(got, ops.resnet.weight_grad(gy, x, taps, 2))


@pytest.mark.parametrize("taps", [1, 9])
def test_weight_grad_stride2_split_plan(gpu, taps):
    """A shape with more than one split: the query, the plan restated in Python, the same bits on two runs, and stride 1 is ops.fpn's."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    N, C, cout, H, W = 3, 32, 128, 17, 35
    tiles, per, splits = ops.resnet.weight_grad_plan(taps, N, C, cout, H, W)
    assert (tiles, splits) == (30, 30) and splits > 1
    assert lib.mvsdet_resnet_dw_s2_splits(taps, N, C, cout, H, W) == splits
    assert lib.mvsdet_resnet_dw_s2_workspace_bytes(taps, N, C, cout, H, W) == splits * taps * cout * C * 4
    for shape in [(40, 256, 512, 60, 80), (2, 64, 128, 9, 11), (1, 32, 128, 1, 1)]:
        assert lib.mvsdet_resnet_dw_s2_splits(taps, *shape) == ops.resnet.weight_grad_plan(taps, *shape)[2]
    assert lib.mvsdet_resnet_dw_s2_splits(taps, N, 48, cout, H, W) == 0 and b"C=48" in lib.mvsdet_last_error()
    gy, x = _rand((N, cout, 9, 18), 31, gpu), _rand((N, C, H, W), 32, gpu)
    assert torch.equal(ops.resnet.weight_grad(gy, x, taps, 2), ops.resnet.weight_grad(gy, x, taps, 2))
    # several tiles per split (the next tile fetched under this tile's products): 30 tiles in 15 splits
    N2, C2, cout2 = 3, 256, 512
    assert ops.resnet.weight_grad_plan(taps, N2, C2, cout2, H, W) == (30, 2, 15)
    gy2, x2 = _rand((N2, cout2, 9, 18), 34, gpu), _rand((N2, C2, H, W), 35, gpu)
    k = 3 if taps == 9 else 1
    mag = G.conv_dw64(gy2.abs(), x2.abs(), k, 2)
    got2 = ops.resnet.weight_grad(gy2, x2, taps, 2)
    _within(f"dw s2 taps={taps} two tiles a split, three-term", got2, G.three_term_dw64(gy2, x2, k, 2), FR.ACC * mag)
    _within(f"dw s2 taps={taps} two tiles a split, float64", got2, G.conv_dw64(gy2, x2, k, 2), FR.CUT * mag)
    x1 = _rand((N, C, 9, 18), 33, gpu)
    assert torch.equal(ops.resnet.weight_grad(gy, x1, taps, 1), ops.fpn.weight_grad(gy, x1, taps))


# ------------------------------------------------------------------------------------------------- memory edges, host refusals
def _in_nan_canvas(t, gpu):
    pad = 4096
    canvas = torch.full((pad + t.numel() + pad,), float("nan"), dtype=torch.float32, device=gpu)
    view = canvas[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return canvas, view


def test_memory_edges(gpu):
    """Every new entry once with its inputs inside NaN canvases and its output between guards: the guards stay, every output element is
    written, no NaN from outside an input reaches an output, and the padding rows of the matrices write nothing."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    nan = float("nan")
    N, C, K, H, W = 2, 64, 128, 5, 7
    # 1x1 input gradient with the spread residual and the gate
    w, scale, _ = _weights(K, C, 1, 41, gpu)
    g, gate, half = _rand((N, K, H, W), 42, gpu), _gate_map((N, C, H, W), 43, gpu), _rand((N, C, 3, 4), 44, gpu)
    want = ops.resnet.conv1x1_input_grad(g, w, scale, gate=gate, residual=half, spread=2)
    wq = ops.gemm_split_weight(ops.resnet.transposed_matrix(w, scale))
    keep = [_in_nan_canvas(t, gpu) for t in (g, half, gate)]
    guard, out = guarded_f32((N, C, H, W), gpu)
    out.fill_(nan)
    ok(lib.mvsdet_resnet_conv1x1_dx_bf16x3(_lib.ptr(keep[0][1]), _lib.ptr(wq), _lib.ptr(keep[1][1]), _lib.ptr(keep[2][1]), guard.ptr(), N, C, K,
                                           H, W, 2, None))
    assert guard.guards_intact() and not bool(torch.isnan(out).any()) and torch.equal(out, want)
    # the gate alone
    guard, out = guarded_f32((N, C, H, W), gpu)
    out.fill_(nan)
    ok(lib.mvsdet_resnet_relu_gate_f32(_lib.ptr(keep[2][1]), _lib.ptr(keep[2][1]), guard.ptr(), gate.numel(), None))
    assert guard.guards_intact() and torch.equal(out, gate)
    # 3x3 input gradients at (6, 8) and (9, 17): even and odd sizes, two tiles
    for stride, (H, W) in ((1, (9, 17)), (2, (6, 8)), (2, (9, 17))):
        w, scale, _ = _weights(K, C, 3, 45 + stride, gpu)
        gb, gate = _rand((N, K, G.out_size(H, stride), G.out_size(W, stride)), 46, gpu), _gate_map((N, C, H, W), 47, gpu)
        want = ops.resnet.conv3x3_input_grad(gb, w, scale, (H, W), stride, gate=gate)
        mats = [ops.resnet.flipped_matrix(w, scale)] if stride == 1 else ops.resnet.class_matrices(w, scale)
        wq = torch.cat([ops.gemm_split_weight(m) for m in mats])
        keep = [_in_nan_canvas(t, gpu) for t in (gb, gate)]
        guard, out = guarded_f32((N, C, H, W), gpu)
        out.fill_(nan)
        ok(lib.mvsdet_resnet_conv3x3_dx_bf16x3(_lib.ptr(keep[0][1]), _lib.ptr(wq), _lib.ptr(keep[1][1]), guard.ptr(), N, C, K, H, W, stride, None))
        assert guard.guards_intact() and not bool(torch.isnan(out).any()) and torch.equal(out, want), (stride, H, W)
    # stride-2 weight gradients: dw and the workspace between guards
    for taps in (1, 9):
        N, C, cout, H, W = 3, 32, 128, 6, 35
        gy, x = _rand((N, cout, 3, 18), 48, gpu), _rand((N, C, H, W), 49, gpu)
        want = ops.resnet.weight_grad(gy, x, taps, 2)
        keep = [_in_nan_canvas(t, gpu) for t in (gy, x)]
        nbytes = lib.mvsdet_resnet_dw_s2_workspace_bytes(taps, N, C, cout, H, W)
        gw, ws = guarded_f32((nbytes // 4,), gpu)
        guard, out = guarded_f32(tuple(want.shape), gpu)
        out.fill_(nan)
        ok(lib.mvsdet_resnet_dw_s2_bf16x3(_lib.ptr(keep[0][1]), _lib.ptr(keep[1][1]), guard.ptr(), gw.ptr(), nbytes, taps, N, C, cout, H, W, None))
        assert guard.guards_intact() and gw.guards_intact() and not bool(torch.isnan(out).any()) and torch.equal(out, want), taps
        assert not bool(torch.isnan(ws).any())


def test_host_refusals_through_the_c_entries(gpu):
    """Each rule returns nonzero with a message before any launch: outputs poisoned beforehand stay as they were."""
    from mvsdet_amd import _lib
    lib = _lib.load()
    out = torch.full((1 << 16,), 7.0, device=gpu)
    buf = torch.zeros(1 << 16, device=gpu)
    p, o = buf.data_ptr(), out.data_ptr()
    vp = ctypes.c_void_p

    def opt(a):
        return vp(a) if a else None

    def d1(g=p, ws=p, res=None, gate=None, out=o, N=1, C=32, Cout=32, H=2, W=2, spread=1):
        return lib.mvsdet_resnet_conv1x1_dx_bf16x3(opt(g), opt(ws), opt(res), opt(gate), opt(out), N, C, Cout, H, W, spread, None)

    def d3(g=p, ws=p, gate=None, out=o, N=1, C=32, Cout=32, H=2, W=2, stride=1):
        return lib.mvsdet_resnet_conv3x3_dx_bf16x3(opt(g), opt(ws), opt(gate), opt(out), N, C, Cout, H, W, stride, None)

    def dw(gy=p, x=p, dw=o, ws=p, nbytes=1 << 18, taps=1, N=1, C=32, Cout=128, H=2, W=2):
        return lib.mvsdet_resnet_dw_s2_bf16x3(opt(gy), opt(x), opt(dw), opt(ws), nbytes, taps, N, C, Cout, H, W, None)

    def refused(rc, word, code=None):
        assert rc != 0 and word.encode() in lib.mvsdet_last_error(), (rc, word, lib.mvsdet_last_error())
        assert code is None or rc == code

    for f in (d1, d3):
        refused(f(g=None), "NULL")
        refused(f(ws=None), "NULL")
        refused(f(out=None), "NULL")
        refused(f(N=0), "bad shape")
        refused(f(H=0), "bad shape")
        refused(f(W=-1), "bad shape")
        refused(f(C=48), "C=48")
        refused(f(C=0), "C=0")
        refused(f(Cout=80), "Cout=80")
        refused(f(H=1 << 16, W=1 << 15), "too large")
        refused(f(ws=p + 4), "aligned")
        refused(f(g=p + 2), "aligned")
        refused(f(out=o + 1), "aligned")
        refused(f(gate=p + 2), "aligned")
    refused(d1(spread=3), "stride")
    refused(d1(spread=0), "stride")
    refused(d1(res=p + 2), "aligned")
    refused(d1(N=1 << 15, H=1 << 8, W=1 << 8), "2^31")
    refused(d3(stride=3), "stride")
    refused(d3(stride=0), "stride")
    refused(d3(N=65536), "bad shape")
    refused(d3(N=1 << 15, H=1 << 8, W=1 << 8), "too large")
    for kw in (dict(gy=None), dict(x=None), dict(dw=None), dict(ws=None)):
        refused(dw(**kw), "NULL")
    refused(dw(taps=3), "taps=3")
    refused(dw(N=0), "bad shape")
    refused(dw(N=65536), "bad shape")
    refused(dw(H=0), "bad shape")
    refused(dw(C=48), "C=48")
    refused(dw(Cout=64), "Cout=64")
    refused(dw(H=1 << 16, W=1 << 15), "too large")
    refused(dw(N=1 << 15, H=1 << 9, W=1 << 9), "2^31")
    refused(dw(gy=p + 2), "aligned")
    refused(dw(ws=p + 1), "aligned")
    refused(dw(nbytes=128 * 32 * 4 - 4), "workspace", code=2)
    refused(lib.mvsdet_resnet_relu_gate_f32(None, vp(p), vp(o), 4, None), "NULL")
    refused(lib.mvsdet_resnet_relu_gate_f32(vp(p), vp(p), vp(o), 0, None), "total")
    refused(lib.mvsdet_resnet_relu_gate_f32(vp(p), vp(p + 2), vp(o), 4, None), "aligned")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------- the module
def _one_block(stride, downsample, gpu, seed=41):
    """A net of one bottleneck of planes 128 on 256 channels (the identity block: 512)."""
    from mvsdet_amd.resnet import ResNetStages
    sd = R.make_params((128,), (1,), seed, stem=256 if downsample else 512)
    if not downsample:
        sd = {k: v for k, v in sd.items() if ".downsample." not in k}
    sd = {k: v.to(gpu) for k, v in sd.items()}
    mod = ResNetStages.from_state_dict(sd, prefix="", route="hip", strides=(stride,), autograd_route="hip").freeze_(frozen_stages=0)
    return mod, sd


def _conv_weights(blk):
    return [blk.conv1.weight, blk.conv2.weight, blk.conv3.weight] + ([blk.down_conv.weight] if blk.down_conv is not None else [])


KEYS = ["x", "conv1", "conv2", "conv3", "downsample"]


@pytest.mark.parametrize("stride,downsample", [(1, True), (2, True), (1, False)])
def test_one_bottleneck(gpu, stride, downsample):
    """dx and the three or four dW within the propagated bound of the gate-imposed restatement; the forward's bits are the no_grad route's;
    two backward passes give the same bits; needs_input_grad is honoured."""
    from mvsdet_amd.resnet import _block_hip
    mod, sd = _one_block(stride, downsample, gpu)
    blk = mod.layers[0][0]
    x = _rand((2, blk.cin, 9, 11), 43, gpu)
    with torch.no_grad():
        plain = mod.forward_from_stem(x)[0]
        out0, a, b = _block_hip(x, blk, want_inner=True)
    xg = x.clone().requires_grad_(True)
    out = mod.forward_from_stem(xg)[0]
    assert type(out.grad_fn).__name__.startswith("_BottleneckFunction")
    assert torch.equal(out, plain) and torch.equal(out0, plain)
    r = _rand(tuple(out.shape), 44, gpu)
    leaves = [xg] + _conv_weights(blk)
    got = torch.autograd.grad((out * r).sum(), leaves, retain_graph=True)
    again = torch.autograd.grad((out * r).sum(), leaves, retain_graph=True)
    assert all(torch.equal(p, q) for p, q in zip(got, again))
    grads, bounds = G.block_backward64(x, a, b, plain, r, sd, "layer1.0", stride)
    for key, t in zip(KEYS, got):
        assert float(grads[key].abs().max()) > 0
        _within(f"bottleneck s{stride} down={downsample} d{key}", t, grads[key], bounds[key])
    # only conv3's weight: the same bits, nothing else computed
    only, = torch.autograd.grad((out * r).sum(), [blk.conv3.weight], retain_graph=True)
    assert torch.equal(only, got[3])
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad((out * r).sum(), [xg], create_graph=True)


def _narrow(gpu, **kw):
    from mvsdet_amd.resnet import ResNetStages
    sd = {k: v.to(gpu) for k, v in R.make_params((32, 128, 128, 128), (1, 2, 1, 1), seed=61).items()}
    return ResNetStages.from_state_dict(sd, prefix="", route="hip", autograd_route="hip", **kw), sd


def test_narrow_net(gpu):
    """Planes (32,128,128,128), depths (1,2,1,1), freeze_(1), a 40 x 56 image: every trained weight's gradient of sum_k (C_k . R_k) against
    float64 with the HIP forward's activations imposed; layer 1 owns no autograd node; the forward's bits are the no_grad route's."""
    from mvsdet_amd.resnet import _block_hip
    mod, sd = _narrow(gpu)
    img = _rand((2, 3, 40, 56), 62, gpu)
    with pytest.raises(ValueError, match="norm_cfg"):
        mod(img)                                              # from_state_dict's BatchNorm parameters require grad
    mod.freeze_(frozen_stages=0)
    with pytest.raises(ValueError, match="frozen_stages"):
        mod(img)                                              # layer 1's conv1 has 32 rows
    mod.freeze_(1)
    with torch.no_grad():
        plain = mod(img)
        s = mod.stem(img)
        blocks = []
        for li, layer in enumerate(mod.layers):
            for bi, blk in enumerate(layer):
                out, a, b = _block_hip(s, blk, want_inner=True)
                if li > 0:
                    blocks.append((f"layer{li + 1}.{bi}", blk.stride, s, a, b, out, li if bi == len(layer) - 1 else None))
                s = out
    stages = mod(img)
    assert [tuple(t.shape[1:]) for t in stages] == [(128, 10, 14), (512, 5, 7), (512, 3, 4), (512, 2, 2)]
    assert all(torch.equal(p, q) for p, q in zip(stages, plain))
    assert stages[0].grad_fn is None and not stages[0].requires_grad          # layer 1: the plain forward, no node
    assert all(type(t.grad_fn).__name__.startswith("_BottleneckFunction") for t in stages[1:])
    Rs = [_rand(tuple(t.shape), 70 + k, gpu) for k, t in enumerate(stages)]
    named = [(f"layer{li + 1}.{bi}", key, w) for li, layer in enumerate(mod.layers) if li > 0 for bi, blk in enumerate(layer)
             for key, w in zip(KEYS[1:], _conv_weights(blk))]
    assert all(w.requires_grad for _, _, w in named) and len(named) == 3 * 4 + 3
    loss = sum((c * r).sum() for c, r in zip(stages, Rs))
    got = torch.autograd.grad(loss, [w for _, _, w in named], retain_graph=True)
    again = torch.autograd.grad(loss, [w for _, _, w in named])
    assert all(torch.equal(p, q) for p, q in zip(got, again))
    grads, bounds = G.net_backward64(blocks, Rs, sd)
    worst = 0.0
    for (name, key, _), t in zip(named, got):
        assert float(grads[name][key].abs().max()) > 0
        _within(f"narrow {name}.{key}", t, grads[name][key], bounds[name][key])
        worst = max(worst, float(((t.double() - grads[name][key]).abs() / bounds[name][key].clamp_min(1e-300)).max()))
    print(f"narrow net: worst |error| / bound over {len(named)} weights = {worst:.3e}")


def test_kept_pieces_follow_the_optimizer(gpu):
    """The forward's kept weight pieces are keyed by `_version`: an optimizer's in-place step moves it, so the next call cuts them again."""
    mod, _ = _one_block(1, True, gpu)
    blk = mod.layers[0][0]
    x = _rand((1, 256, 4, 5), 81, gpu)
    opt = torch.optim.SGD([p for p in mod.parameters() if p.requires_grad], lr=0.1)
    out = mod.forward_from_stem(x)[0]
    key, kept = blk.conv2.__dict__["_mvs_wmat"][:2]
    out.sum().backward()
    assert blk.conv2.weight.grad is not None and float(blk.conv2.weight.grad.abs().max()) > 0
    version = blk.conv2.weight._version
    opt.step()
    assert blk.conv2.weight._version > version
    out2 = mod.forward_from_stem(x)[0]
    key2, kept2 = blk.conv2.__dict__["_mvs_wmat"][:2]
    assert key2 != key and kept2 is not kept and not torch.equal(out2, out)
    with torch.no_grad():
        assert torch.equal(mod.forward_from_stem(x)[0], out2) and blk.conv2.__dict__["_mvs_wmat"][1] is kept2


def test_default_route_is_unchanged(gpu):
    """autograd_route defaults to "torch": a grad-enabled call with trainable weights takes torch's layers, route "hip" raises."""
    from mvsdet_amd.resnet import ResNetStages
    sd = {k: v.to(gpu) for k, v in R.make_params((128,), (1,), 41, stem=256).items()}
    mod = ResNetStages.from_state_dict(sd, prefix="", route="auto")
    x = _rand((1, 256, 4, 5), 82, gpu)
    assert mod.autograd_route == "torch" and mod.resolve_route(x) == "torch"
    assert not type(mod.forward_from_stem(x)[0].grad_fn).__name__.startswith("_BottleneckFunction")
    mod.route = "hip"
    with pytest.raises(RuntimeError, match="requires grad"):
        mod.forward_from_stem(x)


def test_hot_path_from_images_under_grad(gpu):
    """forward_scene_from_images with both modules on "hip": variance, volume and valid are the no_grad call's bits, and the backbone's
    weight gradients of volume.sum() are, bit for bit, the backbone's backward fed with the stage gradients that
    forward_scene_from_stages produces."""
    from mvsdet_amd import synthetic
    from mvsdet_amd.fpn import FPNLevel0
    from mvsdet_amd.hotpath import MVSDetHotPath
    from mvsdet_amd.resnet import ResNetStages
    N, D, hw = 3, 4, (12, 16)
    sd = {k: v.to(gpu) for k, v in R.make_params((32, 128, 128, 256), (1, 1, 1, 1), seed=101).items()}
    img = _rand((N, 3, 48, 64), 102, gpu)
    hp = MVSDetHotPath([8, 8, 4], [0.4, 0.4, 0.4], [0.2, 5.0], D)
    hp.fpn = FPNLevel0.from_state_dict(FR.make_params((128, 512, 512, 1024), 128, seed=103), prefix="", route="hip",
                                       autograd_route="hip").to(gpu)
    hp.backbone = ResNetStages.from_state_dict(sd, prefix="", route="hip", autograd_route="hip").freeze_(1)
    meta = synthetic.make_img_meta(N, hw, seed=9)
    logits = synthetic.make_cost_logits(N, D, hw, seed=9).to(gpu)
    with torch.no_grad():
        a = hp.forward_scene_from_images(img, meta, cost_logits=logits)
    b = hp.forward_scene_from_images(img, meta, cost_logits=logits)
    for key in ("variance", "volume", "valid"):
        assert torch.equal(a[key], b[key]), key
    assert all(torch.equal(p, q) for p, q in zip(a["stages"], b["stages"]))
    weights = [w for layer in list(hp.backbone.layers)[1:] for blk in layer for w in _conv_weights(blk)]
    assert len(weights) == 12 and all(w.requires_grad for w in weights)
    got = torch.autograd.grad(b["volume"].sum(), weights)
    # the same gradient in two steps: the scene's to detached leaf copies of the stages, then the backbone's backward of them
    stages = hp.backbone(img)
    leaves = [s.detach().clone().requires_grad_(True) for s in stages]
    c = hp.forward_scene_from_stages(leaves, meta, cost_logits=logits)
    gs = torch.autograd.grad(c["volume"].sum(), leaves)
    assert all(float(g.abs().max()) > 0 for g in gs[1:])
    want = torch.autograd.grad(stages[1:], weights, grad_outputs=gs[1:])
    for i, (p, q) in enumerate(zip(got, want)):
        assert torch.equal(p, q), i
    assert float(got[0].abs().max()) > 0 and float(got[-1].abs().max()) > 0
