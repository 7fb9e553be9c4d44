"""The FPN's gradients on HIP (csrc/fpn_bwd.hip): the weight-gradient kernel in both forms, the top-down adjoint, the bias sum, the two
input gradients on the forward kernels, their memory edges, the module's chain under `autograd_route="hip"` against float64 autograd
of the restated FPN (tests/fpn_grad_restated.py) and the hot path's entry from grad-carrying stages.

The bounds are the project's (tests/fpn_restated.py), per element with mag = the same sum over absolute values in float64:
    |kernel - float64|                            <= CUT mag = 3 2^-16 mag    in every case
    |kernel - float64 sum of the three products|  <= ACC mag = 4e-7 mag       where the reduction has at most 2304 terms (the longest the
                                                                              bound has been shown at); printed, not asserted, beyond
The float64 references are torch's CPU autograd, computed once per case."""
import pytest
import torch
import torch.nn.functional as F

import fpn_grad_restated as G
import fpn_restated as R
from canvas import guarded_f32, ok

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 2, 16     # the weight gradient's pixel tile: kDwTH x kDwTW of csrc/fpn_bwd.hip (ops.fpn.DW_TILE)
SPLIT_BLOCKS = 512         # kDwSplitBlocks (ops.fpn.DW_SPLIT_BLOCKS)
ACC_TERMS = 2304           # the longest reduction ACC has been shown at: the forward 3x3's 9 x 256
# at Cout = C = 256 a split is 16 blocks, so K is cut into up to 32 runs of tiles: 5 x 7 = 35 tiles are 17 runs of 2 and a ragged 1
MULTI_SPLIT = (1, 5 * TILE_H, 7 * TILE_W)


def _within(name, got, want, bound, check=True):
    err = (got.double().cpu() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |error| / bound = {ratio:.3e}, max |error| = {float(err.max()):.3e}")
    if check:
        assert bool((err <= bound).all()), f"{name}: max |error| / bound = {ratio}"
    return ratio


def _pair(N, cout, C, H, W, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, cout, H, W, generator=g).to(gpu), torch.randn(N, C, H, W, generator=g).to(gpu)


def _check_dw(got, gy, x, taps):
    terms = gy.shape[0] * gy.shape[2] * gy.shape[3]
    mag = G.mag_dw64(gy, x, taps)
    _within(f"three-term ({terms} terms)", got, G.three_term_dw64(gy, x, taps), R.ACC * mag, check=terms <= ACC_TERMS)
    _within("float64", got, G.dw64(gy, x, taps), R.CUT * mag)


def test_constants_are_the_kernels(gpu):
    """The exported tile and split constants against the kernel's own plan: the multi-split case is what its name says."""
    from mvsdet_amd import _lib, ops
    assert ops.fpn.DW_TILE == (TILE_H, TILE_W) and ops.fpn.DW_SPLIT_BLOCKS == SPLIT_BLOCKS
    N, H, W = MULTI_SPLIT
    tiles, per, nsplit = ops.fpn.weight_grad_plan(9, N, 256, 256, H, W)
    assert (tiles, per, nsplit) == (35, 2, 18) and tiles % per != 0
    assert _lib.load().mvsdet_fpn_dw_splits(9, N, 256, 256, H, W) == nsplit
    # one tile is one run; one pixel more on each axis is four tiles
    assert ops.fpn.weight_grad_plan(9, 1, 256, 256, TILE_H, TILE_W)[0] == 1
    assert ops.fpn.weight_grad_plan(9, 1, 256, 256, TILE_H + 1, TILE_W + 1)[0] == 4


@pytest.mark.parametrize("N,C,cout,H,W", [(1, 256, 256, 1, 1), (1, 256, 256, 3, 3), (2, 256, 256, 5, 7), (1, 256, 256, TILE_H, TILE_W),
                                          (1, 256, 256, TILE_H + 1, TILE_W + 1), (1, 256, 256, 9, 33), (1, 256, 256, 60, 80),
                                          (MULTI_SPLIT[0], 256, 256) + MULTI_SPLIT[1:], (1, 32, 128, 9, 33)])
def test_weight_grad_nine_taps(gpu, N, C, cout, H, W):
    """Border taps and tile edges: maps smaller than the tile, the tile itself, one pixel more on each axis, several ragged tiles, a
    whole 60 x 80 view, at least two K splits with a ragged last one, the smallest channel counts the rule allows."""
    from mvsdet_amd import ops
    gy, x = _pair(N, cout, C, H, W, 500 + H * W + C, gpu)
    got = ops.fpn.weight_grad(gy, x, 9)
    assert got.shape == (cout, C, 3, 3)
    assert torch.equal(got, ops.fpn.weight_grad(gy, x, 9))              # the same bits on every run, split K included
    _check_dw(got, gy, x, 9)
    if (H, W) == (1, 1):                                                # only the centre tap sees the one pixel
        off = got.clone()
        off[:, :, 1, 1] = 0
        assert float(off.abs().max()) == 0.0 and float(got[:, :, 1, 1].abs().max()) > 0


@pytest.mark.parametrize("N,C,H,W", [(2, 256, 5, 7), (1, 512, 8, 10), (3, 1024, 15, 20), (1, 2048, 1, 1)])
def test_weight_grad_one_tap(gpu, N, C, H, W):
    """Column tails of 35, 80 and 900 pixels (the last: views that end inside a tile), one pixel."""
    from mvsdet_amd import ops
    gy, x = _pair(N, 256, C, H, W, 600 + C, gpu)
    got = ops.fpn.weight_grad(gy, x, 1)
    assert got.shape == (256, C, 1, 1)
    assert torch.equal(got, ops.fpn.weight_grad(gy, x, 1))
    _check_dw(got, gy, x, 1)


@pytest.mark.parametrize("N,H,W", [(2, 5, 7), (1, TILE_H + 1, TILE_W + 1), (1, 1, 4)])
def test_weight_grad_counts_every_tap_once(gpu, N, H, W):
    """g = 1, x = 1: dW[o,c,dy,dx] = N max(0, H - |dy-1|) max(0, W - |dx-1|) exactly -- small integers, so a missing or doubled border
    column shows as a whole count."""
    from mvsdet_amd import ops
    got = ops.fpn.weight_grad(torch.ones(N, 256, H, W, device=gpu), torch.ones(N, 256, H, W, device=gpu), 9).cpu()
    want = torch.tensor([[float(N * max(0, H - abs(dy - 1)) * max(0, W - abs(dx - 1))) for dx in range(3)] for dy in range(3)])
    assert torch.equal(got, want.expand(256, 256, 3, 3))
    one = ops.fpn.weight_grad(torch.ones(N, 128, H, W, device=gpu), torch.ones(N, 32, H, W, device=gpu), 1).cpu()
    assert torch.equal(one, torch.full((128, 32, 1, 1), float(N * H * W)))


@pytest.mark.parametrize("H,W,Ht,Wt", [(15, 20, 8, 10), (7, 5, 4, 3), (60, 80, 30, 40), (44, 46, 26, 14), (82, 3, 2, 1), (3, 3, 1, 1), (4, 4, 4, 4)])
def test_top_down_grad(gpu, H, W, Ht, Wt):
    """Integer-valued g (every sum exact): ATen's backward of the nearest gather bit for bit.  Random g: within n 2^-24 sum|g| of float64,
    n the size of the pre-image."""
    from mvsdet_amd import ops
    gen = torch.Generator().manual_seed(H * W + Ht)
    g = torch.randint(-8, 9, (2, 128, H, W), generator=gen).float()
    got = ops.fpn.top_down_grad(g.to(gpu), (Ht, Wt))
    assert got.shape == (2, 128, Ht, Wt) and torch.equal(got.cpu(), G.up_t(g, (Ht, Wt)))
    g = torch.randn(2, 128, H, W, generator=gen)
    got = ops.fpn.top_down_grad(g.to(gpu), (Ht, Wt))
    assert torch.equal(got, ops.fpn.top_down_grad(g.to(gpu), (Ht, Wt)))
    bound = G.preimage_size((H, W), (Ht, Wt)) * 2.0 ** -24 * G.up_t64(g.abs(), (Ht, Wt))
    _within("adjoint", got, G.up_t64(g, (Ht, Wt)), bound)


@pytest.mark.parametrize("N,C,H,W", [(2, 256, 5, 7), (1, 512, 8, 10)])
def test_input_grads(gpu, N, C, H, W):
    from mvsdet_amd import ops
    gen = torch.Generator().manual_seed(700 + C)
    g = torch.randn(N, 256, H, W, generator=gen).to(gpu)
    for k in (1, 3):
        w = (torch.randn(256, C, k, k, generator=gen) / (k * k * 256) ** 0.5).to(gpu)
        got = ops.fpn.lateral_input_grad(g, w) if k == 1 else ops.fpn.conv3x3_input_grad(g, w)
        assert got.shape == (N, C, H, W)
        mag = G.mag_dx64(g, w)
        _within(f"{k}x{k} three-term", got, G.three_term_dx64(g, w), R.ACC * mag)
        _within(f"{k}x{k} float64", got, G.dx64(g, w), R.CUT * mag)


@pytest.mark.parametrize("N,C,H,W", [(2, 256, 5, 7), (1, 512, 8, 10), (3, 128, 15, 20), (1, 256, 60, 80), (2, 64, 1, 1)])
def test_bias_grad(gpu, N, C, H, W):
    from mvsdet_amd import ops
    g = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(800 + C)).to(gpu)
    got = ops.fpn.bias_grad(g)
    assert got.shape == (C,) and torch.equal(got, ops.fpn.bias_grad(g))
    g64 = g.double().cpu()
    _within("bias", got, g64.sum((0, 2, 3)), N * H * W * 2.0 ** -24 * g64.abs().sum((0, 2, 3)))


def _in_nan_canvas(t, gpu):
    """t as a contiguous tensor in the middle of a NaN canvas: a stray read comes back as NaN."""
    pad = 4096
    canvas = torch.full((pad + t.numel() + pad,), float("nan"), dtype=torch.float32, device=gpu)
    view = canvas[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return canvas, view


def test_memory_edges(gpu):
    """Every output and the workspace inside guarded canvases pre-filled with NaN, every input inside a NaN canvas: the guards stay
    intact, no NaN is left (every element written, nothing read from outside an input) and the result is the unguarded call's."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    nan = float("nan")
    # nine taps at (2,256,5,7)
    gy, x = _pair(2, 256, 256, 5, 7, 901, gpu)
    want = ops.fpn.weight_grad(gy, x, 9)
    keep = [_in_nan_canvas(t, gpu) for t in (gy, x)]
    nbytes = lib.mvsdet_fpn_dw_workspace_bytes(9, 2, 256, 256, 5, 7)
    assert nbytes == lib.mvsdet_fpn_dw_splits(9, 2, 256, 256, 5, 7) * 9 * 256 * 256 * 4
    gd, dw = guarded_f32((256, 256, 3, 3), gpu)
    gw, ws = guarded_f32((nbytes // 4,), gpu)
    dw.fill_(nan)
    ws.fill_(nan)
    ok(lib.mvsdet_fpn_dw_bf16x3(_lib.ptr(keep[0][1]), _lib.ptr(keep[1][1]), gd.ptr(), gw.ptr(), nbytes, 9, 2, 256, 256, 5, 7, None))
    assert gd.guards_intact() and gw.guards_intact()
    assert not bool(torch.isnan(dw).any()) and not bool(torch.isnan(ws).any()) and torch.equal(dw, want)
    # the adjoint at (5,7) <- (3,4), and the bias sum of the same map
    g = torch.randn(2, 128, 5, 7, generator=torch.Generator().manual_seed(902)).to(gpu)
    want = ops.fpn.top_down_grad(g, (3, 4))
    want_b = ops.fpn.bias_grad(g)
    canvas, gv = _in_nan_canvas(g, gpu)
    gt, out = guarded_f32((2, 128, 3, 4), gpu)
    gb, db = guarded_f32((128,), gpu)
    out.fill_(nan)
    db.fill_(nan)
    ok(lib.mvsdet_fpn_top_down_grad_f32(_lib.ptr(gv), gt.ptr(), 2, 128, 5, 7, 3, 4, None))
    ok(lib.mvsdet_fpn_bias_grad_f32(_lib.ptr(gv), gb.ptr(), 2, 128, 5, 7, None))
    assert gt.guards_intact() and gb.guards_intact()
    assert not bool(torch.isnan(out).any()) and torch.equal(out, want)
    assert not bool(torch.isnan(db).any()) and torch.equal(db, want_b)


CH, COUT = (128, 128, 256, 128), 128
PYRAMIDS = {"halved": [(12, 16), (6, 8), (3, 4), (2, 2)], "odd": [(15, 20), (8, 10), (4, 5), (2, 3)]}


def _module(gpu, seed, channels=CH, **kw):
    from mvsdet_amd.fpn import FPNLevel0
    sd = R.make_params(channels, COUT, seed=seed)
    return sd, FPNLevel0.from_state_dict(sd, prefix="", **kw).to(gpu)


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_chain_against_float64_autograd(gpu, name):
    """Gradients of sum(out * R) with respect to the four stages and the ten parameters on the HIP autograd route against float64
    autograd of the restated level 0, the bound propagated down the chain (fpn_grad_restated.chain_bounds64)."""
    sd, fpn = _module(gpu, 61, route="hip", autograd_route="hip")
    stages = R.make_stages(2, CH, PYRAMIDS[name], seed=62)
    r = torch.randn(2, COUT, *PYRAMIDS[name][0], generator=torch.Generator().manual_seed(63))
    xs = [s.to(gpu).requires_grad_(True) for s in stages]
    out = fpn(xs)                                                   # route "hip" under autograd: no longer raises
    assert out.requires_grad
    with torch.no_grad():
        assert torch.equal(out, fpn(xs))                            # the forward is the no_grad HIP forward, bit for bit
    (out * r.to(gpu)).sum().backward()
    want_x, want_p = G.chain_grads64(stages, sd, r)
    bound_x, bound_p = G.chain_bounds64(stages, sd, r)
    for i in range(4):
        _within(f"d stage {i}", xs[i].grad, want_x[i], bound_x[i])
    got_p = {f"lateral_convs.{i}.conv.weight": fpn.lateral_weights[i].grad for i in range(4)}
    got_p.update({f"lateral_convs.{i}.conv.bias": fpn.lateral_biases[i].grad for i in range(4)})
    got_p.update({"fpn_convs.0.conv.weight": fpn.out_weight.grad, "fpn_convs.0.conv.bias": fpn.out_bias.grad})
    assert sorted(got_p) == sorted(want_p)
    for k in sorted(want_p):
        assert got_p[k].shape == want_p[k].shape, k
        _within("d " + k, got_p[k], want_p[k], bound_p[k])
    # the packed form: the packed maps still come from the 3x3 epilogue, the gradients are the same bits
    from mvsdet_amd import ops
    xs2 = [s.to(gpu).requires_grad_(True) for s in stages]
    out2, packed = fpn(xs2, packed=True)
    assert torch.equal(out2, out) and not packed.requires_grad and torch.equal(packed, ops.pack_features(out2.detach()))
    gx = torch.autograd.grad((out2 * r.to(gpu)).sum(), xs2)
    assert all(torch.equal(a, b.grad) for a, b in zip(gx, xs))


def test_routes(gpu):
    sd, fpn = _module(gpu, 81, route="hip", autograd_route="hip")
    stages = [s.to(gpu) for s in R.make_stages(1, CH, PYRAMIDS["halved"], seed=82)]
    y = fpn(stages)                                                   # trainable parameters, route "hip": runs under autograd
    assert y.requires_grad and type(y.grad_fn).__name__.startswith("_Level0Function")
    # frozen parameters and stages get no gradient
    fpn.lateral_weights[1].requires_grad_(False)
    fpn.lateral_biases[2].requires_grad_(False)
    fpn.out_weight.requires_grad_(False)
    xs = [s.clone().requires_grad_(i != 2) for i, s in enumerate(stages)]
    fpn(xs).sum().backward()
    assert fpn.lateral_weights[1].grad is None and fpn.lateral_biases[2].grad is None and fpn.out_weight.grad is None
    assert xs[2].grad is None and all(xs[i].grad is not None for i in (0, 1, 3))
    assert fpn.lateral_weights[0].grad is not None and fpn.lateral_biases[3].grad is not None and fpn.out_bias.grad is not None
    # only the output convolution trains: nothing below it is computed, nothing else gets a gradient
    for p in fpn.parameters():
        p.requires_grad_(False)
        p.grad = None
    fpn.out_weight.requires_grad_(True)
    fpn(stages).sum().backward()
    assert fpn.out_weight.grad is not None and all(p.grad is None for p in fpn.parameters() if p is not fpn.out_weight)
    # a stage with 96 channels: the forward runs, the autograd route refuses by name, nothing falls back
    sd96, fpn96 = _module(gpu, 83, channels=(96, 128, 256, 128), route="auto", autograd_route="hip")
    st96 = [s.to(gpu) for s in R.make_stages(1, (96, 128, 256, 128), PYRAMIDS["halved"], seed=84)]
    with torch.no_grad():
        assert fpn96(st96).shape == (1, COUT, 12, 16)
    with pytest.raises(ValueError, match="stage 0 has 96 channels, not divisible by 128"):
        fpn96(st96)
    # the default module behaves as before
    _, plain = _module(gpu, 81, route="hip")
    assert plain.autograd_route == "torch"
    with pytest.raises(RuntimeError, match="requires grad"):
        plain(stages)
    plain.route = "auto"
    y = plain(stages)
    assert y.requires_grad and not type(y.grad_fn).__name__.startswith("_Level0Function")
    with torch.no_grad():
        plain.route = "hip"
        with pytest.raises(TypeError, match="float32"):
            plain([s.half() for s in stages])


def test_hot_path_from_stages_under_grad(gpu):
    """forward_scene_from_stages with grad-carrying stages: the same variance, volume and valid as the no_grad call, and stage gradients
    that are the pyramid's backward of the gradient forward_scene gives the feature map."""
    from mvsdet_amd import synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, D, hw = 3, 4, (12, 16)
    _, fpn = _module(gpu, 91, route="hip", autograd_route="hip")
    for p in fpn.parameters():
        p.requires_grad_(False)
    stages = [s.to(gpu) for s in R.make_stages(N, CH, PYRAMIDS["halved"], seed=92)]
    hp = MVSDetHotPath([8, 8, 4], [0.4, 0.4, 0.4], [0.2, 5.0], D)
    hp.fpn = fpn
    meta = synthetic.make_img_meta(N, hw, seed=9)
    logits = synthetic.make_cost_logits(N, D, hw, seed=9).to(gpu)
    with torch.no_grad():
        a = hp.forward_scene_from_stages(stages, meta, cost_logits=logits)
    xs = [s.clone().requires_grad_(True) for s in stages]
    b = hp.forward_scene_from_stages(xs, meta, cost_logits=logits)
    for key in ("variance", "volume", "valid"):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["feature"], b["feature"]) and b["feature"].requires_grad
    got = torch.autograd.grad(b["volume"].sum(), xs)
    # the same gradient in two steps: forward_scene's to a detached leaf copy of the feature, then the pyramid's backward of it
    xs2 = [s.clone().requires_grad_(True) for s in stages]
    feature = fpn(xs2)
    leaf = feature.detach().clone().requires_grad_(True)
    c = hp.forward_scene(leaf, meta, cost_logits=logits)
    gf, = torch.autograd.grad(c["volume"].sum(), leaf)
    assert float(gf.abs().max()) > 0
    want = torch.autograd.grad(feature, xs2, grad_outputs=gf)
    for i in range(4):
        assert torch.equal(got[i], want[i]), i
    assert float(got[3].abs().max()) > 0
