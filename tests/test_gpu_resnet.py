"""The ResNet stages on HIP (csrc/resnet.hip): the 1x1 and the 3x3 kernel of stride 1 and 2 alone, their exact gathers, ReLU's NaN
rule, their memory edges and host refusals, one bottleneck and whole nets against the float64 restatement of the backbone
(tests/resnet_restated.py), the module's derived tensors and routes, and the hot path's entry from the images.

The bounds are the project's (tests/fpn_restated.py), applied per element with mag = conv(|x|, |w'|) + |shift| + |residual| in
float64, w' the folded fp32 weight:
    |kernel - three-term restatement| <= 4e-7 mag      fp32 accumulation of exact products, the epilogue's additions
    |kernel - float64|                <= 3 2^-16 mag   the dropped terms, worst case
ReLU is 1-Lipschitz: both hold behind it.  A chain's bound is propagated layer by layer (`resnet_restated.chain_bounds64`).  The
float64 references are computed once per case, on the device.

Worst |error| / bound measured on MI355X: see DESIGN 4.22."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fpn_restated as FR
import resnet_restated as R
from canvas import guarded_f32, ok

pytestmark = pytest.mark.gpu

TILE = {1: (8, 16), 2: (4, 16)}     # OUTPUT pixels of the 3x3 kernel's tile per stride (ops.resnet.CONV3X3_TILE, CONV3X3_S2_TILE)


def _within(name, got, want, bound):
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |error| / bound = {ratio:.3e}, max |error| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{name}: max |error| / bound = {ratio}"


def _case(N, Cin, Cout, H, W, k, stride, seed, gpu, residual=False):
    """x, the folded matrix, its split, the folded weight as (Cout,Cin,k,k), shift, residual."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).to(gpu)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5).to(gpu)
    scale = (0.5 + torch.rand(Cout, generator=g)).to(gpu)
    shift = (torch.randn(Cout, generator=g) * 0.1).to(gpu)
    res = torch.randn(N, Cout, R.out_size(H, stride), R.out_size(W, stride), generator=g).to(gpu) if residual else None
    wmat = ops.resnet.fold(w, scale)
    assert wmat.shape == (-(-Cout // 128) * 128, k * k * Cin)
    assert torch.equal(wmat[:Cout], (w * scale.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(Cout, -1))   # the same bits, restated
    return x, ops.gemm_split_weight(wmat), R.unfold_matrix(wmat, Cout, k), shift, res


def _check_alone(name, got, x, wf, shift, res, stride, padding, relu):
    mag = R.mag64(x, wf, shift, res, stride, padding)
    add = shift.double().view(1, -1, 1, 1) + (0 if res is None else res.double())
    act = torch.relu if relu else (lambda t: t)
    _within(f"{name} three-term", got, act(R.three_term_conv64(x, wf, stride, padding) + add), FR.ACC * mag)
    _within(f"{name} float64", got, act(R.conv64(x, wf, stride, padding) + add), FR.CUT * mag)


def test_tile_constants_are_the_kernels():
    from mvsdet_amd import ops
    assert ops.resnet.CONV3X3_TILE == TILE[1] and ops.resnet.CONV3X3_S2_TILE == TILE[2]


@pytest.mark.parametrize("N,Cin,Cout,H,W,stride,residual", [
    (2, 64, 64, 5, 7, 1, False),          # masked half block, 70 columns
    (1, 256, 64, 8, 10, 1, False),
    (1, 32, 96, 3, 3, 1, False),          # Cout % 128 == 96
    (2, 256, 512, 5, 7, 2, False),        # output 3x4
    (3, 1024, 2048, 1, 1, 2, False),
    (1, 512, 128, 15, 20, 1, False),
    (2, 128, 512, 4, 6, 1, True)])
def test_conv1x1_alone(gpu, N, Cin, Cout, H, W, stride, residual):
    from mvsdet_amd import ops
    x, wq, wf, shift, res = _case(N, Cin, Cout, H, W, 1, stride, 1000 + Cin + Cout + H, gpu, residual)
    for relu in (True, False):
        got = ops.resnet.conv1x1(x, wq, shift, Cout, stride=stride, residual=res, relu=relu)
        assert got.shape == (N, Cout, R.out_size(H, stride), R.out_size(W, stride))
        _check_alone(f"1x1 relu={relu}", got, x, wf, shift, res, stride, 0, relu)
        assert bool((got < 0).any()) != relu


@pytest.mark.parametrize("H,W", [(5, 7), (15, 20)])
def test_conv1x1_picks_the_strided_pixel(gpu, H, W):
    """W' = the identity, shift = 0, integer x below 2^16 (exact in two bf16 pieces): the output IS x[:, :, ::2, ::2]."""
    from mvsdet_amd import ops
    x = torch.randint(0, 1 << 16, (2, 128, H, W), generator=torch.Generator().manual_seed(H)).float().to(gpu)
    wq = ops.gemm_split_weight(torch.eye(128, device=gpu))
    zero = torch.zeros(128, device=gpu)
    assert torch.equal(ops.resnet.conv1x1(x, wq, zero, 128, stride=2, relu=False), x[:, :, ::2, ::2])
    assert torch.equal(ops.resnet.conv1x1(x, wq, zero, 128, stride=1, relu=True), x)


def _conv3x3_sizes(stride):
    th, tw = TILE[stride]
    return [(1, 64, 64, 1, 1), (1, 64, 64, 2, 2), (1, 64, 64, 3, 3), (2, 128, 128, 5, 7), (1, 64, 64, 9, 33), (1, 128, 128, 15, 20),
            (1, 64, 64, 17, 35), (1, 64, 64, stride * th, stride * tw), (1, 64, 64, stride * th + 1, stride * tw + 1)]


@pytest.mark.parametrize("stride,N,Cin,Cout,H,W", [(s,) + c for s in (1, 2) for c in _conv3x3_sizes(s)])
def test_conv3x3_alone(gpu, stride, N, Cin, Cout, H, W):
    """Border taps and tile edges: maps smaller than the tile, the tile in input pixels, one pixel more in each axis, several tiles
    with ragged edges; Cout = 64: half of the block's rows are padding."""
    from mvsdet_amd import ops
    x, wq, wf, shift, _ = _case(N, Cin, Cout, H, W, 3, stride, 3000 + 97 * H + W + stride, gpu)
    for relu in (True, False):
        got = ops.resnet.conv3x3(x, wq, shift, Cout, stride=stride, relu=relu)
        assert got.shape == (N, Cout, R.out_size(H, stride), R.out_size(W, stride))
        _check_alone(f"3x3 s{stride} relu={relu}", got, x, wf, shift, None, stride, 1, relu)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_counts_every_tap_once(gpu, stride):
    """x = 1, w = 2^-12, no shift, no ReLU: every quantity is a power of two times a small integer, so the output equals F.conv2d's
    exactly and a missing or doubled border tap shows as a whole tap (64 2^-12 = 1/64)."""
    from mvsdet_amd import ops
    th, tw = TILE[stride]
    w = torch.full((64, 64, 3, 3), 2.0 ** -12)
    wq = ops.gemm_split_weight(ops.resnet.fold(w.to(gpu), torch.ones(64, device=gpu)))
    for H, W in [(2, 2), (5, 7), (15, 20), (stride * th + 1, stride * tw + 1)]:
        x = torch.ones(1, 64, H, W)
        got = ops.resnet.conv3x3(x.to(gpu), wq, torch.zeros(64, device=gpu), 64, stride=stride, relu=False).cpu()
        want = F.conv2d(x, w, stride=stride, padding=1)
        assert float(want[0, 0, 0, 0]) == 4 / 64.0
        assert torch.equal(got, want), (H, W)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", [(5, 7), (16, 20)])
def test_conv3x3_reads_the_right_pixel(gpu, stride, H, W):
    """The weight that is the channel identity at ONE tap, integer x: the output IS the shifted, strided, zero-padded x."""
    from mvsdet_amd import ops
    x = torch.randint(1, 1 << 16, (2, 64, H, W), generator=torch.Generator().manual_seed(H + stride)).float().to(gpu)
    xp = F.pad(x, (1, 1, 1, 1))
    ho, wo = R.out_size(H, stride), R.out_size(W, stride)
    one, zero = torch.ones(64, device=gpu), torch.zeros(64, device=gpu)
    for dy in range(3):
        for dx in range(3):
            w = torch.zeros(64, 64, 3, 3, device=gpu)
            w[:, :, dy, dx] = torch.eye(64, device=gpu)
            got = ops.resnet.conv3x3(x, ops.gemm_split_weight(ops.resnet.fold(w, one)), zero, 64, stride=stride, relu=False)
            want = xp[:, :, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride]
            assert torch.equal(got, want), (dy, dx)


def _one_block(stride, downsample, gpu, seed=41, route="hip"):
    """A net of one bottleneck, C = 128, p = 32: (module on the device, state-dict on the device)."""
    from mvsdet_amd.resnet import ResNetStages
    sd = R.make_params((32,), (1,), seed, stem=128)
    if not downsample:
        sd = {k: v for k, v in sd.items() if ".downsample." not in k}
    sd = {k: v.to(gpu) for k, v in sd.items()}
    return ResNetStages.from_state_dict(sd, prefix="", route=route, strides=(stride,)), sd


def test_relu_keeps_a_nan(gpu):
    """One NaN, then one -inf, planted in x: the NaN mask and the zeros of the output are the torch route's, the other view stays
    finite, and a kernel that wrote fmaxf(v, 0) would turn the planted NaN into zeros."""
    mod, _ = _one_block(2, True, gpu)
    x = torch.randn(2, 128, 7, 9, generator=torch.Generator().manual_seed(42)).to(gpu)
    with torch.no_grad():
        clean = mod.forward_from_stem(x)[0]
        assert bool(torch.isfinite(clean).all())
        for bad in (float("nan"), float("-inf")):
            xb = x.clone()
            xb[0, 3, 2, 2] = bad
            mod.route = "hip"
            got = mod.forward_from_stem(xb)[0]
            mod.route = "torch"
            want = mod.forward_from_stem(xb)[0]
            assert bool(torch.isnan(got).any()) and torch.equal(torch.isnan(got), torch.isnan(want))
            assert torch.equal(got == 0, want == 0)
            assert torch.equal(torch.isfinite(got), torch.isfinite(want))
            assert bool(torch.isfinite(got[1]).all()) and torch.equal(got[1], clean[1])
            assert bool(torch.isnan(got[0, :, 1, 1]).all())                  # every channel of the pixel that reads (2, 2)
            assert bool(torch.isfinite(got[0, :, 3, 4]).all())                # ... and none two output pixels away


def _in_nan_canvas(t, gpu):
    """t as a contiguous tensor in the middle of a NaN canvas: a stray read comes back as NaN."""
    pad = 4096
    canvas = torch.full((pad + t.numel() + pad,), float("nan"), dtype=torch.float32, device=gpu)
    view = canvas[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return canvas, view


def test_memory_edges(gpu):
    """Every output inside a guarded canvas, every input inside a NaN canvas: nothing outside the outputs changes, every output element
    is written (pre-filled with NaN, none left), no value read from outside an input reaches an output, and the padding rows 64..127
    of the matrix write nothing (they would land in the next view or in the guard)."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    nan = float("nan")
    # 1x1 stride 2 with residual: (2,256,5,7) -> (2,64,3,4)
    x, wq, wf, shift, res = _case(2, 256, 64, 5, 7, 1, 2, 51, gpu, residual=True)
    want = ops.resnet.conv1x1(x, wq, shift, 64, stride=2, residual=res, relu=True)
    _check_alone("1x1 edges", want, x, wf, shift, res, 2, 0, True)
    keep = [_in_nan_canvas(t, gpu) for t in (x, shift, res)]
    g, out = guarded_f32((2, 64, 3, 4), gpu)
    out.fill_(nan)
    ok(lib.mvsdet_resnet_conv1x1_bf16x3(_lib.ptr(keep[0][1]), _lib.ptr(wq), _lib.ptr(keep[1][1]), _lib.ptr(keep[2][1]), g.ptr(), 2, 256, 64, 5,
                                        7, 2, 1, None))
    assert g.guards_intact() and not bool(torch.isnan(out).any()) and torch.equal(out, want)
    # 3x3 stride 2 at (2,64,9,17) -> (2,64,5,9); stride 1 at (1,64,9,17)
    for N, stride in ((2, 2), (1, 1)):
        x, wq, wf, shift, _ = _case(N, 64, 64, 9, 17, 3, stride, 53 + stride, gpu)
        want = ops.resnet.conv3x3(x, wq, shift, 64, stride=stride, relu=False)
        _check_alone(f"3x3 s{stride} edges", want, x, wf, shift, None, stride, 1, False)
        keep = [_in_nan_canvas(t, gpu) for t in (x, shift)]
        g, out = guarded_f32(tuple(want.shape), gpu)
        out.fill_(nan)
        ok(lib.mvsdet_resnet_conv3x3_bf16x3(_lib.ptr(keep[0][1]), _lib.ptr(wq), _lib.ptr(keep[1][1]), g.ptr(), N, 64, 64, 9, 17, stride, 0, None))
        assert g.guards_intact() and not bool(torch.isnan(out).any()) and torch.equal(out, want)


def test_host_refusals_through_the_c_entry(gpu):
    """Each rule returns nonzero with a message before any launch: NULL stream, outputs poisoned beforehand stay as they were."""
    from mvsdet_amd import _lib
    lib = _lib.load()
    out = torch.full((4096,), 7.0, device=gpu)
    buf = torch.zeros(4096, device=gpu)
    p, o = buf.data_ptr(), out.data_ptr()
    vp = ctypes.c_void_p

    def c1(x=p, ws=p, sh=p, res=None, out=o, N=1, Cin=32, Cout=32, H=2, W=2, stride=1):
        return lib.mvsdet_resnet_conv1x1_bf16x3(vp(x), vp(ws), vp(sh), vp(res) if res else None, vp(out), N, Cin, Cout, H, W, stride, 1, None)

    def c3(x=p, ws=p, sh=p, out=o, N=1, Cin=32, Cout=32, H=2, W=2, stride=1):
        return lib.mvsdet_resnet_conv3x3_bf16x3(vp(x), vp(ws), vp(sh), vp(out), N, Cin, Cout, H, W, stride, 1, None)

    def refused(rc, word):
        assert rc != 0 and word.encode() in lib.mvsdet_last_error(), (rc, word, lib.mvsdet_last_error())

    for f in (c1, c3):
        refused(f(x=None), "NULL")
        refused(f(ws=None), "NULL")
        refused(f(sh=None), "NULL")
        refused(f(out=None), "NULL")
        refused(f(N=0), "bad shape")
        refused(f(H=0), "bad shape")
        refused(f(W=-1), "bad shape")
        refused(f(stride=3), "stride")
        refused(f(stride=0), "stride")
        refused(f(Cin=48), "Cin=48")
        refused(f(Cin=0), "Cin=0")
        refused(f(Cout=80), "Cout=80")
        refused(f(N=1 << 15, H=1 << 8, W=1 << 8), "2^31" if f is c1 else "too large")
        refused(f(H=1 << 16, W=1 << 15), "too large")
        refused(f(ws=p + 4), "aligned")
        refused(f(x=p + 2), "aligned")
        refused(f(out=o + 1), "aligned")
        refused(f(sh=p + 2), "aligned")
    refused(c1(res=p + 2), "aligned")
    refused(c3(N=65536), "bad shape")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("stride,downsample", [(1, True), (2, True), (1, False), (2, False)])
def test_one_bottleneck(gpu, stride, downsample):
    """C = 128, p = 32, N = 2, a 7 x 9 map.  The fourth variant -- stride 2 with the identity as the residual -- is no block of the
    definition (the sum's operands differ in size): the module refuses to build it."""
    if stride == 2 and not downsample:
        with pytest.raises(ValueError, match="downsample"):
            _one_block(stride, downsample, gpu)
        return
    mod, sd = _one_block(stride, downsample, gpu)
    x = torch.randn(2, 128, 7, 9, generator=torch.Generator().manual_seed(43)).to(gpu)
    with torch.no_grad():
        got = mod.forward_from_stem(x)[0]
    want, bound = R.bottleneck_bounds64(x, sd, "layer1.0", stride)
    assert torch.equal(want, R.bottleneck64(x, sd, "layer1.0", stride))
    assert got.shape == (2, 128, R.out_size(7, stride), R.out_size(9, stride))
    _within(f"bottleneck s{stride} down={downsample}", got, want, bound)


NETS = {"narrow": ((32, 64, 128, 256), (1, 2, 1, 1), (3, 50, 70)), "resnet50": ((64, 128, 256, 512), (3, 4, 6, 3), (3, 32, 48))}


@pytest.mark.parametrize("name", sorted(NETS))
def test_stages(gpu, name):
    """Each of C2..C5 within the propagated bound of the float64 restatement; the torch route on the device is the same function."""
    from mvsdet_amd.resnet import ResNetStages
    planes, depths, shape = NETS[name]
    sd = {k: v.to(gpu) for k, v in R.make_params(planes, depths, seed=61).items()}
    img = torch.randn(2, *shape, generator=torch.Generator().manual_seed(62)).to(gpu)
    mod = ResNetStages.from_state_dict(sd, prefix="", route="hip")
    with torch.no_grad():
        got = mod(img)
        assert all(torch.equal(a, b) for a, b in zip(got, mod(img)))          # the same bits on every run
        mod.route = "torch"
        torch_route = mod(img)
    refs = R.chain_bounds64(img, sd)
    if name == "narrow":
        assert [tuple(t.shape[2:]) for t in got] == [(13, 18), (7, 9), (4, 5), (2, 3)]
    else:
        assert [tuple(t.shape[1:]) for t in got] == [(256, 8, 12), (512, 4, 6), (1024, 2, 3), (2048, 1, 2)]
    for i, (g, t, (want, bound)) in enumerate(zip(got, torch_route, refs)):
        assert float(want.abs().max()) > 0.1
        _within(f"{name} C{i + 2}", g, want, bound)
        _within(f"{name} C{i + 2} torch route", t, want, bound)


def test_views_do_not_see_each_other(gpu):
    """The HIP route on a batch with its views permuted gives each view the same bits."""
    from mvsdet_amd.resnet import ResNetStages
    sd = {k: v.to(gpu) for k, v in R.make_params((32, 64, 128, 256), (1, 2, 1, 1), seed=71).items()}
    mod = ResNetStages.from_state_dict(sd, prefix="", route="hip")
    s = torch.randn(5, 64, 13, 18, generator=torch.Generator().manual_seed(72)).to(gpu)
    perm = torch.tensor([3, 0, 4, 1, 2], device=gpu)
    with torch.no_grad():
        a, b = mod.forward_from_stem(s), mod.forward_from_stem(s[perm].contiguous())
    for x, y in zip(a, b):
        assert torch.equal(x[perm], y)


def test_derived_tensors_follow_the_parameters(gpu):
    """An in-place update that moves `_version` is seen by the next call; one through `.data` after `drop_derived_tensors`."""
    from mvsdet_amd.layers import drop_derived_tensors
    from mvsdet_amd.resnet import ResNetStages
    net, _ = R.stand_in((32, 64), (1, 1), seed=81)
    net.to(gpu)
    mod = ResNetStages.from_module(net, route="hip")
    s = torch.randn(2, 64, 6, 5, generator=torch.Generator().manual_seed(82)).to(gpu)

    def fresh():
        """A module of its own, built from copies of the parameters as they are now."""
        with torch.no_grad():
            return ResNetStages.from_state_dict(net.state_dict(), prefix="", route="hip").forward_from_stem(s)[1]

    conv, bn = net.layer2[0].conv2, net.layer1[0].bn3
    with torch.no_grad():
        first = mod.forward_from_stem(s)[1]
        assert torch.equal(first, fresh())
        kept = conv.__dict__["_mvs_wmat"][1]
        assert mod.forward_from_stem(s)[1] is not None and conv.__dict__["_mvs_wmat"][1] is kept   # not cut again
        conv.weight.mul_(2)
        second = mod.forward_from_stem(s)[1]
        assert not torch.equal(second, first) and torch.equal(second, fresh())
        bn.running_var.mul_(2)
        third = mod.forward_from_stem(s)[1]
        assert not torch.equal(third, second) and torch.equal(third, fresh())
        conv.weight.data.mul_(0.5)                                            # `_version` stays: the kept pieces are stale
        assert torch.equal(mod.forward_from_stem(s)[1], third)
        drop_derived_tensors(mod)
        fourth = mod.forward_from_stem(s)[1]
        assert not torch.equal(fourth, third) and torch.equal(fourth, fresh())


def test_routes(gpu):
    from mvsdet_amd.resnet import ResNetStages
    net, _ = R.stand_in((32, 64), (1, 1), seed=91)
    net.to(gpu)
    mod = ResNetStages.from_module(net, route="auto")
    img = torch.randn(1, 3, 20, 24, generator=torch.Generator().manual_seed(92)).to(gpu)
    for p in net.parameters():
        p.requires_grad_(False)
    assert mod.resolve_route(img) in ("hip", "torch")
    from mvsdet_amd import resnet as M
    assert mod.resolve_route(img) == M.AUTO_ON_CUDA                           # nothing requires grad: the measured choice
    x = img.clone().requires_grad_(True)
    assert mod.resolve_route(x) == "torch"
    out = mod(x)
    out[1].sum().backward()
    assert float(x.grad.abs().max()) > 0
    mod.route = "hip"
    with pytest.raises(RuntimeError, match="requires grad"):
        mod(x)
    with torch.no_grad():
        assert mod.resolve_route(x) == "hip"                                  # autograd off: the HIP route runs
        hip = mod(x)
    assert not hip[0].requires_grad and float((hip[1] - out[1].detach()).abs().max()) < 1e-3 * float(out[1].detach().abs().max())
    net.layer2[0].bn2.train()
    with pytest.raises(ValueError, match="norm_eval"):
        mod(img)
    mod.route = "torch"
    with pytest.raises(ValueError, match="norm_eval"):
        mod(img)


def test_hot_path_from_images(gpu):
    """forward_scene_from_images is forward_scene_from_stages behind the backbone: the same variance, volume and valid, bit for bit."""
    from mvsdet_amd import synthetic
    from mvsdet_amd.fpn import FPNLevel0
    from mvsdet_amd.hotpath import MVSDetHotPath
    from mvsdet_amd.resnet import ResNetStages
    N, D, hw = 3, 4, (12, 16)
    sd = {k: v.to(gpu) for k, v in R.make_params((32, 64, 128, 256), (1, 1, 1, 1), seed=101).items()}
    img = torch.randn(N, 3, 48, 64, generator=torch.Generator().manual_seed(102)).to(gpu)
    hp = MVSDetHotPath([8, 8, 4], [0.4, 0.4, 0.4], [0.2, 5.0], D)
    hp.fpn = FPNLevel0.from_state_dict(FR.make_params((128, 256, 512, 1024), 128, seed=103), prefix="", route="hip").to(gpu)
    meta = synthetic.make_img_meta(N, hw, seed=9)
    logits = synthetic.make_cost_logits(N, D, hw, seed=9).to(gpu)
    with torch.no_grad():
        with pytest.raises(ValueError, match="backbone"):
            hp.forward_scene_from_images(img, meta, cost_logits=logits)
        hp.backbone = ResNetStages.from_state_dict(sd, prefix="", route="hip")
        a = hp.forward_scene_from_images(img, meta, cost_logits=logits)
        stages = hp.backbone(img)
        b = hp.forward_scene_from_stages(stages, meta, cost_logits=logits)
    torch.cuda.synchronize()
    assert [tuple(s.shape[1:]) for s in a["stages"]] == [(128, 12, 16), (256, 6, 8), (512, 3, 4), (1024, 2, 2)]
    assert all(torch.equal(x, y) for x, y in zip(a["stages"], stages))
    for key in ("feature", "variance", "volume", "valid"):
        assert torch.equal(a[key], b[key]), key
    assert float(a["variance"].abs().max()) > 0 and int(a["valid"].sum()) > 0
