"""What the ResNet stages' HIP backward rests on that needs no device: the float64 restatement (tests/resnet_grad_restated.py) against
torch's float64 autograd and against scalar loops, the gate table against ATen, every refusal of `ops.resnet.check_grad_shapes`, the
weight matrices of the input gradients, `freeze_` and the resolution of the routes."""
import pytest
import torch
import torch.nn.functional as F

import resnet_grad_restated as G
import resnet_restated as R


def _module(planes=(32,), depths=(1,), seed=5, stem=128, strides=(1,), downsample=True, **kw):
    from mvsdet_amd.resnet import ResNetStages
    sd = R.make_params(planes, depths, seed, stem=stem)
    if not downsample:
        sd = {k: v for k, v in sd.items() if ".downsample." not in k}
    return ResNetStages.from_state_dict(sd, prefix="", strides=strides, **kw), sd


@pytest.mark.parametrize("stride,downsample", [(1, True), (2, True), (1, False)])
def test_restatement_is_torchs_autograd(stride, downsample):
    """The chain with the gates imposed equals torch's float64 autograd of `_block_torch` where no pre-activation is near zero (so the
    float64 forward and the imposed gates agree): the smallest |pre-activation| is asserted."""
    from mvsdet_amd.resnet import _block_torch
    mod, sd = _module(strides=(stride,), downsample=downsample, route="torch")
    mod.double()
    blk = mod.layers[0][0]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 128, 5, 6, generator=g, dtype=torch.float64).requires_grad_(True)

    def conv_bn(t, conv, bn, s, p):
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        y = F.conv2d(t, conv.weight, None, s, p) * scale.view(1, -1, 1, 1) + (bn.bias - bn.running_mean * scale).view(1, -1, 1, 1)
        return y

    a_pre = conv_bn(x, blk.conv1, blk.bn1, 1, 0)
    a = torch.relu(a_pre)
    b_pre = conv_bn(a, blk.conv2, blk.bn2, stride, 1)
    b = torch.relu(b_pre)
    o_pre = conv_bn(b, blk.conv3, blk.bn3, 1, 0) + (x if blk.down_conv is None else conv_bn(x, blk.down_conv, blk.down_bn, stride, 0))
    out = torch.relu(o_pre)
    assert torch.equal(out, _block_torch(x, blk))
    smallest = min(float(t.detach().abs().min()) for t in (a_pre, b_pre, o_pre))
    assert smallest > 1e-9, smallest
    r = torch.randn(out.shape, generator=g, dtype=torch.float64)
    params = [blk.conv1.weight, blk.conv2.weight, blk.conv3.weight] + ([blk.down_conv.weight] if downsample else [])
    want = torch.autograd.grad((out * r).sum(), [x] + params)
    sd64 = {k: v.double() for k, v in mod.state_dict().items()}
    names = {"layers.0.0.conv1.": "b.conv1.", "layers.0.0.bn1.": "b.bn1.", "layers.0.0.conv2.": "b.conv2.", "layers.0.0.bn2.": "b.bn2.",
             "layers.0.0.conv3.": "b.conv3.", "layers.0.0.bn3.": "b.bn3.", "layers.0.0.down_conv.": "b.downsample.0.",
             "layers.0.0.down_bn.": "b.downsample.1."}
    sdb = {new + k[len(old):]: v for k, v in sd64.items() for old, new in names.items() if k.startswith(old)}

    # the restatement folds in float32; here every tensor is float64, so fold in float64 for an exact comparison
    def folded64(sdict, conv, bn):
        s = sdict[bn + ".weight"] / torch.sqrt(sdict[bn + ".running_var"] + G.EPS)
        return sdict[conv + ".weight"] * s.view(-1, 1, 1, 1), s

    old = G.folded
    G.folded = folded64
    try:
        grads, bounds = G.block_backward64(x.detach(), a.detach(), b.detach(), out.detach(), r, sdb, "b", stride)
    finally:
        G.folded = old
    keys = ["x", "conv1", "conv2", "conv3"] + (["downsample"] if downsample else [])
    for key, w in zip(keys, want):
        assert grads[key].shape == w.shape
        assert float((grads[key] - w).abs().max()) <= 1e-12 * float(w.abs().max()), key
        assert bool((bounds[key] >= 0).all())


def test_gate_table_is_atens():
    """The saved output holding 0.0, -0.0, a negative, a positive, NaN and inf: the rule `y <= 0 ? 0 : v` is what torch.relu's backward
    returns, for a NaN gradient as well (dropped with the rest where y <= 0)."""
    y = torch.tensor([0.0, -0.0, -1.5, 2.0, float("nan"), float("inf")])
    for v in (torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), torch.full((6,), float("nan")), torch.full((6,), float("-inf"))):
        want = torch.ops.aten.threshold_backward(v, y, 0)
        got = G.gate64(v, y)
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))
        assert torch.equal(torch.signbit(got[:3]), torch.zeros(3, dtype=torch.bool))      # the dropped gradient is +0.0
        assert [bool(t) for t in (got[:3] == 0)] == [True] * 3
    x = y.clone().requires_grad_(True)
    torch.relu(x).backward(torch.arange(1.0, 7.0))
    assert torch.equal(x.grad, torch.tensor([0.0, 0.0, 0.0, 4.0, 5.0, 6.0]))


@pytest.mark.parametrize("H,W", [(5, 7), (6, 8)])
def test_stride2_formulas_against_loops(H, W):
    g = torch.Generator().manual_seed(H)
    ho, wo = G.out_size(H, 2), G.out_size(W, 2)
    gb = torch.randn(2, 3, ho, wo, generator=g, dtype=torch.float64)
    w = torch.randn(3, 4, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(2, 4, H, W, generator=g, dtype=torch.float64)
    loops, taps = G.convT3x3_s2_loops(gb, w, H, W)
    assert float((G.conv_dx64(gb, w, 2, (H, W)) - loops).abs().max()) < 1e-12
    # 1, 2, 2 or 4 taps by parity class; in an even size the last (odd) row / column has no partner beyond it and keeps one tap
    ny = torch.tensor([1 if y % 2 == 0 else 1 + int((y + 1) // 2 < ho) for y in range(H)])
    nx = torch.tensor([1 if x % 2 == 0 else 1 + int((x + 1) // 2 < wo) for x in range(W)])
    assert torch.equal(taps, ny.view(-1, 1) * nx.view(1, -1))
    assert int(taps[0, 0]) == 1 and int(taps[1, 1]) == 4 and int(taps[1, 0]) == 2 and int(taps[H - 1, W - 1]) == 1
    xr = x.clone().requires_grad_(True)
    want_dx = torch.autograd.grad(F.conv2d(xr, w, stride=2, padding=1), xr, gb)[0]
    assert float((loops - want_dx).abs().max()) < 1e-12
    for k in (1, 3):
        wk = torch.zeros(3, 4, k, k, dtype=torch.float64, requires_grad=True)
        want = torch.autograd.grad(F.conv2d(x, wk, stride=2, padding=k // 2), wk, gb)[0]
        assert float((G.dw_s2_loops(gb, x, k) - want).abs().max()) < 1e-12
        assert float((G.conv_dw64(gb, x, k, 2) - want).abs().max()) < 1e-12
    assert float((G.conv_dw64(gb, x[:, :, :ho, :wo], 3, 1) - torch.autograd.grad(
        F.conv2d(x[:, :, :ho, :wo], wk, padding=1), wk, gb)[0]).abs().max()) < 1e-12


def test_class_matrices_are_the_parity_rule():
    """The four matrices of the stride-2 input gradient, multiplied out on the CPU by the kernel's rule (class pixel (i, j), tap shift
    [parity and first tap]), give the transposed convolution."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(3)
    w = torch.randn(32, 32, 3, 3, generator=g)
    scale = 0.5 + torch.rand(32, generator=g)
    mats = ops.resnet.class_matrices(w, scale)
    assert [tuple(m.shape) for m in mats] == [(128, 32), (128, 64), (128, 64), (128, 128)]
    assert all(float(m[32:].abs().max()) == 0 for m in mats)
    wf = (w * scale.view(-1, 1, 1, 1))
    for H, W in [(5, 7), (6, 8), (1, 1), (2, 3)]:
        ho, wo = G.out_size(H, 2), G.out_size(W, 2)
        gb = torch.randn(1, 32, ho, wo, generator=g)
        gp = F.pad(gb.double(), (0, 1, 0, 1))
        out = torch.zeros(1, 32, H, W, dtype=torch.float64)
        for py in (0, 1):
            for px in (0, 1):
                m = mats[2 * py + px][:32].double()
                t = 0
                for a, dy in enumerate(ops.resnet.parity_taps(py)):
                    for b, dx in enumerate(ops.resnet.parity_taps(px)):
                        sy, sx = int(py and a == 0), int(px and b == 0)
                        for i in range((H - py + 1) // 2):
                            for j in range((W - px + 1) // 2):
                                out[0, :, 2 * i + py, 2 * j + px] += m[:, 32 * t:32 * t + 32] @ gp[0, :, i + sy, j + sx]
                        t += 1
        assert float((out - G.conv_dx64(gb, wf, 2, (H, W))).abs().max()) < 1e-12, (H, W)
    t1 = ops.resnet.transposed_matrix(w[:, :, :1, :1], scale)
    assert tuple(t1.shape) == (128, 32) and torch.equal(t1[:32], wf[:, :, 0, 0].t())
    f1 = ops.resnet.flipped_matrix(w, scale)
    assert tuple(f1.shape) == (128, 288) and torch.equal(f1[:32].reshape(32, 3, 3, 32)[:, 0, 2, :], wf[:, :, 2, 0].t())


def test_check_grad_shapes_refusals():
    from mvsdet_amd import ops
    chk = ops.resnet.check_grad_shapes

    def ws(cin=128, p=128, cout=512, down=True):
        return (torch.zeros(p, cin, 1, 1), torch.zeros(p, p, 3, 3), torch.zeros(cout, p, 1, 1), torch.zeros(cout, cin, 1, 1) if down else None)

    x = torch.zeros(2, 128, 5, 7)
    assert chk(x, *ws(), 2) == (2, 3, 4)
    assert chk(torch.zeros(2, 512, 5, 7), *ws(512, 128, 512, False), 1) == (2, 5, 7)
    with pytest.raises(ValueError, match="stride"):
        chk(x, *ws(), 3)
    with pytest.raises(ValueError, match=r"\(N,C,H,W\)"):
        chk(x[0], *ws(), 1)
    with pytest.raises(ValueError, match=r"\(N,C,H,W\)"):
        chk(None, *ws(), 1)
    with pytest.raises(TypeError, match="float32"):
        chk(x.double(), *ws(), 1)
    with pytest.raises(TypeError, match="float32"):
        chk(x, ws()[0].half(), *ws()[1:], 1)
    with pytest.raises(ValueError, match="empty"):
        chk(torch.zeros(0, 128, 5, 7), *ws(), 1)
    with pytest.raises(ValueError, match="empty"):
        chk(torch.zeros(2, 128, 0, 7), *ws(), 1)
    with pytest.raises(ValueError, match="not a bottleneck"):
        chk(x, *ws(cin=64), 1)
    with pytest.raises(ValueError, match="downsample weight"):
        w = ws()
        chk(x, w[0], w[1], w[2], torch.zeros(512, 64, 1, 1), 1)
    with pytest.raises(ValueError, match="without a downsample"):
        chk(x, *ws(down=False), 1)
    with pytest.raises(ValueError, match="without a downsample"):
        chk(torch.zeros(2, 512, 5, 7), *ws(512, 128, 512, False), 2)
    with pytest.raises(ValueError, match="divisible by 32"):
        chk(torch.zeros(2, 48, 5, 7), *ws(cin=48), 1)
    with pytest.raises(ValueError, match="conv1's weight gradient needs Cout = 64"):
        chk(torch.zeros(2, 64, 5, 7), *ws(64, 64, 256), 1)
    assert chk(torch.zeros(2, 64, 5, 7), *ws(64, 64, 256), 1, (False, False, True, True)) == (2, 5, 7)     # only the 256-row layers
    assert chk(torch.zeros(2, 64, 5, 7), *ws(64, 64, 256), 1, (False,) * 4) == (2, 5, 7)                   # input gradient alone
    with pytest.raises(ValueError, match="65535"):
        chk(torch.zeros(65536, 32, 1, 1), *ws(32, 32, 128), 1, (False,) * 4)
    with pytest.raises(ValueError, match="too large"):
        chk(torch.zeros(1, 32, 1 << 16, 1 << 15, device="meta"), *ws(32, 32, 128), 1, (False,) * 4)
    with pytest.raises(ValueError, match="2\\^31"):
        chk(torch.zeros(1 << 15, 32, 1 << 8, 1 << 8, device="meta"), *ws(32, 32, 128), 1, (False,) * 4)


def test_weight_grad_plan_is_pure_arithmetic():
    from mvsdet_amd import ops
    assert ops.resnet.weight_grad_plan(9, 3, 32, 128, 5, 7) == (3 * 1 * 2, 1, 6)
    tiles, per, splits = ops.resnet.weight_grad_plan(1, 40, 256, 512, 60, 80)
    assert tiles == 40 * 3 * 15 and splits == -(-tiles // per) and splits <= 16 and per == -(-tiles // 16)


def test_freeze():
    from mvsdet_amd.resnet import ResNetStages
    sd = R.make_params((32, 128, 128), (1, 2, 1), seed=7)
    mod = ResNetStages.from_state_dict(sd, prefix="")
    assert all(p.requires_grad for p in mod.parameters())
    assert mod.freeze_() is mod
    frozen = [n for n, p in mod.named_parameters() if not p.requires_grad]
    live = [n for n, p in mod.named_parameters() if p.requires_grad]
    assert all(".bn" not in n and "down_bn" not in n and "stem" not in n and not n.startswith("layers.0.") for n in live)
    assert sorted(live) == sorted(n for n, _ in mod.named_parameters() if n.split(".")[0] == "layers" and n.split(".")[1] in "12"
                                  and "bn" not in n.split(".")[3])
    assert any(n.startswith("stem_conv") for n in frozen)
    mod2 = ResNetStages.from_state_dict(sd, prefix="").freeze_(frozen_stages=-1, norm=False)
    assert all(p.requires_grad for p in mod2.parameters())
    mod3 = ResNetStages.from_state_dict(sd, prefix="").freeze_(frozen_stages=0, norm=False)
    assert not mod3.stem_conv.weight.requires_grad and mod3.layers[0][0].bn1.weight.requires_grad
    mod4 = ResNetStages.from_state_dict(sd, prefix="").freeze_(frozen_stages=3)
    assert not any(p.requires_grad for p in mod4.parameters())
    with pytest.raises(ValueError, match="frozen_stages"):
        mod.freeze_(4)


def test_route_resolution():
    """On the CPU: the default autograd route is today's behaviour; "hip" never turns a CPU call into a HIP call."""
    from mvsdet_amd import resnet as M
    mod, _ = _module()
    assert mod.autograd_route == "torch" and M.AUTOGRAD_ROUTES == ("torch", "hip")
    x = torch.randn(1, 128, 4, 4)
    assert mod.resolve_route(x) == "torch"
    for kw in (dict(autograd_route="hip"), dict(route="auto", autograd_route="hip")):
        m, _ = _module(**kw)
        assert m.resolve_route(x) == "torch"
        out = m.forward_from_stem(x.requires_grad_(True))[0]
        assert out.requires_grad and type(out.grad_fn).__name__ != "_BottleneckFunctionBackward"
    m, _ = _module(route="hip", autograd_route="hip")
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.resolve_route(x)
    with pytest.raises(ValueError, match="autograd_route"):
        _module(autograd_route="auto")
    m.autograd_route = "nope"
    with pytest.raises(ValueError, match="autograd_route"):
        m.resolve_route(x)
    from mvsdet_amd.resnet import ResNetStages
    net, _ = R.stand_in((32,), (1,), seed=3)
    assert ResNetStages.from_module(net, autograd_route="hip").autograd_route == "hip"
    assert ResNetStages.from_module(net).autograd_route == "torch"
