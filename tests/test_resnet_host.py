"""The ResNet stages without a device: the float64 restatement against a stand-in nn.Module, the module's constructors, routes and
refusals, and the operator bindings' shape rules (tests/resnet_restated.py has the definition)."""
import pytest
import torch

import resnet_restated as R

PLANES, DEPTHS = (32, 64, 128, 256), (1, 2, 1, 1)


@pytest.fixture(scope="module")
def narrow():
    net, sd = R.stand_in(PLANES, DEPTHS, seed=11)
    img = torch.randn(2, 3, 50, 70, generator=torch.Generator().manual_seed(12))
    return net, sd, img, R.stages64(img, sd)


def test_restatement_is_the_module_in_eval_mode(narrow):
    net, sd, img, want = narrow
    with torch.no_grad():
        got = net.double()(img.double())
    net.float()
    assert [tuple(t.shape[1:]) for t in want] == [(128, 13, 18), (256, 7, 9), (512, 4, 5), (1024, 2, 3)]
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())
        assert float(w.abs().max()) > 0.1
    # from the stem's map as well
    for g, w in zip(R.stages64(R.stem64(img, sd), sd, from_stem=True), want):
        assert torch.equal(g, w)


def test_training_mode_batchnorm_raises(narrow):
    from mvsdet_amd.resnet import ResNetStages
    net, _ = R.stand_in(PLANES, DEPTHS, seed=11)
    net.train()
    stages = ResNetStages.from_module(net, route="torch")
    with pytest.raises(ValueError, match="norm_eval"):
        stages(narrow[2])
    with pytest.raises(ValueError, match="norm_eval"):
        stages.forward_from_stem(torch.zeros(1, 64, 4, 4))
    net.eval()
    net.layer3[0].downsample[1].train()
    with pytest.raises(ValueError, match="norm_eval"):
        stages(narrow[2])
    net.eval()
    stages.train()                                    # the module's own mode does not touch the BatchNorm layers
    assert not net.bn1.training
    assert len(stages(narrow[2])) == 4


def test_torch_route_on_the_cpu(narrow):
    """Within float32 of the restatement: 1e-4 of each map's largest value (about 1000 float32 roundings of headroom over the
    deepest chain of 5 blocks)."""
    from mvsdet_amd.resnet import ResNetStages
    net, sd, img, want = narrow
    stages = ResNetStages.from_module(net)
    assert stages.resolve_route(img) == "torch"
    with torch.no_grad():
        got = stages(img)
        stem = stages.stem(img)
        again = stages.forward_from_stem(stem)
    assert float((stem.double() - R.stem64(img, sd)).abs().max()) < 1e-5
    for g, a, w in zip(got, again, want):
        assert g.dtype == torch.float32 and torch.equal(g, a)
        assert float((g.double() - w).abs().max()) <= 1e-4 * float(w.abs().max())


def test_from_module_shares_and_from_state_dict_copies(narrow):
    from mvsdet_amd.resnet import ResNetStages
    net, sd, img, _ = narrow
    shared = ResNetStages.from_module(net)
    assert shared.layers[1][0].conv2.weight is net.layer2[0].conv2.weight
    assert shared.layers[1][0].down_bn.running_var.data_ptr() == net.layer2[0].downsample[1].running_var.data_ptr()
    assert shared.stem_conv.weight.data_ptr() == net.conv1.weight.data_ptr()
    assert [len(b) for b in shared.layers] == list(DEPTHS) and [b[0].stride for b in shared.layers] == [1, 2, 2, 2]
    pre = {"backbone." + k: v for k, v in sd.items()}
    pre["backbone.fc.weight"] = torch.zeros(10, 1024)
    pre["backbone.fc.bias"] = torch.zeros(10)
    pre["neck.lateral_convs.0.conv.weight"] = torch.zeros(1)
    copied = ResNetStages.from_state_dict(pre)
    assert copied.layers[1][0].conv2.weight.data_ptr() != pre["backbone.layer2.0.conv2.weight"].data_ptr()
    assert [len(b) for b in copied.layers] == list(DEPTHS)
    with torch.no_grad():
        for a, b in zip(shared(img), copied(img)):
            assert torch.equal(a, b)
    assert ResNetStages.from_state_dict(sd, prefix="").layers[3][0].cout == 1024
    for gone in ("layer2.1.bn2.running_var", "layer3.0.downsample.0.weight", "bn1.weight", "layer1.0.conv3.weight"):
        broken = {k: v for k, v in pre.items() if k != "backbone." + gone}
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            ResNetStages.from_state_dict(broken)
    with pytest.raises(KeyError, match="layer1"):
        ResNetStages.from_state_dict({"backbone.conv1.weight": sd["conv1.weight"]})


def test_module_refusals(narrow):
    from mvsdet_amd.resnet import ResNetStages
    net, sd, img, _ = narrow
    stages = ResNetStages.from_module(net)
    with pytest.raises(ValueError, match="route"):
        ResNetStages.from_module(net, route="cuda")
    with pytest.raises(TypeError, match="float32"):
        stages(img.double())
    with pytest.raises(ValueError, match=r"\(N,3,H,W\)"):
        stages(img[:, :2])
    odd, _ = R.stand_in((24,), (1,), seed=3)
    with pytest.raises(ValueError, match="divisible by 32"):
        ResNetStages.from_module(odd)
    bad, _ = R.stand_in((32,), (2,), seed=3)
    bad.layer1[1].conv2.stride = (2, 2)               # a block that halves the map without a downsample branch
    with pytest.raises(ValueError, match="downsample"):
        ResNetStages.from_module(bad)


def test_route_table(narrow):
    from mvsdet_amd.resnet import ResNetStages
    net, _, img, _ = narrow
    stages = ResNetStages.from_module(net, route="auto")
    assert stages.resolve_route(img) == "torch"
    stages.route = "torch"
    assert stages.resolve_route(img) == "torch"
    stages.route = "hip"
    with pytest.raises(RuntimeError, match="ROCm device"):
        stages(img)
    stages.route = "auto"
    x = img.clone().requires_grad_(True)
    out = stages(x)                                   # the torch route is differentiable
    out[3].sum().backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0 and net.layer2[0].conv2.weight.grad is not None
    net.zero_grad()


@pytest.mark.parametrize("h", [1, 2, 15, 60])
def test_output_sizes(h):
    from mvsdet_amd import ops
    import torch.nn.functional as F
    for s in (1, 2):
        want = (h - 1) // s + 1
        assert ops.resnet.out_size(h, s) == want == R.out_size(h, s)
        x = torch.zeros(1, 32, h, 3)
        assert F.conv2d(x, torch.zeros(32, 32, 1, 1), stride=s).shape[2] == want
        assert F.conv2d(x, torch.zeros(32, 32, 3, 3), stride=s, padding=1).shape[2] == want
        assert ops.resnet.check_shapes(x, 32, 32, torch.zeros(32), s)[2:] == (want, (3 - 1) // s + 1)
        assert ops.resnet.check_shapes(x, 288, 32, torch.zeros(32), s, taps=9)[2:] == (want, (3 - 1) // s + 1)


def test_check_shapes_refuses_each_rule():
    from mvsdet_amd import ops
    cs = ops.resnet.check_shapes
    x, sh = torch.zeros(2, 64, 5, 7), torch.zeros(96)
    assert cs(x, 64, 96, sh, 2, torch.zeros(2, 96, 3, 4)) == (2, 64, 3, 4)
    with pytest.raises(ValueError, match="stride"):
        cs(x, 64, 96, sh, 3)
    with pytest.raises(ValueError, match="stride"):
        cs(x, 64, 96, sh, 0)
    with pytest.raises(ValueError, match="Cin"):
        cs(torch.zeros(2, 48, 5, 7), 48, 96, sh)
    with pytest.raises(ValueError, match="Cout"):
        cs(x, 64, 80, torch.zeros(80))
    with pytest.raises(ValueError, match="columns"):
        cs(x, 9 * 64, 96, sh)
    with pytest.raises(ValueError, match="columns"):
        cs(x, 64, 96, sh, taps=9)
    with pytest.raises(ValueError, match="shift"):
        cs(x, 64, 96, torch.zeros(64))
    with pytest.raises(ValueError, match="residual"):
        cs(x, 64, 96, sh, 2, torch.zeros(2, 96, 5, 7))
    with pytest.raises(ValueError, match="residual"):
        cs(x, 9 * 64, 96, sh, 1, torch.zeros(2, 96, 5, 7), taps=9)
    with pytest.raises(ValueError, match=r"\(N,C,H,W\)"):
        cs(x[0], 64, 96, sh)
    with pytest.raises(ValueError, match="empty"):
        cs(torch.zeros(2, 64, 0, 7), 64, 96, sh)
    for bad in (dict(x=x.double()), dict(shift=sh.half()), dict(residual=torch.zeros(2, 96, 5, 7, dtype=torch.float64))):
        args = dict(x=x, shift=sh, residual=None)
        args.update(bad)
        with pytest.raises(TypeError, match="float32"):
            cs(args["x"], 64, 96, args["shift"], 1, args["residual"])
    # the view and column limits, on tensors that own no memory
    big = torch.zeros(1, 32, 1, 1).expand(65536, 32, 1, 1)
    assert cs(big, 32, 32, torch.zeros(32))[0] == 65536                     # the 1x1 carries no view on a grid axis
    with pytest.raises(ValueError, match="65535"):
        cs(big, 288, 32, torch.zeros(32), taps=9)
    wide = torch.zeros(1, 32, 1, 1).expand(2, 32, 1 << 15, 1 << 15)
    with pytest.raises(ValueError, match="exceed 2\\^31"):
        cs(wide, 32, 32, torch.zeros(32))
    assert cs(wide, 32, 32, torch.zeros(32), 2)[2:] == (1 << 14, 1 << 14)
    # the operators refuse a CPU tensor after the shape rules
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.resnet.conv1x1(x, torch.zeros(1, dtype=torch.bfloat16), sh, 96)
    with pytest.raises(ValueError, match="stride"):
        ops.resnet.conv3x3(x, torch.zeros(1, dtype=torch.bfloat16), sh, 96, stride=4)


def test_fold_pads_and_is_tap_major():
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(5)
    w, scale = torch.randn(64, 32, 3, 3, generator=g), torch.rand(64, generator=g) + 0.5
    m = ops.resnet.fold(w, scale)
    assert m.shape == (128, 288) and m.is_contiguous() and m.dtype == torch.float32
    assert not bool(m[64:].any())
    for o, c, dy, dx in ((0, 0, 0, 0), (5, 7, 1, 2), (63, 31, 2, 2), (17, 30, 2, 0)):
        assert float(m[o, 32 * (3 * dy + dx) + c]) == float(w[o, c, dy, dx] * scale[o])
    assert torch.equal(R.unfold_matrix(m, 64, 3), w * scale.view(-1, 1, 1, 1))
    assert torch.equal(m[:64], ops.fpn.conv3x3_matrix(w * scale.view(-1, 1, 1, 1)))
    m1 = ops.resnet.fold(w[:, :, :1, :1], scale)
    assert m1.shape == (128, 32) and torch.equal(m1[:64], w[:, :, 0, 0] * scale[:, None])
    assert ops.resnet.fold(torch.zeros(256, 32, 1, 1), torch.zeros(256)).shape == (256, 32)
    assert ops.resnet.fold(torch.zeros(96, 32, 1, 1), torch.zeros(96)).shape == (128, 32)
    with pytest.raises(ValueError, match="fold"):
        ops.resnet.fold(w, scale[:32])
    from mvsdet_amd import ops as o2
    assert o2.resnet.CONV3X3_TILE == (8, 16) and o2.resnet.CONV3X3_S2_TILE == (4, 16)


def test_hot_path_needs_a_backbone():
    from mvsdet_amd.hotpath import MVSDetHotPath
    hp = MVSDetHotPath([8, 8, 4], [0.4, 0.4, 0.4], [0.2, 5.0], 4)
    assert hp.backbone is None
    with pytest.raises(ValueError, match="backbone"):
        hp.forward_scene_from_images(torch.zeros(1, 3, 8, 8), {})
