"""Level 0 of the 2-D feature pyramid (mvsdet_amd/fpn.py, ops/fpn.py) where no device is needed: the level-0 chain against the full
four-output restatement of the module (tests/fpn_restated.py), the module's torch route and its constructors, the tap-major matrix
of the 3x3 kernel, the nearest index, and every refusal of `ops.fpn.check_shapes`."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fpn_restated as R

CH, COUT = (32, 64, 96, 128), 128
PYRAMIDS = {"halved": [(12, 16), (6, 8), (3, 4), (2, 2)], "odd": [(15, 20), (8, 10), (4, 5), (2, 3)]}


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_level0_chain_is_the_full_modules_first_output(name):
    sd = R.make_params(CH, COUT, seed=11)
    stages = R.make_stages(2, CH, PYRAMIDS[name], seed=12)
    outs = R.fpn_full64(stages, sd)
    assert [tuple(o.shape[2:]) for o in outs] == PYRAMIDS[name]
    assert torch.equal(R.level0_64(stages, sd), outs[0])


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_module_on_cpu_tensors_and_its_constructors(name):
    from mvsdet_amd.fpn import FPNLevel0
    sd = R.make_params(CH, COUT, seed=21)
    stages = R.make_stages(2, CH, PYRAMIDS[name], seed=22)
    want = R.level0_64(stages, sd)
    prefixed = {"neck." + k: v for k, v in sd.items()}
    prefixed["backbone.conv1.weight"] = torch.zeros(3)
    a = FPNLevel0.from_state_dict(prefixed)                      # the keys of fpn_convs.1..3 are there and ignored
    fpn = R.StandInFPN(sd, 4)
    b = FPNLevel0.from_module(fpn)
    assert b.out_weight is fpn.fpn_convs[0].conv.weight and b.lateral_biases[2] is fpn.lateral_convs[2].conv.bias   # shared
    names = sorted(k for k, _ in a.named_parameters())
    assert names == sorted(k for k, _ in b.named_parameters()) and len(names) == 10
    for (_, p), (_, q) in zip(sorted(a.named_parameters()), sorted(b.named_parameters())):
        assert torch.equal(p, q)
    with torch.no_grad():
        ya, yb = a(stages), b(stages)
    assert torch.equal(ya, yb) and ya.dtype == torch.float32 and ya.shape == want.shape
    # float32 rounding: every sum of |products| is below mag; 2e-6 of it covers the accumulation of up to 9 * 128 + 128 terms
    w3 = sd["fpn_convs.0.conv.weight"]
    _, l0 = R.level0_64(stages, sd, want_laterals=True)
    bound = 2e-6 * (R.mag64(l0.float(), w3, padding=1) + 1.0)
    assert bool(((ya.double() - want).abs() <= bound).all())
    # differentiable: the torch route under autograd
    xs = [s.clone().requires_grad_(True) for s in stages]
    a(xs).sum().backward()
    assert all(x.grad is not None and bool(x.grad.abs().sum() > 0) for x in xs) and a.out_weight.grad is not None
    # route "hip" refuses CPU tensors instead of falling back
    a.route = "hip"
    with pytest.raises(RuntimeError, match="ROCm device"):
        a(stages)


def test_state_dict_missing_a_lateral_raises():
    from mvsdet_amd.fpn import FPNLevel0
    sd = {"neck." + k: v for k, v in R.make_params(CH, COUT, seed=31).items()}
    for gone in ("neck.lateral_convs.1.conv.weight", "neck.lateral_convs.2.conv.bias", "neck.fpn_convs.0.conv.weight"):
        part = {k: v for k, v in sd.items() if k != gone}
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            FPNLevel0.from_state_dict(part)
    with pytest.raises(KeyError, match="lateral_convs"):
        FPNLevel0.from_state_dict(sd, prefix="img_neck.")
    # without the top lateral the checkpoint is a three-level pyramid: four stages are refused
    three = FPNLevel0.from_state_dict({k: v for k, v in sd.items() if ".lateral_convs.3." not in k})
    with pytest.raises(ValueError, match="4 stages for 3 lateral"):
        three(R.make_stages(1, CH, PYRAMIDS["halved"], seed=1))


def test_restated_convolution_is_torchs():
    g = torch.Generator().manual_seed(40)
    x = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64)
    for k, pad in ((3, 1), (1, 0)):
        w = torch.randn(8, 6, k, k, generator=g, dtype=torch.float64)
        b = torch.randn(8, generator=g, dtype=torch.float64)
        torch.testing.assert_close(R.conv64(x, w, b, padding=pad), F.conv2d(x, w, b, padding=pad), rtol=0, atol=1e-12)
    x32 = x.float()
    hi, mid = R.split_bf16(x32)
    assert torch.equal(hi.float() + (x32 - hi.float()), x32) and float((x32 - hi.float() - mid.float()).abs().max()) <= 2.0 ** -16 * float(x32.abs().max())


def test_conv3x3_matrix_is_tap_major():
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(41)
    x = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(8, 6, 3, 3, generator=g, dtype=torch.float64)
    m = ops.fpn.conv3x3_matrix(w)
    assert m.shape == (8, 54) and m.is_contiguous()
    xp = F.pad(x, (1, 1, 1, 1))
    cols = torch.stack([xp[:, :, dy:dy + 5, dx:dx + 7] for dy in range(3) for dx in range(3)], 1)   # (N, tap, C, H, W): k = C tap + c
    got = torch.einsum("mk,nkhw->nmhw", m, cols.reshape(2, 54, 5, 7))
    torch.testing.assert_close(got, F.conv2d(x, w, padding=1), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="3,3"):
        ops.fpn.conv3x3_matrix(torch.zeros(8, 6, 1, 1))


@pytest.mark.parametrize("out_size,in_size", [(46, 14), (82, 2), (44, 26), (20, 10), (15, 8)])
def test_torch_nearest_index_is_the_float32_formula(out_size, in_size):
    """Why the kernel computes the source index in float32: F.interpolate(mode='nearest') by size does, and the integer form
    dst * in / out differs from it at 46 <- 14 and 82 <- 2."""
    src = torch.arange(in_size, dtype=torch.float32).view(1, 1, in_size, 1)
    got = F.interpolate(src, size=(out_size, 1), mode="nearest").view(-1).to(torch.int64)
    assert torch.equal(got, R.nearest_index(out_size, in_size))
    assert torch.equal(F.interpolate(src.double(), size=(out_size, 1), mode="nearest").view(-1).to(torch.int64), got)
    differs = not torch.equal(got, R.nearest_index_integer(out_size, in_size))
    assert differs == ((out_size, in_size) in ((46, 14), (82, 2), (44, 26)))


def test_check_shapes_refusals():
    from mvsdet_amd import ops
    sd = R.make_params(CH, COUT, seed=51)
    lw = [sd[f"lateral_convs.{i}.conv.weight"] for i in range(4)]
    lb = [sd[f"lateral_convs.{i}.conv.bias"] for i in range(4)]
    ow, ob = sd["fpn_convs.0.conv.weight"], sd["fpn_convs.0.conv.bias"]
    stages = R.make_stages(2, CH, PYRAMIDS["odd"], seed=52)
    assert ops.fpn.check_shapes(stages, lw, lb, ow, ob) == (2, COUT)

    def refused(exc, match, st=stages, w=lw, b=lb, o=ow, obias=ob):
        with pytest.raises(exc, match=match):
            ops.fpn.check_shapes(st, w, b, o, obias)

    refused(ValueError, "3 stages for 4 lateral", st=stages[:3])
    refused(ValueError, "5 stages for 4 lateral", st=stages + [stages[3]])
    bad = list(stages)
    bad[1] = torch.zeros(2, 40, 8, 10)
    refused(ValueError, "stage 1 has 40 channels, not divisible by 32", st=bad)
    bad = list(stages)
    bad[2] = torch.zeros(2, 96, 9, 5)
    refused(ValueError, r"top level 2 \(9 x 5\) is larger than the level below it \(8 x 10\)", st=bad)
    bad = list(stages)
    bad[3] = torch.zeros(3, 128, 2, 3)
    refused(ValueError, "stage 3 has batch size 3, stage 0 has 2", st=bad)
    badw = list(lw)
    badw[0] = torch.zeros(COUT, 64, 1, 1)
    refused(ValueError, r"lateral weight 0 \(128, 64, 1, 1\) must be \(128,32,1,1\)", w=badw)
    refused(ValueError, r"output convolution's weight \(128, 128, 1, 1\) must be \(Cout,Cout,3,3\)", o=torch.zeros(COUT, COUT, 1, 1))
    refused(ValueError, "Cout = 64 output channels are not divisible by 128", o=torch.zeros(64, 64, 3, 3))
    bad = list(stages)
    bad[0] = stages[0].double()
    refused(TypeError, "stage 0 must be torch.float32", st=bad)
    bad[0] = stages[0].half()
    refused(TypeError, "stage 0 must be torch.float32", st=bad)


def test_argument_checks_do_not_launch():
    from mvsdet_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    for call, args, word in ((lib.mvsdet_fpn_lateral_bf16x3, (p, p, None, None, p, 1, 32, 128, 4, 4, 0, 0, None), b"NULL"),
                             (lib.mvsdet_fpn_lateral_bf16x3, (p, p, p, None, p, 1, 40, 128, 4, 4, 0, 0, None), b"Cin=40"),
                             (lib.mvsdet_fpn_lateral_bf16x3, (p, p, p, p, p, 1, 32, 128, 4, 4, 5, 4, None), b"top level 5 x 4"),
                             (lib.mvsdet_fpn_lateral_bf16x3, (p, p, p, None, p, 1 << 20, 32, 128, 64, 64, 0, 0, None), b"2^31"),
                             (lib.mvsdet_fpn_conv3x3_bf16x3, (p, p, p, None, None, 1, 32, 128, 4, 4, None), b"at least one"),
                             (lib.mvsdet_fpn_conv3x3_bf16x3, (p, p, p, p, None, 1, 32, 64, 4, 4, None), b"Cout=64"),
                             (lib.mvsdet_fpn_conv3x3_bf16x3, (p, p, p, p, ctypes.c_void_p(4100), 1, 32, 128, 4, 4, None), b"16-byte")):
        rc = call(*args)
        assert rc == 1 and word in lib.mvsdet_last_error(), (rc, word, lib.mvsdet_last_error())


def test_hot_path_attribute_defaults_to_none():
    from mvsdet_amd.hotpath import MVSDetHotPath
    hp = MVSDetHotPath([8, 8, 4], [0.4, 0.4, 0.4], [0.2, 5.0], 4)
    assert hp.fpn is None
    with pytest.raises(ValueError, match="needs `fpn`"):
        hp.forward_scene_from_stages([], {})
