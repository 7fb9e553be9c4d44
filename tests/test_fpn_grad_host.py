"""The FPN's gradients where no device is needed: the float64 yardstick of tests/fpn_grad_restated.py against hand-written sums,
`ops.fpn.check_grad_shapes`' refusals, the module's `autograd_route` keyword, the argument checks of the new C entries (which launch
nothing) and the weight gradient's split / workspace query."""
import ctypes

import pytest
import torch

import fpn_grad_restated as G
import fpn_restated as R

CH, COUT = (128, 128, 256, 128), 128
PYRAMIDS = {"halved": [(12, 16), (6, 8), (3, 4), (2, 2)], "odd": [(15, 20), (8, 10), (4, 5), (2, 3)]}


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("taps,N,H,W", [(9, 2, 5, 7), (9, 1, 1, 1), (9, 1, 1, 4), (1, 2, 5, 7), (1, 3, 1, 1)])
def test_weight_gradient_yardstick_is_the_written_sum(taps, N, H, W):
    gy, x = _rand(N, 8, H, W, seed=1), _rand(N, 6, H, W, seed=2)
    torch.testing.assert_close(G.dw64(gy, x, taps), G.dw_sum(gy, x, taps), rtol=0, atol=1e-12)
    if taps == 9 and (H, W) == (1, 1):
        off_centre = G.dw_sum(gy, x, 9).clone()
        off_centre[:, :, 1, 1] = 0
        assert float(off_centre.abs().max()) == 0.0


@pytest.mark.parametrize("k", [1, 3])
def test_input_gradient_yardstick_is_the_written_sum(k):
    g, w = _rand(2, 8, 5, 7, seed=3), _rand(8, 6, k, k, seed=4)
    torch.testing.assert_close(G.dx64(g, w), G.dx_sum(g, w), rtol=0, atol=1e-12)
    if k == 1:
        torch.testing.assert_close(G.dx64(g, w.view(8, 6)), G.dx_sum(g, w.view(8, 6)), rtol=0, atol=1e-12)


@pytest.mark.parametrize("H,W,Ht,Wt", [(15, 20, 8, 10), (7, 5, 4, 3), (60, 80, 30, 40), (44, 46, 26, 14), (82, 3, 2, 1), (3, 3, 1, 1), (4, 4, 4, 4)])
def test_adjoint_yardstick_is_the_written_sum(H, W, Ht, Wt):
    """ATen's CPU backward of the nearest gather is the index_add over `fpn_restated.nearest_index`, and it is the adjoint:
    <up(t), g> == <t, up^T(g)>."""
    g = torch.randint(-8, 9, (2, 3, H, W), generator=torch.Generator().manual_seed(5)).double()
    got = G.up_t64(g, (Ht, Wt))
    assert torch.equal(got, G.up_t_sum(g, (Ht, Wt)))
    assert torch.equal(G.up_t(g.float(), (Ht, Wt)).double(), got)                       # integers: float32 is exact too
    t = torch.randint(-8, 9, (2, 3, Ht, Wt), generator=torch.Generator().manual_seed(6)).double()
    assert float((R.gather_nearest(t, (H, W)) * g).sum()) == float((t * got).sum())
    assert float(G.preimage_size((H, W), (Ht, Wt)).sum()) == H * W


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_chain_yardstick_is_the_written_chain(name):
    """float64 autograd of level0_64 against the chain of the issue written out with the sums above."""
    small = (8, 8, 16, 8)
    sd = R.make_params(small, 8, seed=11)
    stages = R.make_stages(2, small, PYRAMIDS[name], seed=12)
    r = _rand(2, 8, *PYRAMIDS[name][0], seed=13)
    dx, dp = G.chain_grads64(stages, sd, r)
    _, l0 = R.level0_64(stages, sd, want_laterals=True)
    tol = dict(rtol=0, atol=1e-10)
    torch.testing.assert_close(dp["fpn_convs.0.conv.weight"], G.dw_sum(r, l0, 9), **tol)
    torch.testing.assert_close(dp["fpn_convs.0.conv.bias"], r.sum((0, 2, 3)), **tol)
    gl = G.dx_sum(r, sd["fpn_convs.0.conv.weight"])
    for i in range(4):
        if i > 0:
            gl = G.up_t_sum(gl, stages[i].shape[2:])
        w = sd[f"lateral_convs.{i}.conv.weight"]
        torch.testing.assert_close(dx[i], G.dx_sum(gl, w), **tol)
        torch.testing.assert_close(dp[f"lateral_convs.{i}.conv.weight"], G.dw_sum(gl, stages[i], 1), **tol)
        torch.testing.assert_close(dp[f"lateral_convs.{i}.conv.bias"], gl.sum((0, 2, 3)), **tol)
    xb, pb = G.chain_bounds64(stages, sd, r)
    assert all(bool((b > 0).all()) for b in xb) and sorted(pb) == sorted(dp)
    assert all(pb[k].shape == dp[k].shape for k in dp)


def _params(channels=CH, seed=51):
    sd = R.make_params(channels, COUT, seed=seed)
    lw = [sd[f"lateral_convs.{i}.conv.weight"] for i in range(4)]
    lb = [sd[f"lateral_convs.{i}.conv.bias"] for i in range(4)]
    return sd, lw, lb, sd["fpn_convs.0.conv.weight"], sd["fpn_convs.0.conv.bias"]


def test_check_grad_shapes_refusals():
    from mvsdet_amd import ops
    _, lw, lb, ow, ob = _params()
    stages = R.make_stages(2, CH, PYRAMIDS["odd"], seed=52)
    assert ops.fpn.check_grad_shapes(stages, lw, lb, ow, ob) == (2, COUT)
    # a stage the forward takes and the autograd route cannot: 96 channels
    ch96 = (96, 128, 256, 128)
    _, lw96, lb96, ow96, ob96 = _params(ch96)
    st96 = R.make_stages(2, ch96, PYRAMIDS["odd"], seed=53)
    assert ops.fpn.check_shapes(st96, lw96, lb96, ow96, ob96) == (2, COUT)
    with pytest.raises(ValueError, match="stage 0 has 96 channels, not divisible by 128"):
        ops.fpn.check_grad_shapes(st96, lw96, lb96, ow96, ob96)
    # ... and everything check_shapes refuses
    with pytest.raises(ValueError, match="3 stages for 4 lateral"):
        ops.fpn.check_grad_shapes(stages[:3], lw, lb, ow, ob)
    with pytest.raises(TypeError, match="stage 0 must be torch.float32"):
        ops.fpn.check_grad_shapes([stages[0].double()] + stages[1:], lw, lb, ow, ob)
    with pytest.raises(TypeError, match="parameters must be torch.float32"):
        ops.fpn.check_grad_shapes(stages, lw, lb, ow.double(), ob)
    with pytest.raises(ValueError, match="Cout = 64"):
        ops.fpn.check_grad_shapes(stages, lw, lb, torch.zeros(64, 64, 3, 3), ob)


def test_autograd_route_keyword():
    from mvsdet_amd.fpn import AUTOGRAD_ROUTES, FPNLevel0
    sd, lw, lb, ow, ob = _params()
    assert AUTOGRAD_ROUTES == ("torch", "hip")
    assert FPNLevel0(lw, lb, ow, ob).autograd_route == "torch"
    assert FPNLevel0(lw, lb, ow, ob, autograd_route="hip").autograd_route == "hip"
    assert FPNLevel0.from_state_dict(sd, prefix="", autograd_route="hip").autograd_route == "hip"
    assert FPNLevel0.from_module(R.StandInFPN(sd, 4), autograd_route="hip").autograd_route == "hip"
    with pytest.raises(ValueError, match="autograd_route 'aten' is not one of"):
        FPNLevel0(lw, lb, ow, ob, autograd_route="aten")
    # CPU tensors: the option changes nothing ("auto" takes torch's layers, which are differentiable; "hip" refuses)
    fpn = FPNLevel0(lw, lb, ow, ob, autograd_route="hip")
    stages = R.make_stages(1, CH, PYRAMIDS["halved"], seed=54)
    xs = [s.clone().requires_grad_(True) for s in stages]
    fpn(xs).sum().backward()
    assert all(x.grad is not None for x in xs) and fpn.out_weight.grad is not None
    fpn.route = "hip"
    with pytest.raises(RuntimeError, match="ROCm device"):
        fpn(xs)
    fpn.route, fpn.autograd_route = "auto", "aten"
    with pytest.raises(ValueError, match="autograd_route 'aten'"):
        fpn(stages)


def test_input_gradient_bindings_refuse_without_a_device():
    from mvsdet_amd import ops
    g = torch.zeros(1, 128, 4, 4)
    with pytest.raises(ValueError, match="C = 96 must be divisible by 128"):
        ops.fpn.lateral_input_grad(g, torch.zeros(128, 96, 1, 1))
    with pytest.raises(ValueError, match="C = 96 must be divisible by 128"):
        ops.fpn.conv3x3_input_grad(g, torch.zeros(128, 96, 3, 3))
    with pytest.raises(ValueError, match="taps = 3"):
        ops.fpn.weight_grad(g, g, 3)
    with pytest.raises(ValueError, match="C = 40 must be divisible by 32"):
        ops.fpn.weight_grad(g, torch.zeros(1, 40, 4, 4), 1)
    with pytest.raises(ValueError, match="share N, H and W"):
        ops.fpn.weight_grad(g, torch.zeros(1, 128, 4, 5), 1)
    with pytest.raises(ValueError, match="must lie within"):
        ops.fpn.top_down_grad(g, (5, 4))


def test_argument_checks_do_not_launch():
    from mvsdet_amd import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    big = 1 << 40
    dw, td, bg = lib.mvsdet_fpn_dw_bf16x3, lib.mvsdet_fpn_top_down_grad_f32, lib.mvsdet_fpn_bias_grad_f32
    for call, args, rc_want, word in (
            (dw, (None, p, p, p, big, 9, 1, 32, 128, 4, 4, None), 1, b"NULL"),
            (dw, (p, p, p, None, big, 9, 1, 32, 128, 4, 4, None), 1, b"NULL"),
            (dw, (p, p, p, p, big, 3, 1, 32, 128, 4, 4, None), 1, b"taps=3"),
            (dw, (p, p, p, p, big, 9, 1, 32, 64, 4, 4, None), 1, b"Cout=64"),
            (dw, (p, p, p, p, big, 1, 1, 40, 128, 4, 4, None), 1, b"C=40"),
            (dw, (p, p, p, p, big, 9, 65536, 32, 128, 4, 4, None), 1, b"N=65536"),
            (dw, (p, p, p, p, big, 9, 1 << 15, 32, 128, 256, 256, None), 1, b"2^31"),
            (dw, (p, odd, p, p, big, 9, 1, 32, 128, 4, 4, None), 1, b"4-byte aligned"),
            (dw, (p, p, p, p, 9 * 128 * 32 * 4 - 1, 9, 1, 32, 128, 2, 16, None), 2, b"workspace"),
            (td, (None, p, 1, 8, 4, 4, 2, 2, None), 1, b"NULL"),
            (td, (p, p, 1, 8, 4, 4, 5, 4, None), 1, b"top level 5 x 4"),
            (td, (p, p, 1, 8, 4, 4, 4, 0, None), 1, b"top level 4 x 0"),
            (td, (p, p, 65536, 8, 4, 4, 2, 2, None), 1, b"N=65536"),
            (td, (p, p, 1 << 15, 8, 256, 256, 2, 2, None), 1, b"2^31"),
            (td, (odd, p, 1, 8, 4, 4, 2, 2, None), 1, b"4-byte aligned"),
            (bg, (p, None, 1, 8, 4, 4, None), 1, b"NULL"),
            (bg, (p, p, 1 << 15, 8, 256, 256, None), 1, b"2^31"),
            (bg, (p, odd, 1, 8, 4, 4, None), 1, b"4-byte aligned")):
        rc = call(*args)
        assert rc == rc_want and word in lib.mvsdet_last_error(), (rc, word, lib.mvsdet_last_error())
    assert lib.mvsdet_fpn_dw_splits(3, 1, 32, 128, 4, 4) == 0 and b"taps=3" in lib.mvsdet_last_error()
    assert lib.mvsdet_fpn_dw_workspace_bytes(9, 1, 40, 128, 4, 4) == 0 and b"C=40" in lib.mvsdet_last_error()


SCENE = {40: [(256, 60, 80), (512, 30, 40), (1024, 15, 20), (2048, 8, 10)]}


def test_workspace_query_at_the_scene_shapes():
    """The split of K and the workspace at 40 / 80 / 100 views of the shipped pyramid: about DW_SPLIT_BLOCKS blocks, contiguous runs of
    tiles, the last one ragged or not; one fp32 partial (taps, Cout, C) per split."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    th, tw = ops.fpn.DW_TILE
    assert (th, tw) == (2, 16) and ops.fpn.DW_COL_BLOCK == 32 and ops.fpn.DW_SPLIT_BLOCKS == 512
    # level 0's 3x3 at 40 views: 30 x 5 tiles a view, 16 blocks per split -> 32 splits of 188 tiles (the last: 172), 75.5 MB
    assert ops.fpn.weight_grad_plan(9, 40, 256, 256, 60, 80) == (6000, 188, 32)
    assert lib.mvsdet_fpn_dw_splits(9, 40, 256, 256, 60, 80) == 32
    assert lib.mvsdet_fpn_dw_workspace_bytes(9, 40, 256, 256, 60, 80) == 32 * 9 * 256 * 256 * 4
    # the laterals at 40 views: K of level 3 is 3 tiles a view (80 pixels in tiles of 32)
    assert ops.fpn.weight_grad_plan(1, 40, 2048, 256, 8, 10) == (120, 30, 4)
    assert lib.mvsdet_fpn_dw_workspace_bytes(1, 40, 2048, 256, 8, 10) == 4 * 256 * 2048 * 4
    for N in (40, 80, 100):
        for taps, (C, H, W) in [(9, (256, 60, 80))] + [(1, s) for s in SCENE[40]]:
            tiles, per, nsplit = ops.fpn.weight_grad_plan(taps, N, C, 256, H, W)
            assert lib.mvsdet_fpn_dw_splits(taps, N, C, 256, H, W) == nsplit
            assert lib.mvsdet_fpn_dw_workspace_bytes(taps, N, C, 256, H, W) == nsplit * taps * 256 * C * 4
            assert (nsplit - 1) * per < tiles <= nsplit * per                      # no empty split
            assert nsplit * (C // 32) * 2 <= 512 + (C // 32) * 2                   # about DW_SPLIT_BLOCKS blocks
    # small and odd shapes, the kernel's answer against the restated plan
    for taps, N, C, cout, H, W in [(9, 1, 256, 256, 1, 1), (9, 1, 32, 128, 9, 33), (9, 1, 256, 256, 5 * th, 7 * tw), (1, 3, 1024, 256, 15, 20),
                                   (1, 1, 2048, 256, 1, 1), (9, 2, 256, 256, 5, 7), (1, 65535, 32, 128, 1, 1)]:
        assert lib.mvsdet_fpn_dw_splits(taps, N, C, cout, H, W) == ops.fpn.weight_grad_plan(taps, N, C, cout, H, W)[2], (taps, N, C, H, W)
