"""The per-pixel form of the sweep (homo_warping's depth_values (B,D,H,W), mvs_models/module.py:130-133), host side: the CPU
restatement against fixture G22, the dispatch of `functional.homo_warping` and of the deferred route on the depth's dim, the
fake kernels, the autocast rule and the argument checks of the five C entries.  No GPU here; tests/test_gpu_sweep_pixel.py
runs the kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import sweep_pixel_restated as SP

G22 = [(tag, fam) for tag in ("n3_d8", "n6_d12_arkit") for fam in ("smooth", "rough")]


@pytest.mark.parametrize("tag,family", G22)
def test_restatement_matches_g22(tag, family):
    """tests/sweep_pixel_restated.py reproduces what the reference's homo_warping and the variance lines around it returned for
    the per-pixel depth maps of G22 (1e-5; 0.0 on the generating host), and the fixture meets its own conditions."""
    g2, g = load_golden("g2_variance_" + tag), load_golden(f"g22_sweep_pixel_{tag}_{family}")
    feat, nbr, proj = (torch.from_numpy(g2[k]) for k in ("feature", "neighbor_ids", "proj_rel"))
    depth, cs = torch.from_numpy(g["depth"]), int(g["channel_stride"])
    assert depth.shape == (feat.shape[0], g2["depth_values"].shape[1]) + feat.shape[2:]
    assert float(g["min_abs_z"]) >= 0.05 and np.isfinite(g["warped"]).all() and np.isfinite(g["variance"]).all()
    assert int((depth < 0).sum()) >= 15 and int((depth == 1e6).sum()) >= 15          # the planted pixels
    min_z = min(float(SP.sample_grid(proj[:, j], depth, *feat.shape[2:])[1].abs().min()) for j in range(nbr.shape[1]))
    assert min_z >= 0.05
    warped = SP.homo_warp_pixel(feat[nbr[:, 0]], proj[:, 0], depth)
    var = SP.variance_pixel(feat, nbr, proj, depth)
    ew = float((warped[:, ::cs] - torch.from_numpy(g["warped"])).abs().max())
    ev = float((var[:, ::cs] - torch.from_numpy(g["variance"])).abs().max())
    print(f"G22 {tag}/{family}: restated warp {ew:.2e} variance {ev:.2e}")
    assert ew <= 1e-5 and ev <= 1e-5


def test_restatement_on_a_broadcast_depth_is_the_plane_restatement():
    """A (B,D) depth broadcast to (B,D,H,W) gives the plane form's values, bit for bit (as in the reference itself)."""
    from oracle import torch_restatement as TR
    g2 = load_golden("g2_variance_n6_d12_arkit")
    feat, nbr, proj, dv = (torch.from_numpy(g2[k]) for k in ("feature", "neighbor_ids", "proj_rel", "depth_values"))
    d4 = dv[:, :, None, None].expand(-1, -1, *feat.shape[2:]).contiguous()
    assert torch.equal(SP.homo_warp_pixel(feat[nbr[:, 1]], proj[:, 1], d4), TR.homo_warp(feat[nbr[:, 1]], proj[:, 1], dv))


@pytest.mark.parametrize("half", [False, True])
def test_homo_warping_hands_a_4d_depth_to_the_pixel_operator(monkeypatch, half):
    """functional.homo_warping with depth_values (B,D,H,W): the fp32 relative projection of module.py:116 and the contiguous
    (B,D,H,W) depth reach ops.homo_warp_pixel (recorded, not run) -- also from float16 inputs under autocast."""
    from mvsdet_amd import functional as F_, ops
    seen = []
    monkeypatch.setattr(ops, "homo_warp_pixel", lambda *a: seen.append(a) or "pixel")
    monkeypatch.setattr(ops, "homo_warp", lambda *a: pytest.fail("the plane operator got a 4-D depth"))
    if half:
        monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    B, C, D, H, W = 2, 3, 4, 5, 6
    g = torch.Generator().manual_seed(3)
    dt = torch.float16 if half else torch.float32
    src = torch.randn(B, C, H, W, generator=g).to(dt)
    src_proj = torch.eye(4).repeat(B, 1, 1) + 0.1 * torch.randn(B, 4, 4, generator=g)
    ref_proj = torch.eye(4).repeat(B, 1, 1) + 0.1 * torch.randn(B, 4, 4, generator=g)
    depth = (1.0 + torch.rand(B, H, W, D, generator=g)).to(dt).permute(0, 3, 1, 2)        # (B,D,H,W), not contiguous
    assert not depth.is_contiguous()
    assert F_.homo_warping(src, src_proj, ref_proj, depth) == "pixel"
    (s, p, d), = seen
    assert s.dtype == p.dtype == d.dtype == torch.float32
    assert torch.equal(p, torch.matmul(src_proj, torch.inverse(ref_proj))) and torch.equal(s, src.float())
    assert d.shape == (B, D, H, W) and d.is_contiguous() and torch.equal(d, depth.float())


def test_homo_warping_refuses_other_depth_shapes():
    from mvsdet_amd import functional as F_
    eye, src = torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 3, 5, 6)
    for shape in [(2, 4, 5, 7), (2, 4, 6, 5), (3, 4, 5, 6), (2, 4, 30), (8,), (2, 1, 4, 5, 6)]:
        with pytest.raises(ValueError):
            F_.homo_warping(src, eye, eye, torch.ones(shape))


def test_lazy_route_dispatches_on_the_depth_dim(monkeypatch):
    """Under LAZY_WARP a 4-D depth defers like a 2-D one; the materialising path and the fused collapse pick the pixel operators."""
    from mvsdet_amd import functional as F_, lazywarp, ops
    calls = []
    N, C, D, H, W = 3, 2, 4, 5, 6
    for name in ("homo_warp", "homo_warp_pixel"):
        monkeypatch.setattr(ops, name, lambda s, p, d, name=name: calls.append(name) or torch.ones(N, C, D, H, W))
    for name in ("plane_sweep_variance", "plane_sweep_variance_pixel"):
        monkeypatch.setattr(ops, name, lambda f, i, p, d, name=name: calls.append((name, tuple(p.shape), d)) or torch.zeros(N, C, D, H, W))
    monkeypatch.setattr(F_, "LAZY_WARP", True)
    monkeypatch.setattr(F_, "LAZY_ANY_DEVICE", True)
    feat = torch.arange(N * C * H * W, dtype=torch.float32).view(N, C, H, W)
    ids = torch.tensor([[1, 2], [0, 0], [2, 1]])
    lazywarp.note_neighbor_ids(ids)
    eye = torch.eye(4).repeat(N, 1, 1)
    for depth in (torch.ones(N, D), torch.ones(N, D, H, W)):
        pixel = depth.dim() == 4
        calls.clear()
        before = dict(lazywarp.stats)
        ref_volume = feat.unsqueeze(2).repeat(1, 1, D, 1, 1)
        vsum, vsq = ref_volume, ref_volume ** 2
        warps = [F_.homo_warping(feat[ids[:, j]], eye, eye, depth) for j in range(2)]
        assert all(isinstance(w, lazywarp.LazyVolume) and tuple(w.shape) == (N, C, D, H, W) for w in warps) and not calls
        for w in warps:
            vsum = vsum + w
            vsq = vsq + w ** 2
        var = vsq.div_(3).sub_(vsum.div_(3).pow_(2))                       # mvsdet.py:467
        assert not isinstance(var, lazywarp.LazyVolume) and lazywarp.stats["fused"] == before["fused"] + 1
        (name, pshape, d), = calls
        assert name == ("plane_sweep_variance_pixel" if pixel else "plane_sweep_variance") and pshape == (N, 2, 4, 4)
        assert d.dim() == depth.dim() and torch.equal(d, depth)
        # two warps on DIFFERENT depth tensors are not one sweep: the identity test refuses, the eager kernels run
        calls.clear()
        w0, w1 = F_.homo_warping(feat[ids[:, 0]], eye, eye, depth), F_.homo_warping(feat[ids[:, 1]], eye, eye, depth.clone())
        out = (ref_volume ** 2 + w0 ** 2 + w1 ** 2).div_(3).sub_((ref_volume + w0 + w1).div_(3).pow_(2))
        assert not isinstance(out, lazywarp.LazyVolume)
        assert calls and set(calls) == {"homo_warp_pixel" if pixel else "homo_warp"}


def test_fake_kernels_autocast_rule_and_refusals():
    from mvsdet_amd import ops
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    N, K, C, D, H, W = 3, 2, 40, 5, 9, 21
    nbr = m(N, K, dtype=torch.int64)
    assert torch.ops.mvsdet_amd.homo_warp_pixel(m(N, C, H, W), m(N, 4, 4), m(N, D, H, W)).shape == (N, C, D, H, W)
    assert torch.ops.mvsdet_amd.plane_sweep_variance_pixel(m(N, C, H, W), nbr, m(N, K, 4, 4), m(N, D, H, W)).shape == (N, C, D, H, W)
    assert torch.ops.mvsdet_amd.plane_sweep_variance_pixel_packed(m(N * 2 * H * W * 32), nbr, m(N, K, 4, 4), m(N, D, H, W), C).shape \
        == (N, C, D, H, W)
    assert torch.ops.mvsdet_amd.homo_warp_pixel_backward(m(N, 4, 4), m(N, D, H, W), m(N, C, D, H, W)).shape == (N, C, H, W)
    assert torch.ops.mvsdet_amd.plane_sweep_variance_pixel_backward(m(N, C, H, W), nbr, m(N, K, 4, 4), m(N, D, H, W),
                                                                    m(N, C, D, H, W)).shape == (N, C, H, W)
    assert {op._qualname.split("::")[1] for op in ops.AUTOCAST_FP32_PIXEL_OPS} == {"homo_warp_pixel", "plane_sweep_variance_pixel"}
    for op in ops.AUTOCAST_FP32_PIXEL_OPS:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op._qualname, "AutocastCUDA")
    assert {op._qualname.split("::")[1] for op in ops.AUTOCAST_FP32_OPS} == {
        "homo_warp", "plane_sweep_variance", "plane_sweep_variance_keep", "depth_prob_topk", "sample_depth_prob", "backproject_weigh",
        "backproject_weigh_mean"}
    # the operators have no CPU path (the dispatcher finds no kernel), and the plane operators still refuse a 4-D depth
    with pytest.raises(RuntimeError):
        ops.homo_warp_pixel(torch.zeros(1, 1, 2, 2), torch.zeros(1, 4, 4), torch.zeros(1, 1, 2, 2))
    import inspect
    assert 'depth, "depth", dim=2' in inspect.getsource(ops.sweep._check_sweep)


@pytest.fixture(scope="module")
def lib():
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_c_entries_refuse_null_and_bad_shapes(lib):
    """The five C entries of the per-pixel form: MVSDET_ERR_INVALID_ARG (1) and a message, before anything is launched (the
    pointers are never dereferenced; no GPU here)."""
    p, ws = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    err = lambda: lib.mvsdet_last_error()
    assert lib.mvsdet_homo_warp_pixel_f32(p, p, None, p, 1, 1, 1, 2, 2, None) == 1 and b"NULL" in err()
    assert lib.mvsdet_homo_warp_pixel_f32(p, p, p, p, 1, 1, 1, 1, 2, None) == 1 and b"bad shape" in err()
    assert lib.mvsdet_homo_warp_pixel_f32(p, p, p, p, 70000, 1, 1, 2, 2, None) == 1 and b"65535" in err()
    assert lib.mvsdet_homo_warp_pixel_f32(p, p, p, p, 1, 1, 512, 2048, 2048, None) == 1 and b"2^31" in err()
    assert lib.mvsdet_plane_sweep_variance_pixel_packed_f32(None, p, p, p, p, 2, 2, 4, 3, 8, 8, None) == 1 and b"NULL" in err()
    assert lib.mvsdet_plane_sweep_variance_pixel_packed_f32(p, p, p, None, p, 2, 2, 4, 3, 8, 8, None) == 1 and b"NULL" in err()
    assert lib.mvsdet_plane_sweep_variance_pixel_packed_f32(p, p, p, p, p, 2, 9, 4, 3, 8, 8, None) == 1 and b"K=9" in err()
    assert lib.mvsdet_plane_sweep_variance_pixel_packed_f32(p, p, p, p, p, 2, 2, 4, 3, 8, 1, None) == 1 and b"bad shape" in err()
    assert lib.mvsdet_plane_sweep_variance_pixel_packed_f32(p, p, p, p, p, 2, 2, 4, 513, 8, 8, None) == 1 and b"D >" in err()
    assert lib.mvsdet_plane_sweep_variance_pixel_packed_f32(p, p, p, p, p, 2, 2, 4, 3, 5000, 5000, None) == 1 and b"2^31" in err()
    assert lib.mvsdet_plane_sweep_variance_pixel_packed_f32(p, p, p, p, p, 1 << 20, 2, 4, 3, 2000, 2000, None) == 1 and b"grid" in err()
    need = lib.mvsdet_plane_sweep_pixel_bwd_workspace_bytes(3, 40, 9, 21)
    assert need == (lib.mvsdet_packed_bytes(3, 40, 9, 21) + 255) // 256 * 256 == 3 * 2 * 189 * 128
    bwd = lib.mvsdet_plane_sweep_variance_pixel_bwd_packed_f32
    assert bwd(p, p, p, p, p, None, ws, need, 3, 2, 40, 5, 9, 21, None) == 1 and b"NULL" in err()
    assert bwd(p, p, p, p, p, p, None, need, 3, 2, 40, 5, 9, 21, None) == 1 and b"NULL" in err()
    assert bwd(p, None, p, p, p, p, ws, need, 3, 2, 40, 5, 9, 21, None) == 1 and b"NULL" in err()
    assert bwd(p, p, p, p, p, p, ws, need, 3, 5, 40, 5, 9, 21, None) == 1 and b"K=5" in err()
    assert bwd(p, p, p, p, p, p, ws, need, 3, 2, 40, 0, 9, 21, None) == 1 and b"bad shape" in err()
    assert bwd(p, p, p, p, p, p, ws, need - 1, 3, 2, 40, 5, 9, 21, None) == 2 and b"workspace" in err()
    assert bwd(p, p, p, p, p, p, ctypes.c_void_p(8196), need, 3, 2, 40, 5, 9, 21, None) == 1 and b"aligned" in err()
    wb = lib.mvsdet_homo_warp_pixel_bwd_f32
    assert wb(p, p, None, p, ws, need, 3, 40, 5, 9, 21, None) == 1 and b"NULL" in err()
    assert wb(p, p, p, p, ws, need, 3, 40, 5, 1, 21, None) == 1 and b"bad shape" in err()
    assert wb(p, p, p, p, ws, need - 1, 3, 40, 5, 9, 21, None) == 2 and b"workspace" in err()
