"""The group-wise correlation cost volume (mvs_models/lss_fpn.py:499-506 around homo_warping), host side: the CPU restatement
against fixture G23, what `functional.groupwise_correlation` hands to the operator, the refusals, the fake kernels and the
argument checks of the two C entries.  No GPU here; tests/test_gpu_groupcorr.py runs the kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import groupcorr_restated as GR
import sweep_pixel_restated as SP

G23 = [(tag, kind, G) for tag, gs in (("n3_d8", (1, 2, 4, 8)), ("n6_d12_arkit", (1, 2))) for kind in ("plane", "pixel") for G in gs]


def g23_inputs(tag, kind, G):
    """(fixture, feat, nbr, proj, depth) of a G23 case: the scene of G2, the depths G23 was generated on."""
    g2, g = load_golden("g2_variance_" + tag), load_golden(f"g23_groupcorr_{tag}_{kind}_g{G}")
    feat, nbr, proj = (torch.from_numpy(g2[k]) for k in ("feature", "neighbor_ids", "proj_rel"))
    if kind == "plane":
        depth = torch.from_numpy(g2["depth_values"][:, int(g["first_plane"]):]).contiguous()
    else:
        depth = torch.from_numpy(load_golden(f"g22_sweep_pixel_{tag}_rough")["depth"])
    return g, feat, nbr, proj, depth


@pytest.mark.parametrize("tag,kind,G", G23)
def test_restatement_matches_g23(tag, kind, G):
    """tests/groupcorr_restated.py reproduces what the reference returned (1e-5), and the fixture meets its own conditions."""
    g, feat, nbr, proj, depth = g23_inputs(tag, kind, G)
    N, C, H, W = feat.shape
    assert int(g["groups"]) == G and int(g["inline_restated"]) == 1 and str(g["kind"]) == kind
    assert float(g["min_abs_z"]) >= 0.05 and np.isfinite(g["corr"]).all() and np.isfinite(g["grad_feature"]).all()
    assert os.path.getsize(os.path.join(GOLDEN, f"g23_groupcorr_{tag}_{kind}_g{G}.npz")) < (1 << 20)
    d4 = GR.depth4(depth, H, W)
    assert min(float(SP.sample_grid(proj[:, j], d4, H, W)[1].abs().min()) for j in range(nbr.shape[1])) >= 0.05
    gs, ds = int(g["group_stride"]), int(g["depth_stride"])
    got = GR.groupcorr(feat, nbr, proj, depth, G)
    assert got.shape == (N, nbr.shape[1], G, depth.shape[1], H, W) and g["corr"].shape == got[:, :, ::gs, ::ds].shape
    err = float((got[:, :, ::gs, ::ds] - torch.from_numpy(g["corr"]).double()).abs().max())
    print(f"G23 {tag}/{kind}/G={G}: restated {err:.2e}")
    assert err <= 1e-5


def test_restatement_on_a_broadcast_depth_has_the_same_bits():
    g, feat, nbr, proj, dv = g23_inputs("n6_d12_arkit", "plane", 2)
    d4 = dv[:, :, None, None].expand(-1, -1, *feat.shape[2:]).contiguous()
    assert torch.equal(GR.groupcorr(feat, nbr, proj, dv, 2), GR.groupcorr(feat, nbr, proj, d4, 2))
    assert torch.equal(GR.groupcorr(feat, nbr, proj, dv, 2, torch.float32), GR.groupcorr(feat, nbr, proj, d4, 2, torch.float32))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("pixel", [False, True])
def test_groupwise_correlation_hands_the_operator_fp32_projections_and_a_contiguous_depth(monkeypatch, half, pixel):
    """The fp32 relative projections of module.py:116, one per neighbour, and the contiguous depth of either dim reach
    ops.sweep.plane_sweep_groupcorr (recorded, not run) -- also from float16 inputs under autocast; reduce="mean" is the mean over dim 1."""
    from mvsdet_amd import functional as F_, ops
    N, K, C, D, H, W, G = 3, 2, 16, 4, 5, 6, 2
    gen = torch.Generator().manual_seed(4)
    fake = torch.randn(N, K, G, D, H, W, generator=gen)
    seen = []
    monkeypatch.setattr(ops.sweep, "plane_sweep_groupcorr", lambda *a: seen.append(a) or fake)
    if half:
        monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    dt = torch.float16 if half else torch.float32
    feat = torch.randn(N, C, H, W, generator=gen).to(dt)
    ids = torch.tensor([[1, 2], [0, 0], [2, 1]])
    ref_proj = torch.eye(4).repeat(N, 1, 1) + 0.1 * torch.randn(N, 4, 4, generator=gen)
    nei = tuple(torch.eye(4).repeat(N, 1, 1) + 0.1 * torch.randn(N, 4, 4, generator=gen) for _ in range(K))
    if pixel:
        depth = (1.0 + torch.rand(N, H, W, D, generator=gen)).to(dt).permute(0, 3, 1, 2)      # (N,D,H,W), not contiguous
    else:
        depth = (1.0 + torch.rand(D, N, generator=gen)).to(dt).t()                            # (N,D), not contiguous
    assert not depth.is_contiguous()
    out = F_.groupwise_correlation(feat, ids, ref_proj, nei, depth, G)
    assert out is fake
    (f, i, p, d, groups), = seen
    assert f.dtype == p.dtype == d.dtype == torch.float32 and groups == G and torch.equal(i, ids) and torch.equal(f, feat.float())
    assert torch.equal(p, torch.stack([torch.matmul(n_, torch.inverse(ref_proj)) for n_ in nei], dim=1))
    assert d.dim() == (4 if pixel else 2) and d.is_contiguous() and torch.equal(d, depth.float())
    mean = F_.groupwise_correlation(feat, ids, ref_proj, nei, depth, G, reduce="mean")
    assert mean.shape == (N, G, D, H, W) and torch.equal(mean, fake.mean(dim=1))


def test_refusals():
    from mvsdet_amd import functional as F_, ops
    eye = torch.eye(4).repeat(2, 1, 1)
    ids = torch.tensor([[1], [0]])
    call = lambda C, G, depth=None, nei=(eye,), ids=ids, **k: F_.groupwise_correlation(
        torch.zeros(2, C, 5, 6), ids, eye, nei, torch.ones(2, 4) if depth is None else depth, G, **k)
    for C, G in [(32, 5), (32, 0), (8, 8), (8, 4), (48, 4), (48, 2), (48, 1), (96, 2), (40, 20)]:   # C % G; Cg = 1, 2, 12, 24, 48, 48, 2
        with pytest.raises(ValueError, match="4, 8, 16"):
            call(C, G)
    for cg in (1, 2, 12, 24, 48):
        with pytest.raises(ValueError, match="multiple of 32"):
            ops.sweep._check_groups("t", 2 * cg, 2)
    for C, G in [(32, 8), (32, 4), (32, 2), (32, 1), (40, 10), (40, 5), (48, 3), (96, 1), (96, 3), (256, 8), (256, 32), (64, 1)]:
        ops.sweep._check_groups("t", C, G)
    with pytest.raises(ValueError):                                       # K = 0
        call(32, 4, nei=(), ids=torch.zeros(2, 0, dtype=torch.int64))
    for shape in [(2, 4, 5, 7), (2, 4, 6, 5), (3, 4, 5, 6), (3, 4), (2, 4, 30), (8,), (2, 1, 4, 5, 6)]:
        with pytest.raises(ValueError):
            call(32, 4, depth=torch.ones(shape))
    with pytest.raises(ValueError, match="reduce"):
        call(32, 4, reduce="sum")


def test_fake_kernels_and_autocast_rule():
    from mvsdet_amd import ops
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    N, K, C, D, H, W, G = 3, 2, 40, 5, 9, 21, 10
    nbr = m(N, K, dtype=torch.int64)
    for depth in (m(N, D), m(N, D, H, W)):
        out = torch.ops.mvsdet_amd.plane_sweep_groupcorr(m(N, C, H, W), nbr, m(N, K, 4, 4), depth, G)
        assert out.shape == (N, K, G, D, H, W) and out.dtype == torch.float32
        out = torch.ops.mvsdet_amd.plane_sweep_groupcorr_packed(m(N * 2 * H * W * 32), nbr, m(N, K, 4, 4), depth, C, G, H, W)
        assert out.shape == (N, K, G, D, H, W) and out.dtype == torch.float32
        out = torch.ops.mvsdet_amd.plane_sweep_groupcorr_backward(m(N, C, H, W), nbr, m(N, K, 4, 4), depth, m(N, K, G, D, H, W), G)
        assert out.shape == (N, C, H, W) and out.dtype == torch.float32
    assert torch.ops.mvsdet_amd.plane_sweep_groupcorr_packed(m(N * 2 * H * W * 32), nbr, m(N, K, 4, 4), m(N, D, H, W), C, G).shape \
        == (N, K, G, D, H, W)
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mvsdet_amd::plane_sweep_groupcorr", "AutocastCUDA")
    with pytest.raises(RuntimeError):       # no CPU path: the dispatcher finds no kernel
        ops.sweep.plane_sweep_groupcorr(torch.zeros(1, 4, 2, 2), torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1, 4, 4), torch.ones(1, 1), 1)


@pytest.fixture(scope="module")
def lib():
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_c_entries_refuse_null_and_bad_arguments(lib):
    """MVSDET_ERR_INVALID_ARG (1) or MVSDET_ERR_WORKSPACE (2) and a message, before anything is launched (the device pointers are
    never dereferenced; no GPU here)."""
    p, ws = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    err = lambda: lib.mvsdet_last_error()
    ds = (ctypes.c_int64 * 3)(5 * 189, 189, 1)
    fwd = lib.mvsdet_plane_sweep_groupcorr_packed_f32
    N, K, C, G, D, H, W = 3, 2, 40, 10, 5, 9, 21
    assert fwd(None, p, p, p, ds, p, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert fwd(p, p, p, p, ds, None, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert fwd(p, None, p, p, ds, p, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert fwd(p, p, p, None, ds, p, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert fwd(p, p, p, p, None, p, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert fwd(p, p, p, p, ds, p, N, 0, C, G, D, H, W, None) == 1 and b"K=0" in err()
    assert fwd(p, p, p, p, ds, p, N, 5, C, G, D, H, W, None) == 1 and b"K=5" in err()
    assert fwd(p, p, p, p, ds, p, N, K, C, G, D, H, 1, None) == 1 and b"bad shape" in err()
    assert fwd(p, p, p, p, ds, p, N, K, C, G, 513, H, W, None) == 1 and b"D >" in err()
    for c, g in [(40, 3), (40, 0), (40, 40), (40, 20), (48, 4), (48, 2), (48, 1)]:
        assert fwd(p, p, p, p, ds, p, N, K, c, g, D, H, W, None) == 1 and b"4, 8, 16" in err() and b"multiple of 32" in err()
    assert fwd(p, p, p, p, ds, p, N, K, C, G, 3, 5000, 5000, None) == 1 and b"2^31" in err()
    assert fwd(p, p, p, p, ds, p, 70000, K, C, G, D, H, W, None) == 1 and b"65535" in err()
    assert fwd(p, p, p, p, (ctypes.c_int64 * 3)(945, -189, 1), p, N, K, C, G, D, H, W, None) == 1 and b"stride" in err()
    need = lib.mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W)
    bwd = lib.mvsdet_plane_sweep_groupcorr_bwd_packed_f32
    assert bwd(p, p, p, p, ds, p, None, ws, need, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert bwd(p, p, p, p, ds, None, p, ws, need, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert bwd(p, p, p, p, ds, p, p, None, need, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert bwd(p, None, p, p, ds, p, p, ws, need, N, K, C, G, D, H, W, None) == 1 and b"NULL" in err()
    assert bwd(p, p, p, p, ds, p, p, ws, need, N, 0, C, G, D, H, W, None) == 1 and b"K=0" in err()
    assert bwd(p, p, p, p, ds, p, p, ws, need, N, K, C, 3, D, H, W, None) == 1 and b"4, 8, 16" in err()
    assert bwd(p, p, p, p, ds, p, p, ws, need, N, K, C, G, 0, H, W, None) == 1 and b"bad shape" in err()
    assert bwd(p, p, p, p, ds, p, p, ws, need - 1, N, K, C, G, D, H, W, None) == 2 and b"workspace" in err()
    assert bwd(p, p, p, p, ds, p, p, ctypes.c_void_p(8196), need, N, K, C, G, D, H, W, None) == 1 and b"aligned" in err()
