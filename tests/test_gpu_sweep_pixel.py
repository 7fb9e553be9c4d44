"""The per-pixel form of the sweep on the GPU (csrc/planesweep_pixel.hip): homo_warping with depth_values (B,D,H,W) and the
fused variance around it, forward and backward.

  1. broadcast identity -- a (B,D) depth broadcast to (B,D,H,W) gives the plane operators' bits (and the device-rounding oracle's);
  2. palette identity   -- every (pixel, hypothesis) picks one of 6 depths (three ordinary, one negative, +inf, NaN): the bits of
                           the plane operator run on the 6 values as planes, gathered per pixel (NaN equal to NaN);
  3. fixture G22        -- the reference's own output on smooth and rough per-pixel depth maps, at the project's forward bar;
  4. gradients          -- against the float64 gradient of tests/sweep_pixel_restated.py;
  5. contention         -- every tap gradient of a neighbour into four texels;
  6. guarded memory     -- the five C entries inside tests/canvas.py frames;
  7. the deferred route -- the reference's variance loop with a 4-D depth collapses into one fused pixel launch.

Shapes (N, K, C, D, H, W): S-odd (3, 2, 40, 5, 9, 21) partial tiles, W % 4 != 0, a partial second slab; S-fast (2, 1, 32, 1, 8, 32)
the whole-vector stores; S-80 (4, 2, 64, 12, 16, 80) the width at which the plane kernel picks its other tile shape.  Neighbour
ids include a view that is its own neighbour and a repeated neighbour.

Gradient bound (rule 4): |g - g64| <= max(1e-4 |g64| + 1.25e-6 max|g64|, 4 x grad_err_fp32 of G22) -- the project's stage-1 bar
(test_backward_stage1_shapes: 2e-5 at scale 16) made relative to scale, or four times the reference's own fp32 summation error
(atomics arrive in any order)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
import sweep_pixel_restated as SP
from pixel_scenes import check_grad as _check_grad, scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from lcg import lcg_uniform  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4   # the project's forward bar (test_gpu_parity.py)
SHAPES = {"S-odd": (3, 2, 40, 5, 9, 21), "S-fast": (2, 1, 32, 1, 8, 32), "S-80": (4, 2, 64, 12, 16, 80)}
NBR = {"S-odd": [[0, 1], [2, 2], [1, 0]], "S-fast": [[1], [1]], "S-80": [[1, 2], [1, 1], [3, 3], [0, 2]]}
# two small shapes of this file's own for the broadcast identity: the K = 3 and K = 4 instantiations (two decode passes)
SHAPES.update({"S-k3": (4, 3, 16, 2, 6, 10), "S-k4": (5, 4, 8, 3, 6, 10)})
NBR.update({"S-k3": [[1, 2, 3], [0, 0, 2], [2, 3, 1], [0, 1, 2]], "S-k4": [[1, 2, 3, 4], [0, 0, 2, 2], [2, 3, 4, 0], [4, 1, 1, 0], [3, 2, 1, 0]]})
G22 = [(tag, fam) for tag in ("n3_d8", "n6_d12_arkit") for fam in ("smooth", "rough")]


def _scene(name):
    return scene(SHAPES[name], NBR[name])


def _same(a, b, what):
    """Equal bit for bit; a NaN for a NaN."""
    assert a.shape == b.shape, what
    bad = ~((a == b) | (torch.isnan(a) & torch.isnan(b)))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ"


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(SHAPES))
def test_broadcast_depth_gives_the_plane_operators_bits(gpu, oracle, name):
    from mvsdet_amd import ops
    N, K, C, D, H, W = SHAPES[name]
    feat, nbr, proj, depth2 = _scene(name)
    f, i, p, d2 = feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth2.to(gpu)
    d4 = d2[:, :, None, None].expand(N, D, H, W)            # the operators make it contiguous
    for j in range(K):
        src, pj = f[i[:, j]], p[:, j].contiguous()
        assert torch.equal(ops.homo_warp_pixel(src, pj, d4), ops.homo_warp(src, pj, d2)), f"warp of neighbour {j}"
    var = ops.plane_sweep_variance_pixel(f, i, p, d4)
    assert torch.equal(var, ops.plane_sweep_variance(f, i, p, d2))
    assert torch.equal(var.cpu(), torch.from_numpy(oracle.plane_sweep_variance(feat, nbr, proj, depth2, mode=1)))
    assert torch.equal(var, ops.plane_sweep_variance_pixel_packed(ops.pack_features(f), i, p, d4.contiguous(), C))


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["S-odd", "S-80"])
def test_palette_of_depths_gives_the_plane_operators_bits_per_pixel(gpu, name):
    """Scattered footprints, zero padding, samples behind the camera and non-finite depths: a non-finite depth at one pixel
    must not touch its neighbours."""
    from mvsdet_amd import ops
    N, K, C, D, H, W = SHAPES[name]
    feat, nbr, proj, _ = _scene(name)
    f, i, p = feat.to(gpu), nbr.to(gpu), proj.to(gpu)
    palette = torch.tensor([0.7, 1.9, 3.3, -1.2, float("inf"), float("nan")])
    pick = torch.from_numpy(((lcg_uniform(N * D * H * W, 77).astype(np.float64) + 1.0) * 3.0).astype(np.int64).clip(0, 5)).reshape(N, D, H, W)
    assert all(int((pick == k).sum()) > 0 for k in range(6))
    d4 = palette[pick].to(gpu)
    planes = palette[None].repeat(N, 1).to(gpu)
    gather = pick.to(gpu)[:, None].expand(N, C, D, H, W)
    for j in range(K):
        src, pj = f[i[:, j]], p[:, j].contiguous()
        _same(ops.homo_warp_pixel(src, pj, d4), torch.gather(ops.homo_warp(src, pj, planes), 2, gather), f"warp of neighbour {j}")
    var = ops.plane_sweep_variance_pixel(f, i, p, d4)
    _same(var, torch.gather(ops.plane_sweep_variance(f, i, p, planes), 2, gather), "variance")
    finite = torch.isfinite(d4)[:, None].expand(N, C, D, H, W)
    assert bool(torch.isfinite(var[finite]).all()) and bool(torch.isnan(var[~finite]).all())


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("tag,family", G22)
def test_g22_forward(gpu, tag, family):
    from mvsdet_amd import functional as F_, ops
    g2, g = load_golden("g2_variance_" + tag), load_golden(f"g22_sweep_pixel_{tag}_{family}")
    feat, nbr, proj = (torch.from_numpy(g2[k]).to(gpu) for k in ("feature", "neighbor_ids", "proj_rel"))
    depth, cs = torch.from_numpy(g["depth"]).to(gpu), int(g["channel_stride"])
    want_w, want_v = torch.from_numpy(g["warped"]), torch.from_numpy(g["variance"])
    src = feat[nbr[:, 0]]
    warped = ops.homo_warp_pixel(src, proj[:, 0].contiguous(), depth)
    var = ops.plane_sweep_variance_pixel(feat, nbr, proj, depth)
    via_f = F_.homo_warping(src, torch.from_numpy(g2["nei_projs"][:, 0]), torch.from_numpy(g2["ref_proj"]), depth)
    errs = [float((t[:, ::cs].cpu() - w).abs().max()) for t, w in ((warped, want_w), (var, want_v), (via_f, want_w))]
    print(f"G22 {tag}/{family}: warp {errs[0]:.2e} variance {errs[1]:.2e} functional.homo_warping {errs[2]:.2e}")
    assert all(torch.isfinite(t).all() for t in (warped, var, via_f)) and max(errs) <= TOL


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("tag,family", G22)
def test_g22_gradients(gpu, tag, family):
    # measured on an MI355X: max |g - g64| 1.20e-5 / 1.25e-5 (n3_d8 smooth / rough, max |g64| 9.2 / 8.1) and 3.4e-6 / 3.5e-6 (arkit, 9.1 / 8.8):
    # 0.21 / 0.15 / 0.15 / 0.15 of the bound
    from mvsdet_amd import ops
    g2, g = load_golden("g2_variance_" + tag), load_golden(f"g22_sweep_pixel_{tag}_{family}")
    feat, nbr, proj = (torch.from_numpy(g2[k]) for k in ("feature", "neighbor_ids", "proj_rel"))
    depth = torch.from_numpy(g["depth"])
    N, C, H, W = feat.shape
    D = depth.shape[1]
    R = torch.from_numpy(lcg_uniform(N * C * D * H * W, int(g["R_seed"]))).reshape(N, C, D, H, W)
    f64 = feat.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((SP.variance_pixel_f64(f64, nbr, proj, depth) * R.double()).sum(), f64)
    # the fixture's fp32 gradient is the reference's: its distance to float64 is what the fixture says it is
    cs = int(g["channel_stride"])
    assert float((torch.from_numpy(g["grad_feature"]).double() - g64[:, ::cs]).abs().max()) <= float(g["grad_err_fp32"]) * (1 + 1e-6)
    f = feat.to(gpu).requires_grad_(True)
    (ops.plane_sweep_variance_pixel(f, nbr.to(gpu), proj.to(gpu), depth.to(gpu)) * R.to(gpu)).sum().backward()
    _check_grad(f.grad, g64, float(g["grad_err_fp32"]), f"variance gradient, G22 {tag}/{family}")


def test_gradients_of_the_plane_backward_and_the_pixel_warp(gpu):
    """The same bound for the existing plane backward on a broadcast depth, the pixel backward on that depth, and
    homo_warp_pixel's own backward (G22 n6_d12_arkit).  Measured on an MI355X: 3.5e-6, 3.3e-6 and 5.5e-6 (0.22, 0.20, 0.24 of the bound)."""
    from mvsdet_amd import ops
    g2, g = load_golden("g2_variance_n6_d12_arkit"), load_golden("g22_sweep_pixel_n6_d12_arkit_rough")
    feat, nbr, proj, d2 = (torch.from_numpy(g2[k]) for k in ("feature", "neighbor_ids", "proj_rel", "depth_values"))
    err = float(g["grad_err_fp32"])
    N, C, H, W = feat.shape
    D = d2.shape[1]
    d4 = d2[:, :, None, None].expand(N, D, H, W).contiguous()
    R = torch.from_numpy(lcg_uniform(N * C * D * H * W, int(g["R_seed"]))).reshape(N, C, D, H, W)
    f64 = feat.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((SP.variance_pixel_f64(f64, nbr, proj, d4) * R.double()).sum(), f64)
    for what, op, depth in (("plane backward", ops.plane_sweep_variance, d2), ("pixel backward", ops.plane_sweep_variance_pixel, d4)):
        f = feat.to(gpu).requires_grad_(True)
        (op(f, nbr.to(gpu), proj.to(gpu), depth.to(gpu)) * R.to(gpu)).sum().backward()
        _check_grad(f.grad, g64, err, what + " on the broadcast depth")
    depth = torch.from_numpy(g["depth"])
    src = feat[nbr[:, 1]]
    s64 = src.double().requires_grad_(True)
    (w64,) = torch.autograd.grad((SP.homo_warp_pixel_f64(s64, proj[:, 1], depth) * R.double()).sum(), s64)
    s = src.to(gpu).requires_grad_(True)
    (ops.homo_warp_pixel(s, proj[:, 1].contiguous().to(gpu), depth.to(gpu)) * R.to(gpu)).sum().backward()
    _check_grad(s.grad, w64, err, "homo_warp_pixel backward, G22 rough")


# ---------------------------------------------------------------------------------------------------------------- 5
def test_contention_all_taps_of_a_view_in_four_texels(gpu):
    """Every depth 1e6 and a projection whose rotation block is zero: every sample of a batch row lands on ONE position, so
    all H*W*D = 945 tap gradients of a channel go into that position's texels: four in row 0, one in row 1 (a corner: the other
    three taps are padding), two in row 2 (the right border).  R in (0.5, 1.5) and bilinear weights >= 0: all terms are
    positive, so any fp32 summation order is within n 2^-24 < 1e-4 relative of the exact sum -- rtol 1e-4, no absolute term
    (derived, not measured; the MI355X gave 2.5e-6)."""
    from mvsdet_amd import ops
    N, K, C, D, H, W = SHAPES["S-odd"]
    feat = torch.from_numpy(lcg_uniform(N * C * H * W, 9)).reshape(N, C, H, W)
    proj = torch.zeros(N, 4, 4)
    proj[:, 3, 3] = 1.0
    proj[:, 2, 3] = 1.0                                       # Z = 1
    proj[:, 0, 3] = torch.tensor([7.3, 0.2, 19.6])            # the one sample position of each batch row (the last: on the border)
    proj[:, 1, 3] = torch.tensor([3.4, 7.9, 5.5])
    depth = torch.full((N, D, H, W), 1e6)
    R = (torch.from_numpy(lcg_uniform(N * C * D * H * W, 10)).reshape(N, C, D, H, W) + 2.0) / 2.0
    assert float(R.min()) >= 0.5 and float(R.max()) <= 1.5
    s64 = feat.double().requires_grad_(True)
    (w64,) = torch.autograd.grad((SP.homo_warp_pixel_f64(s64, proj, depth) * R.double()).sum(), s64)
    assert int((w64 != 0).sum()) == C * (4 + 1 + 2) and float(w64.min()) >= 0
    s = feat.to(gpu).requires_grad_(True)
    (ops.homo_warp_pixel(s, proj.to(gpu), depth.to(gpu)) * R.to(gpu)).sum().backward()
    got = s.grad.double().cpu()
    rel = ((got - w64).abs() / w64.abs().clamp_min(1e-300))[w64 != 0]
    print(f"contention: max relative error {float(rel.max()):.3e}")
    assert bool((got[w64 == 0] == 0).all()) and float(rel.max()) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- 6
def test_c_entries_in_guarded_memory(gpu):
    """The five C entries on S-odd: features as a strided view in a NaN canvas (packed by mvsdet_pack_features_f32), packed maps,
    outputs and workspaces exactly as long as the ABI says between sentinel guards, pre-filled with NaN: guards intact, the
    bits of the plain call (the tolerance of the gradient tests for the float atomics), everything overwritten; a neighbour
    id outside [0, N) reads inside the packed maps (it is clamped)."""
    from canvas import Guarded, guarded_f32, nan_view, ok, strides
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    N, K, C, D, H, W = SHAPES["S-odd"]
    feat, nbr, proj, d2 = _scene("S-odd")
    depth = (d2[:, :, None, None] + 0.3 * torch.from_numpy(lcg_uniform(N * D * H * W, 31)).reshape(N, D, H, W)).contiguous()
    f, i, p, d = feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu)
    R = torch.from_numpy(lcg_uniform(N * C * D * H * W, 32)).reshape(N, C, D, H, W).to(gpu)
    NAN = 0x7FC00000

    def out(shape):
        g, v = guarded_f32(shape, gpu)
        g.region.fill_(NAN)
        return g, v
    _canvas, fv = nan_view(feat.unsqueeze(2), gpu)
    fv = fv[:, :, 0]
    pk_g, pk = out((lib.mvsdet_packed_bytes(N, C, H, W) // 4,))
    ok(lib.mvsdet_pack_features_f32(_lib.ptr(fv), strides(fv), pk_g.ptr(), N, C, H, W, None))
    assert pk_g.guards_intact() and torch.equal(pk, ops.pack_features(f))
    # forward variance; then with ids outside [0, N): clamped to 0 and N - 1
    var_g, var = out((N, C, D, H, W))
    ok(lib.mvsdet_plane_sweep_variance_pixel_packed_f32(pk_g.ptr(), _lib.ptr(i), _lib.ptr(p), _lib.ptr(d), var_g.ptr(), N, K, C, D, H, W, None))
    plain = ops.plane_sweep_variance_pixel(f, i, p, d)
    assert var_g.guards_intact() and torch.equal(var, plain) and bool(torch.isfinite(var).all())
    wild = i.clone()
    wild[0, 0], wild[2, 1] = -5, N + 3
    var_g.region.fill_(NAN)
    ok(lib.mvsdet_plane_sweep_variance_pixel_packed_f32(pk_g.ptr(), _lib.ptr(wild), _lib.ptr(p), _lib.ptr(d), var_g.ptr(), N, K, C, D, H, W, None))
    assert var_g.guards_intact() and torch.equal(var, ops.plane_sweep_variance_pixel(f, wild.clamp(0, N - 1), p, d))
    # compatibility warp
    src, pj = f[i[:, 1]].contiguous(), p[:, 1].contiguous()
    wp_g, wp = out((N, C, D, H, W))
    ok(lib.mvsdet_homo_warp_pixel_f32(_lib.ptr(src), _lib.ptr(pj), _lib.ptr(d), wp_g.ptr(), N, C, D, H, W, None))
    assert wp_g.guards_intact() and torch.equal(wp, ops.homo_warp_pixel(src, pj, d))
    # the two backward passes: gradient and workspace start as NaN
    wbytes = lib.mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W)
    for which in ("variance", "warp"):
        ws_g = Guarded(wbytes // 4, gpu)
        ws_g.region.fill_(NAN)
        gf_g, gf = out((N, C, H, W))
        if which == "variance":
            ok(lib.mvsdet_plane_sweep_variance_pixel_bwd_packed_f32(pk_g.ptr(), _lib.ptr(i), _lib.ptr(p), _lib.ptr(d), _lib.ptr(R), gf_g.ptr(),
                                                                    ws_g.ptr(), wbytes, N, K, C, D, H, W, None))
            plain = ops.plane_sweep_variance_pixel_backward(f, i, p, d, R)
        else:
            ok(lib.mvsdet_homo_warp_pixel_bwd_f32(_lib.ptr(pj), _lib.ptr(d), _lib.ptr(R), gf_g.ptr(), ws_g.ptr(), wbytes, N, C, D, H, W, None))
            plain = ops.homo_warp_pixel_backward(pj, d, R)
        assert gf_g.guards_intact() and ws_g.guards_intact(), which
        assert bool(torch.isfinite(gf).all()) and bool(torch.isfinite(ws_g.region.view(torch.float32)).all()), which
        torch.testing.assert_close(gf, plain, rtol=1e-4, atol=1.25e-6 * float(plain.abs().max()))
    assert pk_g.guards_intact() and torch.equal(pk, ops.pack_features(f))      # the inputs were only read


# ---------------------------------------------------------------------------------------------------------------- 7
def test_reference_variance_loop_with_a_4d_depth_collapses_into_one_pixel_launch(gpu, oracle):
    """mvsdet.py:430-467 (restated as in test_gpu_parity.py) on the patched functions with per-pixel depth_values: one fused
    launch, the bits of ops.plane_sweep_variance_pixel, gradients reach the feature; hotpath.cost_volume(depth=...) is that call."""
    from mvsdet_amd import functional as F_, lazywarp, ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 5, 32, 8, (24, 32)
    hp = MVSDetHotPath([8, 8, 4], [.8, .8, .8], [0.2, 5.0], D)
    meta = synthetic.make_img_meta(N, hw, seed=8)
    geo = hp.prepare_scene(meta, gpu)
    w2c = torch.tensor(np.array(meta["lidar2img"]["extrinsic"]))
    K_feat = torch.tensor(oracle.feat_intrinsics(meta["lidar2img"]["intrinsic"], meta["img_shape"], meta["ori_shape"]))
    c2w = w2c.inverse()
    depth = (geo.depth_values[:, :, None, None]
             + 0.2 * torch.from_numpy(lcg_uniform(N * D * hw[0] * hw[1], 41)).reshape(N, D, *hw).to(gpu)).contiguous()
    feature = synthetic.make_features(N, C, hw, seed=8).to(gpu).requires_grad_(True)
    expected = ops.plane_sweep_variance_pixel(feature.detach(), geo.neighbor_ids, geo.proj_rel, depth)
    assert torch.equal(hp.cost_volume(feature.detach(), geo, depth=depth), expected)
    assert torch.equal(hp.cost_volume(feature.detach(), geo, packed=ops.pack_features(feature.detach()), depth=depth), expected)
    old = F_.LAZY_WARP
    F_.LAZY_WARP = True
    try:
        before = dict(lazywarp.stats)
        k = min(2, N - 1)
        neighbor_ids = F_.get_nearest_pose_ids(c2w, c2w, k, maskself=True)
        ref_volume = feature.unsqueeze(2).repeat(1, 1, D, 1, 1)
        volume_sum = ref_volume
        volume_sq_sum = ref_volume ** 2
        del ref_volume
        nei_features = torch.unbind(feature[neighbor_ids.view(-1)].view(N, k, *feature.shape[1:]), dim=1)
        ref_proj, nei_projs = F_.collect_proj(w2c, K_feat, neighbor_ids)
        for nei_fea, nei_proj in zip(nei_features, nei_projs):
            warped_volume = F_.homo_warping(nei_fea, nei_proj, ref_proj, depth)
            assert isinstance(warped_volume, lazywarp.LazyVolume)
            volume_sum = volume_sum + warped_volume
            volume_sq_sum = volume_sq_sum + warped_volume ** 2
            del warped_volume
        var = volume_sq_sum.div_(k + 1).sub_(volume_sum.div_(k + 1).pow_(2))
        assert type(var) is torch.Tensor and lazywarp.stats["fused"] == before["fused"] + 1
        assert lazywarp.stats["materialized"] == before["materialized"]
        assert torch.equal(neighbor_ids.to(gpu), geo.neighbor_ids) and torch.equal(var, expected)
        var.square().mean().backward()
        g_lazy = feature.grad.clone()
        feature.grad = None
        ops.plane_sweep_variance_pixel(feature, geo.neighbor_ids, geo.proj_rel, depth).square().mean().backward()
        assert float(g_lazy.abs().max()) > 0
        torch.testing.assert_close(g_lazy, feature.grad, rtol=1e-4, atol=1.25e-6 * float(feature.grad.abs().max()))
    finally:
        F_.LAZY_WARP = old
