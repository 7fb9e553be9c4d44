"""The group-wise correlation cost volume on the GPU (csrc/groupcorr.hip), forward and backward, plane and per-pixel depths.

  1. decomposition      -- corr against the float64 mean_c(f * w_j) of the GPU's own homo_warp[_pixel] output w_j;
  2. broadcast identity -- the (N,D) call and its (N,D,H,W) broadcast give the same bits, and so do two runs;
  3. fixture G23        -- the reference's own output, at the project's forward bar, through ops and through functional;
  4. gradients          -- against the float64 gradient of tests/groupcorr_restated.py (G23 and shapes A, C, F);
  5. contention         -- every tap gradient of a (view, neighbour) pair into four texels;
  6. guarded memory     -- the two C entries inside tests/canvas.py frames;
  7. refusals           -- an unsupported group width and a gradient of the wrong shape raise.

Shapes (N, K, C, D, H, W; G): A (3, 2, 40, 5, 9, 21; 10 and 5) Cg 4 and 8, a partial second slab, partial tiles, W % 4 != 0;
B (2, 1, 48, 2, 8, 32; 3) Cg 16, half a slab of padding, the whole-vector stores; C (3, 2, 96, 3, 9, 21; 1 and 3) Cg 96 and 32: a
group over three slabs and one slab per group; D (4, 3, 64, 2, 6, 10; 1) Cg 64, K = 3: the second decode pass; E (4, 2, 64, 12,
16, 80; 8) the 80-wide map; F (5, 4, 32, 2, 6, 10; 8, 4, 2 and 1) Cg 4, 8, 16 and 32: every forward mode at K = 4, half a tile,
test_gpu_sweep_pixel.py's S-k4 neighbours.  Neighbour ids include a view that is its own neighbour and a repeated neighbour.

Bound of rule 1 (derived, not measured): |corr - mean64| <= (Cg + 2) 2^-24 mean_c|f w_j| -- the worst case of Cg fp32 roundings of a
running sum plus the product's and the final scale's.  Gradient bound (rule 4), test_gpu_sweep_pixel.py's:
|g - g64| <= max(1e-4 |g64| + 1.25e-6 max|g64|, 4 x grad_err_fp32), grad_err_fp32 being the reference's own fp32 summation error
(from the fixture; for A, C and F that of the fp32 restatement, computed here).

Measured on an MI355X: rule 1 at most 0.35 of its bound; G23 forward 2.4e-7 through ops, 5.5e-5 through functional;
gradients at most 0.25 of their bound; contention 3.7e-6 relative."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
import groupcorr_restated as GR
from pixel_scenes import check_grad as _check_grad, scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from lcg import lcg_uniform  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4   # the project's forward bar (test_gpu_parity.py)
SHAPES = {"A": (3, 2, 40, 5, 9, 21), "B": (2, 1, 48, 2, 8, 32), "C": (3, 2, 96, 3, 9, 21), "D": (4, 3, 64, 2, 6, 10),
          "E": (4, 2, 64, 12, 16, 80), "F": (5, 4, 32, 2, 6, 10)}
GROUPS = {"A": (10, 5), "B": (3,), "C": (1, 3), "D": (1,), "E": (8,), "F": (8, 4, 2, 1)}
NBR = {"A": [[0, 1], [2, 2], [1, 0]], "B": [[1], [1]], "C": [[0, 1], [2, 2], [1, 0]], "D": [[1, 2, 3], [0, 0, 2], [2, 3, 1], [0, 1, 2]],
       "E": [[1, 2], [1, 1], [3, 3], [0, 2]], "F": [[1, 2, 3, 4], [0, 0, 2, 2], [2, 3, 4, 0], [4, 1, 1, 0], [3, 2, 1, 0]]}
CASES = [(name, G) for name in SHAPES for G in GROUPS[name]]
G23 = [(tag, kind, G) for tag, gs in (("n3_d8", (1, 2, 4, 8)), ("n6_d12_arkit", (1, 2))) for kind in ("plane", "pixel") for G in gs]


def _scene(name):
    return scene(SHAPES[name], NBR[name])


def _palette_depth(name):
    """Every (pixel, hypothesis) picks one of 6 depths: three ordinary, one negative, +inf, NaN."""
    N, K, C, D, H, W = SHAPES[name]
    palette = torch.tensor([0.7, 1.9, 3.3, -1.2, float("inf"), float("nan")])
    pick = torch.from_numpy(((lcg_uniform(N * D * H * W, 77).astype(np.float64) + 1.0) * 3.0).astype(np.int64).clip(0, 5)).reshape(N, D, H, W)
    assert all(int((pick == k).sum()) > 0 for k in range(6))
    return palette[pick].contiguous()


def _rough_depth(name, seed):
    N, K, C, D, H, W = SHAPES[name]
    return (2.3 + 1.7 * torch.from_numpy(lcg_uniform(N * D * H * W, seed)).reshape(N, D, H, W)).contiguous()


def _g23_inputs(tag, kind, G):
    g2, g = load_golden("g2_variance_" + tag), load_golden(f"g23_groupcorr_{tag}_{kind}_g{G}")
    feat, nbr, proj = (torch.from_numpy(g2[k]) for k in ("feature", "neighbor_ids", "proj_rel"))
    if kind == "plane":
        depth = torch.from_numpy(g2["depth_values"][:, int(g["first_plane"]):]).contiguous()
    else:
        depth = torch.from_numpy(load_golden(f"g22_sweep_pixel_{tag}_rough")["depth"])
    return g2, g, feat, nbr, proj, depth


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("pixel", [False, True], ids=["plane", "pixel"])
@pytest.mark.parametrize("name,G", CASES)
def test_decomposition_into_the_gpu_warp_and_a_float64_mean(gpu, name, G, pixel):
    from mvsdet_amd import ops
    N, K, C, D, H, W = SHAPES[name]
    Cg = C // G
    feat, nbr, proj, d2 = _scene(name)
    depth = _palette_depth(name) if pixel else d2
    f, i, p, d = feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu)
    corr = ops.sweep.plane_sweep_groupcorr(f, i, p, d, G)
    assert corr.shape == (N, K, G, D, H, W) and corr.dtype == torch.float32
    f64 = f.double().reshape(N, G, Cg, 1, H, W)
    worst = 0.0
    for j in range(K):
        src, pj = f[i[:, j]], p[:, j].contiguous()
        w = (ops.homo_warp_pixel if pixel else ops.homo_warp)(src, pj, d)
        prod = f64 * w.double().reshape(N, G, Cg, D, H, W)
        want, scale = prod.mean(dim=2), prod.abs().mean(dim=2)
        got = corr[:, j].double()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), f"neighbour {j}: NaN where the float64 value is none, or none where it is"
        fin = ~torch.isnan(want)
        assert bool(torch.isfinite(got[fin]).all())
        bound = (Cg + 2) * 2.0 ** -24 * scale[fin]
        err = (got[fin] - want[fin]).abs()
        assert bool((err <= bound).all()), f"neighbour {j}: {int((err > bound).sum())} elements outside the bound, worst {float((err - bound).max()):.3e}"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    if pixel:
        fin_d = torch.isfinite(d)[:, None, None].expand(N, K, G, D, H, W)
        assert bool(torch.isfinite(corr[fin_d]).all()) and bool(torch.isnan(corr[~fin_d]).all())
    print(f"decomposition {name} G={G} {'pixel' if pixel else 'plane'}: worst ratio to the bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name,G", CASES)
def test_broadcast_depth_and_a_second_run_give_the_same_bits(gpu, name, G):
    from mvsdet_amd import ops
    N, K, C, D, H, W = SHAPES[name]
    feat, nbr, proj, d2 = _scene(name)
    f, i, p, d2 = feat.to(gpu), nbr.to(gpu), proj.to(gpu), d2.to(gpu)
    d4 = d2[:, :, None, None].expand(N, D, H, W)            # the operator makes it contiguous
    plane = ops.sweep.plane_sweep_groupcorr(f, i, p, d2, G)
    assert bool(torch.isfinite(plane).all())
    assert torch.equal(plane, ops.sweep.plane_sweep_groupcorr(f, i, p, d4, G))
    assert torch.equal(plane, ops.sweep.plane_sweep_groupcorr(f, i, p, d2, G))
    assert torch.equal(plane, ops.sweep.plane_sweep_groupcorr_packed(ops.pack_features(f), i, p, d2, C, G, H, W))
    assert torch.equal(plane, ops.sweep.plane_sweep_groupcorr_packed(ops.pack_features(f), i, p, d4.contiguous(), C, G))
    rough = _rough_depth(name, 21).to(gpu)
    assert torch.equal(ops.sweep.plane_sweep_groupcorr(f, i, p, rough, G), ops.sweep.plane_sweep_groupcorr(f, i, p, rough, G))


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("tag,kind,G", G23)
def test_g23_forward(gpu, tag, kind, G):
    from mvsdet_amd import functional as F_, ops
    g2, g, feat, nbr, proj, depth = _g23_inputs(tag, kind, G)
    gs, ds = int(g["group_stride"]), int(g["depth_stride"])
    want = torch.from_numpy(g["corr"])
    corr = ops.sweep.plane_sweep_groupcorr(feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu), G)
    nei = tuple(torch.from_numpy(g2["nei_projs"][:, j]) for j in range(nbr.shape[1]))
    via_f = F_.groupwise_correlation(feat.to(gpu), nbr.to(gpu), torch.from_numpy(g2["ref_proj"]), nei, depth.to(gpu), G)
    mean = F_.groupwise_correlation(feat.to(gpu), nbr.to(gpu), torch.from_numpy(g2["ref_proj"]), nei, depth.to(gpu), G, reduce="mean")
    errs = [float((t[:, :, ::gs, ::ds].cpu() - want).abs().max()) for t in (corr, via_f)]
    errs.append(float((mean[:, ::gs, ::ds].cpu() - want.mean(dim=1)).abs().max()))
    print(f"G23 {tag}/{kind}/G={G}: ops {errs[0]:.2e} functional.groupwise_correlation {errs[1]:.2e} reduce='mean' {errs[2]:.2e}")
    assert all(torch.isfinite(t).all() for t in (corr, via_f, mean)) and max(errs) <= TOL


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("tag,kind,G", G23)
def test_g23_gradients(gpu, tag, kind, G):
    from mvsdet_amd import ops
    g2, g, feat, nbr, proj, depth = _g23_inputs(tag, kind, G)
    N, C, H, W = feat.shape
    K, D = nbr.shape[1], depth.shape[1]
    R = torch.from_numpy(lcg_uniform(N * K * G * D * H * W, int(g["R_seed"]))).reshape(N, K, G, D, H, W)
    f64 = feat.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((GR.groupcorr_f64(f64, nbr, proj, depth, G) * R.double()).sum(), f64)
    # the fixture's fp32 gradient is the reference's: its distance to float64 is what the fixture says it is
    cs = int(g["channel_stride"])
    assert float((torch.from_numpy(g["grad_feature"]).double() - g64[:, ::cs]).abs().max()) <= float(g["grad_err_fp32"]) * (1 + 1e-6)
    f = feat.to(gpu).requires_grad_(True)
    (ops.sweep.plane_sweep_groupcorr(f, nbr.to(gpu), proj.to(gpu), depth.to(gpu), G) * R.to(gpu)).sum().backward()
    _check_grad(f.grad, g64, float(g["grad_err_fp32"]), f"groupcorr gradient, G23 {tag}/{kind}/G={G}")


@pytest.mark.parametrize("pixel", [False, True], ids=["plane", "pixel"])
@pytest.mark.parametrize("name,G", [c for c in CASES if c[0] in "ACF"])
def test_gradients_of_shapes_a_c_and_f(gpu, name, G, pixel):
    from mvsdet_amd import ops
    N, K, C, D, H, W = SHAPES[name]
    feat, nbr, proj, d2 = _scene(name)
    depth = _rough_depth(name, 23) if pixel else d2
    R = torch.from_numpy(lcg_uniform(N * K * G * D * H * W, 24)).reshape(N, K, G, D, H, W)
    f64 = feat.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((GR.groupcorr_f64(f64, nbr, proj, depth, G) * R.double()).sum(), f64)
    f32 = feat.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad((GR.groupcorr(f32, nbr, proj, depth, G, torch.float32) * R).sum(), f32)
    grad_err_fp32 = float((g32.double() - g64).abs().max())
    f = feat.to(gpu).requires_grad_(True)
    (ops.sweep.plane_sweep_groupcorr(f, nbr.to(gpu), proj.to(gpu), depth.to(gpu), G) * R.to(gpu)).sum().backward()
    _check_grad(f.grad, g64, grad_err_fp32, f"groupcorr gradient, shape {name} G={G} {'pixel' if pixel else 'plane'}")
    direct = ops.sweep.plane_sweep_groupcorr_backward(f.detach(), nbr.to(gpu), proj.to(gpu), depth.to(gpu), R.to(gpu), G)
    _check_grad(direct, g64, grad_err_fp32, "the backward operator called directly")


# ---------------------------------------------------------------------------------------------------------------- 5
def test_contention_all_taps_of_a_pair_in_four_texels(gpu):
    """A projection whose rotation block is zero: every sample of a (view, neighbour) pair lands on ONE position, so all
    D*H*W = 945 tap gradients of a channel go into that position's texels (the six pairs of shape A on six positions more than
    two texels apart; one a corner with a single tap inside, one on the right border).  Features and R in (0.5, 1.5), bilinear
    weights >= 0: all terms are positive, so any fp32 order of at most 945 + K*D terms, each a product of three roundings, is
    within (945 + 10 + 3) 2^-24 = 5.7e-5 < 1e-4 relative of the exact sum -- rtol 1e-4, no absolute term (derived, not measured)."""
    from mvsdet_amd import ops
    N, K, C, D, H, W = SHAPES["A"]
    G = 5
    feat = (torch.from_numpy(lcg_uniform(N * C * H * W, 9)).reshape(N, C, H, W) + 2.0) / 2.0
    nbr = torch.tensor(NBR["A"])
    proj = torch.zeros(N, K, 4, 4)
    proj[:, :, 3, 3] = 1.0
    proj[:, :, 2, 3] = 1.0                                                               # Z = 1
    proj[:, :, 0, 3] = torch.tensor([[7.3, 14.6], [0.2, 12.1], [19.6, 3.3]])             # the one sample position of each pair
    proj[:, :, 1, 3] = torch.tensor([[3.4, 6.1], [7.9, 2.2], [5.5, 1.2]])
    depth = torch.full((N, D, H, W), 1e6)
    R = (torch.from_numpy(lcg_uniform(N * K * G * D * H * W, 10)).reshape(N, K, G, D, H, W) + 2.0) / 2.0
    assert float(R.min()) >= 0.5 and float(R.max()) <= 1.5 and float(feat.min()) >= 0.5
    f64 = feat.double().requires_grad_(True)
    (w64,) = torch.autograd.grad((GR.groupcorr_f64(f64, nbr, proj, depth, G) * R.double()).sum(), f64)
    assert float(w64.min()) >= 0 and int((w64 > 10 * w64.median()).sum()) >= C * 6      # the contended texels stand out
    f = feat.to(gpu).requires_grad_(True)
    (ops.sweep.plane_sweep_groupcorr(f, nbr.to(gpu), proj.to(gpu), depth.to(gpu), G) * R.to(gpu)).sum().backward()
    got = f.grad.double().cpu()
    rel = ((got - w64).abs() / w64.abs().clamp_min(1e-300))[w64 != 0]
    print(f"contention: max relative error {float(rel.max()):.3e}")
    assert bool((got[w64 == 0] == 0).all()) and float(rel.max()) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- 6
def test_c_entries_in_guarded_memory(gpu):
    """The two C entries on shape A (G = 10), plane and per-pixel depth strides: packed maps, outputs and the workspace exactly as
    long as the ABI says between sentinel guards, pre-filled with NaN: guards intact, the bits of the plain call (the tolerance of
    the gradient tests for the float atomics), everything overwritten; a neighbour id outside [0, N) reads inside the packed maps."""
    import ctypes
    from canvas import Guarded, guarded_f32, ok
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    N, K, C, D, H, W = SHAPES["A"]
    G = 10
    feat, nbr, proj, d2 = _scene("A")
    d4 = _rough_depth("A", 31)
    f, i, p = feat.to(gpu), nbr.to(gpu), proj.to(gpu)
    R = torch.from_numpy(lcg_uniform(N * K * G * D * H * W, 32)).reshape(N, K, G, D, H, W).to(gpu)
    NAN = 0x7FC00000

    def out(shape):
        g, v = guarded_f32(shape, gpu)
        g.region.fill_(NAN)
        return g, v
    pk_g, pk = out((lib.mvsdet_packed_bytes(N, C, H, W) // 4,))
    pk.copy_(ops.pack_features(f))
    wbytes = lib.mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W)
    for depth, strides in ((d2.to(gpu), (D, 1, 0)), (d4.to(gpu), (D * H * W, H * W, 1))):
        ds = (ctypes.c_int64 * 3)(*strides)
        corr_g, corr = out((N, K, G, D, H, W))
        ok(lib.mvsdet_plane_sweep_groupcorr_packed_f32(pk_g.ptr(), _lib.ptr(i), _lib.ptr(p), _lib.ptr(depth), ds, corr_g.ptr(),
                                                       N, K, C, G, D, H, W, None))
        assert corr_g.guards_intact() and bool(torch.isfinite(corr).all())
        assert torch.equal(corr, ops.sweep.plane_sweep_groupcorr(f, i, p, depth, G))
        wild = i.clone()
        wild[0, 0], wild[2, 1] = -5, N + 3
        corr_g.region.fill_(NAN)
        ok(lib.mvsdet_plane_sweep_groupcorr_packed_f32(pk_g.ptr(), _lib.ptr(wild), _lib.ptr(p), _lib.ptr(depth), ds, corr_g.ptr(),
                                                       N, K, C, G, D, H, W, None))
        assert corr_g.guards_intact() and torch.equal(corr, ops.sweep.plane_sweep_groupcorr(f, wild.clamp(0, N - 1), p, depth, G))
        ws_g = Guarded(wbytes // 4, gpu)
        ws_g.region.fill_(NAN)
        gf_g, gf = out((N, C, H, W))
        ok(lib.mvsdet_plane_sweep_groupcorr_bwd_packed_f32(pk_g.ptr(), _lib.ptr(i), _lib.ptr(p), _lib.ptr(depth), ds, _lib.ptr(R), gf_g.ptr(),
                                                           ws_g.ptr(), wbytes, N, K, C, G, D, H, W, None))
        plain = ops.sweep.plane_sweep_groupcorr_backward(f, i, p, depth, R, G)
        assert gf_g.guards_intact() and ws_g.guards_intact()
        assert bool(torch.isfinite(gf).all()) and bool(torch.isfinite(ws_g.region.view(torch.float32)).all())
        torch.testing.assert_close(gf, plain, rtol=1e-4, atol=1.25e-6 * float(plain.abs().max()))
    assert pk_g.guards_intact() and torch.equal(pk, ops.pack_features(f))      # the inputs were only read


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals_on_the_device_path(gpu):
    from mvsdet_amd import ops
    z = lambda *s, **k: torch.zeros(*s, device=gpu, **k)
    N, K, D, H, W = 2, 1, 3, 6, 10
    nbr, proj, depth = z(N, K, dtype=torch.int64), z(N, K, 4, 4), torch.ones(N, D, device=gpu)
    for C, G in [(48, 4), (48, 1), (32, 5), (8, 8), (24, 1)]:
        with pytest.raises(ValueError, match="4, 8, 16"):
            ops.sweep.plane_sweep_groupcorr(z(N, C, H, W), nbr, proj, depth, G)
        with pytest.raises(ValueError, match="4, 8, 16"):
            ops.sweep.plane_sweep_groupcorr_backward(z(N, C, H, W), nbr, proj, depth, z(N, K, G, D, H, W), G)
    for shape in [(N, K, 4, D, H, W + 1), (N, K, 2, D, H, W), (N, 4, D, H, W), (N, K, 4, D + 1, H, W)]:
        with pytest.raises(ValueError, match="grad"):
            ops.sweep.plane_sweep_groupcorr_backward(z(N, 32, H, W), nbr, proj, depth, z(*shape), 4)
    with pytest.raises(ValueError):
        ops.sweep.plane_sweep_groupcorr(z(N, 32, H, W), z(N, 0, dtype=torch.int64), z(N, 0, 4, 4), depth, 4)
    with pytest.raises(ValueError):
        ops.sweep.plane_sweep_groupcorr(z(N, 32, H, W), nbr, proj, torch.ones(N, D, H, W + 1, device=gpu), 4)
