"""The per-pixel form of the sweep (csrc/pixel_form.h, planesweep_pixel.hip, groupcorr.hip) at SEVERAL depth hypotheses per block and
at every dealing of units to XCDs.  The other two GPU files of the form run shapes whose grids are so small that every block walks one
hypothesis (tests/pixel_blocking_cases.py: EXISTING), so the loops over a block's hypotheses -- the depth read a hypothesis ahead, the
sums re-seeded per hypothesis, load_ref per slab and hypothesis, the barrier at the top of the backward's loop, the reference view's
own term summed in LDS and flushed once, a ragged last block -- ran one trip.  Here they run several, under option "pixel_dsplit" and
under the default rule at shapes where it picks several itself.  Every case reads its blocking through mvsdet_pixel_form_blocking and
asserts it before it launches: a later change of the rule cannot quietly turn these cases back into one-per-block runs.

  a. forward   -- the split must not change a bit: no atomics, and a hypothesis' arithmetic does not depend on which block walks it;
  b. backward  -- against float64 at every split, at the bound of test_gpu_sweep_pixel.py (pixel_scenes.check_grad, not re-tuned);
                  the contention cases and the guarded-memory cases of the two files once more with every hypothesis in one block;
  c. default   -- Q4, Q5, Q3 (pixel_blocking_cases.py), float64 references computed on the device;
  d. units     -- 4, 5, 8 and 9 units for the variance, 1, 2, 4, 8 and 8 for the correlation, with and without "sweep_xcd".

Bounds: forward variance the project's bar 1e-4 (test_gpu_sweep_pixel.py); forward correlation rule 1 of test_gpu_groupcorr.py,
|corr - mean64| <= (Cg + 2) 2^-24 mean_c|f w_j| against the float64 mean of the GPU's own homo_warp[_pixel] (another kernel: one thread
per pixel and hypothesis, no loop over hypotheses); gradients |g - g64| <= max(1e-4 |g64| + 1.25e-6 max|g64|, 4 x grad_err_fp32),
grad_err_fp32 that of the fp32 restatement.  A float64 gradient that is zero everywhere (K = 0) leaves the bound 0: exactly 0 is asked.

Measured on an MI355X (worst ratio to the bound per family): see DESIGN.md 4.11."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

import groupcorr_restated as GR
import pixel_blocking_cases as PB
import sweep_pixel_restated as SP
import test_gpu_groupcorr as TG
import test_gpu_sweep_pixel as TS
from pixel_scenes import check_grad, scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from lcg import lcg_uniform  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = TS.TOL
V_SHAPES = dict(TS.SHAPES)                       # name -> (N, K, C, D, H, W)
V_NBR = dict(TS.NBR)
V_SHAPES["S-odd-K0"] = (3, 0, 40, 5, 9, 21)      # no neighbour: the K = 0 instantiations
V_NBR["S-odd-K0"] = [[], [], []]
C_SHAPES = dict(TG.SHAPES, A7=PB.A7)
C_NBR = dict(TG.NBR, A7=TG.NBR["A"])
C_CASES = list(TG.CASES) + [("A7", 10), ("A7", 5)]
for _n, _s in (("Q3", PB.Q3), ("Q4", PB.Q4), ("Q5", PB.Q5)):
    V_SHAPES[_n] = C_SHAPES[_n] = _s
    V_NBR[_n] = C_NBR[_n] = PB.Q_NBR[_n]
for _C in PB.UNIT_WIDTHS:
    V_SHAPES[f"U-{_C}"] = C_SHAPES[f"U-{_C}"] = PB.unit_shape(_C)
    V_NBR[f"U-{_C}"] = C_NBR[f"U-{_C}"] = [[1, 1], [1, 0]]


@contextlib.contextmanager
def options(**values):
    """Set library options for a block; what they were comes back in a finally."""
    from mvsdet_amd import _lib
    saved = {k: _lib.get_option(k) for k in ("pixel_dsplit", "sweep_xcd")}
    try:
        for k, v in values.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


def blocking(shape, G, backward):
    """(units, xcd_parts, hypotheses per block) of the launch that follows, from the library; checked against the restatement."""
    from mvsdet_amd import _lib
    N, K, C, D, H, W = shape
    got = _lib.pixel_form_blocking(N, C, G, D, H, W, backward)
    assert got == PB.restated(N, C, G, D, H, W, backward, _lib.get_option("pixel_dsplit"), _lib.get_option("sweep_xcd")), (shape, G, got)
    return got


def per_block(D, dsplit, backward):
    """What "pixel_dsplit" = dsplit > 0 stands for."""
    dpb = -(-D // min(dsplit, D))
    return dpb if backward else min(dpb, PB.MAX_FORWARD)


def table_default(name, G, shape, backward):
    """The row of pixel_blocking_cases.py is what the library gives with no option set."""
    u, p, fwd, bwd = PB.expected(name, G)
    got = blocking(shape, G, backward)
    assert got == ((-(-shape[2] // 32), 1, bwd) if backward else (u, p, fwd)), (name, G, got)
    return got[2]


def rough(shape, seed):
    """Per-pixel depths in [0.6, 4]: another value at every pixel and hypothesis."""
    N, K, C, D, H, W = shape
    return (2.3 + 1.7 * torch.from_numpy(lcg_uniform(N * D * H * W, seed)).reshape(N, D, H, W)).contiguous()


def palette(shape, seed=77):
    """Every (pixel, hypothesis) picks one of 6 depths: three ordinary, one negative, +inf, NaN."""
    N, K, C, D, H, W = shape
    values = torch.tensor([0.7, 1.9, 3.3, -1.2, float("inf"), float("nan")])
    pick = torch.from_numpy(((lcg_uniform(N * D * H * W, seed).astype(np.float64) + 1.0) * 3.0).astype(np.int64).clip(0, 5)).reshape(N, D, H, W)
    assert all(int((pick == k).sum()) > 0 for k in range(6))
    return values[pick].contiguous()


def lcg(shape, seed):
    return torch.from_numpy(lcg_uniform(int(np.prod(shape)), seed)).reshape(shape)


def v_scene(name):
    shape = V_SHAPES[name]
    N, K = shape[:2]
    if K == 0:
        feat, _, _, d2 = scene((N, 1) + shape[2:], [[0]] * N)
        return feat, torch.zeros(N, 0, dtype=torch.int64), torch.zeros(N, 0, 4, 4), d2
    return scene(shape, V_NBR[name])


def c_scene(name):
    return scene(C_SHAPES[name], C_NBR[name])


def decomposition(f, i, p, d, G, corr):
    """Rule 1 of test_gpu_groupcorr.py on device tensors: corr against the float64 mean over a group's channels of f * w_j, w_j the GPU's
    own homo_warp[_pixel].  Finite depths.  -> the worst ratio to the bound (Cg + 2) 2^-24 mean_c|f w_j|."""
    from mvsdet_amd import ops
    N, C, H, W = f.shape
    K, D, Cg = i.shape[1], d.shape[1], C // G
    assert corr.shape == (N, K, G, D, H, W) and corr.dtype == torch.float32 and bool(torch.isfinite(corr).all())
    f64 = f.double().reshape(N, G, Cg, 1, H, W)
    worst = 0.0
    for j in range(K):
        w = (ops.homo_warp_pixel if d.dim() == 4 else ops.homo_warp)(f[i[:, j]], p[:, j].contiguous(), d)
        prod = f64 * w.double().reshape(N, G, Cg, D, H, W)
        want, scale = prod.mean(dim=2), prod.abs().mean(dim=2)
        del prod, w
        bound = (Cg + 2) * 2.0 ** -24 * scale
        err = (corr[:, j].double() - want).abs()
        assert bool((err <= bound).all()), f"neighbour {j}: {int((err > bound).sum())} elements outside the bound, worst {float((err - bound).max()):.3e}"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


def variance_grads(feat, nbr, proj, depth, R):
    """(float64 variance, its gradient, grad_err_fp32 of the fp32 restatement) for the loss sum(var * R), on the inputs' device."""
    f64 = feat.double().requires_grad_(True)
    v64 = SP.variance_pixel_f64(f64, nbr, proj, depth)
    (g64,) = torch.autograd.grad((v64 * R.double()).sum(), f64)
    f32 = feat.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad((SP.variance_pixel(f32, nbr, proj, depth) * R).sum(), f32)
    return v64.detach(), g64, float((g32.double() - g64).abs().max())


def groupcorr_grads(feat, nbr, proj, depth, G, R):
    f64 = feat.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((GR.groupcorr_f64(f64, nbr, proj, depth, G) * R.double()).sum(), f64)
    f32 = feat.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad((GR.groupcorr(f32, nbr, proj, depth, G, torch.float32) * R).sum(), f32)
    return g64, float((g32.double() - g64).abs().max())


def same(a, b, what):
    """Equal bit for bit; a NaN for a NaN."""
    assert a.shape == b.shape, what
    bad = ~((a == b) | (torch.isnan(a) & torch.isnan(b)))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ"


# =============================================================================================================== a. forward
@pytest.mark.parametrize("name", ["S-odd", "S-fast", "S-80", "S-k3", "S-k4", "S-odd-K0"])
def test_variance_forward_has_the_same_bits_at_every_split(gpu, name):
    from mvsdet_amd import ops
    shape = V_SHAPES[name]
    N, K, C, D, H, W = shape
    feat, nbr, proj, _ = v_scene(name)
    f, i, p, d = feat.to(gpu), nbr.to(gpu), proj.to(gpu), rough(shape, 51).to(gpu)
    assert blocking(shape, 0, False)[2] == 1                     # the default at these shapes: the gap
    default = ops.plane_sweep_variance_pixel(f, i, p, d)
    assert bool(torch.isfinite(default).all())
    if K == 0:   # no other test runs it: var = fma(-f, f, round(f f)), the rounding error of f^2: at most half an ulp, <= 2^-24 f^2
        assert bool((default.double().abs() <= 2.0 ** -24 * (f.double() ** 2)[:, :, None].expand_as(default)).all())
    walked = set()
    for dsplit in sorted({1, 2, 3, D}):
        with options(pixel_dsplit=dsplit):
            dpb = blocking(shape, 0, False)[2]
            assert dpb == per_block(D, dsplit, False)
            walked.add(dpb)
            assert torch.equal(ops.plane_sweep_variance_pixel(f, i, p, d), default), f"pixel_dsplit {dsplit}: {dpb} per block"
    assert max(walked) == min(D, 4)


@pytest.mark.parametrize("pixel", [False, True], ids=["plane", "pixel"])
@pytest.mark.parametrize("name,G", C_CASES)
def test_groupcorr_forward_has_the_same_bits_at_every_split(gpu, name, G, pixel):
    from mvsdet_amd import ops
    shape = C_SHAPES[name]
    N, K, C, D, H, W = shape
    feat, nbr, proj, d2 = c_scene(name)
    depth = rough(shape, 52) if pixel else d2
    f, i, p, d = feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu)
    assert blocking(shape, G, False)[2] == 1
    default = ops.sweep.plane_sweep_groupcorr(f, i, p, d, G)
    assert bool(torch.isfinite(default).all())
    if name == "A7":   # the one shape here that no other file compares with float64
        print(f"decomposition A7 G={G}: worst ratio to the bound {decomposition(f, i, p, d, G, default):.3f}")
    walked = set()
    for dsplit in sorted({1, 2, 3, D}):
        with options(pixel_dsplit=dsplit):
            dpb = blocking(shape, G, False)[2]
            assert dpb == per_block(D, dsplit, False)
            walked.add(dpb)
            assert torch.equal(ops.sweep.plane_sweep_groupcorr(f, i, p, d, G), default), f"pixel_dsplit {dsplit}: {dpb} per block"
    assert max(walked) == min(D, 4)
    if name == "A7":
        assert walked == {4, 3, 1}          # 4 + 3, 4 + 3 (the cap), 3 + 3 + 1, 1 x 7


def test_broadcast_depth_gives_the_plane_operators_bits_at_four_per_block(gpu, oracle):
    """test_gpu_sweep_pixel.py's broadcast identity on S-odd with one block for the five hypotheses (forward: 4 + 1)."""
    with options(pixel_dsplit=1):
        assert blocking(V_SHAPES["S-odd"], 0, False)[2] == 4
        TS.test_broadcast_depth_gives_the_plane_operators_bits(gpu, oracle, "S-odd")


@pytest.mark.parametrize("name", ["S-odd", "S-80"])
def test_variance_palette_of_depths_at_four_per_block(gpu, name):
    """test_gpu_sweep_pixel.py's palette identity (the plane operator's bits gathered per pixel, NaN exactly where the depth is not
    finite) with four hypotheses per block: a NaN at hypothesis d must not reach d + 1 through the depth read ahead."""
    with options(pixel_dsplit=1):
        assert blocking(V_SHAPES[name], 0, False)[2] == 4
        TS.test_palette_of_depths_gives_the_plane_operators_bits_per_pixel(gpu, name)


@pytest.mark.parametrize("name,G", [("A", 10), ("A7", 5), ("C", 1), ("E", 8), ("F", 1)])
def test_groupcorr_palette_of_depths_at_every_hypothesis_in_one_block(gpu, name, G):
    from mvsdet_amd import ops
    shape = C_SHAPES[name]
    N, K, C, D, H, W = shape
    feat, nbr, proj, _ = c_scene(name)
    f, i, p, d = feat.to(gpu), nbr.to(gpu), proj.to(gpu), palette(shape).to(gpu)
    assert blocking(shape, G, False)[2] == 1
    default = ops.sweep.plane_sweep_groupcorr(f, i, p, d, G)
    fin = torch.isfinite(d)[:, None, None].expand(N, K, G, D, H, W)
    assert bool(torch.isfinite(default[fin]).all()) and bool(torch.isnan(default[~fin]).all())
    with options(pixel_dsplit=1):
        assert blocking(shape, G, False)[2] == min(D, 4)
        got = ops.sweep.plane_sweep_groupcorr(f, i, p, d, G)
    assert torch.equal(torch.isnan(got), torch.isnan(default)), "the NaN pattern moved with the split"
    same(got, default, f"shape {name} G={G} under pixel_dsplit 1")


# ============================================================================================================== b. backward
@pytest.mark.parametrize("name", ["S-odd", "S-k3", "S-k4", "S-odd-K0"])
def test_variance_backward_against_float64_at_every_split(gpu, name):
    from mvsdet_amd import ops
    shape = V_SHAPES[name]
    N, K, C, D, H, W = shape
    feat, nbr, proj, _ = v_scene(name)
    depth, R = rough(shape, 53), lcg((N, C, D, H, W), 54)
    _, g64, err32 = variance_grads(feat, nbr, proj, depth, R)
    f, i, p, d, r = feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu), R.to(gpu)
    for dsplit in sorted({1, 2, D}):
        with options(pixel_dsplit=dsplit):
            dpb = blocking(shape, 0, True)[2]
            assert dpb == per_block(D, dsplit, True)
            got = ops.plane_sweep_variance_pixel_backward(f, i, p, d, r)
        if K == 0:   # one value per pixel: var = f^2 - f^2 is 0 for every f, its gradient is 0 and so is the bound: exactly 0 is asked
            assert float(g64.abs().max()) <= 1e-12 and bool((got == 0).all()), f"pixel_dsplit {dsplit}"
        else:
            check_grad(got, g64, err32, f"variance gradient {name}, pixel_dsplit {dsplit} ({dpb} per block)")


def test_warp_backward_against_float64_at_every_split(gpu):
    from mvsdet_amd import ops
    shape = V_SHAPES["S-odd"]
    N, K, C, D, H, W = shape
    feat, nbr, proj, _ = v_scene("S-odd")
    depth, R = rough(shape, 55), lcg((N, C, D, H, W), 56)
    src, pj = feat[nbr[:, 1]].contiguous(), proj[:, 1].contiguous()
    s64 = src.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((SP.homo_warp_pixel_f64(s64, pj, depth) * R.double()).sum(), s64)
    s32 = src.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad((SP.homo_warp_pixel(s32, pj, depth) * R).sum(), s32)
    err32 = float((g32.double() - g64).abs().max())
    for dsplit in (1, D):
        with options(pixel_dsplit=dsplit):
            dpb = blocking(shape, 0, True)[2]
            assert dpb == per_block(D, dsplit, True)
            got = ops.homo_warp_pixel_backward(pj.to(gpu), depth.to(gpu), R.to(gpu))
        check_grad(got, g64, err32, f"homo_warp_pixel gradient S-odd, pixel_dsplit {dsplit} ({dpb} per block)")


@pytest.mark.parametrize("pixel", [False, True], ids=["plane", "pixel"])
@pytest.mark.parametrize("name,G", [("A", 10), ("A", 5), ("C", 1), ("C", 3), ("F", 8), ("F", 1), ("A7", 10), ("A7", 5)])
def test_groupcorr_backward_against_float64_at_every_split(gpu, name, G, pixel):
    from mvsdet_amd import ops
    shape = C_SHAPES[name]
    N, K, C, D, H, W = shape
    feat, nbr, proj, d2 = c_scene(name)
    depth, R = (rough(shape, 57) if pixel else d2), lcg((N, K, G, D, H, W), 58)
    g64, err32 = groupcorr_grads(feat, nbr, proj, depth, G, R)
    f, i, p, d, r = feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu), R.to(gpu)
    for dsplit in sorted({1, 2, D}):
        with options(pixel_dsplit=dsplit):
            dpb = blocking(shape, G, True)[2]
            assert dpb == per_block(D, dsplit, True)
            got = ops.sweep.plane_sweep_groupcorr_backward(f, i, p, d, r, G)
        check_grad(got, g64, err32, f"groupcorr gradient {name} G={G} {'pixel' if pixel else 'plane'}, pixel_dsplit {dsplit} ({dpb} per block)")


def test_contention_cases_with_every_hypothesis_in_one_block(gpu):
    """The two contention cases (all 945 tap gradients of a pair / a view in four texels, all terms positive, derived rtol 1e-4, exact
    zeros where the float64 gradient is zero), here with the five hypotheses of a block's taps and of its reference term in one block."""
    with options(pixel_dsplit=1):
        assert blocking(TG.SHAPES["A"], 5, True)[2] == 5 and blocking(TS.SHAPES["S-odd"], 0, True)[2] == 5
        TG.test_contention_all_taps_of_a_pair_in_four_texels(gpu)
        TS.test_contention_all_taps_of_a_view_in_four_texels(gpu)


def test_c_entries_in_guarded_memory_with_every_hypothesis_in_one_block(gpu):
    """The canvas cases of the two files (packed maps, outputs and workspaces between guards, NaN-prefilled; guards intact, everything
    overwritten, no NaN) once more: forward 4 + 1 per block, backward 5."""
    with options(pixel_dsplit=1):
        assert blocking(TS.SHAPES["S-odd"], 0, False)[2] == 4 and blocking(TS.SHAPES["S-odd"], 0, True)[2] == 5
        TS.test_c_entries_in_guarded_memory(gpu)
        assert blocking(TG.SHAPES["A"], 10, False)[2] == 4 and blocking(TG.SHAPES["A"], 10, True)[2] == 5
        TG.test_c_entries_in_guarded_memory(gpu)


# =============================================================================================== c. the default rule's own choice
# Q4 (5, 2, 40, 11, 45, 91): H W = 4095 (a partial last tile, scalar stores), C = 40 (a partial second slab), 2 per block, the last
# block of a tile 1; Cg 4 and 8.  Q5 (6, 3, 72, 9, 45, 91): K = 3 (the second decode pass), 3 units (id % U), Cg 8, 3 per block.
# Q3 (4, 2, 256, 3, 64, 128): the workload's 8 slabs, every hypothesis in one block; Cg 32 (a slab per group), 256 (one group over 8
# slabs: load_ref per slab and hypothesis) and 4.  float64 on the device: Q3's variance is 25 M values.
def _device_scene(name, gpu):
    feat, nbr, proj, _ = scene(V_SHAPES[name], V_NBR[name])
    return feat.to(gpu), nbr.to(gpu), proj.to(gpu), rough(V_SHAPES[name], 61).to(gpu)


GC_DEFAULT = [("Q4", 10), ("Q4", 5), ("Q5", 9), ("Q3", 8), ("Q3", 1), ("Q3", 64)]


@pytest.mark.parametrize("name", ["Q4", "Q3"])
def test_default_rule_variance_forward(gpu, name):
    from mvsdet_amd import ops
    shape = V_SHAPES[name]
    N, K, C, D, H, W = shape
    f, i, p, d = _device_scene(name, gpu)
    with torch.no_grad():
        v64 = SP.variance_pixel_f64(f, i, p, d)
    fwd = table_default(name, 0, shape, False)
    assert fwd > 1
    var = ops.plane_sweep_variance_pixel(f, i, p, d)
    err = float((var.double() - v64).abs().max())
    print(f"default rule {name}: variance forward max |v - v64| = {err:.3e} ({fwd} per block)")
    assert bool(torch.isfinite(var).all()) and err <= TOL
    del v64
    with options(pixel_dsplit=D):
        assert blocking(shape, 0, False)[2] == 1
        assert torch.equal(ops.plane_sweep_variance_pixel(f, i, p, d), var)


@pytest.mark.parametrize("name", ["Q4", "Q3"])
def test_default_rule_variance_backward(gpu, name):
    """Measured on an MI355X: Q4 max |g - g64| 1.77e-5 (max |g64| 4.53, grad_err_fp32 1.76e-5), 0.24 of the bound; Q3 8.9e-7 (2.81, 4.5e-7),
    0.07.  The sampling grid under g64 is built on the CPU (sweep_pixel_restated.sample_grid says why): built with torch's GPU kernels
    it is one rounding away in gx and gy, which alone put Q3 at 3.2 times the bound -- 1.78e-5, on a power-of-two map whose own fp32
    error is 4.5e-7 and whose bound is therefore at its floor of 1.25e-6 max|g64|."""
    from mvsdet_amd import ops
    shape = V_SHAPES[name]
    N, K, C, D, H, W = shape
    f, i, p, d = _device_scene(name, gpu)
    R = lcg((N, C, D, H, W), 62).to(gpu)
    _, g64, err32 = variance_grads(f, i, p, d, R)
    bwd = table_default(name, 0, shape, True)
    assert bwd > 1
    got = ops.plane_sweep_variance_pixel_backward(f, i, p, d, R)
    check_grad(got, g64.cpu(), err32, f"default rule {name}: variance gradient ({bwd} per block)")


@pytest.mark.parametrize("name,G", GC_DEFAULT)
def test_default_rule_groupcorr_forward(gpu, name, G):
    """One group over all of C is ONE unit, which the forward's default rule cuts into single hypotheses at Q3 (8 XCD parts, 256
    blocks): that forward runs under "pixel_dsplit" 1 as well, all three hypotheses and all eight slabs in one block."""
    from mvsdet_amd import ops
    shape = C_SHAPES[name]
    N, K, C, D, H, W = shape
    f, i, p, d = _device_scene(name, gpu)
    fwd = table_default(name, G, shape, False)
    assert fwd > 1 or (name, G) == ("Q3", 1)
    corr = ops.sweep.plane_sweep_groupcorr(f, i, p, d, G)
    print(f"default rule {name} G={G}: decomposition, worst ratio to the bound {decomposition(f, i, p, d, G, corr):.3f} ({fwd} per block)")
    other = 1 if fwd == 1 else D
    with options(pixel_dsplit=other):
        assert blocking(shape, G, False)[2] == (D if fwd == 1 else 1)
        again = ops.sweep.plane_sweep_groupcorr(f, i, p, d, G)
    if fwd == 1:
        print(f"... and with {D} per block {decomposition(f, i, p, d, G, again):.3f}")
    assert torch.equal(again, corr)


@pytest.mark.parametrize("name,G", GC_DEFAULT)
def test_default_rule_groupcorr_backward(gpu, name, G):
    """Measured on an MI355X, worst ratio to the bound: Q4 G = 10 0.22, G = 5 0.25, Q5 G = 9 0.21, Q3 G = 8 / 1 / 64 0.05."""
    from mvsdet_amd import ops
    shape = C_SHAPES[name]
    N, K, C, D, H, W = shape
    f, i, p, d = _device_scene(name, gpu)
    R = lcg((N, K, G, D, H, W), 63).to(gpu)
    g64, err32 = groupcorr_grads(f, i, p, d, G, R)
    bwd = table_default(name, G, shape, True)
    assert bwd > 1
    got = ops.sweep.plane_sweep_groupcorr_backward(f, i, p, d, R, G)
    check_grad(got, g64.cpu(), err32, f"default rule {name} G={G}: groupcorr gradient ({bwd} per block)")


# ============================================================================================================ d. unit dealing
@pytest.mark.parametrize("C,parts", list(zip(PB.UNIT_WIDTHS, (2, 1, 1, 1))))
def test_unit_dealing_of_the_variance(gpu, C, parts):
    """4, 5, 8 and 9 slabs: an XCD owns a unit and there are two parts; a count that does not divide 8; the workload's count; more
    than 8.  With and without "sweep_xcd"; three hypotheses in one block."""
    from mvsdet_amd import ops
    name = f"U-{C}"
    shape = V_SHAPES[name]
    N, K, _, D, H, W = shape
    feat, nbr, proj, _ = v_scene(name)
    depth, R = rough(shape, 71), lcg((N, C, D, H, W), 72)
    v64, g64, err32 = variance_grads(feat, nbr, proj, depth, R)
    f, i, p, d, r = feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu), R.to(gpu)
    table_default(name, 0, shape, False)
    assert blocking(shape, 0, False)[:2] == (C // 32, parts)
    with options(pixel_dsplit=1):
        assert blocking(shape, 0, False) == (C // 32, parts, D) and blocking(shape, 0, True) == (C // 32, 1, D)
        var = ops.plane_sweep_variance_pixel(f, i, p, d)
        err = float((var.double().cpu() - v64).abs().max())
        print(f"unit dealing C={C}: variance forward max |v - v64| = {err:.3e}")
        assert bool(torch.isfinite(var).all()) and err <= TOL
        check_grad(ops.plane_sweep_variance_pixel_backward(f, i, p, d, r), g64, err32, f"unit dealing C={C}: variance gradient")
        with options(sweep_xcd=0):
            assert blocking(shape, 0, False) == (C // 32, 1, D)
            assert torch.equal(ops.plane_sweep_variance_pixel(f, i, p, d), var)
    with options(sweep_xcd=0):
        assert blocking(shape, 0, False)[:2] == (C // 32, 1)
        assert torch.equal(ops.plane_sweep_variance_pixel(f, i, p, d), var)
    assert torch.equal(ops.plane_sweep_variance_pixel(f, i, p, d), var)


@pytest.mark.parametrize("G,units", list(zip(PB.UNIT_GROUPS, (1, 2, 4, 8, 8))))
def test_unit_dealing_of_the_correlation(gpu, G, units):
    """C = 256: one group over 8 slabs, 2 x 4 slabs, 4 x 2, a slab per group, and Cg 4 (8 groups in each of 8 slabs)."""
    from mvsdet_amd import ops
    name, C = "U-256", 256
    shape = C_SHAPES[name]
    N, K, _, D, H, W = shape
    feat, nbr, proj, _ = c_scene(name)
    depth, R = rough(shape, 73), lcg((N, K, G, D, H, W), 74)
    g64, err32 = groupcorr_grads(feat, nbr, proj, depth, G, R)
    f, i, p, d, r = feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu), R.to(gpu)
    table_default(name, G, shape, False)
    parts = 8 // units if units < 8 else 1
    assert blocking(shape, G, False)[:2] == (units, parts)
    with options(pixel_dsplit=1):
        assert blocking(shape, G, False) == (units, parts, D) and blocking(shape, G, True) == (8, 1, D)
        corr = ops.sweep.plane_sweep_groupcorr(f, i, p, d, G)
        print(f"unit dealing G={G}: decomposition, worst ratio to the bound {decomposition(f, i, p, d, G, corr):.3f}")
        check_grad(ops.sweep.plane_sweep_groupcorr_backward(f, i, p, d, r, G), g64, err32, f"unit dealing G={G}: groupcorr gradient")
        with options(sweep_xcd=0):
            assert blocking(shape, G, False) == (units, 1, D)
            assert torch.equal(ops.sweep.plane_sweep_groupcorr(f, i, p, d, G), corr)
    with options(sweep_xcd=0):
        assert blocking(shape, G, False)[:2] == (units, 1)
        assert torch.equal(ops.sweep.plane_sweep_groupcorr(f, i, p, d, G), corr)
    assert torch.equal(ops.sweep.plane_sweep_groupcorr(f, i, p, d, G), corr)
