"""torch.ops.mvsdet_amd.depth_diagnostics on the GPU against the float64 restatement (tests/depth_diag_restated.py).

The restatement is fed the oracle's x, y, z, window weights and refined validity (the lifting kernels are bit-identical to the oracle,
test_gpu_parity.py) and ATen-CPU's F.interpolate of the same ground-truth map.  The maps are planted (tests/depth_diag_planted.py):
every decision that hangs on the resized map -- z against g -+ vz, g > 0 -- has a margin of 1e-4 m / 1e-5, four hundred times what
two evaluations of the resize can differ by, so no voxel and no pixel is left out of any comparison.

Bars
  counts                      exact
  the two float64 sums        rounded to fp32, within 2 ulp of the restatement's (the kernel adds the same fp32 terms in another order:
                              float64 rounding, far below fp32's; the squared depth error also sees the resize's last bit -- bar below)
  gap_i                       within 2 ulp; orig_gap, new_gap, n_reduce are quotients of exact counts: equal
  gap_all, rmse               bit-equal to the restated last step (:1484 in fp32; float64 quotient) applied to the kernel's own per-view
                              numbers and sums, and within 2 ulp of the restatement's
  gt_resized                  |kernel - ATen-CPU| <= 8 * 2^-24 * max|tap|: the formula rounds four times on the way to a pixel (a product, the
                              row sum, the product with the row weight, the last sum), each time by at most 2^-24 of a value no larger
                              than the largest tap (the weights of a pair sum to one); two evaluations that place those roundings differently
                              (a fused multiply-add, another order of the two products) are each within 4 * 2^-24 * max|tap| of the exact
                              value.  NaN where ATen gives NaN.
Measured on one MI355X: every sum 0 ulp (1 ulp at 70 views), gap_i and the scalars 0 ulp, gt_resized at most 0.38 of its bar (bit-equal
for the identity resize, 16 % to 25 % of the pixels one ulp off otherwise); the whole file takes 5 s.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import canvas
import depth_diag_planted as planted
from depth_diag_restated import F32, margins, resize_aten_cpu, restate
from lcg import lcg_uniform

pytestmark = pytest.mark.gpu
VZ = 0.2


# --------------------------------------------------------------------------------------------------------------- inputs
def make_case(N, V, J, gt_hw, hw, seed, behind=None, empty=(), kind="planted"):
    """A small scene from the LCG: voxels in a box in front of N translated pinhole cameras (the last ones on and behind the camera
    plane: q2 == 0 and q2 < 0), J depth candidates and densities per pixel in padded maps, a depth expectation in a padded map, and
    a planted ground truth.  `behind`: that view looks away from the grid; `empty`: views whose candidates match no voxel."""
    h, w = hw
    Hg, Wg = gt_hw
    Hp, Wp = h + 1, w + 3
    u = lcg_uniform(3 * V + 2 * N * J * Hp * Wp + N * Hp * Wp, seed).astype(np.float64)
    pts = np.stack([1.5 * u[:V], 1.1 * u[V:2 * V], 2.5 + 2.0 * u[2 * V:3 * V]]).astype(F32)
    pts[:, 0] = (0.05, -0.05, 2.0)                                   # one voxel every forward camera sees
    if V >= 16:
        pts[2, -1], pts[2, -2], pts[2, -3] = 0.0, -1.0, -0.25        # q2 == 0 and q2 < 0
    o = 3 * V
    est_depth = (2.5 + 2.0 * u[o:o + N * J * Hp * Wp]).reshape(N, J, Hp, Wp).astype(F32)
    o += N * J * Hp * Wp
    est_dens = (0.55 + 0.5 * u[o:o + N * J * Hp * Wp]).reshape(N, J, Hp, Wp).astype(F32)
    o += N * J * Hp * Wp
    dmean = (est_depth[:, 0] + 0.1 * u[o:o + N * Hp * Wp].reshape(N, Hp, Wp)).astype(F32)
    if V == 1:
        est_depth[:, 0] = 2.05                                       # the one voxel (z = 2) finds a candidate: its views are kept
    proj = np.zeros((N, 3, 4), F32)
    for i in range(N):
        K = np.array([[0.9 * w, 0, w / 2], [0, 0.9 * w, h / 2], [0, 0, 1]], np.float64)
        t = np.array([0.07 * (i % 5) - 0.14, 0.05 * (i % 3) - 0.05, 0.0])      # no z translation: q2 is the voxel's z exactly
        proj[i] = (K @ np.concatenate([np.eye(3), t[:, None]], 1)).astype(F32)
    if behind is not None:
        proj[behind, 2] = (0, 0, -1, -10)
    case = dict(N=N, V=V, J=J, h=h, w=w, points=pts, projection=proj, est_depth=est_depth, est_dens=est_dens, depth_mean=dmean)
    if kind == "zeros":
        gt = np.zeros((N, Hg, Wg), F32)
    elif kind == "nan":
        gt = np.full((N, Hg, Wg), np.nan, F32)
    else:
        gt = planted.base_gt(est_depth[:, 0, :h, :w], Hg, Wg, seed + 1, holes=1 if min(Hg, Wg) >= 7 else 0)
        if kind == "one_nan":
            gt[0, Hg // 2, Wg // 2] = np.nan
    case["gt"] = gt
    for i in empty:
        est_depth[i] = 100.0
    return case


def reference_of(case, oracle):
    """The oracle's stage 3 + ATen-CPU's resize + the restatement; plants the ground truth first (in place)."""
    N, h, w = case["N"], case["h"], case["w"]
    o = oracle.backproject_weigh(np.ones((N, 1, h, w), F32), case["points"], case["projection"], case["est_depth"][:, :, :h, :w],
                                 case["est_dens"][:, :, :h, :w], VZ, want_index=True)
    gt = case["gt"]
    if np.isfinite(gt).any() and (gt[np.isfinite(gt)] > 0).any():
        planted.plant(gt, o["x"], o["y"], o["z"], h, w, VZ)
    g = resize_aten_cpu(gt, h, w)
    win, pos = margins(o["x"], o["y"], o["z"], g, VZ)
    assert win > planted.WINDOW_MARGIN and pos > planted.POSITIVE_MARGIN, (win, pos)
    r = restate(o["x"], o["y"], o["z"], g, o["volume"][:, 0], o["valid"], case["depth_mean"][:, :h, :w], VZ)
    r.update(g=g, oracle=o, window_margin=win, positive_margin=pos)
    return r


def device_inputs(case, gpu, transposed=False):
    h, w = case["h"], case["w"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    gt = t(case["gt"])
    if transposed:
        gt = t(case["gt"].transpose(0, 2, 1)).transpose(1, 2)       # the same values, column-major in memory
        assert not gt.is_contiguous()
    return (t(case["points"]), t(case["projection"]), t(case["est_depth"])[:, :, :h, :w], t(case["est_dens"])[:, :, :h, :w],
            t(case["depth_mean"])[:, :h, :w], gt)


# --------------------------------------------------------------------------------------------------------------- bars
def ulps(a, b):
    """Distance in units of the last place between float32 arrays (0 where both are NaN, a large number where one is)."""
    a, b = np.asarray(a, F32).ravel(), np.asarray(b, F32).ravel()
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    d = np.abs(ia - ib)
    d[np.isnan(a) & np.isnan(b)] = 0
    d[np.isnan(a) ^ np.isnan(b)] = 1 << 40
    return d


def tap_max(gt, h, w):
    """max |tap| over the source pixels that can feed each resized pixel (one more on either side than the float64 index says),
    NaN taps left out.  -> (N,h,w) float64"""
    a = np.abs(np.nan_to_num(np.asarray(gt, np.float64), nan=0.0))
    Hg, Wg = a.shape[1:]
    rows = np.stack([a[:, slice(*_span(y, Hg, h))].max(1) for y in range(h)], 1)               # (N,h,Wg)
    return np.stack([rows[:, :, slice(*_span(x, Wg, w))].max(2) for x in range(w)], 2)


def _span(d, n_in, n_out):
    lo, hi = planted._taps(d, n_in, n_out)
    return lo, hi + 1


def last_step(per_view, sums):
    """mvsdet.py:1484 and :1445 from per-view numbers: the fp32 list sum over the views that kept a voxel; the float64 quotient."""
    kept = [i for i in range(len(sums)) if sums[i, 2] > 0]
    acc = F32(0)
    for i in kept:
        acc = F32(acc + per_view[i, 0])
    gap_all = F32(acc / F32(len(kept))) if kept else F32(np.nan)
    sq = np.float64(0)
    for v in sums[:, 3]:
        sq = sq + v
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([gap_all, F32(sq / sums[:, 4].sum())], F32)


def check(out, ref, case, label=""):
    scalars, per_view, sums, gt_resized = [t.cpu().numpy() for t in out]
    N, h, w = case["N"], case["h"], case["w"]
    assert scalars.shape == (2,) and per_view.shape == (N, 4) and sums.shape == (N, 6) and gt_resized.shape == (N, h, w)
    assert sums.dtype == np.float64 and scalars.dtype == np.float32
    np.testing.assert_array_equal(sums[:, [1, 2, 4, 5]], ref["sums"][:, [1, 2, 4, 5]])              # counts: exact
    d_sum = max(int(ulps(sums[:, 0], ref["sums"][:, 0]).max()), int(ulps(sums[:, 3], ref["sums"][:, 3]).max()))
    d_gap = int(ulps(per_view[:, 0], ref["per_view"][:, 0]).max())
    d_sc = int(ulps(scalars, ref["scalars"]).max())
    bar = 8 * 2.0 ** -24 * tap_max(case["gt"], h, w)
    nan_ref = np.isnan(ref["g"])
    np.testing.assert_array_equal(np.isnan(gt_resized), nan_ref)
    with np.errstate(invalid="ignore"):
        excess = np.where(nan_ref, 0.0, np.abs(gt_resized.astype(np.float64) - ref["g"]) / np.maximum(bar, 1e-300))
    print(f"{label}: sums {d_sum} ulp, gap_i {d_gap} ulp, scalars {d_sc} ulp, gt_resized {float(excess.max()):.3f} of its bar "
          f"({int((gt_resized != ref['g'])[~nan_ref].sum())} of {gt_resized.size} pixels differ), margins {ref['window_margin']:.2e} "
          f"{ref['positive_margin']:.2e}, skipped {ref['n_skipped']}")
    assert d_sum <= 2 and d_gap <= 2 and d_sc <= 2
    assert float(excess.max()) <= 1.0
    np.testing.assert_array_equal(per_view[:, 1:], ref["per_view"][:, 1:])
    assert int(ulps(scalars, last_step(per_view, sums)).max()) == 0
    return scalars, per_view, sums, gt_resized


def same_bits(a, b):
    return all(torch.equal(x.reshape(-1).contiguous().view(torch.uint8), y.reshape(-1).contiguous().view(torch.uint8))
               for x, y in zip(a, b))


# --------------------------------------------------------------------------------------------------------------- shapes
SHAPES = [
    # N, V, J, (Hg,Wg), (h,w), behind, empty views, transposed gt
    (2, 1, 1, (1, 1), (15, 20), None, (), False),
    (1, 255, 3, (7, 13), (15, 20), None, (), False),
    (6, 256, 8, (59, 80), (59, 80), 4, (1,), False),                  # identity resize
    (2, 257, 3, (30, 40), (59, 80), None, (), True),                  # upscale, column-major ground truth
    (6, 40 * 40 * 16, 3, (239, 320), (59, 80), 1, (2,), True),        # the shipped grid and map sizes
    (70, 257, 1, (7, 13), (15, 20), 33, (5, 69), False),
]


@pytest.mark.parametrize("N,V,J,gt_hw,hw,behind,empty,transposed", SHAPES)
def test_operator_matches_the_restatement(gpu, oracle, N, V, J, gt_hw, hw, behind, empty, transposed):
    from mvsdet_amd import ops
    case = make_case(N, V, J, gt_hw, hw, seed=100 + N + V + J, behind=behind, empty=empty)
    ref = reference_of(case, oracle)
    out = ops.depth_diagnostics(*device_inputs(case, gpu, transposed), VZ)
    _, per_view, sums, _ = check(out, ref, case, f"N={N} V={V} J={J} {gt_hw}->{hw}")
    if behind is not None:
        assert sums[behind, 1] == 0 and sums[behind, 2] == 0 and np.isnan(per_view[behind, 0])     # behind the grid: nothing in the frustum
    for i in empty:
        assert sums[i, 1] > 0 and sums[i, 2] == 0 and np.isnan(per_view[i, 0])                    # skipped: no valid' voxel
    if V >= 16:
        assert ref["oracle"]["z"][0, -1] == 0 and ref["oracle"]["z"][0, -2] < 0                    # the q2 <= 0 voxels were there
    assert ref["n_skipped"] == len(empty) + (behind is not None) and np.isfinite(out[0].cpu().numpy()).all()


@pytest.mark.parametrize("kind", ["all_skipped", "zeros", "nan", "one_nan"])
def test_hand_placed_cases(gpu, oracle, kind):
    from mvsdet_amd import ops
    N = 3
    case = make_case(N, 257, 3, (7, 13), (15, 20), seed=7, empty=(0, 1, 2) if kind == "all_skipped" else (),
                     kind=kind if kind != "all_skipped" else "planted")
    ref = reference_of(case, oracle)
    scalars, per_view, sums, gt_resized = check(ops.depth_diagnostics(*device_inputs(case, gpu), VZ), ref, case, kind)
    if kind == "all_skipped":
        assert np.isnan(scalars[0]) and np.isnan(per_view[:, 0]).all() and np.isfinite(scalars[1])   # the reference raises here; NaN
    elif kind in ("zeros", "nan"):
        assert np.isnan(scalars[1]) and np.isfinite(scalars[0]) and (sums[:, 4] == 0).all()           # empty mask: mean of nothing
        assert np.isnan(gt_resized).all() if kind == "nan" else (gt_resized == 0).all()
    else:
        # every pixel a NaN tap touches is NaN (a zero weight included: NaN * 0) and left the mask; the others are all there
        assert 0 < np.isnan(gt_resized).sum() < gt_resized[0].size and sums[:, 4].sum() == (ref["g"] > 0).sum()
        assert np.isfinite(scalars).all()


def test_two_launches_are_bit_identical(gpu, oracle):
    """Same inputs on two streams, the second beside a kernel that keeps the chip busy: every output, bit for bit."""
    from mvsdet_amd import ops
    case = make_case(6, 40 * 40 * 16, 3, (239, 320), (59, 80), seed=11, behind=1, empty=(2,))
    reference_of(case, oracle)
    args = device_inputs(case, gpu)
    first = ops.depth_diagnostics(*args, VZ)
    torch.cuda.synchronize(gpu)
    a, b = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    load = torch.randn(4096, 4096, device=gpu)
    torch.cuda.synchronize(gpu)
    with torch.cuda.stream(a):
        for _ in range(8):
            load = load @ load * 1e-3
    with torch.cuda.stream(b):
        second = ops.depth_diagnostics(*args, VZ)
    torch.cuda.synchronize(gpu)
    assert same_bits(first, second)


def test_captures_into_a_graph(gpu, oracle):
    """One stream, one branch: capture, replay on new inputs, the same bits as the eager call."""
    from mvsdet_amd import ops
    case = make_case(2, 257, 3, (30, 40), (59, 80), seed=13)
    reference_of(case, oracle)
    args = list(device_inputs(case, gpu))
    static = [a.clone() for a in args]                 # clones of the cropped views are contiguous: static inputs of the graph
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        ops.depth_diagnostics(*static, VZ)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops.depth_diagnostics(*static, VZ)
    for scale in (1.0, 1.03125):
        static[5].copy_(args[5] * scale)
        static[4].copy_(args[4] * scale)
        graph.replay()
        torch.cuda.synchronize(gpu)
        eager = ops.depth_diagnostics(static[0], static[1], static[2], static[3], static[4], static[5], VZ)
        torch.cuda.synchronize(gpu)
        assert same_bits(outs, eager)


def test_canvas_guards_and_null_gt_resized(gpu, oracle):
    """Through the C ABI: inputs as strided views inside NaN canvases, outputs and the workspace at exactly their queried sizes
    between guard words, gt_resized = NULL.  Nothing outside is written, nothing outside is read (a NaN would reach the sums), and
    the numbers are those of the operator."""
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    case = make_case(3, 257, 3, (7, 13), (15, 20), seed=17, empty=(1,))
    reference_of(case, oracle)
    N, V, J, h, w = case["N"], case["V"], case["J"], case["h"], case["w"]
    want = ops.depth_diagnostics(*device_inputs(case, gpu), VZ)

    def framed(a, pad):
        flat = torch.full((a.size + 2 * pad,), float("nan"), dtype=torch.float32, device=gpu)
        flat[pad:pad + a.size].copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
        return flat, flat[pad:pad + a.size]

    _, points = framed(case["points"], 64)
    _, projection = framed(case["projection"], 64)
    _, depth = canvas.nan_view(torch.from_numpy(case["est_depth"][:, :, None, :h, :w].copy()), gpu)
    _, dens = canvas.nan_view(torch.from_numpy(case["est_dens"][:, :, None, :h, :w].copy()), gpu)
    assert depth.stride() == dens.stride()
    _, dm5 = canvas.nan_view(torch.from_numpy(case["depth_mean"][:, None, None, :h, :w].copy()), gpu)
    _, gt5 = canvas.nan_view(torch.from_numpy(case["gt"][:, None, None].copy()), gpu)
    dm, gt = dm5[:, 0, 0], gt5[:, 0, 0]
    st3 = lambda t: (ctypes.c_int64 * 3)(*[int(s) for s in t.stride()])
    st4 = (ctypes.c_int64 * 4)(depth.stride(0), depth.stride(1), depth.stride(3), depth.stride(4))
    ws_bytes = int(lib.mvsdet_depth_diagnostics_workspace_bytes(N, h, w, V))
    assert ws_bytes % 4 == 0
    g_sc, scalars = canvas.guarded_f32((2,), gpu)
    g_pv, per_view = canvas.guarded_f32((N, 4), gpu)
    g_su = canvas.Guarded(N * 6 * 2, gpu)
    g_ws = canvas.Guarded(ws_bytes // 4, gpu)
    canvas.ok(lib.mvsdet_depth_diagnostics_f32(
        _lib.ptr(points), _lib.ptr(projection), _lib.ptr(depth), _lib.ptr(dens), st4, _lib.ptr(dm), st3(dm), _lib.ptr(gt), st3(gt),
        _lib.ptr(scalars), _lib.ptr(per_view), g_su.ptr(), None, g_ws.ptr(), ws_bytes, N, h, w, V, J, 7, 13, VZ,
        _lib.current_stream(gpu)))
    for g in (g_sc, g_pv, g_su, g_ws):
        assert g.guards_intact()
    sums = g_su.region.view(torch.float64).view(N, 6)
    assert same_bits((scalars, per_view, sums), want[:3])
    assert torch.isfinite(sums).all()
    # one byte short of the queried workspace is refused before anything is launched
    assert lib.mvsdet_depth_diagnostics_f32(
        _lib.ptr(points), _lib.ptr(projection), _lib.ptr(depth), _lib.ptr(dens), st4, _lib.ptr(dm), st3(dm), _lib.ptr(gt), st3(gt),
        _lib.ptr(scalars), _lib.ptr(per_view), g_su.ptr(), None, g_ws.ptr(), ws_bytes - 1, N, h, w, V, J, 7, 13, VZ,
        _lib.current_stream(gpu)) == 2


# --------------------------------------------------------------------------------------------------------------- fixture G20
@pytest.fixture(scope="module")
def g20(oracle):
    from test_depth_diag_host import g20_case
    return {tag: g20_case(tag, oracle) for tag in ("scannet", "arkit")}


@pytest.mark.parametrize("tag", ["scannet", "arkit"])
def test_g20_through_the_operator_and_the_mirror(gpu, g20, tag):
    """What the reference returns on G5's inputs with the planted ground truth, through ops.depth_diagnostics and through
    functional.backproject_Weigh (eager route): within the summation bound of test_depth_diag_host.py, per-view numbers to the
    printed 5 decimals; volume and valid bit-identical to the call without gt_depth."""
    from mvsdet_amd import functional as F_, ops
    from test_depth_diag_host import check_against_g20
    c = g20[tag]
    g5, N, h, w = c["g5"], c["N"], c["h"], c["w"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    points, projection, est_depth, est_dens = t(g5["points"]), t(g5["projection"]), t(g5["est_depth"]), t(g5["est_dens"])
    dm, gt = t(c["depth_mean"]), t(c["gt"])
    ref = restate(c["x"], c["y"], c["z"], resize_aten_cpu(c["gt"], h, w), c["weight"], c["valid2"], c["depth_mean"], c["vz"])
    scalars, per_view, sums, _ = [v.cpu().numpy() for v in ops.depth_diagnostics(points, projection, est_depth, est_dens, dm, gt, c["vz"])]
    np.testing.assert_array_equal(sums[:, [1, 2, 4, 5]], ref["sums"][:, [1, 2, 4, 5]])
    check_against_g20(scalars, per_view, ref["n_gap_terms"], ref["n_rmse_terms"], c["g20"], tag + " operator")
    feat = t(g5["feature"])[:, :, :h, :w]
    d_r = est_depth.reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)                     # mvsdet.py:484,495
    p_r = est_dens.reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)
    vs = [float(v) for v in g5["voxel_size"]]
    plain = F_.backproject_Weigh(feat, points, projection, d_r, vs, p_r)
    with_gt = F_.backproject_Weigh(feat, points, projection, d_r, vs, p_r, gt_depth=gt, depth_mean=dm)
    assert torch.equal(plain[0], with_gt[0]) and torch.equal(plain[1], with_gt[1])
    assert float(plain[2]) == 1.0 and float(plain[3]) == 1.0
    gap_all, rmse = with_gt[2], with_gt[3]
    assert gap_all.dim() == 0 and rmse.dim() == 0 and gap_all.device == feat.device and gap_all.dtype == torch.float32
    assert float(gap_all) == float(scalars[0]) and float(rmse) == float(scalars[1])


def test_forward_scene_with_gt_depth(gpu, oracle, g20):
    """MVSDetHotPath.forward_scene(gt_depth=...) on G5's ScanNet-like scene: the four new keys, volume and count bit-identical to the
    call without gt_depth, and the diagnostics those of the operator -- and of the restatement -- on the scene's own depth candidates
    and depth expectation (they come from the depth-distribution kernel here, not from G5, so G20's numbers do not apply)."""
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    from test_host_logic import meta_from
    c = g20["scannet"]
    g5, N, h, w = c["g5"], c["N"], c["h"], c["w"]
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12, topk=3)
    feature = torch.from_numpy(g5["feature"]).to(gpu)
    logits = synthetic.make_cost_logits(N, 12, (60, 80), seed=51, sharp=2.0).to(gpu)
    gt = torch.from_numpy(c["gt"]).to(gpu)
    meta = meta_from(g5)
    plain = hp.forward_scene(feature, meta, cost_logits=logits)
    assert not any(k in plain for k in ("weight_gap", "src_rmse", "depth_diagnostics", "gt_depth_resized"))
    for mode in (False, True):
        hp.overlap_detector = mode
        out = hp.forward_scene(feature, meta, cost_logits=logits, gt_depth=gt)
        assert torch.equal(out["volume"], plain["volume"]) and torch.equal(out["valid"], plain["valid"])
        geo = out["geometry"]
        want = ops.depth_diagnostics(geo.points, geo.projection, out["est_depth"], out["est_densities"], out["depth_coding"][:, 0], gt,
                                     0.2)
        torch.cuda.synchronize(gpu)
        assert out["weight_gap"].dim() == 0 and out["src_rmse"].device == feature.device
        assert same_bits((out["weight_gap"], out["src_rmse"], out["depth_diagnostics"], out["gt_depth_resized"]),
                         (want[0][0], want[0][1], want[1], want[3]))
    # the restatement on the scene's own intermediates; the planted margins (2e-4 m) cover the last bits by which this projection
    # may differ from G5's
    ed, en = out["est_depth"].cpu().numpy(), out["est_densities"].cpu().numpy()
    o = oracle.backproject_weigh(np.ones((N, 1, h, w), F32), geo.points.cpu().numpy(), geo.projection.cpu().numpy(), ed, en, 0.2,
                                 want_index=True)
    case = dict(N=N, h=h, w=w, gt=c["gt"])
    g = resize_aten_cpu(c["gt"], h, w)
    win, pos = margins(o["x"], o["y"], o["z"], g, 0.2)
    assert win > planted.WINDOW_MARGIN
    ref = restate(o["x"], o["y"], o["z"], g, o["volume"][:, 0], o["valid"], out["depth_coding"][:, 0].cpu().numpy(), 0.2)
    ref.update(g=g, window_margin=win, positive_margin=pos)
    check(want, ref, case, "forward_scene")
