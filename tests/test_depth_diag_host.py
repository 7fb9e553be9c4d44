"""Depth diagnostics of the lifting block (the gt_depth branch of backproject_Weigh, mvsdet.py:1435-1484) without a GPU: the float64
restatement of tests/depth_diag_restated.py against fixture G20 -- what the reference itself returns and prints on G5's inputs
(tests/golden/make_goldens_g20.py) -- plus the host side of the new entry point: argument checks, workspace query, the mirror's
refusals and the operator's registrations.

Bars.  The reference adds its fp32 terms in fp32 (torch.mean), the restatement exactly: the two scalars may differ by the rounding
of an fp32 summation of n non-negative terms, (ceil(log2 n) + 3) * 2^-24 relative (`summation_bound`; n is counted, the measured
distance printed).  The per-view numbers are compared to the 5 decimals the reference prints.
Measured: gap_all 0 / 0, rmse 7.1e-8 / 0 relative (scannet / arkit; 0 = the same fp32 number) under bounds of 1.0e-6 and 1.1e-6.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from depth_diag_restated import margins, resize_aten_cpu, restate, summation_bound
import depth_diag_planted as planted

GT_HW = (239, 320)


def g20_case(tag, oracle):
    """-> dict of everything the G20 tests need for one case, the ground truth rebuilt from its seed and the stored moved pixels."""
    g5, g20 = load_golden("g5_backproject_" + tag), load_golden("g20_depth_diag")
    h, w = int(g5["img_shape"][0] // 4), int(g5["img_shape"][1] // 4)
    N = g5["est_depth"].shape[0]
    vz = float(g5["voxel_size"][-1])
    gt = planted.base_gt(g5["est_depth"][:, 0], int(g20[f"{tag}:gt_hw"][0]), int(g20[f"{tag}:gt_hw"][1]), int(g20[f"{tag}:gt_seed"]),
                         zero_view=int(g20[f"{tag}:zero_view"]))
    planted.apply_bumps(gt, g20[f"{tag}:bumps"])
    ed, en = g5["est_depth"].astype(np.float64), g5["est_dens"].astype(np.float64)
    depth_mean = ((ed * en).sum(1) / en.sum(1)).astype(np.float32)
    # the window weight alone: the oracle's lifting of a one-channel map of ones (bit-identical to the reference, test_oracle_golden.py)
    o = oracle.backproject_weigh(np.ones((N, 1, h, w), np.float32), g5["points"], g5["projection"], g5["est_depth"], g5["est_dens"], vz,
                                 want_index=True)
    assert np.array_equal(o["valid"], g5["valid"].reshape(N, -1)) and np.array_equal(o["z"], g5["z"])
    return dict(g5=g5, g20={k.split(":", 1)[1]: g20[k] for k in g20.files if k.startswith(tag + ":")}, h=h, w=w, N=N, vz=vz, gt=gt,
                depth_mean=depth_mean, weight=o["volume"][:, 0], valid2=o["valid"], x=o["x"], y=o["y"], z=o["z"])


def check_against_g20(got_scalars, got_per_view, n_gap_terms, n_rmse_terms, g20, label):
    """The G20 bars: scalars within the fp32 summation bound of the reference's, per-view numbers to the printed 5 decimals."""
    for k, (name, n) in enumerate((("gap_all", n_gap_terms), ("rmse", n_rmse_terms))):
        ref = float(g20[name])
        dist, bound = abs(float(got_scalars[k]) - ref) / abs(ref), summation_bound(n)
        print(f"{label} {name}: {float(got_scalars[k])!r} reference {ref!r} relative distance {dist:.3e} bound {bound:.3e} (n = {n})")
        assert dist <= bound, (name, dist, bound)
    printed = g20["printed"]                       # rows: orig_gap - new_gap, n_reduce, gap_i of the views the reference did not skip
    kept = [i for i in range(len(got_per_view)) if not np.isnan(got_per_view[i, 0])]
    assert len(kept) == len(printed) and len(got_per_view) - len(kept) == int(g20["n_skipped"])
    for row, i in zip(printed, kept):
        pv = got_per_view[i]
        assert abs(float(np.float32(pv[1] - pv[2])) - row[0]) <= 5.5e-6, (i, pv, row)      # half a unit of the fifth decimal + fp32
        assert int(pv[3]) == int(row[1]), (i, pv, row)
        assert abs(float(pv[0]) - row[2]) <= 5.5e-6, (i, pv, row)


@pytest.mark.parametrize("tag", ["scannet", "arkit"])
def test_restatement_matches_the_reference_on_g20(oracle, tag):
    c = g20_case(tag, oracle)
    g = resize_aten_cpu(c["gt"], c["h"], c["w"])
    win, pos = margins(c["x"], c["y"], c["z"], g, c["vz"])
    print(f"{tag}: window margin {win:.3e} (stored {float(c['g20']['window_margin']):.3e}), smallest positive resized value {pos:.3e}")
    assert win > planted.WINDOW_MARGIN and pos > planted.POSITIVE_MARGIN
    assert (g[int(c["g20"]["zero_view"])] == 0).all() and (g == 0).sum() > (g[0] == 0).size   # the zero view and the holes are there
    r = restate(c["x"], c["y"], c["z"], g, c["weight"], c["valid2"], c["depth_mean"], c["vz"])
    assert r["n_skipped"] == int(c["g20"]["n_skipped"])
    check_against_g20(r["scalars"], r["per_view"], r["n_gap_terms"], r["n_rmse_terms"], c["g20"], tag)
    # the six sums are consistent with the per-view numbers
    V = c["z"].shape[1]
    assert np.array_equal(r["per_view"][:, 3], (r["sums"][:, 1] - r["sums"][:, 2]).astype(np.float32))
    assert np.allclose(r["per_view"][:, 2], r["sums"][:, 5] / V, rtol=1e-7, atol=0)


def test_restatement_on_hand_made_views():
    """A skipped view, all views skipped, an empty mask and a NaN pixel, on six voxels and a 1 x 2 map."""
    f = np.float32
    x = np.array([[0, 1, 1, 5, 0, 1]] * 2)
    y = np.zeros((2, 6), np.int64)
    z = np.array([[1.0, 2.0, 2.15, 1.0, -1.0, 2.5]] * 2, f)          # voxel 3 outside the map, voxel 4 behind the camera
    g = np.array([[[1.1, 2.0]], [[0.0, np.nan]]], f)
    weight = np.array([[0.5, 0.25, 0.0, 0.0, 0.0, 0.0], [0.0] * 6], f)
    valid2 = np.array([[1, 1, 0, 0, 0, 0], [0] * 6], bool)
    dm = np.array([[[1.0, 2.5]], [[3.0, 3.0]]], f)
    r = restate(x, y, z, g, weight, valid2, dm, 0.2)
    # view 0: original_valid = voxels 0, 1, 2, 5; gt_valid = 0 (|1.0 - 1.1| < .2), 1, 2 (2.15 < 2.2), not 5
    t = [f(f(1) - f(.5)) ** 2, f(f(1) - f(.25)) ** 2, f(1) ** 2, f(0)]             # fp32 differences and squares
    e = [f(f(1.0) - f(1.1)) ** 2, f(f(2.5) - f(2.0)) ** 2]
    assert r["sums"][0].tolist() == [float(sum(map(np.float64, t))), 4, 2, float(sum(map(np.float64, e))), 2, 1]
    assert r["per_view"][0].tolist() == [f(r["sums"][0, 0] / 4), f(1 / 6), f(1 / 6), 2.0]
    # view 1: no valid' voxel -> skipped, gap_i NaN; its map has no positive pixel (0 and NaN)
    assert np.isnan(r["per_view"][1, 0]) and r["sums"][1, 4] == 0 and r["n_skipped"] == 1
    assert r["scalars"][0] == r["per_view"][0, 0] and r["scalars"][1] == f(r["sums"][0, 3] / 2)
    only = restate(x[1:], y[1:], z[1:], g[1:], weight[1:], valid2[1:], dm[1:], 0.2)
    assert np.isnan(only["scalars"]).all() and only["n_skipped"] == 1            # every view skipped, empty mask


def test_entry_point_checks_arguments_without_launching():
    from mvsdet_amd import _lib
    lib = _lib.load()
    q = lib.mvsdet_depth_diagnostics_workspace_bytes
    # the resized map (16-byte granules), 16 bytes per (view, block of 256 pixels), 24 per (view, block of 256 voxels)
    assert q(40, 59, 80, 25600) == 40 * 59 * 80 * 4 + 40 * 19 * 16 + 40 * 100 * 24
    assert q(1, 1, 1, 1) == 16 + 16 + 24 and q(3, 1, 3, 257) == 48 + 3 * 16 + 3 * 2 * 24
    assert q(0, 4, 4, 4) == 0 and q(1, 4, 4, 0) == 0
    one = ctypes.c_void_p(4096)
    st3, st4 = (ctypes.c_int64 * 3)(12, 4, 1), (ctypes.c_int64 * 4)(36, 12, 4, 1)
    f = lib.mvsdet_depth_diagnostics_f32

    def call(ws=one, ws_bytes=1 << 20, N=1, h=3, w=4, V=5, J=3, Hg=6, Wg=8, scalars=one, gt=one):
        return f(one, one, one, one, st4, one, st3, gt, st3, scalars, one, one, None, ws, ws_bytes, N, h, w, V, J, Hg, Wg, 0.2, None)

    assert call(scalars=None) == 1 and b"NULL" in lib.mvsdet_last_error()
    assert call(gt=None) == 1 and b"NULL" in lib.mvsdet_last_error()
    assert call(N=0) == 1 and b"bad shape" in lib.mvsdet_last_error()
    assert call(J=9) == 1 and b"J=9" in lib.mvsdet_last_error()
    assert call(Hg=0) == 1 and b"gt_depth" in lib.mvsdet_last_error()
    assert call(N=65536) == 1 and b"65535" in lib.mvsdet_last_error()
    assert call(ws=ctypes.c_void_p(4100)) == 1 and b"aligned" in lib.mvsdet_last_error()
    assert call(ws_bytes=q(1, 3, 4, 5) - 1) == 2 and b"workspace" in lib.mvsdet_last_error()


def test_mirror_refuses_what_it_cannot_do():
    """save_dir needs the reference's image dumper; gt_depth without depth_mean would fail at None[mask] in the reference.  Both are
    refused before anything is launched (CPU tensors reach no operator here)."""
    import torch
    from mvsdet_amd import functional as F_
    feat, pts = torch.zeros(2, 3, 4, 5), torch.zeros(3, 2, 2, 2)
    proj, d = torch.zeros(2, 3, 4), torch.ones(2, 20, 1, 3)
    gt = torch.ones(2, 8, 10)
    with pytest.raises(NotImplementedError, match="save_dir"):
        F_.backproject_Weigh(feat, pts, proj, d, [.16, .16, .2], d, gt_depth=gt, save_dir="x", depth_mean=torch.ones(2, 4, 5))
    with pytest.raises(ValueError, match="depth_mean"):
        F_.backproject_Weigh(feat, pts, proj, d, [.16, .16, .2], d, gt_depth=gt)
    with pytest.raises((RuntimeError, NotImplementedError), match="depth_diagnostics"):   # with both it reaches the operator: no CPU form
        F_.backproject_Weigh(feat, pts, proj, d, [.16, .16, .2], d, gt_depth=gt, depth_mean=torch.ones(2, 4, 5))


def test_operator_registrations():
    """torch.ops.mvsdet_amd.depth_diagnostics: fp32 autocast rule, a fake implementation with the documented shapes, no autograd."""
    import torch
    from mvsdet_amd import ops
    assert ops.depth_diagnostics in ops.AUTOCAST_FP32_DIAGNOSTICS and ops.depth_diagnostics not in ops.AUTOCAST_FP32_OPS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mvsdet_amd::depth_diagnostics", "AutocastCUDA")
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    out = torch.ops.mvsdet_amd.depth_diagnostics(m(3, 4, 4, 2), m(5, 3, 4), m(5, 3, 6, 7), m(5, 3, 6, 7), m(5, 6, 7), m(5, 9, 11), 0.2)
    assert [tuple(t.shape) for t in out] == [(2,), (5, 4), (5, 6), (5, 6, 7)]
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.float64, torch.float32]
