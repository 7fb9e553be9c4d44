"""The view-synthesis scores on the GPU (csrc/nvsmetric.hip through ops.nvsmetric.nvs_score, functional, evaluation.NVSEvaluator / MVSEvaluator
and MVSDetHotPath.nvs_scores) against the float64 restatement of tests/nvs_score_restated.py (form (a), which test_nvs_score_host.py
holds against the filter-free form (b)).

skimage, cv2 and matplotlib are not installed where this package is developed, and the reference's save_rendered_img.py imports all
three: no fixture can be recorded from the reference's own code, so there is no tests/golden file for this.

Shapes (n_tgt, H, W): one window; the small odd ones; exactly one tile of window centres (tile + 6 both ways); one row and one
column more (the second tile of each direction then holds a single centre); three tiles each way with a single centre in the last.

TOL = 1e-9 absolute, derived and not tuned: the inputs are float32, so every product the kernel forms is exact in float64; a sum has
at most a few thousand float64 terms of magnitude <= 1 and its error stays below 1e-12; S divides by B2 >= C2 = 9e-4, which
amplifies an error of the variance terms by at most 1.1e3 -> 1.1e-9 worst case per window, far less in the mean; PSNR's error is
4.34 * dmse / mse with mse near 1e-2.  Every test prints its figures before it asserts (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import nvs_score_restated as R
from canvas import Guarded, nan_view, ok

pytestmark = pytest.mark.gpu
TOL = 1e-9
TW, TH = 32, 16      # ops.nvsmetric.NVS_TILE_W / _H, checked below
SHAPES = [(1, 7, 7), (2, 8, 9), (3, 13, 39), (2, 23, 70), (2, TH + 6, TW + 6), (2, TH + 7, TW + 7), (1, 2 * TH + 7, 2 * TW + 7)]


def dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy()


def err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


def strides_of(t):
    return None if t is None else (ctypes.c_int64 * t.dim())(*[int(s) for s in t.stride()])


def raw_score(gpu, pred, gt, pred_depth=None, gt_depth=None, with_state=True):
    """mvsdet_nvs_score_f32 with workspace, rows, scene and state between guards -> (per_view, scene, state) and the guards' verdict."""
    from mvsdet_amd import _lib
    from mvsdet_amd.ops import nvsmetric
    n, H, W = int(pred.shape[0]), int(pred.shape[-2]), int(pred.shape[-1])
    wbytes = nvsmetric.workspace_bytes(n, H, W, pred_depth is not None)
    assert wbytes > 0 and wbytes % 8 == 0
    ws, rows, scene, state = Guarded(wbytes // 4, gpu), Guarded(4 * n, gpu), Guarded(6, gpu), Guarded(8, gpu)
    lib = _lib.load()
    ok(lib.mvsdet_nvs_score_f32(state.ptr() if with_state else None, _lib.ptr(pred), strides_of(pred), _lib.ptr(gt), strides_of(gt),
                                _lib.ptr(pred_depth), strides_of(pred_depth), _lib.ptr(gt_depth), strides_of(gt_depth), n, H, W,
                                rows.ptr(), scene.ptr(), ws.ptr(), wbytes, _lib.current_stream(gpu)))
    intact = all(g.guards_intact() for g in (ws, rows, scene, state))
    f64 = lambda g: g.region.view(torch.float64).clone()   # noqa: E731
    return f64(rows).view(n, 2), f64(scene), f64(state), intact


def test_tile_shape_the_cases_are_built_on():
    from mvsdet_amd.ops import nvsmetric
    assert (nvsmetric.NVS_TILE_W, nvsmetric.NVS_TILE_H) == (TW, TH)


@pytest.mark.parametrize("shape", SHAPES)
def test_views_and_scene_against_the_restatement(gpu, shape):
    """Case 1 and case 6: per-view PSNR and SSIM, the scene's triple with its depth error."""
    from mvsdet_amd import ops
    n, H, W = shape
    ref = R.reference(n, H, W)
    sc = ref["scene"]
    st = ops.nvsmetric.nvs_state(gpu)
    per_view, scene = ops.nvsmetric.nvs_score(st, dev(sc["pred"], gpu), dev(sc["gt"], gpu), dev(sc["pred_depth"], gpu), dev(sc["gt_depth"], gpu))
    e_views, e_scene = err(per_view.cpu().numpy(), ref["views"]), err(scene.cpu().numpy(), ref["triple"])
    print(f"{shape}: per view {e_views:.3g}, scene {e_scene:.3g}  (psnr {ref['triple'][0]:.3f} dB, ssim {ref['triple'][1]:.4f}, "
          f"rmse {ref['triple'][2]:.4f})")
    assert per_view.dtype == torch.float64 and tuple(per_view.shape) == (n, 2)
    assert e_views <= TOL and e_scene <= TOL
    assert st.cpu().tolist() == scene.cpu().tolist() + [1.0]
    assert err(ops.nvsmetric.nvs_result(st).cpu().numpy(), ref["triple"]) <= TOL


def test_closed_forms_on_the_device(gpu):
    """Case 2: identical images give SSIM exactly 1 and PSNR +inf; a constant pair its closed form."""
    from mvsdet_amd import functional as F_
    x = dev(R.scene(1, 23, 39, depth=False)["gt"][0].transpose(1, 2, 0), gpu)
    ssim, psnr = float(F_.compute_ssim(x, x)), float(F_.compute_psnr(x, x))
    c1, c2 = float(np.float32(0.3)), float(np.float32(0.8))
    a, b = torch.full((23, 39, 3), c1, device=gpu), torch.full((23, 39, 3), c2, device=gpu)
    want = (2 * c1 * c2 + R.C1) / (c1 ** 2 + c2 ** 2 + R.C1)
    got = float(F_.compute_ssim(a, b))
    print(f"identical: ssim {ssim!r} psnr {psnr!r}; constant pair {got!r} against {want!r}")
    assert ssim == 1.0 and psnr == math.inf
    assert abs(got - want) <= 1e-12
    assert F_.compute_ssim(a, b).is_cuda and F_.compute_ssim(a, b).dim() == 0


@pytest.mark.parametrize("shape", [(2, 23, 70), (2, TH + 7, TW + 7)])
def test_strides_and_guards(gpu, shape):
    """Case 3: a permuted (n,H,W,3) view, a window of a NaN canvas and contiguous copies give the same bits; nothing is written
    outside workspace, rows, scene and state."""
    n, H, W = shape
    ref = R.reference(n, H, W)
    sc = ref["scene"]
    pred, gt, pd, gd = (dev(sc[k], gpu) for k in ("pred", "gt", "pred_depth", "gt_depth"))
    runs = [raw_score(gpu, pred, gt, pd, gd)]
    hwc = lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # noqa: E731
    assert hwc(pred).stride(3) == 3
    runs.append(raw_score(gpu, hwc(pred), hwc(gt), pd, gd))
    canvases = [nan_view(torch.from_numpy(sc[k][:, :, None]), gpu) for k in ("pred", "gt")]
    canvases += [nan_view(torch.from_numpy(sc[k][:, None, None]), gpu) for k in ("pred_depth", "gt_depth")]
    runs.append(raw_score(gpu, canvases[0][1][:, :, 0], canvases[1][1][:, :, 0], canvases[2][1][:, 0, 0], canvases[3][1][:, 0, 0]))
    for name, (views, scene, state, intact) in zip(("contiguous", "permuted", "canvas window"), runs):
        print(f"{shape} {name}: scene {scene.cpu().tolist()} guards intact {intact}")
        assert intact
        assert not torch.isnan(views).any() and not torch.isnan(scene).any()
        assert np.array_equal(bits(views), bits(runs[0][0])) and np.array_equal(bits(scene), bits(runs[0][1]))
        assert state.cpu().tolist() == scene.cpu().tolist() + [1.0]
    assert err(runs[0][0].cpu().numpy(), ref["views"]) <= TOL and err(runs[0][1].cpu().numpy(), ref["triple"]) <= TOL


def test_a_nan_pixel_stays_in_its_view(gpu):
    """Case 4: one NaN pixel in view 1 of 3: that view and the scene's means are NaN, views 0 and 2 keep their bits."""
    from mvsdet_amd import ops
    sc = R.reference(3, 23, 70)["scene"]
    pred, gt = dev(sc["pred"], gpu), dev(sc["gt"], gpu)
    clean, _ = ops.nvsmetric.nvs_score(None, pred, gt)
    bad = pred.clone()
    bad[1, 2, 11, 40] = float("nan")
    views, scene = ops.nvsmetric.nvs_score(None, bad, gt)
    print(f"views {views.cpu().tolist()} scene {scene.cpu().tolist()}")
    assert torch.isnan(views[1]).all() and torch.isnan(scene[:2]).all() and float(scene[2]) == 0.0
    assert np.array_equal(bits(views[[0, 2]]), bits(clean[[0, 2]]))


def test_same_bits_twice_and_alone(gpu):
    """Case 5: two runs give equal bits; view 0 of the 3-view call is bit-equal to the same view scored alone."""
    from mvsdet_amd import ops
    sc = R.reference(3, TH + 7, TW + 7)["scene"]
    pred, gt, pd, gd = (dev(sc[k], gpu) for k in ("pred", "gt", "pred_depth", "gt_depth"))
    a, b = ops.nvsmetric.nvs_score(None, pred, gt, pd, gd), ops.nvsmetric.nvs_score(None, pred, gt, pd, gd)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    alone, _ = ops.nvsmetric.nvs_score(None, pred[:1], gt[:1])
    assert np.array_equal(bits(alone[0]), bits(a[0][0]))


def test_depth_alone_and_a_scene_without_depth(gpu):
    """Case 6: the depth error by itself (functional.save_rendered_depth); a scene without depth leaves rmse at 0 and still counts."""
    from mvsdet_amd import functional as F_
    from mvsdet_amd import ops
    ref = R.reference(2, 23, 70)
    sc = ref["scene"]
    got = F_.save_rendered_depth(dev(sc["pred_depth"], gpu), dev(sc["gt_depth"], gpu))
    print(f"depth error {float(got)!r} against {ref['triple'][2]!r}")
    assert got.is_cuda and got.dim() == 0 and abs(float(got) - ref["triple"][2]) <= TOL
    psnr, ssim, zero = F_.save_rendered_img_Image(dev(sc["pred"], gpu), dev(sc["gt"], gpu))
    assert psnr.is_cuda and zero == 0 and err([float(psnr), float(ssim)], ref["triple"][:2]) <= TOL
    st = ops.nvsmetric.nvs_state(gpu)
    ops.nvsmetric.nvs_score(st, dev(sc["pred"], gpu), dev(sc["gt"], gpu), dev(sc["pred_depth"], gpu), dev(sc["gt_depth"], gpu))
    ops.nvsmetric.nvs_score(st, dev(sc["pred"], gpu), dev(sc["gt"], gpu))
    state = st.cpu().tolist()
    assert state[3] == 2.0 and abs(state[2] - ref["triple"][2]) <= TOL
    assert abs(float(ops.nvsmetric.nvs_result(st)[2]) - ref["triple"][2] / 2) <= TOL


def test_evaluators_without_a_synchronisation(gpu):
    """Case 7: NVSEvaluator over three scenes of different n_tgt and size and MVSEvaluator over three pairs against the restated
    metrics; the update calls run with synchronisations forbidden; reset() brings back a clean state."""
    from mvsdet_amd.evaluation import MVSEvaluator, NVSEvaluator
    refs = [R.reference(2, 8, 9), R.reference(1, 13, 39, depth=False), R.reference(3, 23, 70)]
    feeds = [tuple(dev(r["scene"][k], gpu) for k in ("pred", "gt", "pred_depth", "gt_depth")) for r in refs]
    feeds[0] = (feeds[0][0][None],) + feeds[0][1:]                          # (1,n_tgt,3,H,W) as novel_views returns it
    pairs = [(0.25, 1.5), (0.75, 0.5), (0.125, 2.25)]
    dev_pairs = [tuple(torch.tensor(v, device=gpu) for v in p) for p in pairs]
    ev, mv = NVSEvaluator(device=gpu), MVSEvaluator()
    ev.update(*feeds[0])                                                    # warm: library load, allocator
    mv.update(dev_pairs[0])
    ev.reset()
    mv.reset()
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for f, p in zip(feeds, dev_pairs):
            ev.update(*f)
            mv.update(p)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    got, want = ev.compute(), R.nvs_metric([r["triple"] for r in refs])
    print(f"NVSEvaluator {got} against {want}")
    assert list(got) == ["psnr", "ssim", "rmse"] and all(abs(got[k] - want[k]) <= TOL for k in want)
    assert err(ev.last_scene.cpu().numpy(), refs[2]["triple"]) <= TOL
    assert mv.compute() == R.mvs_metric(pairs)
    ev.reset()
    with pytest.raises(RuntimeError):
        ev.compute()
    ev.update(*feeds[1])
    again = ev.compute()
    assert all(abs(again[k] - refs[1]["triple"][i]) <= TOL for i, k in enumerate(("psnr", "ssim", "rmse")))


def test_error_paths_before_any_launch(gpu):
    from mvsdet_amd import ops
    z = lambda *s: torch.zeros(*s, device=gpu)   # noqa: E731
    with pytest.raises(ValueError):
        ops.nvsmetric.nvs_score(None, z(1, 3, 6, 9), z(1, 3, 6, 9))
    with pytest.raises(ValueError):
        ops.nvsmetric.nvs_score(None, z(1, 3, 8, 9), z(1, 3, 9, 8))
    with pytest.raises(TypeError):
        ops.nvsmetric.nvs_score(None, z(1, 3, 8, 9).half(), z(1, 3, 8, 9).half())
    with torch.autocast("cuda", dtype=torch.float16):
        views, _ = ops.nvsmetric.nvs_score(None, z(1, 3, 8, 9).half(), z(1, 3, 8, 9).half())
    assert float(views[0, 1]) == 1.0


def test_chain_from_the_rasteriser(gpu):
    """Case 8: functional.pixel_gaussians -> functional.decode_splatting -> MVSDetHotPath.nvs_scores on the composition scene of
    tests/adapter_scene.py, against the restatement applied to the rendered image."""
    import adapter_restated as A
    import adapter_scene as AS
    from mvsdet_amd import functional as F_
    from mvsdet_amd.evaluation import NVSEvaluator
    from mvsdet_amd.hotpath import MVSDetHotPath
    c, tgt = AS.composition()
    g = F_.pixel_gaussians(dev(c["extrinsics"], gpu), dev(c["intrinsics"], gpu), dev(c["raw"], gpu), dev(c["depth"], gpu),
                           dev(c["opacity"], gpu), (c["h"], c["w"]), c["s_min"], c["s_max"], A.degree_of(c["d_sh"]))
    colour = F_.decode_splatting(g, dev(tgt["tgt_extrinsics"], gpu)[None], dev(tgt["tgt_intrinsics"], gpu)[None], dev(tgt["near"], gpu)[None],
                                 dev(tgt["far"], gpu)[None], (AS.H, AS.W), dev(tgt["bg"], gpu))
    assert tuple(colour.shape) == (1, 1, 3, AS.H, AS.W)
    hot = MVSDetHotPath.__new__(MVSDetHotPath)                             # nvs_scores keeps no state
    ev = NVSEvaluator(device=gpu)
    out = hot.nvs_scores(colour, dev(tgt["gt"], gpu), evaluator=ev)
    (psnr, ssim, rmse), _ = R.scene_triple(colour[0].detach().cpu().numpy(), tgt["gt"])
    print(f"chain: psnr {float(out['psnr'])!r} against {psnr!r}, ssim {float(out['ssim'])!r} against {ssim!r}")
    assert all(v.is_cuda and v.dim() == 0 for v in out.values())
    assert abs(float(out["psnr"]) - psnr) <= TOL and abs(float(out["ssim"]) - ssim) <= TOL and float(out["rmse"]) == 0.0
    assert abs(ev.compute()["ssim"] - ssim) <= TOL
