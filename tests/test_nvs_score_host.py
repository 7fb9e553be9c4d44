"""The view-synthesis scores above the kernel, on the CPU route (ops.nvsmetric.nvs_score's torch float64 expressions): both restatements of
tests/nvs_score_restated.py against each other, the closed forms, every public function and both evaluators against the restatement,
the error paths and the integration patch on a stub module.

skimage, cv2 and matplotlib are not installed where this package is developed, and the reference's save_rendered_img.py imports all
three: no fixture can be recorded from the reference's own code, so there is no tests/golden file for this and the defaults of
structural_similarity are written out in nvs_score_restated.py instead.

Bars.  RESTATED_TOL: forms (a) and (b) add the same 49 exact float64 products in two orders; a window mean then carries at most
49 * 2**-53 = 5.5e-15, and S amplifies an error of its variance terms by at most 1 / C2 = 1.1e3: 1e-11 covers both forms' errors.
TOL = 1e-9 is the bar of the GPU test (test_gpu_nvs_score.py derives it); the CPU route is held to the same."""
import math
import types

import numpy as np
import pytest
import torch

import nvs_score_restated as R

RESTATED_TOL = 1e-11
TOL = 1e-9
SHAPES = [(1, 7, 7), (2, 8, 9), (3, 13, 39), (2, 23, 70)]


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= tol))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_two_restatements_agree(shape):
    n, H, W = shape
    sc = R.scene(n, H, W, depth=False)
    worst = 0.0
    for v in range(n):
        p, g = sc["pred"][v].transpose(1, 2, 0), sc["gt"][v].transpose(1, 2, 0)
        worst = max(worst, abs(R.compute_ssim(p, g, "filter") - R.compute_ssim(p, g, "direct")))
    print(f"{shape}: filter form against direct form, float64: {worst:.3g}")
    assert worst <= RESTATED_TOL


@pytest.mark.parametrize("shape", SHAPES)
def test_distance_of_the_reference_float32_order_is_recorded(shape):
    """Printed, not gated: how far the reference's own float32 order lies from the float64 value (DESIGN 4.17 quotes these)."""
    n, H, W = shape
    sc = R.scene(n, H, W, depth=False)
    (_, _, _), v64 = R.save_rendered_img_Image(sc["pred"], sc["gt"])
    (_, _, _), v32 = R.save_rendered_img_Image(sc["pred"], sc["gt"], f32=True)
    d = np.abs(v64 - v32).max(axis=0)
    print(f"{shape}: reference float32 order against float64: psnr {d[0]:.3g} dB, ssim {d[1]:.3g}")
    assert np.isfinite(d).all()


def test_closed_form_of_constant_images():
    from mvsdet_amd import functional as F_
    c1, c2 = np.float32(0.3), np.float32(0.8)
    a, b = torch.full((9, 12, 3), float(c1)), torch.full((9, 12, 3), float(c2))
    want = (2 * float(c1) * float(c2) + R.C1) / (float(c1) ** 2 + float(c2) ** 2 + R.C1)
    got = float(F_.compute_ssim(a, b))
    print(f"constant pair: {got!r} against {want!r}")
    assert abs(got - want) <= 1e-12
    assert abs(R.compute_ssim(a.numpy(), b.numpy()) - want) <= 1e-12


def test_identical_images_give_one_and_infinity():
    from mvsdet_amd import functional as F_
    x = t(R.scene(1, 11, 17, depth=False)["gt"][0].transpose(1, 2, 0))
    assert float(F_.compute_ssim(x, x)) == 1.0
    assert float(F_.compute_psnr(x, x)) == math.inf


@pytest.mark.parametrize("shape", SHAPES)
def test_public_functions_against_the_restatement(shape):
    from mvsdet_amd import functional as F_
    from mvsdet_amd import ops
    n, H, W = shape
    ref = R.reference(n, H, W)
    sc, (psnr, ssim, rmse), views = ref["scene"], ref["triple"], ref["views"]
    pred, gt = t(sc["pred"]), t(sc["gt"])
    per_view, scene = ops.nvsmetric.nvs_score(None, pred, gt, t(sc["pred_depth"]), t(sc["gt_depth"]))
    assert per_view.dtype == torch.float64 and tuple(per_view.shape) == (n, 2) and tuple(scene.shape) == (3,)
    assert close(per_view.numpy(), views) and close(scene.numpy(), [psnr, ssim, rmse])
    for v in range(n):
        p, g = pred[v].permute(1, 2, 0), gt[v].permute(1, 2, 0)
        assert close(F_.compute_psnr(p, g), views[v, 0]) and close(F_.compute_ssim(p, g), views[v, 1])
        assert F_.compute_psnr(p, g).dim() == 0
    out = F_.save_rendered_img_Image(pred, gt, img_meta=None)
    assert close(out[0], psnr) and close(out[1], ssim) and out[2] == 0
    assert close(F_.save_rendered_depth(t(sc["pred_depth"]), t(sc["gt_depth"])), rmse)
    # a permuted view and a scene without depth
    per_view2, scene2 = ops.nvsmetric.nvs_score(None, pred.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), gt)
    assert close(per_view2.numpy(), views) and float(scene2[2]) == 0.0


def _three_scenes():
    return [R.reference(2, 8, 9), R.reference(1, 13, 39, depth=False), R.reference(3, 23, 70)]


def test_nvs_evaluator_over_scenes_of_different_shapes():
    from mvsdet_amd.evaluation import NVSEvaluator, nvs_eval
    refs = _three_scenes()
    want = R.nvs_metric([r["triple"] for r in refs])
    ev = NVSEvaluator(device="cpu")
    with pytest.raises(RuntimeError):
        ev.compute()
    for i, r in enumerate(refs):
        sc = r["scene"]
        pred = t(sc["pred"])[None] if i == 0 else t(sc["pred"])            # (1,n_tgt,3,H,W) as novel_views returns it, or without
        ev.update(pred, t(sc["gt"]), t(sc["pred_depth"]), t(sc["gt_depth"]))
        assert close(ev.last_scene.numpy(), r["triple"])
    got = ev.compute()
    assert list(got) == ["psnr", "ssim", "rmse"] and all(isinstance(v, float) for v in got.values())
    assert all(abs(got[k] - want[k]) <= TOL for k in want)
    assert refs[1]["triple"][2] == 0                                        # the scene without depth counted rmse 0
    ev.reset()
    with pytest.raises(RuntimeError):
        ev.compute()
    ev.update(t(refs[0]["scene"]["pred"]), t(refs[0]["scene"]["gt"]))
    assert abs(ev.compute()["psnr"] - refs[0]["triple"][0]) <= TOL and ev.compute()["rmse"] == 0.0
    lists = nvs_eval([t(r["scene"]["pred"]) for r in refs], [t(r["scene"]["gt"]) for r in refs],
                     [t(r["scene"]["pred_depth"]) for r in refs], [t(r["scene"]["gt_depth"]) for r in refs], device="cpu")
    assert all(abs(lists[k] - want[k]) <= TOL for k in want)


def test_mvs_evaluator_keeps_the_last_weight_gap():
    from mvsdet_amd.evaluation import MVSEvaluator
    pairs = [(0.25, 1.5), (0.75, 0.5), (0.125, 2.25)]
    want = R.mvs_metric(pairs)
    assert want["weight_gap"] == 0.125 and want["src_rmse"] == (1.5 + 0.5 + 2.25) / 3
    ev = MVSEvaluator()
    with pytest.raises(RuntimeError):
        ev.compute()
    ev.update((torch.tensor(pairs[0][0]), torch.tensor(pairs[0][1])))
    ev.update(dict(weight_gap=torch.tensor(pairs[1][0]), src_rmse=torch.tensor(pairs[1][1])))
    ev.update(pairs[2])
    assert ev.compute() == want
    ev.reset()
    with pytest.raises(RuntimeError):
        ev.compute()


def test_error_paths():
    from mvsdet_amd import functional as F_
    from mvsdet_amd import ops
    from mvsdet_amd.evaluation import NVSEvaluator
    with pytest.raises(ValueError):
        ops.nvsmetric.nvs_score(None, torch.zeros(1, 3, 6, 9), torch.zeros(1, 3, 6, 9))
    with pytest.raises(ValueError):
        F_.compute_ssim(torch.zeros(9, 6, 3), torch.zeros(9, 6, 3))
    with pytest.raises(ValueError):
        R.compute_ssim(np.zeros((9, 6, 3), np.float32), np.zeros((9, 6, 3), np.float32))
    with pytest.raises(ValueError):
        ops.nvsmetric.nvs_score(None, torch.zeros(1, 3, 8, 9), torch.zeros(1, 3, 8, 10))
    with pytest.raises(ValueError):
        ops.nvsmetric.nvs_score(None, torch.zeros(1, 3, 8, 9), torch.zeros(1, 3, 8, 9), torch.zeros(2, 8, 9), torch.zeros(2, 8, 9))
    with pytest.raises(ValueError):
        F_.compute_psnr(torch.zeros(8, 9, 3), torch.zeros(8, 9, 4))
    with pytest.raises(TypeError):
        ops.nvsmetric.nvs_score(None, torch.zeros(1, 3, 8, 9, dtype=torch.int32), torch.zeros(1, 3, 8, 9, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.nvsmetric.nvs_score(None, torch.zeros(1, 3, 8, 9, dtype=torch.float16), torch.zeros(1, 3, 8, 9, dtype=torch.float16))
    mask = torch.ones(8, 9, dtype=torch.bool)
    with pytest.raises(NotImplementedError):
        F_.compute_psnr(torch.zeros(8, 9, 3), torch.zeros(8, 9, 3), mask=mask)
    with pytest.raises(NotImplementedError):
        F_.compute_ssim(torch.zeros(8, 9, 3), torch.zeros(8, 9, 3), mask)
    with pytest.raises(NotImplementedError):
        F_.save_rendered_img_Image(torch.zeros(1, 3, 8, 9), torch.zeros(1, 3, 8, 9), None, save_dir="out")
    with pytest.raises(NotImplementedError):
        F_.save_rendered_depth(torch.zeros(1, 8, 9), torch.zeros(1, 8, 9), None, save_dir="out")
    with pytest.raises(ValueError):
        NVSEvaluator(device="cpu").update([torch.zeros(1, 3, 8, 9)], [])


def test_hotpath_nvs_scores_feeds_an_evaluator():
    from mvsdet_amd.evaluation import NVSEvaluator
    from mvsdet_amd.hotpath import MVSDetHotPath
    ref = R.reference(2, 8, 9)
    hot = MVSDetHotPath.__new__(MVSDetHotPath)                             # nvs_scores keeps no state
    ev = NVSEvaluator(device="cpu")
    pred, gt = t(ref["scene"]["pred"])[None], t(ref["scene"]["gt"])
    for out in (hot.nvs_scores(pred, gt), hot.nvs_scores(pred, gt, evaluator=ev)):
        assert list(out) == ["psnr", "ssim", "rmse"] and all(v.dim() == 0 for v in out.values())
        assert close([float(out[k]) for k in out], [ref["triple"][0], ref["triple"][1], 0.0])
    assert abs(ev.compute()["ssim"] - ref["triple"][1]) <= TOL


def test_integration_patch_on_a_stub_module():
    from mvsdet_amd import integration
    calls = []

    def img_original(pred, gt, img_meta, save_dir=None):
        calls.append(("img", save_dir))
        return "original image triple"

    def depth_original(pred, gt, img_meta, save_dir=None):
        calls.append(("depth", save_dir))
        return "original depth"

    stub = types.ModuleType("mvsdet_stub")
    stub.save_rendered_img_Image, stub.save_rendered_depth = img_original, depth_original
    ref = R.reference(2, 8, 9)
    sc = ref["scene"]
    originals = integration.patch_reference_nvs_scores(stub)
    try:
        assert stub.save_rendered_img_Image is not img_original and stub.save_rendered_depth is not depth_original
        psnr, ssim, rmse = stub.save_rendered_img_Image(t(sc["pred"]), t(sc["gt"]), {"img_path": ["a/scene/b.jpg"]}, save_dir=None)
        assert isinstance(psnr, float) and isinstance(ssim, float) and rmse == 0
        assert close([psnr, ssim], ref["triple"][:2])
        depth = stub.save_rendered_depth(t(sc["pred_depth"]), t(sc["gt_depth"]), {}, save_dir=None)
        assert isinstance(depth, float) and abs(depth - ref["triple"][2]) <= TOL
        assert calls == []
        assert stub.save_rendered_img_Image(None, None, {}, save_dir="vis") == "original image triple"
        assert stub.save_rendered_depth(None, None, {}, save_dir="vis") == "original depth"
        assert calls == [("img", "vis"), ("depth", "vis")]
    finally:
        integration.unpatch_reference_nvs_scores(stub, originals)
    assert stub.save_rendered_img_Image is img_original and stub.save_rendered_depth is depth_original
