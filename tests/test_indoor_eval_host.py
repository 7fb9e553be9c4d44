"""Indoor mAP / recall (csrc/evalmap.hip, mvsdet_amd/evaluation.py): the host side, no GPU.  The NumPy restatement of the reference's
indoor_eval (tests/indoor_eval_restated.py) against what the reference itself returned on G21 (tests/golden/make_goldens_g21.py);
the host-side assembly of the dict; the argument checks of the C entries, which launch nothing; refusals off a ROCm device."""
import ctypes
import types

import numpy as np
import pytest
import torch

import indoor_eval_cases as C
import indoor_eval_restated as R

AP_TOL = 2.0 ** -24    # float64 sums in another order than np.sum's: far below a float32 spacing, at most one after rounding


@pytest.fixture(scope="module")
def lib():
    from mvsdet_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_fixture_flags_its_stand_ins():
    s = str(C.golden()["stand_in"])
    assert "overlaps" in s and "not mmcv's box_iou_rotated rounding" in s and "AsciiTable" in s and "print_log" in s


@pytest.mark.parametrize("case", C.CASES)
def test_restatement_equals_the_reference(case):
    g, ev = C.golden(), C.restated(case)
    order = [int(l) for l in g[f"{case}_label_order"]]
    assert list(ev) == order
    n_flags = 0
    for k, lab in enumerate(order):
        for t in range(len(C.thresholds_of(case))):
            rec, pre = g[f"{case}_recall_{t}_{lab}"], g[f"{case}_precision_{t}_{lab}"]
            if ev[lab]["ndet"] == 0:     # ground truth and no prediction: the reference's zeros(1)
                assert rec.tolist() == [0.0] and pre.tolist() == [0.0] and g[f"{case}_ap"][t, k] == 0.0
                continue
            assert np.array_equal(ev[lab]["tp"][t], C.reference_flags(case, t, lab)), (lab, t)
            assert np.array_equal(ev[lab]["recall"][t], rec, equal_nan=True) and np.array_equal(ev[lab]["precision"][t], pre)
            assert C.same_or_both_nan(float(ev[lab]["ap"][t]), float(g[f"{case}_ap"][t, k]), AP_TOL), (lab, t)
            n_flags += len(rec)
    assert n_flags == 2 * int(g[f"{case}_counts"].sum())      # no detection is left out


@pytest.mark.parametrize("case", C.CASES)
def test_restated_dict_has_the_reference_keys_order_and_values(case):
    want = C.ret_dict_of(case)
    got = R.indoor_eval(C.scenes_of(case), C.thresholds_of(case), C.label2cat_of(case))
    assert list(got) == list(want)
    for k in want:
        assert C.same_or_both_nan(got[k], want[k], AP_TOL), (k, got[k], want[k])
    keys = list(want)
    n = len(C.golden()[f"{case}_label_order"])
    assert keys[n] == "mAP_0.25" and keys[2 * n + 1] == "mAR_0.25" and keys[3 * n + 2] == "mAP_0.50" and keys[-1] == "mAR_0.50"
    assert keys[0].endswith("_AP_0.25") and keys[n + 1].endswith("_rec_0.25")


def test_nan_case():
    """A label predicted without ground truth anywhere: NaN AP and recall, NaN mAP and mAR (ARKit case); none in the ScanNet case."""
    want, ev = C.ret_dict_of("arkit"), C.restated("arkit")
    ghosts = [l for l in ev if ev[l]["npos"] == 0]
    assert ghosts and all(ev[l]["ndet"] > 0 for l in ghosts)
    cat = C.label2cat_of("arkit")
    for l in ghosts:
        assert np.isnan(want[f"{cat[l]}_AP_0.25"]) and np.isnan(want[f"{cat[l]}_rec_0.50"]) and np.isnan(ev[l]["ap"]).all()
        assert not ev[l]["tp"].any()
    assert np.isnan(want["mAP_0.25"]) and np.isnan(want["mAR_0.50"])
    assert np.isfinite(list(C.ret_dict_of("scannet").values())).all()


@pytest.mark.parametrize("case", C.CASES)
def test_package_assembly_uses_the_reference_expressions_and_dtypes(case):
    """evaluation.assemble from the reference's own per-label values gives the reference's dict to the last bit: np.mean over
    float32 arrays with a float64 zeros(1) among them where a label has no prediction."""
    from mvsdet_amd import evaluation
    g, ev = C.golden(), C.restated(case)
    order = [int(l) for l in g[f"{case}_label_order"]]
    T = len(C.thresholds_of(case))
    ap = g[f"{case}_ap"].astype(np.float32)
    rec = np.array([[g[f"{case}_recall_{t}_{l}"][-1] for l in order] for t in range(T)])
    ndet = np.array([ev[l]["ndet"] for l in order])
    assert (ndet == 0).any()
    got = evaluation.assemble(order, ap, rec, ndet, C.thresholds_of(case), C.label2cat_of(case))
    want = C.ret_dict_of(case)
    assert list(got) == list(want)
    for k in want:
        assert C.same_or_both_nan(got[k], want[k]), (k, got[k], want[k])


def test_visiting_order_of_the_restatement():
    s = np.array([0.5, np.nan, np.inf, -np.inf, 0.5, -0.0, 0.0], np.float32)
    scene, row = np.array([1, 0, 0, 0, 0, 1, 0]), np.array([0, 0, 1, 2, 3, 1, 4])
    assert R.visiting_order(s, scene, row).tolist() == [2, 4, 0, 6, 5, 3, 1]


def test_restated_iou_planted_values():
    cube = [0, 0, 0, 1, 1, 1, 0]
    assert R.iou3d([cube], [[0, 0.5, 0, 1, 2, 2, 0]])[0, 0] == np.float32(0.25)
    assert R.iou3d([cube], [[0, 0, 0, 1, 1, 2, 0]])[0, 0] == np.float32(0.5)
    rot = R.iou3d([[0, 0, 0, 1, 1, 1, np.pi / 2]], [[0, 0.5, 0, 1, 2, 2, 0]])[0, 0]
    assert abs(float(rot) - 0.25) < 1e-6
    assert R.iou3d([cube], [[3, 0, 0, 1, 1, 1, 0.3]])[0, 0] == 0.0


def test_entry_argument_checks_launch_nothing(lib):
    one = ctypes.c_void_p(4096)
    thr = (ctypes.c_float * 2)(0.25, 0.5)
    err = lambda: lib.mvsdet_last_error()  # noqa: E731
    # sizes
    assert lib.mvsdet_eval_state_bytes(18, 1024, 256) > 6 * 1024 * 4
    assert lib.mvsdet_eval_state_bytes(0, 1024, 256) == 0 and lib.mvsdet_eval_state_bytes(4096, 1024, 256) == 0
    assert lib.mvsdet_eval_state_bytes(18, (1 << 20) + 1, 256) == 0 and lib.mvsdet_eval_state_bytes(18, 1024, 0) == 0
    assert lib.mvsdet_eval_state_bytes(18, -1, 256) == 0
    assert lib.mvsdet_eval_workspace_bytes(18, 100, 256, 2) == lib.mvsdet_eval_workspace_bytes(18, 2048, 256, 2) > 0
    assert lib.mvsdet_eval_workspace_bytes(18, 2049, 256, 2) > lib.mvsdet_eval_workspace_bytes(18, 2048, 256, 2)
    assert lib.mvsdet_eval_workspace_bytes(18, 100, 256, 0) == 0 and lib.mvsdet_eval_workspace_bytes(18, 100, 256, 9) == 0
    assert lib.mvsdet_eval_workspace_bytes(18, -1, 256, 2) == 0
    # reset
    assert lib.mvsdet_eval_reset(None, 1 << 30, 18, 1024, 256, None) == 1 and b"NULL" in err()
    assert lib.mvsdet_eval_reset(one, 1 << 30, 18, 0, 256, None) == 1 and b"capacity=0" in err()
    assert lib.mvsdet_eval_reset(one, 1 << 30, 5000, 1024, 256, None) == 1 and b"n_labels=5000" in err()
    assert lib.mvsdet_eval_reset(one, 16, 18, 1024, 256, None) == 2 and b"needed" in err()
    # match
    args = (18, 1024, 256)
    assert lib.mvsdet_eval_match_f32(None, *args, one, one, one, one, 1, 4, one, one, one, 2, 0, None) == 1 and b"NULL" in err()
    assert lib.mvsdet_eval_match_f32(one, *args, None, one, one, one, 1, 4, one, one, one, 2, 0, None) == 1 and b"predictions" in err()
    assert lib.mvsdet_eval_match_f32(one, *args, one, one, one, None, 1, 4, one, one, one, 2, 0, None) == 1 and b"counts" in err()
    assert lib.mvsdet_eval_match_f32(one, *args, one, one, one, one, 1, 4, None, one, one, 2, 0, None) == 1 and b"ground truth" in err()
    assert lib.mvsdet_eval_match_f32(one, *args, one, one, one, one, -1, 4, one, one, one, 2, 0, None) == 1 and b"B=-1" in err()
    assert lib.mvsdet_eval_match_f32(one, *args, one, one, one, one, 1, -4, one, one, one, 2, 0, None) == 1 and b"Nmax=-4" in err()
    assert lib.mvsdet_eval_match_f32(one, *args, one, one, one, one, 1, 4, one, one, one, 2, -1, None) == 1 and b"scene0=-1" in err()
    assert lib.mvsdet_eval_match_f32(one, 18, 1 << 21, 256, one, one, one, one, 1, 4, one, one, one, 2, 0, None) == 1 and b"capacity" in err()
    assert lib.mvsdet_eval_match_f32(one, *args, None, None, None, None, 0, 0, None, None, None, 0, 0, None) == 0   # nothing to do
    # compute
    outs = (one,) * 8
    assert lib.mvsdet_eval_compute(None, *args, 100, thr, 2, *outs, one, 1 << 30, None) == 1 and b"NULL" in err()
    assert lib.mvsdet_eval_compute(one, *args, 100, None, 2, *outs, one, 1 << 30, None) == 1 and b"NULL" in err()
    assert lib.mvsdet_eval_compute(one, *args, 1025, thr, 2, *outs, one, 1 << 30, None) == 1 and b"n_bound=1025" in err()
    assert lib.mvsdet_eval_compute(one, *args, -1, thr, 2, *outs, one, 1 << 30, None) == 1 and b"n_bound=-1" in err()
    assert lib.mvsdet_eval_compute(one, *args, 100, thr, 9, *outs, one, 1 << 30, None) == 1 and b"thresholds" in err()
    assert lib.mvsdet_eval_compute(one, *args, 100, thr, 2, *outs[:5], None, one, one, one, 1 << 30, None) == 1 and b"flags" in err()
    need = lib.mvsdet_eval_workspace_bytes(18, 100, 256, 2)
    assert lib.mvsdet_eval_compute(one, *args, 100, thr, 2, *outs, one, need - 1, None) == 2 and b"workspace" in err()
    # pairwise IoU
    assert lib.mvsdet_eval_iou_f32(None, 2, one, 2, one, None) == 1 and b"NULL" in err()
    assert lib.mvsdet_eval_iou_f32(one, -2, one, 2, one, None) == 1 and b"n=-2" in err()
    assert lib.mvsdet_eval_iou_f32(None, 0, None, 2, None, None) == 0


def test_inputs_off_a_rocm_device_raise():
    from mvsdet_amd import evaluation, ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        evaluation.IndoorEvaluator(18, device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.eval_iou(torch.zeros(2, 7), torch.zeros(3, 7))
    with pytest.raises(RuntimeError, match="ROCm device"):
        evaluation.indoor_eval([], [], [0.25], {0: "a"}, device="cpu")


def test_patch_reference_indoor_eval_on_a_stand_in():
    from mvsdet_amd import evaluation, integration
    mod = types.SimpleNamespace(indoor_eval=lambda *a, **k: "original")
    saved = integration.patch_reference_indoor_eval(mod, device="cpu")
    try:
        assert mod.indoor_eval is not saved["indoor_eval"]
        with pytest.raises(RuntimeError, match="ROCm device"):      # routed to the package, which refuses the CPU
            mod.indoor_eval([], [], [0.25], {0: "a"})
    finally:
        integration.unpatch_reference_indoor_eval(mod, saved)
    assert mod.indoor_eval() == "original" and evaluation.indoor_eval.__name__ == "indoor_eval"
