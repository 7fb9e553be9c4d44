"""The ARKit head's rotated detection post-processing (csrc/detect.hip: mvsdet_detect_head_rotated_f32, mvsdet_nms3d_f32,
mvsdet_bev_iou_rotated_f32; ops.head_predict_rotated / nms3d / bev_iou_rotated; integration.patch_reference_nms3d): the host side, no
GPU.  Argument checks of the C ABI run on the host and launch nothing; the NumPy restatement of mmcv's nms3d (tests/nms3d_restated.py,
the GPU tests' yardstick) against exact float64 geometry.  `-m refcheck`: G16 regenerated from its seeds."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

import nms3d_restated as R
from conftest import GOLDEN, load_golden

LIMIT = 16384


@pytest.fixture(scope="module")
def lib():
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _expected_workspace(B, points, ncap, C):
    a = lambda v: (v + 255) // 256 * 256  # noqa: E731
    caps = min(ncap, LIMIT)
    words = (caps + 63) // 64
    S = B * C
    return (3 * a(S * 4) + a(B * points * 4) + a(B * ncap * 28) + a(S * ncap * 4)
            + sum(a(S * caps * e) for e in (4, 28, 4, 4, 56, 4)) + a(S * caps * words * 8))


@pytest.mark.parametrize("B,points,ncap,C", [(1, 0, 1, 1), (1, 29200, 2400, 17), (2, 29200, 2400, 17), (1, 29200, 29200, 17),
                                             (1, 0, 16384, 1), (3, 0, 65, 2)])
def test_rotated_workspace_formula(lib, B, points, ncap, C):
    assert lib.mvsdet_detect_rotated_workspace_bytes(B, points, ncap, C) == _expected_workspace(B, points, ncap, C)


def test_rotated_workspace_query_rejects_bad_sizes(lib):
    assert lib.mvsdet_detect_rotated_workspace_bytes(0, 10, 10, 17) == 0
    assert lib.mvsdet_detect_rotated_workspace_bytes(1, -1, 10, 17) == 0
    assert lib.mvsdet_detect_rotated_workspace_bytes(1, 10, 10, 0) == 0


def _head_call(lib, B=1, L=3, dims=(40, 40, 16, 20, 20, 8, 10, 10, 4), n_classes=17, nms_pre=1000, nmax=17 * 2400,
               ws_bytes=1 << 40, null=None):
    one = ctypes.c_void_p(256)
    arr = ctypes.c_void_p * 4
    ptrs = arr(256, 256, 256, 256)
    args = dict(center=ptrs, bbox=ptrs, cls=ptrs, dims=(ctypes.c_int * len(dims))(*dims), valid=one, geom=one, boxes=one,
                scores=one, labels=one, count=one, ws=one)
    if null:
        args[null] = None
    return lib.mvsdet_detect_head_rotated_f32(args["center"], args["bbox"], args["cls"], args["dims"], args["valid"], args["geom"],
                                              B, L, n_classes, 40, 40, 16, nms_pre, 0.01, 0.25, args["boxes"], args["scores"],
                                              args["labels"], args["count"], nmax, args["ws"], ws_bytes, None)


@pytest.mark.parametrize("null", ["center", "bbox", "cls", "dims", "valid", "geom", "boxes", "scores", "labels", "count"])
def test_rotated_head_entry_rejects_null(lib, null):
    assert _head_call(lib, null=null) == 1
    assert b"NULL" in lib.mvsdet_last_error()


def test_rotated_head_entry_argument_checks(lib):
    assert _head_call(lib, L=0) == 1 and b"L=0" in lib.mvsdet_last_error()
    assert _head_call(lib, L=5) == 1 and b"L=5" in lib.mvsdet_last_error()
    assert _head_call(lib, B=0) == 1 and b"B=0" in lib.mvsdet_last_error()
    assert _head_call(lib, n_classes=0) == 1 and b"n_classes" in lib.mvsdet_last_error()
    assert _head_call(lib, n_classes=257, nmax=257 * 2400) == 1 and b"n_classes=257" in lib.mvsdet_last_error()
    assert _head_call(lib, B=4000) == 1 and b"65535 segments" in lib.mvsdet_last_error()
    assert _head_call(lib, nms_pre=-1) == 1 and b"nms_pre" in lib.mvsdet_last_error()
    assert _head_call(lib, dims=(40, 0, 16, 20, 20, 8, 10, 10, 4)) == 1 and b"level 0" in lib.mvsdet_last_error()
    # Nmax: at least n_classes x min(candidates, limit): 17 x 2400 here; 17 x 16384 with nms_pre = 0 (29 200 candidates)
    assert _head_call(lib, nmax=17 * 2400 - 1) == 1 and b"Nmax=40799" in lib.mvsdet_last_error()
    assert _head_call(lib, nms_pre=0, nmax=17 * LIMIT - 1) == 1 and b"278528" in lib.mvsdet_last_error()
    need = lib.mvsdet_detect_rotated_workspace_bytes(1, 40 * 40 * 16 + 20 * 20 * 8 + 10 * 10 * 4, 2400, 17)
    assert _head_call(lib, ws_bytes=need - 1) == 2 and b"workspace" in lib.mvsdet_last_error()


def test_nms3d_entry_argument_checks(lib):
    one = ctypes.c_void_p(256)
    assert lib.mvsdet_nms3d_f32(one, one, 4, 0.25, None, one, one, 1 << 30, None) == 1
    assert b"NULL" in lib.mvsdet_last_error()
    assert lib.mvsdet_nms3d_f32(None, one, 4, 0.25, one, one, one, 1 << 30, None) == 1
    assert lib.mvsdet_nms3d_f32(one, one, -1, 0.25, one, one, one, 1 << 30, None) == 1
    assert lib.mvsdet_nms3d_f32(one, one, LIMIT + 1, 0.25, one, one, one, 1 << 40, None) == 1
    assert b"candidate limit" in lib.mvsdet_last_error() and b"16384" in lib.mvsdet_last_error()
    need = lib.mvsdet_detect_rotated_workspace_bytes(1, 0, 100, 1)
    assert lib.mvsdet_nms3d_f32(one, one, 100, 0.25, one, one, one, need - 1, None) == 2
    assert b"workspace" in lib.mvsdet_last_error()


def test_bev_iou_entry_argument_checks(lib):
    one = ctypes.c_void_p(256)
    assert lib.mvsdet_bev_iou_rotated_f32(one, -1, one, 3, one, None) == 1 and b"n=-1" in lib.mvsdet_last_error()
    assert lib.mvsdet_bev_iou_rotated_f32(one, 1 << 16, one, 1 << 16, one, None) == 1
    assert lib.mvsdet_bev_iou_rotated_f32(None, 2, one, 3, one, None) == 1 and b"NULL" in lib.mvsdet_last_error()
    assert lib.mvsdet_bev_iou_rotated_f32(None, 0, None, 3, None, None) == 0   # nothing to do, nothing launched


# --------------------------------------------------------------------------------------------- Python refusals
def test_rotated_ops_refuse_cpu_tensors():
    from mvsdet_amd import ops
    b = torch.zeros(4, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.nms3d(b, torch.zeros(4), 0.25)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bev_iou_rotated(b, b)


def test_arkit_head_on_cpu_maps_names_nms3d():
    from mvsdet_amd.head import NerfDetHeadConvs
    head = NerfDetHeadConvs(17, 3, 128, 7, arkit_head=True, test_cfg=dict(nms_pre=1000, score_thr=.01, iou_thr=.25))
    sizes = ((40, 40, 16), (20, 20, 8), (10, 10, 4))
    c, r, k = ([torch.zeros(1, ch, *s) for s in sizes] for ch in (1, 7, 17))
    with pytest.raises(NotImplementedError, match="nms3d"):
        head.predict_by_feat(c, r, k, torch.ones(1, 1, 40, 40, 16), [{"lidar2img": {"origin": np.zeros(3, np.float32)}}])


def test_patch_reference_nms3d_on_a_stand_in():
    from mvsdet_amd import integration
    calls = []

    def original(boxes, scores, iou_threshold):
        calls.append(iou_threshold)
        return torch.arange(boxes.shape[0])

    mod = types.ModuleType("nerfdet_head")
    mod.nms3d = original
    saved = integration.patch_reference_nms3d(mod)
    assert mod.nms3d is not original and saved == {"nms3d": original}
    assert mod.nms3d(torch.zeros(3, 7), torch.zeros(3), 0.25).tolist() == [0, 1, 2] and calls == [0.25]   # CPU: the original
    integration.unpatch_reference_nms3d(mod, saved)
    assert mod.nms3d is original


# --------------------------------------------------------------------------------------------- the restatement
def random_boxes(n, seed, spread=2.0):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0, spread, (n, 3)), rng.uniform(0.2, 1.5, (n, 3)), rng.uniform(-4, 4, (n, 1))],
                          1).astype(np.float32)


def test_restatement_matches_exact_geometry():
    a, b = random_boxes(60, 1), random_boxes(70, 2)
    got = R.bev_iou(a, b)
    checked = 0
    for i in range(len(a)):
        for j in range(len(b)):
            if R.corner_in_margin_band(a[i], b[j]):
                continue
            assert abs(float(got[i, j]) - R.exact_iou(a[i], b[j])) < 1e-5, (i, j)
            checked += 1
    assert checked > 2000 and (got > 0).sum() > 500


def test_restatement_hand_cases():
    sq = np.array([[1, 2, 0, 2, 2, 1, 0.4]], np.float32)
    turned = sq.copy()
    turned[0, 6] += np.float32(np.pi / 2)
    assert abs(float(R.bev_iou(sq, turned)[0, 0]) - 1) < 1e-6
    # heading 0: the aligned BEV IoU (corners 1e-2 apart are in each other's margin: stay away from that)
    a = np.array([[0, 0, 0, 2, 1, 1, 0]], np.float32)
    b = np.array([[0.5, 0.25, 5, 2, 1, 3, 0]], np.float32)
    assert abs(float(R.bev_iou(a, b)[0, 0]) - 1.125 / (4 - 1.125)) < 1e-6
    far = np.array([[9, 9, 0, 1, 1, 1, 0.3]], np.float32)
    assert R.bev_iou(a, far)[0, 0] == 0 and R.bev_iou(a, far, skip_far=True)[0, 0] == 0


def test_restatement_far_skip_changes_nothing():
    a = random_boxes(200, 3, spread=6.0)
    assert np.array_equal(R.bev_iou(a[:100], a[100:]), R.bev_iou(a[:100], a[100:], skip_far=True))


# --------------------------------------------------------------------------------------------- against the reference
@pytest.fixture(scope="module")
def reference_predict():
    sys.path.insert(0, GOLDEN)
    import make_goldens_g16 as g
    try:
        return g, g.load_reference_predict()
    except FileNotFoundError:
        pytest.skip("reference tree not mounted")


@pytest.mark.refcheck
def test_g16_regenerates(reference_predict):
    g, RefPredict = reference_predict
    gold = load_golden("g16_detect_arkit")
    for name, (kinds, nms_pre) in g.CASES.items():
        assert list(gold[f"{name}:kinds"]) == list(kinds) and int(gold[f"{name}:nms_pre"]) == nms_pre
        seeds = [int(v) for v in gold[f"{name}:seeds"]]
        res, inputs = g.run_reference(RefPredict, kinds, seeds, nms_pre)
        for i, rs in enumerate(res):
            assert np.array_equal(rs.bboxes_3d.numpy(), gold[f"{name}:{i}:boxes"]), name
            assert np.array_equal(rs.scores_3d.numpy(), gold[f"{name}:{i}:scores"]), name
            assert np.array_equal(rs.labels_3d.numpy(), gold[f"{name}:{i}:labels"]), name
