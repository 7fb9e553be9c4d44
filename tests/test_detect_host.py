"""Detection post-processing (csrc/detect.hip, ops.head_predict / ops.aligned_3d_nms, NerfDetHeadConvs.predict_by_feat,
integration.patch_reference_head): the host side, no GPU.  Argument checks of the C ABI run on the host and launch nothing; the
refusals of the Python layer come before any device work.  `-m refcheck`: the NumPy restatement of the greedy loop below (which the
GPU tests use as their yardstick) against the reference's own aligned_3d_nms, and G15 regenerated from its seeds."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden


# --------------------------------------------------------------------------------------------- the greedy walk, restated
def nms_restated(boxes, scores, classes, thresh):
    """aligned_3d_nms in float32 NumPy: visit the boxes by score (highest first; NaN of either sign above +inf, as the
    reference's argsort places it last and its loop takes from the end; NaNs equal to each other, -0 equal to +0; equal scores by
    lower index); keep a box that
    no kept box has removed; remove every later box j with NOT (iou <= thresh), where the IoU is zeroed for another class and
    written with the reference's association: ((l * w) * h) / ((area_i + area_j) - inter).  A NaN IoU (empty or infinite boxes)
    therefore removes, also across classes.  Returns the kept indices in pick order."""
    b = np.asarray(boxes, np.float32)
    s = np.asarray(scores, np.float32)
    c = np.asarray(classes).astype(np.int64)
    t = np.float32(thresh)
    lo, hi = b[:, :3], b[:, 3:]
    area = ((hi[:, 0] - lo[:, 0]) * (hi[:, 1] - lo[:, 1])) * (hi[:, 2] - lo[:, 2])
    nan = np.isnan(s)
    order = np.lexsort((np.arange(len(s)), -np.where(nan, np.float32(0), s), ~nan))
    picks = []
    with np.errstate(invalid="ignore", over="ignore"):
        while order.size:
            i, rest = order[0], order[1:]
            picks.append(int(i))
            ext = np.maximum(np.minimum(hi[i], hi[rest]) - np.maximum(lo[i], lo[rest]), np.float32(0))
            inter = (ext[:, 0] * ext[:, 1]) * ext[:, 2]
            iou = inter / ((area[i] + area[rest]) - inter)
            iou = iou * (c[rest] == c[i]).astype(np.float32)
            order = rest[iou <= t]
    return np.array(picks, dtype=np.int64)


def nms_case(n, n_classes, seed):
    """Boxes in a 4 m room (0.1 .. 1 m edges), distinct scores, every 37th box of zero volume and every 53rd infinite."""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0, 4, (n, 3)).astype(np.float32)
    half = rng.uniform(0.05, 0.5, (n, 3)).astype(np.float32)
    boxes = np.concatenate([ctr - half, ctr + half], 1).astype(np.float32)
    boxes[::37, 3] = boxes[::37, 0]
    boxes[5::53, 4] = np.inf
    scores = (rng.permutation(n).astype(np.float32) + 1) / np.float32(n + 1)
    classes = rng.integers(0, n_classes, n).astype(np.int64)
    return boxes, scores, classes


# --------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _expected_workspace(B, points, ncap):
    a = lambda v: (v + 255) // 256 * 256  # noqa: E731
    caps = min(ncap, 16384)
    words = (caps + 63) // 64
    return (a(B * 4 * 4) + a(B * 4) + 2 * a(B * points * 4) + a(B * ncap * 24) + a(B * ncap * 4) + a(B * ncap * 8)
            + a(B * caps * 24) + a(B * caps * 4) + a(B * caps * 8) + a(B * caps * 4) + a(B * caps * words * 8))


@pytest.mark.parametrize("B,points,ncap", [(1, 0, 0), (1, 0, 1), (1, 29200, 2400), (2, 29200, 2400), (1, 29200, 29200),
                                           (3, 0, 16384), (1, 0, 65)])
def test_workspace_formula(lib, B, points, ncap):
    assert lib.mvsdet_detect_workspace_bytes(B, points, ncap) == _expected_workspace(B, points, ncap)


def test_workspace_query_rejects_bad_sizes(lib):
    assert lib.mvsdet_detect_workspace_bytes(0, 10, 10) == 0
    assert lib.mvsdet_detect_workspace_bytes(1, -1, 10) == 0


def _head_call(lib, B=1, L=3, dims=(40, 40, 16, 20, 20, 8, 10, 10, 4), n_classes=18, nms_pre=1000, nmax=2400, ws_bytes=1 << 40,
               null=None):
    one = ctypes.c_void_p(256)
    arr = ctypes.c_void_p * 4
    ptrs = arr(256, 256, 256, 256)
    args = dict(center=ptrs, bbox=ptrs, cls=ptrs, dims=(ctypes.c_int * len(dims))(*dims), valid=one, geom=one, boxes=one,
                scores=one, labels=one, count=one, ws=one)
    if null:
        args[null] = None
    return lib.mvsdet_detect_head_f32(args["center"], args["bbox"], args["cls"], args["dims"], args["valid"], args["geom"], B, L,
                                      n_classes, 40, 40, 16, nms_pre, 0.01, 0.25, args["boxes"], args["scores"], args["labels"],
                                      args["count"], nmax, args["ws"], ws_bytes, None)


@pytest.mark.parametrize("null", ["center", "bbox", "cls", "dims", "valid", "geom", "boxes", "scores", "labels", "count"])
def test_head_entry_rejects_null(lib, null):
    assert _head_call(lib, null=null) == 1
    assert b"NULL" in lib.mvsdet_last_error()


def test_head_entry_argument_checks(lib):
    assert _head_call(lib, L=0) == 1 and b"L=0" in lib.mvsdet_last_error()
    assert _head_call(lib, L=5) == 1 and b"L=5" in lib.mvsdet_last_error()
    assert _head_call(lib, B=0) == 1 and b"B=0" in lib.mvsdet_last_error()
    assert _head_call(lib, n_classes=0) == 1 and b"n_classes" in lib.mvsdet_last_error()
    assert _head_call(lib, nms_pre=-1) == 1 and b"nms_pre" in lib.mvsdet_last_error()
    assert _head_call(lib, dims=(40, 0, 16, 20, 20, 8, 10, 10, 4)) == 1 and b"level 0" in lib.mvsdet_last_error()
    # Nmax: at least min(candidates, limit): 1000 + 1000 + 400 here; 16384 with nms_pre = 0 (29 200 candidates)
    assert _head_call(lib, nmax=2399) == 1 and b"Nmax=2399" in lib.mvsdet_last_error()
    assert _head_call(lib, nms_pre=0, nmax=16383) == 1 and b"16384" in lib.mvsdet_last_error()
    need = lib.mvsdet_detect_workspace_bytes(1, 40 * 40 * 16 + 20 * 20 * 8 + 10 * 10 * 4, 2400)
    assert _head_call(lib, ws_bytes=need - 1) == 2 and b"workspace" in lib.mvsdet_last_error()


def test_nms_entry_argument_checks(lib):
    one = ctypes.c_void_p(256)
    assert lib.mvsdet_aligned_3d_nms_f32(one, one, one, 4, 0.25, None, one, one, 1 << 30, None) == 1
    assert b"NULL" in lib.mvsdet_last_error()
    assert lib.mvsdet_aligned_3d_nms_f32(None, one, one, 4, 0.25, one, one, one, 1 << 30, None) == 1
    assert lib.mvsdet_aligned_3d_nms_f32(one, one, one, -1, 0.25, one, one, one, 1 << 30, None) == 1
    assert lib.mvsdet_aligned_3d_nms_f32(one, one, one, 16385, 0.25, one, one, one, 1 << 40, None) == 1
    assert b"candidate limit" in lib.mvsdet_last_error() and b"16384" in lib.mvsdet_last_error()
    need = lib.mvsdet_detect_workspace_bytes(1, 0, 100)
    assert lib.mvsdet_aligned_3d_nms_f32(one, one, one, 100, 0.25, one, one, one, need - 1, None) == 2
    assert b"workspace" in lib.mvsdet_last_error()


# --------------------------------------------------------------------------------------------- Python refusals
def test_aligned_3d_nms_refuses_cpu_tensors():
    from mvsdet_amd import ops
    b, s, c = nms_case(8, 2, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.aligned_3d_nms(torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(c), 0.25)


def _maps(B=1, n_reg=6, C=18):
    sizes = ((40, 40, 16), (20, 20, 8), (10, 10, 4))
    return ([torch.zeros(B, 1, *s) for s in sizes], [torch.zeros(B, n_reg, *s) for s in sizes],
            [torch.zeros(B, C, *s) for s in sizes], torch.ones(B, 1, 40, 40, 16))


def test_arkit_head_has_no_nms():
    from mvsdet_amd.head import NerfDetHeadConvs
    head = NerfDetHeadConvs(17, 3, 128, 7, arkit_head=True, test_cfg=dict(nms_pre=1000, score_thr=.01, iou_thr=.25))
    c, r, k, v = _maps(n_reg=7, C=17)
    with pytest.raises(NotImplementedError, match="nms3d"):
        head.predict_by_feat(c, r, k, v, [{"lidar2img": {"origin": np.zeros(3, np.float32)}}])


def test_float64_origin_is_refused():
    from mvsdet_amd.head import NerfDetHeadConvs
    head = NerfDetHeadConvs(test_cfg=types.SimpleNamespace(nms_pre=1000, score_thr=.01, iou_thr=.25))
    c, r, k, v = _maps()
    with pytest.raises(ValueError, match="float32"):
        head.predict_by_feat(c, r, k, v, [{"lidar2img": {"origin": np.zeros(3, np.float64)}}])


def test_predict_without_test_cfg_is_refused():
    from mvsdet_amd.head import NerfDetHeadConvs
    c, r, k, v = _maps()
    with pytest.raises(ValueError, match="test_cfg"):
        NerfDetHeadConvs().predict_by_feat(c, r, k, v, [{"lidar2img": {"origin": np.zeros(3, np.float32)}}])


def test_level_geometry_is_the_reference_arithmetic():
    from mvsdet_amd import ops
    o = torch.tensor([3.1, 2.9, 1.4])
    g = ops.detect_level_geometry([(40, 40, 16), (20, 20, 8)], [o])
    assert g.shape == (1, 2, 6) and g.dtype == torch.float32
    vs = torch.tensor([.16, .16, .2]) * 2
    assert torch.equal(g[0, 1, :3], vs) and torch.equal(g[0, 1, 3:], o - torch.tensor([20, 20, 8]) / 2. * vs)
    assert ops.detect_candidates([(40, 40, 16), (20, 20, 8), (10, 10, 4)], 1000) == 2400
    assert ops.detect_candidates([(40, 40, 16), (20, 20, 8), (10, 10, 4)], 0) == 29200
    assert ops.detect_candidates([(40, 40, 16), (20, 20, 8), (10, 10, 4)], 30000) == 29200


def test_patch_reference_head_on_a_stand_in():
    from mvsdet_amd import integration

    class NerfDetHead:
        @staticmethod
        def aligned_3d_nms(boxes, scores, classes, thresh):
            return "original"

    mod = types.ModuleType("nerfdet_head_stand_in")
    mod.NerfDetHead = NerfDetHead
    before = NerfDetHead.__dict__["aligned_3d_nms"]
    orig = integration.patch_reference_head(mod)
    try:
        assert NerfDetHead.__dict__["aligned_3d_nms"] is not before
        assert orig == {"NerfDetHead.aligned_3d_nms": before}
        b, s, c = (torch.from_numpy(a) for a in nms_case(4, 2, 1))
        assert NerfDetHead.aligned_3d_nms(b, s, c, 0.25) == "original"          # CPU tensors: the original
        assert NerfDetHead().aligned_3d_nms(b, s, c, 0.25) == "original"        # still a static method
    finally:
        integration.unpatch_reference_head(mod, orig)
    assert NerfDetHead.__dict__["aligned_3d_nms"] is before


def test_restatement_on_a_small_hand_case():
    # 0 and 1 overlap by half (IoU 1/3); 2 and 3 are infinite boxes of two classes: inf / NaN = NaN, NaN * 0 = NaN removes 3
    inf = np.inf
    boxes = np.array([[0, 0, 0, 2, 1, 1], [1, 0, 0, 3, 1, 1], [0, 0, 0, inf, 1, 1], [0, 0, 0, inf, 1, 1]], np.float32)
    scores = np.array([.9, .8, .7, .6], np.float32)
    classes = np.array([0, 0, 1, 0])
    assert nms_restated(boxes, scores, classes, .25).tolist() == [0, 2]
    assert nms_restated(boxes, scores, classes, .5).tolist() == [0, 1, 2]
    boxes[3] = [4, 4, 4, 5, 5, 5]
    assert nms_restated(boxes, scores, classes, .5).tolist() == [0, 1, 2, 3]


def f32_bits(*words):
    return np.array(words, np.uint32).view(np.float32)


NEG_NAN, POS_NAN = f32_bits(0xffc00000)[0], f32_bits(0x7fc00000)[0]   # torch.zeros(1) / 0 on x86 is the first


def test_restatement_orders_nan_zero_and_inf():
    # disjoint boxes, so every box is kept and the pick order is the visiting order: NaN of either sign first (by index), +inf,
    # the finite scores, -0 and +0 as equals (by index), -inf last
    boxes = np.array([[3 * i, 0, 0, 3 * i + 1, 1, 1] for i in range(8)], np.float32)
    scores = np.array([.5, NEG_NAN, 0., -0., np.inf, -np.inf, POS_NAN, .5], np.float32)
    assert nms_restated(boxes, scores, np.zeros(8), .25).tolist() == [1, 6, 4, 0, 7, 2, 3, 5]
    assert nms_restated(boxes, scores[::-1].copy(), np.zeros(8), .25).tolist() == [1, 6, 3, 0, 7, 4, 5, 2]
    # the two cases of identical same-class boxes: the NaN-scored one is the reference's pick; -0 and +0 tie, index 0 first
    same = np.array([[0, 0, 0, 1, 1, 1]] * 2, np.float32)
    assert nms_restated(same, np.array([.5, NEG_NAN], np.float32), [0, 0], .25).tolist() == [1]
    assert nms_restated(same, np.array([-0., 0.], np.float32), [0, 0], .25).tolist() == [0]


# --------------------------------------------------------------------------------------------- against the reference
@pytest.fixture(scope="module")
def reference_predict():
    sys.path.insert(0, GOLDEN)
    import make_goldens_g15 as g
    try:
        return g, g.load_reference_predict()
    except FileNotFoundError:
        pytest.skip("reference tree not mounted")


@pytest.mark.refcheck
@pytest.mark.parametrize("n,n_classes,thresh", [(1, 1, .25), (65, 1, .25), (300, 18, .25), (300, 1, 0.0), (300, 18, 1.0),
                                                (1000, 4, .25)])
def test_restatement_matches_reference_nms(reference_predict, n, n_classes, thresh):
    _, RefPredict = reference_predict
    b, s, c = nms_case(n, n_classes, 100 + n)
    ref = RefPredict.aligned_3d_nms(torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(c), thresh)
    assert ref.tolist() == nms_restated(b, s, c, thresh).tolist()


@pytest.mark.refcheck
def test_g15_regenerates(reference_predict):
    g, RefPredict = reference_predict
    gold = load_golden("g15_detect")
    for name, (kinds, nms_pre) in g.CASES.items():
        assert list(gold[f"{name}:kinds"]) == list(kinds) and int(gold[f"{name}:nms_pre"]) == nms_pre
        seeds = [int(v) for v in gold[f"{name}:seeds"]]
        res, inputs = g.run_reference(RefPredict, kinds, seeds, nms_pre)
        assert not g.near_decisions(inputs, nms_pre), name
        for i, rs in enumerate(res):
            assert np.array_equal(rs.bboxes_3d.numpy(), gold[f"{name}:{i}:boxes"]), name
            assert np.array_equal(rs.scores_3d.numpy(), gold[f"{name}:{i}:scores"]), name
            assert np.array_equal(rs.labels_3d.numpy(), gold[f"{name}:{i}:labels"]), name


@pytest.mark.refcheck
@pytest.mark.parametrize("nan", ["+nan", "-nan"])
@pytest.mark.parametrize("n,n_classes", [(2, 1), (9, 2), (16, 1), (300, 1), (300, 18)])
def test_restatement_matches_reference_nms_with_a_nan(reference_predict, nan, n, n_classes):
    # distinct scores but one NaN: no ties, so the reference's order does not hang on its sort being stable
    _, RefPredict = reference_predict
    b, s, c = nms_case(n, n_classes, 200 + n)
    s[n // 2] = NEG_NAN if nan == "-nan" else POS_NAN
    b[n // 2] = b[0]                      # the NaN-scored box overlaps box 0: it is picked first and removes box 0 (same class)
    c[n // 2] = c[0]
    for thresh in (.25, 1.0):
        ref = RefPredict.aligned_3d_nms(torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(c), thresh)
        want = nms_restated(b, s, c, thresh)
        assert ref.tolist() == want.tolist()
        assert want[0] == n // 2


@pytest.mark.refcheck
@pytest.mark.parametrize("name", ["l1_c18", "l4_ragged_c40_b3_pre440", "l4_ragged_c1_pre439", "l4_ragged_c2_b3_pre441",
                                  "l2_larger_than_valid_c2_pre0", "l2_larger_than_valid_c18_b3_pre1", "l3_scannet_c40_b3_pre1000"])
def test_head_restatement_matches_reference(reference_predict, name):
    # tests/detect_restated.predict (the GPU tests' yardstick) against the reference's predict_by_feat, both on the CPU: counts,
    # labels and pick order equal, boxes and scores bit for bit, at the level counts, shapes and class counts of family (a)
    import detect_restated as R
    g, RefPredict = reference_predict
    (c, r, k, v, origins), nms_pre = R.case_a(name)
    assert not R.near_decisions(c, r, k, v, origins, nms_pre, R.SCORE_THR, R.IOU_THR), name
    cfg = types.SimpleNamespace(nms_pre=nms_pre, score_thr=R.SCORE_THR, iou_thr=R.IOU_THR)
    with torch.no_grad():
        ref = RefPredict(cfg).predict_by_feat(c, r, k, v, g.metas_for(origins))
    want = R.predict(c, r, k, v, origins, nms_pre, R.SCORE_THR, R.IOU_THR)
    for i, (rs, w) in enumerate(zip(ref, want)):
        assert len(rs.scores_3d) == w["count"] > 0, (name, i)
        assert np.array_equal(rs.labels_3d.numpy(), w["labels"]), (name, i)
        assert np.array_equal(rs.bboxes_3d.numpy().view(np.uint32), w["boxes"].view(np.uint32)), (name, i)
        assert np.array_equal(rs.scores_3d.numpy().view(np.uint32), w["scores"].view(np.uint32)), (name, i)
