"""Detection kernels (csrc/detect.hip) at the edges of their input space, each case against the CPU restatement of
tests/detect_restated.py (itself checked against the reference's predict_by_feat by test_detect_host's refcheck tests):
(a) level counts 1..4, non-integer upsampling ratios, a level larger than the valid volume, 1..40 classes, batches, nms_pre around
a level's size; (b) exact ties (logits of -inf / 0 / +inf: scores of exactly 0, .25, .5, 1); (c) NaN and +-inf in the maps;
(d) the candidate limit inside a batch; (e) the standalone NMS on quantised, NaN, signed-zero and infinite scores; (f) both entry
points through the C ABI with their outputs and workspace inside sentinel canvases."""
import ctypes
import types

import numpy as np
import pytest
import torch

import detect_restated as R
from test_detect_host import NEG_NAN, POS_NAN, f32_bits, nms_case, nms_restated

pytestmark = pytest.mark.gpu

INF = float("inf")
SENTINEL = 0x5A5A5A5A      # guard word of the canvases
GARBAGE = 0x7F7F7F7F       # what the region holds before a call: rows the kernels must zero are not zero already
GUARD = 1 << 16            # 256 KiB of 4-byte words on each side


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits_nan(got, want):
    """Bit for bit, except that a NaN may carry another sign or payload."""
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def run(gpu, maps, nms_pre, score_thr=R.SCORE_THR, iou_thr=R.IOU_THR):
    from mvsdet_amd import ops
    c, r, k, v, origins = maps
    dev = lambda ts: [t.to(gpu) for t in ts]  # noqa: E731
    pred = ops.head_predict(dev(c), dev(r), dev(k), v.to(gpu), origins, nms_pre, score_thr, iou_thr)
    return pred, R.predict(c, r, k, v, origins, nms_pre, score_thr, iou_thr)


def check(pred, want, exact, tag=""):
    """Every scene: count, labels and pick order equal, boxes bit for bit (NaN as NaN), scores bit for bit or within 1e-6, zero rows
    past the count (all rows for a count above the limit)."""
    counts = pred.counts.cpu().tolist()
    assert counts == [w["count"] for w in want], tag
    boxes, scores, labels = pred.boxes.cpu().numpy(), pred.scores.cpu().numpy(), pred.labels.cpu().numpy()
    for i, w in enumerate(want):
        n = max(w["count"], 0)
        assert np.array_equal(labels[i, :n], w["labels"]), f"{tag} scene {i}: labels / pick order"
        assert same_bits_nan(boxes[i, :n], w["boxes"]), f"{tag} scene {i}: boxes"
        if exact:
            assert np.array_equal(bits(scores[i, :n]), bits(w["scores"])), f"{tag} scene {i}: scores"
        else:
            np.testing.assert_allclose(scores[i, :n], w["scores"], rtol=1e-6, atol=0, err_msg=f"{tag} scene {i}")
        assert not bits(boxes[i, n:]).any() and not bits(scores[i, n:]).any() and not labels[i, n:].any(), f"{tag} scene {i}: pad"


# ------------------------------------------------------------------------------------------------ (a) shapes, general logits
@pytest.mark.parametrize("name", list(R.CASES_A))
def test_shapes(gpu, name):
    maps, nms_pre = R.case_a(name)
    assert not R.near_decisions(*maps, nms_pre, R.SCORE_THR, R.IOU_THR), name
    pred, want = run(gpu, maps, nms_pre)
    assert all(w["count"] > 0 for w in want)
    check(pred, want, exact=False, tag=name)


@pytest.mark.parametrize("nms_pre", [1, 439, 440, 441, 1000])
def test_nms_pre_around_a_level_size(gpu, nms_pre):
    # the ragged levels have 3192, 440, 60 and 9 points: nms_pre 439 / 440 / 441 cut level 1 by one, exactly not, and not
    # (nms_pre 0 is test_shapes' l2_larger_than_valid_c2_pre0)
    maps, _ = R.case_a("l4_ragged_c2_b3_pre441")
    assert not R.near_decisions(*maps, nms_pre, R.SCORE_THR, R.IOU_THR), nms_pre
    pred, want = run(gpu, maps, nms_pre)
    check(pred, want, exact=False, tag=f"nms_pre={nms_pre}")


# ------------------------------------------------------------------------------------------------ (b) exact ties
def tie_maps(sizes, valid_shape, C, B, seed, p_cls=(.6, .3, .1), p_ctr=(0., .5, .5), reg=(.05, .3)):
    """Logits drawn from {-inf, 0, +inf}: every score is exactly 0, .25, .5 or 1 on any device.  Box regressions uniform in reg."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-INF, 0., INF])
    pick = lambda p, shape: vals[torch.multinomial(torch.tensor(p), int(np.prod(shape)), True, generator=g)].view(shape)  # noqa
    centers = [pick(p_ctr, (B, 1) + tuple(s)) for s in sizes]
    clss = [pick(p_cls, (B, C) + tuple(s)) for s in sizes]
    bboxes = [reg[0] + (reg[1] - reg[0]) * torch.rand((B, 6) + tuple(s), generator=g) for s in sizes]
    valid = torch.ones((B, 1) + tuple(valid_shape))
    origins = [torch.tensor([3.0, 3.0, 1.5]) for _ in range(B)]
    return centers, bboxes, clss, valid, origins


def eq_taken(maps, nms_pre, b=0, lvl=0):
    """Voxel indices of the points a level's top-k takes from the run of scores equal to its boundary score."""
    c, r, k, v, origins = maps
    vm = R.upsampled_valid(v, [c[lvl].shape[-3:]])[0][b].round().bool()
    _, ms, _ = R.level_scores(c[lvl][b], k[lvl][b], vm)
    ids = R.topk_ids(ms, nms_pre)
    t = ms[ids].min()
    return ids[(ms[ids] == t).numpy()], int((ms > t).sum())


def test_ties_topk_boundary_spans_chunks(gpu):
    # 25 600 points, about 1/3 at 1.0 / .5 and the rest .25 / 0: the 6000th score sits inside a run of equal scores whose taken part
    # (lowest voxel first) spans several 1024-point chunks of the select kernel
    maps = tie_maps([(40, 40, 16)], (40, 40, 16), 3, 1, 7, p_cls=(.75, .2, .05), p_ctr=(0., .6, .4))
    taken, _ = eq_taken(maps, 6000)
    assert len(taken) > 1 and taken.max() // 1024 - taken.min() // 1024 >= 2
    pred, want = run(gpu, maps, 6000)
    assert want[0]["count"] > 64
    check(pred, want, exact=True)


@pytest.mark.parametrize("k", [2047, 2048, 2049])
def test_ties_need_eq_ends_on_a_chunk_edge(gpu, k):
    # every score .5 but 100 points at 1.0 in the first chunk: with k = 2048 the last taken equal point is voxel 2047, the last of
    # the second chunk; 2047 and 2049 stop one before and one after it
    maps = tie_maps([(40, 40, 16)], (40, 40, 16), 1, 1, 8, reg=(.01, .02))
    c, r, cls, v, o = maps
    cls[0].fill_(INF)
    c[0].fill_(0.)
    c[0].view(-1)[100:200] = INF
    taken, above = eq_taken(maps, k)
    assert above == 100 and taken.max() == k - 1 and len(taken) == k - 100
    pred, want = run(gpu, maps, k)
    assert want[0]["count"] == k
    check(pred, want, exact=True)


def test_ties_across_levels_and_nms_blocks(gpu):
    # three levels of tied scores, boxes large enough to suppress across 64-box blocks; equal scores go level, then voxel
    maps = tie_maps([(20, 20, 8), (10, 10, 4), (5, 5, 2)], (20, 20, 8), 2, 3, 9, p_cls=(.4, .4, .2), reg=(.1, .5))
    pred, want = run(gpu, maps, 700)
    assert all(w["count"] > 64 for w in want)
    check(pred, want, exact=True)


def test_ties_first_class_wins(gpu):
    # several classes at +inf in a voxel: the first of them is the label (max / first argmax)
    maps = tie_maps([(10, 10, 4)], (10, 10, 4), 6, 1, 10, p_cls=(.5, .2, .3), reg=(.01, .05))
    c, r, k, v, o = maps
    k[0][0, :, 0, 0, 0] = torch.tensor([0., -INF, INF, 0., INF, INF])
    c[0][0, 0, 0, 0, 0] = INF
    pred, want = run(gpu, maps, 0)
    first = k[0][0].reshape(6, -1).t() == INF
    assert (first.sum(1) >= 2).sum() > 10
    check(pred, want, exact=True)
    assert 2 in want[0]["labels"].tolist()


def test_ties_negative_score_thr(gpu):
    # score_thr < 0: zero scores (invalid voxels, -inf logits) survive and tie at the top-k boundary
    maps = tie_maps([(20, 20, 8), (10, 10, 4)], (20, 20, 8), 3, 3, 11, p_cls=(.9, .08, .02), reg=(.01, .05))
    maps[3][1].zero_()     # scene 1: no views anywhere, every score is 0
    pred, want = run(gpu, maps, 1000, score_thr=-0.5)
    assert all(w["count"] > 1000 for w in want)
    assert (want[1]["scores"] == 0).all()
    check(pred, want, exact=True)


# ------------------------------------------------------------------------------------------------ (c) non-finite maps
def test_nan_logits_take_topk_slots(gpu):
    # NaN class or centre logits at points that would otherwise win top-k slots: NaN is the largest score, takes a slot, and
    # score_thr then drops it, so fewer boxes come out than nms_pre allows
    maps = tie_maps([(20, 20, 8), (10, 10, 4)], (20, 20, 8), 4, 3, 12, p_cls=(.7, .2, .1), reg=(.05, .3))
    c, r, k, v, o = maps
    g = torch.Generator().manual_seed(13)
    for lvl in range(2):
        n = c[lvl].shape[2] * c[lvl].shape[3] * c[lvl].shape[4]
        ids = torch.randperm(n, generator=g)[:n // 40]
        k[lvl].view(3, 4, -1)[:, 1, ids[::2]] = float("nan")
        c[lvl].view(3, 1, -1)[:, 0, ids[1::2]] = -float("nan")
    pred, want = run(gpu, maps, 300)
    assert all(0 < w["count"] < 600 for w in want)
    check(pred, want, exact=True)


def test_nan_and_inf_box_regression(gpu):
    # NaN / +-inf regressions make NaN IoUs, which suppress across classes (NaN * 0); kept NaN boxes come out as NaN
    maps = tie_maps([(10, 10, 4), (5, 5, 2)], (10, 10, 4), 3, 3, 14, p_cls=(.5, .3, .2), reg=(.05, .3))
    c, r, k, v, o = maps
    g = torch.Generator().manual_seed(15)
    for lvl in range(2):
        flat = r[lvl].view(-1)
        ids = torch.randperm(flat.numel(), generator=g)[:flat.numel() // 40]
        flat[ids[0::3]] = float("nan")
        flat[ids[1::3]] = INF
        flat[ids[2::3]] = -INF
    pred, want = run(gpu, maps, 0)
    assert any(not np.isfinite(w["boxes"]).all() for w in want)
    check(pred, want, exact=True)


# ------------------------------------------------------------------------------------------------ (d) the candidate limit
def test_candidate_limit_in_a_batch(gpu):
    # one level of 17 x 31 x 32 = 16 864 points, nms_pre 0; scene 0 has 16 385 survivors (count -16 385, zero rows), scene 1
    # exactly 16 384 (the full 128 KiB sort, all 256 removed[] words), scene 2 a few hundred
    from mvsdet_amd.head import NerfDetHeadConvs, unpad_predictions
    maps = tie_maps([(17, 31, 32)], (17, 31, 32), 2, 3, 16, p_cls=(0., .7, .3), p_ctr=(0., .5, .5), reg=(.05, .12))
    c, r, k, v, o = maps
    for b, n in enumerate((16385, 16384, 300)):
        k[0].view(3, 2, -1)[b, :, n:] = -INF
    pred, want = run(gpu, maps, 0)
    assert [w["count"] for w in want][0] == -16385 and want[1]["count"] > 0 and want[2]["count"] > 0
    check(pred, want, exact=True)
    with pytest.raises(RuntimeError, match="16385 boxes.*candidate limit 16384"):
        unpad_predictions(pred, [{} for _ in range(3)])
    head = NerfDetHeadConvs(test_cfg=types.SimpleNamespace(nms_pre=0, score_thr=R.SCORE_THR, iou_thr=R.IOU_THR))
    metas = [{"lidar2img": {"origin": oi.numpy()}} for oi in o]
    with pytest.raises(RuntimeError, match="MVSDET_DETECT_MAX_CANDIDATES"):
        head.predict_by_feat([c[0].to(gpu)], [r[0].to(gpu)], [k[0].to(gpu)], v.to(gpu), metas)


# ------------------------------------------------------------------------------------------------ (e) standalone NMS
def nms_gpu(gpu, b, s, c, thresh):
    from mvsdet_amd import ops
    return ops.aligned_3d_nms(torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu), torch.from_numpy(c).to(gpu),
                              thresh).cpu().numpy()


SAME = np.array([[0, 0, 0, 1, 1, 1]] * 2, np.float32)     # two identical same-class boxes: only the first visited is kept


def test_nms_hand_case_negative_nan(gpu):
    # x86's 0/0 NaN (sign bit set) is the reference's first pick (its argsort puts every NaN last, the loop takes from the end)
    assert nms_gpu(gpu, SAME, np.array([.5, NEG_NAN], np.float32), np.zeros(2, np.int64), .25).tolist() == [1]


def test_nms_hand_case_signed_zero(gpu):
    # -0 and +0 are equal scores: the lower index first
    assert nms_gpu(gpu, SAME, np.array([-0., 0.], np.float32), np.zeros(2, np.int64), .25).tolist() == [0]


def test_nms_hand_case_order(gpu):
    # disjoint boxes, all kept: NaN of either sign first, +inf, .5 twice, -0 and +0 as equals, -inf (test_detect_host's case)
    boxes = np.array([[3 * i, 0, 0, 3 * i + 1, 1, 1] for i in range(8)], np.float32)
    scores = np.array([.5, NEG_NAN, 0., -0., INF, -INF, POS_NAN, .5], np.float32)
    assert nms_gpu(gpu, boxes, scores, np.zeros(8, np.int64), .25).tolist() == [1, 6, 4, 0, 7, 2, 3, 5]


@pytest.mark.parametrize("n", [2, 17, 64, 65, 1000, 16384])
@pytest.mark.parametrize("kind", ["quantised", "non_finite"])
def test_nms_tied_and_non_finite_scores(gpu, n, kind):
    b, _, c = nms_case(n, 3, 3000 + n)
    rng = np.random.default_rng(n)
    if kind == "quantised":       # at most 8 distinct values: long runs of ties, broken by the index
        levels = np.array([.1, .2, .3, .4, .5, .6, .7, .8], np.float32)
    else:                         # NaN of both signs (and other payloads), -0, +0, +-inf and two finite values
        levels = np.concatenate([f32_bits(0x7fc00000, 0xffc00000, 0x7f800001, 0xffc12345, 0x80000000),
                                 np.array([0., INF, -INF, .5, .25], np.float32)])
    s = levels[rng.integers(0, len(levels), n)]
    for thresh in ((.25,) if n == 16384 else (0., .25, 1.)):
        got = nms_gpu(gpu, b, s, c, thresh)
        assert np.array_equal(got, nms_restated(b, s, c, thresh)), (kind, n, thresh)


# ------------------------------------------------------------------------------------------------ (f) guard canvases
class Guarded:
    """nwords 4-byte words in the middle of a sentinel canvas; the region starts as GARBAGE."""

    def __init__(self, nwords, dev):
        self.n = int(nwords)
        self.canvas = torch.full((GUARD + (self.n + 63) // 64 * 64 + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.region = self.canvas[GUARD:GUARD + self.n]
        self.region.fill_(GARBAGE)

    def ptr(self):
        return ctypes.c_void_p(self.region.data_ptr())

    def guards_intact(self):
        return bool((self.canvas[:GUARD] == SENTINEL).all()) and bool((self.canvas[GUARD + self.n:] == SENTINEL).all())


def ok(rc):
    from mvsdet_amd import _lib
    if rc != 0:
        raise AssertionError(_lib.load().mvsdet_last_error().decode())
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["ragged", "limit"])
def test_head_entry_inside_guards(gpu, case):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    if case == "ragged":
        (c, r, k, v, o), nms_pre = R.case_a("l4_ragged_c2_b3_pre441")
    else:
        c, r, k, v, o = tie_maps([(17, 31, 32)], (17, 31, 32), 2, 2, 16, p_cls=(0., .7, .3), reg=(.05, .12))
        k[0].view(2, 2, -1)[0, :, 16385:] = -INF
        k[0].view(2, 2, -1)[1, :, 16384:] = -INF
        nms_pre = 0
    c, r, k, v = [t.to(gpu) for t in c], [t.to(gpu) for t in r], [t.to(gpu) for t in k], v.to(gpu)
    ref = ops.head_predict(c, r, k, v, o, nms_pre, R.SCORE_THR, R.IOU_THR)
    sizes = [tuple(t.shape[2:]) for t in c]
    B, L, C = v.shape[0], len(c), k[0].shape[1]
    points, ncap = sum(int(np.prod(s)) for s in sizes), ops.detect_candidates(sizes, nms_pre)
    nmax = min(ncap, ops.DETECT_MAX_CANDIDATES)
    wsb = int(lib.mvsdet_detect_workspace_bytes(B, points, ncap))
    gws, gbox, gsc, glab, gcnt = (Guarded(wsb // 4, gpu), Guarded(B * nmax * 6, gpu), Guarded(B * nmax, gpu),
                                  Guarded(B * nmax * 2, gpu), Guarded(B, gpu))
    geom = ops.detect_level_geometry(sizes, o).to(gpu)
    arr = ctypes.c_void_p * L
    dims = [int(d) for s in sizes for d in s]
    ok(lib.mvsdet_detect_head_f32(arr(*[t.data_ptr() for t in c]), arr(*[t.data_ptr() for t in r]), arr(*[t.data_ptr() for t in k]),
                                  (ctypes.c_int * len(dims))(*dims), _lib.ptr(v), _lib.ptr(geom), B, L, C, *v.shape[2:], nms_pre,
                                  R.SCORE_THR, R.IOU_THR, gbox.ptr(), gsc.ptr(), glab.ptr(), gcnt.ptr(), nmax, gws.ptr(), wsb, None))
    assert all(g.guards_intact() for g in (gws, gbox, gsc, glab, gcnt))
    assert torch.equal(gcnt.region, ref.counts)
    assert torch.equal(gbox.region.view(B, nmax, 6), ref.boxes.view(torch.int32))
    assert torch.equal(gsc.region.view(B, nmax), ref.scores.view(torch.int32))
    assert torch.equal(glab.region.view(torch.int64).view(B, nmax), ref.labels)
    for i, n in enumerate(ref.counts.cpu().tolist()):      # rows past each count: zero, the garbage overwritten
        n = max(n, 0)
        assert not gbox.region.view(B, nmax, 6)[i, n:].any() and not gsc.region.view(B, nmax)[i, n:].any()
        assert not glab.region.view(B, nmax * 2)[i, 2 * n:].any()
    if case == "limit":
        assert ref.counts.cpu().tolist()[0] == -16385


@pytest.mark.parametrize("n", [1, 65, 16384])
def test_nms_entry_inside_guards(gpu, n):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    b, s, c = nms_case(n, 3, 4000 + n)
    s = s[np.random.default_rng(n).integers(0, n, n)]          # repeated scores: ties
    bt, st, ct = torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu), torch.from_numpy(c).to(gpu)
    want = ops.aligned_3d_nms(bt, st, ct, .25)
    wsb = int(lib.mvsdet_detect_workspace_bytes(1, 0, n))
    gws, gout, gcnt = Guarded(wsb // 4, gpu), Guarded(2 * n, gpu), Guarded(1, gpu)
    ok(lib.mvsdet_aligned_3d_nms_f32(_lib.ptr(bt), _lib.ptr(st), _lib.ptr(ct), n, .25, gout.ptr(), gcnt.ptr(), gws.ptr(), wsb, None))
    assert gws.guards_intact() and gout.guards_intact() and gcnt.guards_intact()
    k = int(gcnt.region[0])
    assert k == len(want) and torch.equal(gout.region.view(torch.int64)[:k], want)
    assert np.array_equal(want.cpu().numpy(), nms_restated(b, s, c, .25))
