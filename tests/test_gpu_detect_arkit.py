"""The ARKit head's rotated detection post-processing on the GPU (csrc/detect.hip): G16 (the reference's ImVoxelHead_ARKit
predict_by_feat on CPU, tests/golden/make_goldens_g16.py) through NerfDetHeadConvs(arkit_head=True).predict_by_feat; ops.nms3d and
ops.bev_iou_rotated against the NumPy restatement of mmcv's nms3d (tests/nms3d_restated.py) and exact geometry; overflow, ties,
NaN logits, determinism, no host sync, guard canvases, MVSDetHotPath's ARKit detections and the reference patch."""
import ctypes
import math
import sys
import types

import numpy as np
import pytest
import torch

import nms3d_restated as R
from conftest import GOLDEN, load_golden
from test_gpu_detect_edges import Guarded, ok

pytestmark = pytest.mark.gpu
sys.path.insert(0, GOLDEN)
import make_goldens_g16 as g16  # noqa: E402  (its inputs are LCG-made: no reference tree needed)

CFG = dict(score_thr=0.01, iou_thr=0.25)
INF, NAN = float("inf"), float("nan")


def _case(name, gpu):
    gold = load_golden("g16_detect_arkit")
    kinds = list(gold[f"{name}:kinds"])
    seeds = [int(v) for v in gold[f"{name}:seeds"]]
    c, r, k, v, origins = g16.batch_inputs(kinds, seeds)
    dev = lambda ts: [t.to(gpu) for t in ts]  # noqa: E731
    metas = [{"lidar2img": {"origin": o.numpy().astype(np.float32)}} for o in origins]
    return gold, dev(c), dev(r), dev(k), v.to(gpu), metas, int(gold[f"{name}:nms_pre"])


def _head(nms_pre):
    from mvsdet_amd.head import NerfDetHeadConvs
    return NerfDetHeadConvs(17, 3, 128, 7, arkit_head=True, test_cfg=types.SimpleNamespace(nms_pre=nms_pre, **CFG))


def _origins(metas):
    return [torch.from_numpy(m["lidar2img"]["origin"]) for m in metas]


@pytest.mark.parametrize("name", list(g16.CASES))
def test_g16_predict_by_feat(gpu, name):
    gold, c, r, k, v, metas, nms_pre = _case(name, gpu)
    res = _head(nms_pre).predict_by_feat(c, r, k, v, metas)
    assert len(res) == len(metas)
    for i, rs in enumerate(res):
        boxes, scores, labels = gold[f"{name}:{i}:boxes"], gold[f"{name}:{i}:scores"], gold[f"{name}:{i}:labels"]
        assert len(rs) == len(scores), f"{name} scene {i}: {len(rs)} boxes, the reference {len(scores)}"
        assert rs.labels_3d.dtype == torch.int64
        assert np.array_equal(rs.labels_3d.cpu().numpy(), labels.astype(np.int64)), f"{name} scene {i}: labels / pick order"
        got = rs.bboxes_3d.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (len(scores), 7)
        assert np.array_equal(got[:, 3:].view(np.uint32), boxes[:, 3:].view(np.uint32)), f"{name} scene {i}: sizes / angles"
        tol = 1e-6 * np.maximum(1, np.abs(boxes[:, :3]))
        assert (np.abs(got[:, :3] - boxes[:, :3]) <= tol).all(), f"{name} scene {i}: centres"
        np.testing.assert_allclose(rs.scores_3d.cpu().numpy(), scores, rtol=1e-6, atol=0)


def test_g16_cases_are_not_trivial():
    gold = load_golden("g16_detect_arkit")
    assert len(gold["planted:0:scores"]) > 0 and len(np.unique(gold["random:0:labels"])) == 17
    assert len(gold["empty:0:scores"]) == 0 and len(gold["nms_pre_zero:0:scores"]) > 0
    assert np.abs(gold["random:0:boxes"][:, 6]).max() > math.pi


def test_g16_box_type_3d_is_applied(gpu):
    gold, c, r, k, v, metas, nms_pre = _case("planted", gpu)
    seen = {}

    def box_type(t, box_dim, with_yaw, origin):
        seen.update(box_dim=box_dim, with_yaw=with_yaw, origin=origin)
        return ("boxed", t)

    res = _head(nms_pre).predict_by_feat(c, r, k, v, [dict(metas[0], box_type_3d=box_type)])
    assert res[0].bboxes_3d[0] == "boxed" and seen == dict(box_dim=7, with_yaw=True, origin=(.5, .5, .5))
    assert res[0].bboxes_3d[1].shape == gold["planted:0:boxes"].shape


# ------------------------------------------------------------------------------------------------ standalone nms3d
def screened_case(n, seed, thresholds):
    """n boxes at a constant density with distinct scores, reseeded until no pair's restated IoU lies within 1e-4 of a threshold
    (where an ulp of the device's sin / cos could tip a decision)."""
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        spread = 4.0 * math.sqrt(max(n, 1) / 64)
        b = np.concatenate([rng.uniform(0, spread, (n, 2)), rng.uniform(0, 1, (n, 1)), rng.uniform(0.2, 1.2, (n, 3)),
                            rng.uniform(-4, 4, (n, 1))], 1).astype(np.float32)
        sc = ((rng.permutation(n) + 1) / np.float32(n + 1)).astype(np.float32)
        m = R.bev_iou(b, b, skip_far=True) if n else np.zeros((0, 0), np.float32)
        if not any((np.abs(m.astype(np.float64) - t) < 1e-4).any() for t in thresholds):
            return b, sc
    raise AssertionError("no screened case")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 500])
def test_nms3d_equals_restatement(gpu, n):
    from mvsdet_amd import ops
    ths = (0.1, 0.25, 0.5)
    b, s = screened_case(n, 100 + n, ths)
    bt, st = torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu)
    for t in ths:
        got = ops.nms3d(bt, st, t)
        assert got.dtype == torch.int64 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), R.nms3d(b, s, t)), (n, t)


def _hand(gpu, boxes, scores, ths=(0.25, 0.5)):
    from mvsdet_amd import ops
    b, s = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    for t in ths:
        got = ops.nms3d(torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu), t).cpu().numpy()
        assert np.array_equal(got, R.nms3d(b, s, t)), (t, got)
    return [ops.nms3d(torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu), t).tolist() for t in ths]


def test_nms3d_hand_cases(gpu):
    box = [1, 2, 0, 2, 1, 1, 0.3]
    assert _hand(gpu, [box, box], [.9, .8]) == [[0], [0]]                                   # identical: IoU 1
    sq = [0, 0, 0, 2, 2, 1, 0.4]
    assert _hand(gpu, [sq, [0, 0, 0, 2, 2, 1, 0.4 + math.pi / 2]], [.5, .9]) == [[1], [1]]  # a square turned 90 degrees
    _hand(gpu, [[0, 0, 0, 2, 1, 1, 0], [2, 0, 0, 2, 1, 1, 0], [0, 1, 0, 2, 1, 1, 0]], [.9, .8, .7])   # edge to edge
    _hand(gpu, [[0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 1, 0.2], [0, 0, 0, 1, 1, 1, 0]], [.9, .8, .7, .6])
    _hand(gpu, [[NAN, 0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, NAN], [0, 0, 0, INF, 1, 1, 0], [0, 0, 0, 1, 1, 1, 0],
                [0.1, 0, 0, 1, 1, 1, INF], [0, 0, 0, 1, 1, 1, 0.1]], [.9, .8, .7, .6, .5, .4])
    _hand(gpu, [box] * 3 + [sq], [NAN, .5, -NAN, .5])                                       # NaN scores first, ties by index
    got = _hand(gpu, [[3 * i, 0, 0, 1, 1, 1, 0.1 * i] for i in range(10)] + [box], [.5] * 11)   # equal scores: index order
    assert got[0][:10] == list(range(10))


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_nms3d_block_edges_all_suppressed(gpu, n):
    from mvsdet_amd import ops
    b = np.tile(np.array([[1, 1, 0, 1, 1, 1, 0.2]], np.float32), (n, 1))
    b[:, 0] += np.arange(n, dtype=np.float32) * np.float32(1e-3)
    s = np.linspace(1, 0.1, n).astype(np.float32)
    got = ops.nms3d(torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu), 0.25)
    assert got.tolist() == R.nms3d(b, s, 0.25).tolist() == [0]


# ------------------------------------------------------------------------------------------------ bev_iou_rotated
def test_bev_iou_equals_restatement_and_geometry(gpu):
    from mvsdet_amd import ops
    rng = np.random.default_rng(7)
    a = np.concatenate([rng.uniform(0, 3, (80, 3)), rng.uniform(0.2, 1.5, (80, 3)), rng.uniform(-7, 7, (80, 1))], 1).astype(np.float32)
    b = np.concatenate([rng.uniform(0, 3, (90, 3)), rng.uniform(0.2, 1.5, (90, 3)), rng.uniform(-7, 7, (90, 1))], 1).astype(np.float32)
    got = ops.bev_iou_rotated(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)).cpu().numpy()
    want = R.bev_iou(a, b)
    assert np.abs(got - want).max() < 1e-6
    assert (got > 0).sum() > 1000 and (got == 0).sum() > 1000   # near pairs and pairs that take the early exit
    for i in range(0, 80, 3):
        for j in range(90):
            if not R.corner_in_margin_band(a[i], b[j]):
                assert abs(float(got[i, j]) - R.exact_iou(a[i], b[j])) < 1e-5, (i, j)


def test_bev_iou_at_heading_zero_is_the_aligned_iou(gpu):
    from mvsdet_amd import ops
    rng = np.random.default_rng(8)
    a = np.concatenate([rng.uniform(0, 2, (60, 3)), rng.uniform(0.3, 1.5, (60, 3)), np.zeros((60, 1))], 1).astype(np.float32)
    got = ops.bev_iou_rotated(torch.from_numpy(a).to(gpu), torch.from_numpy(a).to(gpu)).cpu().numpy()
    a64 = a.astype(np.float64)
    lo, hi = a64[:, :2] - a64[:, 3:5] / 2, a64[:, :2] + a64[:, 3:5] / 2
    ext = np.maximum(np.minimum(hi[:, None], hi[None]) - np.maximum(lo[:, None], lo[None]), 0)
    inter = ext[..., 0] * ext[..., 1]
    area = a64[:, 3] * a64[:, 4]
    want = inter / (area[:, None] + area[None] - inter)
    # corners within the 1e-2 margin of the other box count as inside (mmcv's MARGIN): leave those pairs out
    gap = np.minimum(np.abs(lo[:, None] - lo[None]), np.abs(hi[:, None] - hi[None]))
    gap = np.minimum(gap, np.minimum(np.abs(lo[:, None] - hi[None]), np.abs(hi[:, None] - lo[None]))).min(-1)
    clean = gap > 2e-2
    assert clean.sum() > 2000 and np.abs(got - want)[clean].max() < 1e-5


# ------------------------------------------------------------------------------------------------ batches and edges
def _maps_one_level(B, size, C, cls_val, reg_val, ctr_val=5.0):
    c = [torch.full((B, 1) + size, ctr_val)]
    r = [torch.full((B, 7) + size, reg_val)]
    r[0][:, 6] = 0.3
    k = [torch.full((B, C) + size, cls_val)]
    return c, r, k, torch.ones((B, 1) + size)


def test_class_overflow_leaves_the_neighbour_alone(gpu):
    from mvsdet_amd import ops
    _, c, r, k, v, metas, _ = _case("planted", gpu)
    big = [t.repeat(2, 1, 1, 1, 1) for t in c], [t.repeat(2, 1, 1, 1, 1) for t in r], [t.repeat(2, 1, 1, 1, 1) for t in k]
    big[2][0][0, 3] = 10.0          # scene 0, class 3: every level-0 point (25 600) above score_thr
    big[0][0][0] = 10.0
    vv = v.repeat(2, 1, 1, 1, 1)
    o = _origins(metas) * 2
    pred = ops.head_predict_rotated(*big, vv, o, 0, **CFG)
    alone = ops.head_predict_rotated(c, r, k, v, o[:1], 0, **CFG)
    counts = pred.counts.cpu().tolist()
    assert counts[0] <= -25600 and counts[1] == int(alone.counts[0]) > 0
    assert not pred.boxes[0].any() and not pred.scores[0].any() and not pred.labels[0].any()
    for t, u in zip(pred, alone):
        if t.dim() > 1:
            assert torch.equal(t[1], u[0])


def test_equal_scores_go_by_level_then_voxel(gpu):
    from mvsdet_amd import ops
    sizes = ((4, 4, 1), (2, 2, 1))   # one z layer: boxes of a layer above would have the same BEV box
    c = [torch.full((1, 1) + s, 5.0, device=gpu) for s in sizes]
    r = [torch.full((1, 7) + s, 0.01, device=gpu) for s in sizes]
    k = [torch.full((1, 2) + s, 5.0, device=gpu) for s in sizes]   # every score of a class equal
    for t in r:
        t[:, 6] = 0.0
    r[1][:, 0] = -0.07    # level 1's points lie on level 0's: its 0.02 m boxes move 0.08 m along x
    r[1][:, 1] = 0.09
    o = [torch.tensor([1.0, 1.0, 0.5])]
    pred = ops.head_predict_rotated(c, r, k, torch.ones(1, 1, 4, 4, 1, device=gpu), o, 0, **CFG)
    geom = ops.detect_level_geometry(sizes, o)[0]
    pts = []
    for lvl, s in enumerate(sizes):
        g = torch.stack(torch.meshgrid([torch.arange(d) for d in s], indexing="ij")).reshape(3, -1).t().float()
        pts.append(g * geom[lvl, :3] + geom[lvl, 3:] + torch.tensor([0.08 * lvl, 0.0, 0.0]))
    pts = torch.cat(pts)
    n = len(pts)
    assert int(pred.counts[0]) == 2 * n
    assert pred.labels[0, :2 * n].tolist() == [0] * n + [1] * n
    for cl in range(2):
        assert torch.allclose(pred.boxes[0, cl * n:(cl + 1) * n, :3].cpu(), pts, atol=1e-6)


def test_nan_logits_take_topk_slots(gpu):
    from mvsdet_amd import ops
    size = (8, 8, 1)                                            # one z layer: no two points share a BEV box
    c, r, k, v = _maps_one_level(1, size, 2, -10.0, 0.01)
    k[0][0, 0].view(-1)[:] = torch.linspace(-1, 1, 64)         # distinct class-0 scores, the largest at the end
    k[0][0, 1].view(-1)[[3, 17, 40]] = NAN                      # NaN in class 1: max score NaN, class 0 still counts
    pred = ops.head_predict_rotated([t.to(gpu) for t in c], [t.to(gpu) for t in r], [t.to(gpu) for t in k], v.to(gpu),
                                    [torch.zeros(3)], 5, **CFG)
    n = int(pred.counts[0])
    assert n == 5 and pred.labels[0, :n].tolist() == [0] * 5
    geom = ops.detect_level_geometry([size], [torch.zeros(3)])[0, 0]
    g = torch.stack(torch.meshgrid([torch.arange(d) for d in size], indexing="ij")).reshape(3, -1).t().float() * geom[:3] + geom[3:]
    want = g[[63, 62, 40, 17, 3]]                               # class-0 score order: the two largest, then the NaN points'
    assert torch.allclose(pred.boxes[0, :n, :3].cpu(), want, atol=1e-6)


def test_head_predict_rotated_is_deterministic_and_sync_free(gpu):
    from mvsdet_amd import ops
    _, c, r, k, v, metas, nms_pre = _case("batch2", gpu)
    o = _origins(metas)
    a = ops.head_predict_rotated(c, r, k, v, o, nms_pre, **CFG)
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = ops.head_predict_rotated(c, r, k, v, o, nms_pre, **CFG)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert int(a.counts[1]) > 1000


def test_rotated_entries_inside_guards(gpu):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    _, c, r, k, v, metas, nms_pre = _case("batch2", gpu)
    o = _origins(metas)
    ref = ops.head_predict_rotated(c, r, k, v, o, nms_pre, **CFG)
    sizes = [tuple(t.shape[2:]) for t in c]
    B, L, C = v.shape[0], len(c), k[0].shape[1]
    points, ncap = sum(int(np.prod(s)) for s in sizes), ops.detect_candidates(sizes, nms_pre)
    nmax = C * min(ncap, ops.DETECT_MAX_CANDIDATES)
    wsb = int(lib.mvsdet_detect_rotated_workspace_bytes(B, points, ncap, C))
    gws, gbox, gsc, glab, gcnt = (Guarded(wsb // 4, gpu), Guarded(B * nmax * 7, gpu), Guarded(B * nmax, gpu),
                                  Guarded(B * nmax * 2, gpu), Guarded(B, gpu))
    geom = ops.detect_level_geometry(sizes, o).to(gpu)
    arr = ctypes.c_void_p * L
    dims = [int(d) for s in sizes for d in s]
    ok(lib.mvsdet_detect_head_rotated_f32(arr(*[t.data_ptr() for t in c]), arr(*[t.data_ptr() for t in r]),
                                          arr(*[t.data_ptr() for t in k]), (ctypes.c_int * len(dims))(*dims), _lib.ptr(v),
                                          _lib.ptr(geom), B, L, C, *v.shape[2:], nms_pre, CFG["score_thr"], CFG["iou_thr"], gbox.ptr(),
                                          gsc.ptr(), glab.ptr(), gcnt.ptr(), nmax, gws.ptr(), wsb, None))
    assert all(g.guards_intact() for g in (gws, gbox, gsc, glab, gcnt))
    assert torch.equal(gcnt.region, ref.counts)
    assert torch.equal(gbox.region.view(B, nmax, 7), ref.boxes.view(torch.int32))
    assert torch.equal(gsc.region.view(B, nmax), ref.scores.view(torch.int32))
    assert torch.equal(glab.region.view(torch.int64).view(B, nmax), ref.labels)
    # the standalone NMS and the IoU matrix
    b, s = screened_case(129, 900, (0.25,))
    bt, st = torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu)
    wsb = int(lib.mvsdet_detect_rotated_workspace_bytes(1, 0, 129, 1))
    gws, gout, gcnt, giou = Guarded(wsb // 4, gpu), Guarded(2 * 129, gpu), Guarded(1, gpu), Guarded(129 * 129, gpu)
    ok(lib.mvsdet_nms3d_f32(_lib.ptr(bt), _lib.ptr(st), 129, 0.25, gout.ptr(), gcnt.ptr(), gws.ptr(), wsb, None))
    ok(lib.mvsdet_bev_iou_rotated_f32(_lib.ptr(bt), 129, _lib.ptr(bt), 129, giou.ptr(), None))
    assert all(g.guards_intact() for g in (gws, gout, gcnt, giou))
    n = int(gcnt.region[0])
    assert gout.region.view(torch.int64)[:n].tolist() == R.nms3d(b, s, 0.25).tolist()
    assert torch.equal(giou.region.view(129, 129), ops.bev_iou_rotated(bt, bt).view(torch.int32))


# ------------------------------------------------------------------------------------------------ hot path and the reference patch
class _ArkitMaps:
    """Stands in for the neck and ARKit head: the G16 random maps, scene-independent."""
    arkit_head = True

    def __init__(self, c, r, k):
        self.maps = c, r, k

    def __call__(self, levels):
        B = levels[0].shape[0]
        return tuple([t.expand(B, *t.shape[1:]).contiguous() for t in part] for part in self.maps)


@pytest.mark.parametrize("overlap", [False, True])
def test_hotpath_arkit_detections(gpu, overlap):
    from mvsdet_amd import synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    _, c, r, k, _, _, _ = _case("random", gpu)
    cfg = types.SimpleNamespace(nms_pre=1000, **CFG)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12, topk=3, neck_3d=lambda vol: [vol],
                       bbox_head=_ArkitMaps(c, r, k), test_cfg=cfg)
    hp.overlap_detector = overlap
    hw, N = (60, 80), 5
    metas = [synthetic.make_img_meta(N, hw, seed=310 + i) for i in range(2)]
    feats = [synthetic.make_features(N, 32, hw, seed=310 + i).to(gpu) for i in range(2)]
    logits = [synthetic.make_cost_logits(N, 12, hw, seed=310 + i).to(gpu) for i in range(2)]
    head = _head(1000)
    with torch.no_grad():
        out = hp.forward_scene(feats[0], metas[0], cost_logits=logits[0])
        batch = hp.forward_scenes(feats, metas, cost_logits=logits)
    for det, maps, valid, ms in ((out["detections"], out["head"], out["valid"].unsqueeze(0), [metas[0]]),
                                 (batch["detections"], batch["head"], batch["valid"], metas)):
        want = head.predict_by_feat(*maps, valid.float(), ms)
        counts = det.counts.cpu().tolist()
        assert counts == [len(w) for w in want] and all(n > 0 for n in counts)
        assert det.boxes.shape[-1] == 7
        for i, w in enumerate(want):
            n = counts[i]
            assert torch.equal(det.boxes[i, :n], w.bboxes_3d) and torch.equal(det.scores[i, :n], w.scores_3d)
            assert torch.equal(det.labels[i, :n], w.labels_3d)
            assert not det.boxes[i, n:].any() and not det.scores[i, n:].any() and not det.labels[i, n:].any()


def test_reference_patch_runs_nms3d_on_the_gpu(gpu):
    from mvsdet_amd import integration
    mod = types.ModuleType("nerfdet_head")
    cpu_calls = []
    mod.nms3d = lambda b, s, t: cpu_calls.append(t) or g16.nms3d_stand_in(b, s, t)
    saved = integration.patch_reference_nms3d(mod)
    try:
        b, s = screened_case(300, 500, (0.25,))
        got = mod.nms3d(torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu), 0.25)
        assert got.is_cuda and got.tolist() == R.nms3d(b, s, 0.25).tolist() and cpu_calls == []
        assert mod.nms3d(torch.from_numpy(b), torch.from_numpy(s), 0.25).tolist() == got.tolist() and cpu_calls == [0.25]
    finally:
        integration.unpatch_reference_nms3d(mod, saved)
