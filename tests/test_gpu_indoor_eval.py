"""Indoor mAP / recall on the device (csrc/evalmap.hip through mvsdet_amd.evaluation.IndoorEvaluator and ops.eval_*) against what the
reference's own indoor_eval returned on G21 (tests/golden/make_goldens_g21.py) and the NumPy restatement
(tests/indoor_eval_restated.py): true-positive flags bit for bit, AP within 2**-24 (float64 sums in another order, rounded to
float32), recall and counts equal; the device IoU against float64 geometry; planted decisions of the walk; orders of equal, NaN
and infinite scores; more records than one sort block and one scan chunk; overflow and the heads' negative count between guards;
two streams and two evaluators at once."""
import logging

import numpy as np
import pytest
import torch

import indoor_eval_cases as C
import indoor_eval_restated as R
from canvas import Guarded

pytestmark = pytest.mark.gpu
AP_TOL = 2.0 ** -24
IOU_TOL = 1e-5      # what tests/test_gpu_detect_arkit.py allows the device IoU against exact geometry
THR = (0.25, 0.5)
F = np.float32


def annos(scenes):
    dets = [dict(bboxes_3d=torch.from_numpy(np.ascontiguousarray(s["boxes"], F).reshape(-1, 7)),
                 scores_3d=torch.from_numpy(np.ascontiguousarray(s["scores"], F)),
                 labels_3d=torch.from_numpy(np.ascontiguousarray(s["labels"], np.int64))) for s in scenes]
    gts = [dict(gt_bboxes_3d=torch.from_numpy(np.ascontiguousarray(s["gt_boxes"], F).reshape(-1, 7)),
                gt_labels_3d=np.ascontiguousarray(s["gt_labels"], np.int64)) for s in scenes]
    return dets, gts


def scene(boxes, scores, labels, gt_boxes, gt_labels):
    return dict(boxes=np.array(boxes, F).reshape(-1, 7), scores=np.array(scores, F), labels=np.array(labels, np.int64),
                gt_boxes=np.array(gt_boxes, F).reshape(-1, 7), gt_labels=np.array(gt_labels, np.int64))


def evaluate(gpu, scenes, n_labels, per_scene=False, thr=THR, label2cat=None, capacity=None, gt_capacity=None):
    from mvsdet_amd.evaluation import IndoorEvaluator
    nd, ng = sum(len(s["scores"]) for s in scenes), sum(len(s["gt_labels"]) for s in scenes)
    nmax = max(len(s["scores"]) for s in scenes)
    ev = IndoorEvaluator(n_labels, thr, capacity=capacity or max(nd, nmax * len(scenes), 1), gt_capacity=gt_capacity or max(ng, 1),
                         device=gpu, label2cat=label2cat)
    dets, gts = annos(scenes)
    if per_scene:
        for d, g in zip(dets, gts):
            ev.update([d], [g])
    else:
        ev.update(dets, gts)
    return ev, ev.compute()


def detail(ev):
    """{label: (feeding index of its records in visiting order, tp (T,nd) bool)} from the device outputs."""
    res = ev.last_result
    ndet, order, tp = res.ndet.cpu().numpy(), res.order.cpu().numpy(), res.tp.cpu().numpy().astype(bool)
    ends = np.cumsum(ndet)
    return {lab: (order[e - n:e], tp[:, e - n:e]) for lab, (n, e) in enumerate(zip(ndet, ends)) if n}


def flags_by_record(ev):
    """tp (T, records) in FEEDING order."""
    res = ev.last_result
    n = int(res.info[0])
    order, tp = res.order.cpu().numpy()[:n], res.tp.cpu().numpy()[:, :n].astype(bool)
    out = np.zeros_like(tp)
    out[:, order] = tp
    return out


def same_dict(a, b, tol=0.0):
    return list(a) == list(b) and all(C.same_or_both_nan(a[k], b[k], tol) for k in a)


# ------------------------------------------------------------------------------------------------ G21
@pytest.mark.parametrize("case", C.CASES)
def test_g21_through_the_evaluator(gpu, case):
    g, scenes, cat = C.golden(), C.scenes_of(case), C.label2cat_of(case)
    order = [int(l) for l in g[f"{case}_label_order"]]
    want, rest = C.ret_dict_of(case), C.restated(case)
    results = []
    for per_scene in (False, True):
        ev, ret = evaluate(gpu, scenes, len(cat), per_scene, label2cat=cat)
        det, res = detail(ev), ev.last_result
        ap, rec = res.ap.cpu().numpy(), res.recall.cpu().numpy()
        npos, ndet = res.npos.cpu().numpy(), res.ndet.cpu().numpy()
        compared = 0
        for k, lab in enumerate(order):
            assert npos[lab] == rest[lab]["npos"] and ndet[lab] == rest[lab]["ndet"]
            for t in range(len(THR)):
                if ndet[lab] == 0:
                    assert ap[t, lab] == 0 and rec[t, lab] == 0
                    continue
                assert np.array_equal(det[lab][0], rest[lab]["index"]), (lab, "visiting order")
                assert np.array_equal(det[lab][1][t], C.reference_flags(case, t, lab)), (lab, t, "flags")
                assert C.same_or_both_nan(float(ap[t, lab]), float(g[f"{case}_ap"][t, k]), AP_TOL), (lab, t, ap[t, lab])
                assert C.same_or_both_nan(float(rec[t, lab]), float(g[f"{case}_recall_{t}_{lab}"][-1])), (lab, t)
                compared += ndet[lab]
        assert compared == 2 * int(g[f"{case}_counts"].sum())     # no detection is left out
        assert list(ret) == list(want)
        for key in want:
            # per-label AP: one float32 rounding of sums that agree far below it; the means: that, through np.mean in float32
            tol = 0.0 if "_rec_" in key or key.startswith("mAR") else AP_TOL if "_AP_" in key and not key.startswith("mAP") else 2 * AP_TOL
            assert C.same_or_both_nan(ret[key], want[key], tol), (key, ret[key], want[key])
        results.append((ret, res.tp.cpu().numpy()[:, :int(res.info[0])], res.order.cpu().numpy()[:int(res.info[0])]))
    assert same_dict(results[0][0], results[1][0]), "one update and one update per scene differ"
    assert np.array_equal(results[0][1], results[1][1]) and np.array_equal(results[0][2], results[1][2])
    assert np.isnan(want["mAP_0.25"]) == (case == "arkit")


@pytest.mark.parametrize("case", C.CASES)
def test_device_iou_against_float64_geometry(gpu, case):
    from mvsdet_amd import ops
    worst, pairs = 0.0, 0
    for s in C.scenes_of(case):
        if len(s["scores"]) == 0 or len(s["gt_labels"]) == 0:
            continue
        got = ops.eval_iou(torch.from_numpy(s["boxes"]).to(gpu), torch.from_numpy(s["gt_boxes"]).to(gpu)).cpu().numpy()
        want = R.iou3d(s["boxes"], s["gt_boxes"])
        worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
        pairs += got.size
    print(f"device IoU against float64 geometry, G21 {case}: max |difference| {worst:.3e} over {pairs} pairs (bar {IOU_TOL})")
    assert pairs > 1000 and worst <= IOU_TOL


# ------------------------------------------------------------------------------------------------ planted decisions
def head_prediction(gpu, rows, scores, labels):
    """A HeadPrediction of one scene from gravity-centred rows (n, 6 | 7)."""
    from mvsdet_amd import ops
    b = torch.tensor(rows, dtype=torch.float32, device=gpu).unsqueeze(0)
    return ops.HeadPrediction(b, torch.tensor([scores], dtype=torch.float32, device=gpu),
                              torch.tensor([labels], dtype=torch.int64, device=gpu),
                              torch.tensor([len(scores)], dtype=torch.int32, device=gpu))


def padded_gt(gpu, rows, labels):
    """The tuple of head.pad_ground_truth (6 values a box) or pad_ground_truth_rotated (7) for one scene."""
    b = torch.tensor(rows, dtype=torch.float32, device=gpu).unsqueeze(0)
    vol = b[..., 3] * b[..., 4] * b[..., 5]
    lab = torch.tensor([labels], dtype=torch.int64, device=gpu)
    cnt = torch.tensor([len(labels)], dtype=torch.int32, device=gpu)
    if b.shape[-1] == 6:
        return b, vol, lab, cnt
    return b, torch.stack((torch.cos(b[..., 6]), torch.sin(b[..., 6])), dim=-1), vol, lab, cnt


@pytest.mark.parametrize("rotated", [False, True])
def test_planted_exact_ious_at_the_thresholds(gpu, rotated):
    """Gravity-centred rows through the HeadPrediction route.  A unit cube inside a 1 x 2 x 2 box: IoU exactly 0.25, NOT above
    0.25 -> false positive at 0.25.  A unit cube inside a 1 x 1 x 2 box: exactly 0.5 -> true positive at 0.25, false at 0.5.
    Rotated route: the detections carry yaw = float32(pi / 2), the ground truth yaw 0."""
    from mvsdet_amd import ops
    from mvsdet_amd.evaluation import IndoorEvaluator
    yaw = [float(F(np.pi / 2))] if rotated else []
    zero = [0.0] if rotated else []
    dets = [[0, 0, 0.5, 1, 1, 1] + yaw, [10, 0, 0.5, 1, 1, 1] + yaw]
    gts = [[0, 0.5, 1.0, 1, 2, 2] + zero, [10, 0, 1.0, 1, 1, 2] + zero]
    ev = IndoorEvaluator(3, THR, capacity=8, gt_capacity=8, device=gpu)
    ev.update(head_prediction(gpu, dets, [0.9, 0.8], [1, 2]), padded_gt(gpu, gts, [1, 2]))
    ret = ev.compute()
    assert flags_by_record(ev).tolist() == [[False, True], [False, False]]
    assert ret["1_AP_0.25"] == 0.0 and ret["2_AP_0.25"] == 1.0 and ret["2_AP_0.50"] == 0.0 and ret["2_rec_0.25"] == 1.0
    bottom = lambda rows: [[r[0], r[1], r[2] - r[5] / 2] + r[3:6] + [r[6] if rotated else 0.0] for r in rows]  # noqa: E731
    iou = ops.eval_iou(torch.tensor(bottom(dets), device=gpu), torch.tensor(bottom(gts), device=gpu)).cpu().numpy()
    assert iou[0, 0] == F(0.25) and iou[1, 1] == F(0.5) and iou[0, 1] == 0 and iou[1, 0] == 0


CUBE = [0, 0, 0, 1, 1, 1, 0]


def shifted(dx=0.0, dz=0.0):
    return [dx, 0, dz, 1, 1, 1, 0]


def test_twin_boxes_the_first_index_is_claimed_and_the_twin_is_not_taken(gpu):
    sc = [scene([CUBE, CUBE], [0.9, 0.8], [0, 0], [CUBE, CUBE], [0, 0])]
    ev, ret = evaluate(gpu, sc, 1)
    assert flags_by_record(ev).tolist() == [[True, False], [True, False]]
    assert ret["0_rec_0.25"] == 0.5 and ret["0_AP_0.25"] == 0.5
    slot = R.match(sc)[0]
    assert [r[4] for r in slot] == [0, 0]


def test_best_box_taken_second_best_free_is_a_false_positive(gpu):
    """The second detection overlaps box 0 by 2/3 and box 1 by 3/7 > 0.25; box 0 is taken, box 1 free: false positive."""
    sc = [scene([CUBE, shifted(0.2)], [0.9, 0.8], [0, 0], [CUBE, shifted(0.6)], [0, 0])]
    ev, ret = evaluate(gpu, sc, 1)
    assert flags_by_record(ev).tolist() == [[True, False], [True, False]]
    assert ret["0_rec_0.25"] == 0.5
    assert np.array_equal(flags_by_record(ev), np.stack([R.evaluate(sc, THR)[0]["tp"][t] for t in range(2)]))


def test_two_detections_on_one_box_each_threshold_has_its_own_claim(gpu):
    """IoU 1/3 at the higher score, 0.6 at the lower: at 0.25 the first is the true positive, at 0.5 the second."""
    sc = [scene([shifted(dz=0.5), shifted(dz=0.25)], [0.9, 0.8], [0, 0], [CUBE], [0])]
    ev, ret = evaluate(gpu, sc, 1)
    assert flags_by_record(ev).tolist() == [[True, False], [False, True]]
    assert ret["0_AP_0.25"] == 1.0 and ret["0_AP_0.50"] == 0.5 and ret["0_rec_0.50"] == 1.0


def test_equal_scores_are_visited_by_scene_then_row(gpu):
    """Three scenes, one score: the visiting order is the feeding order, and of two equal detections on one box row 0 is the true
    positive."""
    sc = [scene([CUBE, CUBE], [0.5, 0.5], [0, 0], [CUBE], [0]),
          scene([CUBE], [0.5], [0], [CUBE], [0]),
          scene([CUBE, CUBE, CUBE], [0.5, 0.5, 0.5], [0, 0, 0], [CUBE], [0])]
    for per_scene in (False, True):
        ev, ret = evaluate(gpu, sc, 1, per_scene)
        assert detail(ev)[0][0].tolist() == [0, 1, 2, 3, 4, 5]
        assert flags_by_record(ev)[0].tolist() == [True, False, True, True, False, False]
        # precision 1, 1/2, 2/3, 3/4, 3/5, 3/6 -> envelope 1, 3/4, 3/4
        assert abs(ret["0_AP_0.25"] - (1 + 0.75 + 0.75) / 3) <= AP_TOL


def test_nan_scores_last_infinite_scores_ordered_zero_signs_equal(gpu):
    nan, inf = float("nan"), float("inf")
    sc = [scene([CUBE] * 5, [nan, inf, -inf, 0.5, 0.0], [0] * 5, [CUBE], [0]),
          scene([CUBE] * 2, [0.5, -0.0], [0] * 2, [CUBE], [0])]
    ev, _ = evaluate(gpu, sc, 1)
    got = detail(ev)[0][0].tolist()
    assert got == [1, 3, 5, 4, 6, 2, 0]
    scores = np.concatenate([s["scores"] for s in sc])
    assert got == R.visiting_order(scores, [0] * 5 + [1] * 2, [0, 1, 2, 3, 4, 0, 1]).tolist()
    assert flags_by_record(ev)[0].tolist() == [False, True, False, False, False, True, False]


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("seed, counts, n_gt", [(2, (70, 0, 130), 5), (1, (125,) * 40, 6), (3, (300, 0, 2100), 7)],
                         ids=["70-0-130", "5000", "300-0-2100"])
def test_one_label_over_block_and_chunk_edges_against_the_restatement(gpu, seed, counts, n_gt):
    """One label: 200 records (inside one sort block of 2048 and one scan chunk of 256), 5 000 (three sort blocks merged across
    blocks, twenty scan chunks) and 2 400 with an empty scene between (a sort size of 4096 = two blocks)."""
    sc = C.random_scenes(seed, counts, n_gt)
    assert C.margins_ok(sc, THR)
    want = R.evaluate(sc, THR)[0]
    for per_scene in (False, True) if sum(counts) < 1000 else (False,):
        ev, ret = evaluate(gpu, sc, 1, per_scene)
        idx, tp = detail(ev)[0]
        assert np.array_equal(idx, want["index"]) and np.array_equal(tp, want["tp"])
        res = ev.last_result
        for t in range(2):
            assert abs(float(res.ap[t, 0]) - float(want["ap"][t])) <= AP_TOL
            assert float(res.recall[t, 0]) == want["recall"][t][-1]
        assert int(res.npos[0]) == want["npos"] == n_gt * len(counts) and int(res.ndet[0]) == sum(counts)
        assert same_dict(ret, R.indoor_eval(sc, THR, {0: "0"}), AP_TOL)


def test_several_labels_in_one_sort(gpu):
    """Four labels over 600 records: segments that begin and end inside scan chunks."""
    sc = C.random_scenes(5, (150,) * 4, 8, n_labels=4)
    assert C.margins_ok(sc, THR)
    want = R.evaluate(sc, THR)
    ev, ret = evaluate(gpu, sc, 4)
    det = detail(ev)
    for lab in want:
        assert np.array_equal(det[lab][0], want[lab]["index"]) and np.array_equal(det[lab][1], want[lab]["tp"]), lab
    assert same_dict(ret, R.indoor_eval(sc, THR, {i: str(i) for i in range(4)}), 2 * AP_TOL)


# ------------------------------------------------------------------------------------------------ limits between guards
def guarded_state(gpu, n_labels, capacity, gt_capacity):
    from mvsdet_amd import _lib, ops
    lib = _lib.load()
    sb = int(lib.mvsdet_eval_state_bytes(n_labels, capacity, gt_capacity))
    wb = int(lib.mvsdet_eval_workspace_bytes(n_labels, capacity, gt_capacity, 2))
    gs, gw = Guarded(sb // 4, gpu), Guarded(wb // 4, gpu)
    assert sb % 4 == 0 and wb % 4 == 0
    st = ops.EvalState(gs.region.view(torch.uint8), gw.region.view(torch.uint8), n_labels, capacity, gt_capacity, 2)
    ops.eval_reset(st)
    return st, gs, gw


@pytest.mark.parametrize("what", ["records", "slots", "negative count", "fits"])
def test_overflow_and_negative_count_raise_at_compute_and_write_nothing_outside(gpu, what):
    from mvsdet_amd.evaluation import IndoorEvaluator
    sc = C.random_scenes(7, (9, 8), 4)
    cap, gcap = (16, 8) if what == "records" else (17, 7) if what == "slots" else (17, 8)
    st, gs, gw = guarded_state(gpu, 1, cap, gcap)
    ev = IndoorEvaluator(1, THR, capacity=cap, gt_capacity=gcap, device=gpu)
    ev._st = st
    dets, gts = annos(sc)
    ev.update(dets[:1], gts[:1])
    before = gs.region.clone()
    if what == "negative count":
        from mvsdet_amd import ops
        pred = ops.HeadPrediction(torch.zeros((1, 4, 6), device=gpu), torch.zeros((1, 4), device=gpu),
                                  torch.zeros((1, 4), dtype=torch.int64, device=gpu), torch.tensor([-20000], dtype=torch.int32, device=gpu))
        ev.update(pred, padded_gt(gpu, [CUBE[:6]], [0]))
    else:
        ev.update(dets[1:], gts[1:])
    if what == "fits":
        ret = ev.compute()
        assert same_dict(ret, R.indoor_eval(sc, THR, {0: "0"}), AP_TOL)
    else:
        with pytest.raises(RuntimeError, match={"records": "capacity", "slots": "gt_capacity", "negative count": "negative count"}[what]):
            ev.compute()
        # the refused batch wrote the flag and nothing else
        after = gs.region.clone()
        after[2] = before[2]
        assert torch.equal(after, before) and int(gs.region[2]) != 0
    torch.cuda.synchronize()
    assert gs.guards_intact() and gw.guards_intact()


# ------------------------------------------------------------------------------------------------ streams, two evaluators
def test_two_streams_and_two_evaluators_give_the_same_bits(gpu):
    from mvsdet_amd.evaluation import IndoorEvaluator
    a, b = C.scenes_of("scannet"), C.scenes_of("arkit")
    ref = []
    for scenes, n in ((a, 18), (b, 17)):
        ev, ret = evaluate(gpu, scenes, n)
        ref.append((ret, ev.last_result.tp.cpu().numpy(), ev.last_result.order.cpu().numpy()))
    evs = [IndoorEvaluator(n, THR, capacity=1024, gt_capacity=128, device=gpu) for n in (18, 17)]
    fed = [annos(a), annos(b)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    for s in range(12):                       # interleaved: one scene of each evaluator on its own stream
        for ev, (dets, gts), stream in zip(evs, fed, streams):
            with torch.cuda.stream(stream):
                ev.update(dets[s:s + 1], gts[s:s + 1])
    got = []
    for ev, stream in zip(evs, streams):
        with torch.cuda.stream(stream):
            ret = ev.compute()
            n = int(ev.last_result.info[0])
            got.append((ret, ev.last_result.tp.cpu().numpy()[:, :n], ev.last_result.order.cpu().numpy()[:n]))
    torch.cuda.synchronize()
    for (r0, tp0, o0), (r1, tp1, o1) in zip(ref, got):
        n = len(o1)
        assert same_dict(r0, r1) and np.array_equal(tp0[:, :n], tp1) and np.array_equal(o0[:n], o1)


# ------------------------------------------------------------------------------------------------ the function and the patch
def test_indoor_eval_function_reset_and_reference_patch(gpu, caplog):
    import types

    from mvsdet_amd import evaluation, integration
    case = "scannet"
    scenes, cat = C.scenes_of(case), C.label2cat_of(case)
    dets, gts = annos(scenes)

    class Boxes:                               # what the reference hands over: a box object with .tensor and convert_to
        def __init__(self, t):
            self.tensor = t

        def convert_to(self, mode):
            return self

    dt = [dict(d, bboxes_3d=Boxes(d["bboxes_3d"])) for d in dets]
    gt = [dict(g, gt_bboxes_3d=Boxes(g["gt_bboxes_3d"])) for g in gts]
    ev, want = evaluate(gpu, scenes, len(cat), label2cat=cat)
    with caplog.at_level(logging.INFO, logger="mvsdet_amd.evaluation"):
        got = evaluation.indoor_eval(gt, dt, list(THR), cat, device=gpu)
    assert same_dict(got, want) and "Overall" in caplog.text and "AP_0.25" in caplog.text
    mod = types.SimpleNamespace(indoor_eval=None)
    saved = integration.patch_reference_indoor_eval(mod, device=gpu)
    assert same_dict(mod.indoor_eval(gt, dt, list(THR), cat), want)
    integration.unpatch_reference_indoor_eval(mod, saved)
    # reset: the same evaluator, fed again, gives the same dict; without reset the set would be doubled
    ev.reset()
    ev.update(dets, gts)
    assert same_dict(ev.compute(), want)


def test_update_makes_no_host_sync_on_either_route(gpu):
    """HeadPrediction + head.pad_ground_truth (stand-in ground-truth instances: what the reference's data samples carry) and the
    list route, under torch's synchronisation check; compute() afterwards sees both batches."""
    import types

    from mvsdet_amd import head
    from mvsdet_amd.evaluation import IndoorEvaluator
    t = torch.tensor([[0, 0, 0, 1, 1, 1], [5, 0, 0, 1, 1, 2]], dtype=torch.float32)      # bottom-centred, as the box classes hold them
    boxes = types.SimpleNamespace(tensor=t, gravity_center=t[:, :3] + t[:, 3:6] * torch.tensor([0, 0, 0.5]), volume=t[:, 3:6].prod(1))
    inst = [types.SimpleNamespace(bboxes_3d=boxes, labels_3d=torch.tensor([0, 1]))]
    pred = head_prediction(gpu, [[0, 0, 0.5, 1, 1, 1], [5, 0, 0.5, 1, 1, 1]], [0.9, 0.8], [0, 1])
    dets, gts = annos([scene([CUBE], [0.7], [0], [CUBE], [0])])
    ev = IndoorEvaluator(2, THR, capacity=16, gt_capacity=8, device=gpu)
    ev.update(pred, head.pad_ground_truth(inst, gpu))      # warm: library load, allocator, pinned memory
    ev.update(dets, gts)
    ev.reset()
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.update(pred, head.pad_ground_truth(inst, gpu))
        ev.update(dets, gts)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ret = ev.compute()
    # label 0: cube on cube twice (two scenes, both true positives); label 1: a unit cube inside the 1 x 1 x 2 box, IoU exactly 0.5
    assert flags_by_record(ev).tolist() == [[True, True, True], [True, False, True]]
    assert ret["0_AP_0.50"] == 1.0 and ret["1_AP_0.25"] == 1.0 and ret["1_AP_0.50"] == 0.0 and ret["mAR_0.25"] == 1.0
