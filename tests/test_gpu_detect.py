"""Detection post-processing on the GPU (csrc/detect.hip): G15 (the reference's predict_by_feat on CPU, tests/golden/
make_goldens_g15.py) through NerfDetHeadConvs.predict_by_feat, the standalone NMS against the NumPy restatement of
test_detect_host.py, no host syncs inside ops.head_predict, MVSDetHotPath's opt-in detections, determinism."""
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from test_detect_host import nms_case, nms_restated

pytestmark = pytest.mark.gpu
sys.path.insert(0, GOLDEN)
import make_goldens_g15 as g15  # noqa: E402  (its inputs are LCG-made: no reference tree needed)

CFG = dict(score_thr=0.01, iou_thr=0.25)


def _case(name, gpu):
    gold = load_golden("g15_detect")
    kinds = list(gold[f"{name}:kinds"])
    seeds = [int(v) for v in gold[f"{name}:seeds"]]
    c, r, k, v, origins = g15.batch_inputs(kinds, seeds)
    dev = lambda ts: [t.to(gpu) for t in ts]  # noqa: E731
    metas = [{"lidar2img": {"origin": o.numpy().astype(np.float32)}} for o in origins]
    return gold, dev(c), dev(r), dev(k), v.to(gpu), metas, int(gold[f"{name}:nms_pre"])


def _head(nms_pre):
    from mvsdet_amd.head import NerfDetHeadConvs
    return NerfDetHeadConvs(test_cfg=types.SimpleNamespace(nms_pre=nms_pre, **CFG))


@pytest.mark.parametrize("name", list(g15.CASES))
def test_g15_predict_by_feat(gpu, name):
    gold, c, r, k, v, metas, nms_pre = _case(name, gpu)
    res = _head(nms_pre).predict_by_feat(c, r, k, v, metas)
    assert len(res) == len(metas)
    for i, rs in enumerate(res):
        boxes, scores, labels = gold[f"{name}:{i}:boxes"], gold[f"{name}:{i}:scores"], gold[f"{name}:{i}:labels"]
        assert len(rs) == len(scores), f"{name} scene {i}: {len(rs)} boxes, the reference {len(scores)}"
        assert np.array_equal(rs.labels_3d.cpu().numpy(), labels), f"{name} scene {i}: labels / pick order"
        got = rs.bboxes_3d.cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), boxes.view(np.uint32)), f"{name} scene {i}: boxes"
        np.testing.assert_allclose(rs.scores_3d.cpu().numpy(), scores, rtol=1e-6, atol=0)


def test_g15_box_type_3d_is_applied(gpu):
    gold, c, r, k, v, metas, nms_pre = _case("planted", gpu)
    seen = {}

    def box_type(t, box_dim, with_yaw, origin):
        seen.update(box_dim=box_dim, with_yaw=with_yaw, origin=origin)
        return ("boxed", t)

    res = _head(nms_pre).predict_by_feat(c, r, k, v, [dict(metas[0], box_type_3d=box_type)])
    assert res[0].bboxes_3d[0] == "boxed" and seen == dict(box_dim=6, with_yaw=False, origin=(.5, .5, .5))
    assert np.array_equal(res[0].bboxes_3d[1].cpu().numpy(), gold["planted:0:boxes"])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129, 2400, 16384])
@pytest.mark.parametrize("n_classes", [1, 18])
def test_aligned_3d_nms_equals_restatement(gpu, n, n_classes):
    from mvsdet_amd import ops
    b, s, c = nms_case(n, n_classes, 1000 + n + n_classes)
    bt, st, ct = torch.from_numpy(b).to(gpu), torch.from_numpy(s).to(gpu), torch.from_numpy(c).to(gpu)
    for thresh in (0.0, 0.25, 1.0):
        got = ops.aligned_3d_nms(bt, st, ct, thresh)
        assert got.dtype == torch.int64 and got.is_cuda
        want = nms_restated(b, s, c, thresh)
        assert np.array_equal(got.cpu().numpy(), want), (n, n_classes, thresh, len(got), len(want))


def test_aligned_3d_nms_nan_suppresses_across_classes(gpu):
    from mvsdet_amd import ops
    inf = float("inf")
    boxes = torch.tensor([[0, 0, 0, 2, 1, 1], [1, 0, 0, 3, 1, 1], [0, 0, 0, inf, 1, 1], [0, 0, 0, inf, 1, 1],
                          [7, 7, 7, 7, 8, 8], [7, 7, 7, 7, 8, 8]], device=gpu)
    scores = torch.tensor([.9, .8, .7, .6, .5, .4], device=gpu)
    classes = torch.tensor([0, 0, 1, 0, 2, 3], device=gpu)
    assert ops.aligned_3d_nms(boxes, scores, classes, .25).tolist() == [0, 2, 4]
    assert ops.aligned_3d_nms(boxes, scores, classes, .5).tolist() == [0, 1, 2, 4]


def test_head_predict_has_no_host_sync(gpu):
    from mvsdet_amd import ops
    _, c, r, k, v, metas, nms_pre = _case("random", gpu)
    origins = [torch.from_numpy(m["lidar2img"]["origin"]) for m in metas]
    ops.head_predict(c, r, k, v, origins, nms_pre, 0.01, 0.25)   # warm: library load, allocator
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        pred = ops.head_predict(c, r, k, v, origins, nms_pre, 0.01, 0.25)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert int(pred.counts[0]) > 0


def test_head_predict_is_deterministic(gpu):
    from mvsdet_amd import ops
    _, c, r, k, v, metas, nms_pre = _case("batch2", gpu)
    origins = [torch.from_numpy(m["lidar2img"]["origin"]) for m in metas]
    a = ops.head_predict(c, r, k, v, origins, nms_pre, 0.01, 0.25)
    b = ops.head_predict(c, r, k, v, origins, nms_pre, 0.01, 0.25)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert torch.equal(a.boxes[:, :, 0] == 0, b.boxes[:, :, 0] == 0)


def _hotpath(gpu, maps, test_cfg):
    from mvsdet_amd.hotpath import MVSDetHotPath
    return MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12, topk=3, neck_3d=lambda vol: [vol],
                         bbox_head=lambda levels: maps(levels[0].shape[0]), test_cfg=test_cfg)


@pytest.mark.parametrize("overlap", [False, True])
def test_hotpath_detections(gpu, overlap):
    from mvsdet_amd import synthetic
    from mvsdet_amd.head import NerfDetHeadConvs
    _, c, r, k, _, _, _ = _case("random", gpu)
    cfg = types.SimpleNamespace(nms_pre=1000, **CFG)

    def maps(B):   # the G15 random maps stand in for the neck and head, scene-independent
        rep = lambda ts: [t.expand(B, *t.shape[1:]).contiguous() for t in ts]  # noqa: E731
        return rep(c), rep(r), rep(k)

    hw, N = (60, 80), 5
    metas = [synthetic.make_img_meta(N, hw, seed=300 + i) for i in range(2)]
    feats = [synthetic.make_features(N, 32, hw, seed=300 + i).to(gpu) for i in range(2)]
    logits = [synthetic.make_cost_logits(N, 12, hw, seed=300 + i).to(gpu) for i in range(2)]
    head = NerfDetHeadConvs(test_cfg=cfg)
    plain = _hotpath(gpu, maps, None)
    plain.overlap_detector = overlap
    hp = _hotpath(gpu, maps, cfg)
    hp.overlap_detector = overlap
    with torch.no_grad():
        assert "detections" not in plain.forward_scene(feats[0], metas[0], cost_logits=logits[0])
        out = hp.forward_scene(feats[0], metas[0], cost_logits=logits[0])
        batch = hp.forward_scenes(feats, metas, cost_logits=logits)
    det = out["detections"]
    want = head.predict_by_feat(*out["head"], out["valid"].unsqueeze(0).float(), [metas[0]])
    assert int((out["valid"] > 0).sum()) > 0
    _same_detections(det, want)
    bdet = batch["detections"]
    want = head.predict_by_feat(*batch["head"], batch["valid"].float(), metas)
    _same_detections(bdet, want)


def _same_detections(det, want):
    counts = det.counts.cpu().tolist()
    assert counts == [len(w) for w in want]
    for i, w in enumerate(want):
        n = counts[i]
        assert torch.equal(det.boxes[i, :n], w.bboxes_3d) and torch.equal(det.scores[i, :n], w.scores_3d)
        assert torch.equal(det.labels[i, :n], w.labels_3d)
        assert not det.boxes[i, n:].any() and not det.scores[i, n:].any() and not det.labels[i, n:].any()
