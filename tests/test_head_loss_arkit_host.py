"""The ARKit head's training objective without a GPU: fixture G19 is self-consistent (tests/head_loss_arkit_restated.py reproduces
it: labels and chosen boxes equal, box targets bit for bit, centerness targets within 1e-4, losses and gradients within 1e-5, a
tenth of the GPU bar, which leaves room for float32 sums of up to 29200 x 17 terms taken in another order); the stand-in for
mmcv's diff_iou_rotated_3d (tests/rotated_iou_restated.py) equals the float64 clipping of tests/nms3d_restated.exact_iou and its
autograd gradient equals central differences; config.head_from_config builds the head; the refusals come before any device work."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import head_loss_arkit_restated as A
import head_loss_restated as R
import nms3d_restated as N
import rotated_iou_restated as RI

CASES = ("one", "twelve", "sixty", "no_valid", "valid_no_pos", "batch2")
NAMES = ("center_loss", "bbox_loss", "cls_loss")
SIZES = [tuple(s) for s in A.ARKIT_LEVELS]


def check_targets(gold, name, b, labels, box_index, center_t, bbox_t):
    """labels and chosen box of every point equal; box targets at assigned points bit for bit (copies of the input); centerness
    targets there within 1e-4 relative (the bar of the issue: the rotation's sum may differ in its last bit).  Returns the largest
    relative centerness deviation."""
    want = gold[f"{name}:{b}:labels"].astype(np.int64)
    assert np.array_equal(labels, want), name
    assert np.array_equal(box_index, gold[f"{name}:{b}:box_index"].astype(np.int64)), name
    assigned = np.nonzero(want >= 0)[0]
    assert np.array_equal(bbox_t[assigned].view(np.int32), gold[f"{name}:{b}:bbox_targets"].view(np.int32)), name
    ct = gold[f"{name}:{b}:center_targets"]
    if len(assigned) == 0:
        return 0.0
    rel = np.abs(center_t[assigned] - ct) / np.abs(ct)
    assert float(rel.max()) <= 1e-4, (name, float(rel.max()))
    return float(rel.max())


def check_gradients(gold, name, grads, n_levels, bar):
    """every stored element within `bar` of the map's largest absolute reference value; returns the largest deviation seen."""
    worst = 0.0
    for j, kind in enumerate(("center", "bbox", "cls")):
        for l in range(n_levels):
            g = grads[j * n_levels + l].detach().cpu().reshape(-1).numpy()
            idx, want = gold[f"{name}:grad:{kind}:{l}:index"], gold[f"{name}:grad:{kind}:{l}:values"]
            s = gold[f"{name}:grad:{kind}:{l}:sums"]
            top = float(s[2])
            dev = float(np.abs(g[idx] - want).max())
            if top == 0.0:
                assert dev == 0.0 and not g.any(), (name, kind, l)
                continue
            worst = max(worst, dev / top)
            assert dev <= bar * top, (name, kind, l, dev, top)
            assert abs(float(g.astype(np.float64).sum()) - s[0]) <= 10 * bar * max(s[1], top), (name, kind, l)
    return worst


def restated_case(gold, name):
    kinds, seeds = [str(k) for k in gold[f"{name}:kinds"]], [int(s) for s in gold[f"{name}:seeds"]]
    c, r, k, v, origins, gts = A.batch(kinds, seeds)
    maps = [t.requires_grad_(True) for t in c + r + k]
    losses, targets = A.loss_by_feat(c, r, k, v, [A.gt_triplet(g) for g in gts], origins, int(gold["pts_assign_threshold"]),
                                     int(gold["pts_center_threshold"]))
    total = losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]
    if total.requires_grad:
        total.backward()
    return losses, targets, [m.grad if m.grad is not None else torch.zeros_like(m) for m in maps], (c, r, k, v, origins, gts)


def positive_pairs(gold, name):
    """(predicted, target) boxes of every positive point of a case, float32."""
    kinds, seeds = [str(k) for k in gold[f"{name}:kinds"]], [int(s) for s in gold[f"{name}:seeds"]]
    c, r, k, v, origins, gts = A.batch(kinds, seeds)
    pred, tgt = [], []
    for b, (o, gt) in enumerate(zip(origins, gts)):
        labels, _, _, bbox_t = A.assign(SIZES, o, *A.gt_triplet(gt))
        pos = (labels >= 0) & R.upsampled_valid(v, SIZES, b)
        bbox = R.flatten_maps(c, r, k, b)[1]
        points = torch.cat([R.level_points(s, l, o) for l, s in enumerate(SIZES)])
        pred.append(A.pred_to_box(points[pos], bbox[pos]))
        tgt.append(bbox_t[pos])
    return torch.cat(pred), torch.cat(tgt)


@pytest.mark.parametrize("name", CASES)
def test_g19_is_self_consistent(name):
    gold = load_golden("g19_head_loss_arkit")
    losses, targets, grads, _ = restated_case(gold, name)
    for b, t in enumerate(targets):
        check_targets(gold, name, b, *[x.numpy() for x in t])
    want, f64 = gold[f"{name}:losses"], gold[f"{name}:losses_f64"]
    for i, n in enumerate(NAMES):
        assert abs(float(losses[n].detach()) - float(want[i])) <= 1e-5 * abs(float(want[i])), (name, n)
        assert abs(float(want[i]) - f64[i]) <= 1e-5 * abs(f64[i]), (name, n)    # a tenth of the bar: else DESIGN 4.9 must say so
    check_gradients(gold, name, grads, 3, 1e-5)


def test_g19_holds_the_cases_it_is_meant_to():
    gold = load_golden("g19_head_loss_arkit")
    text = str(gold["stand_in"])
    assert "the mathematical function, not mmcv's rounding" in text and "reduce_mean: identity" in text
    assert all(int(gold[f"{n}:seeds_tried"]) <= 5 for n in CASES)               # a handful at the most
    seed = int(gold["twelve:seeds"][0])
    *_, origin, gt = A.scene("twelve", seed)
    boxes, volumes, labels = A.gt_triplet(gt)
    yaw = boxes[:, 6]
    assert abs(float(yaw[7])) < 0.01 and abs(float(yaw[8]) - np.pi / 2) < 0.01 and abs(float(yaw[9]) - np.pi) < 0.01
    assert float(yaw.max()) > 2.0 and float(yaw.min()) < -2.0                   # the whole circle
    extent = torch.tensor([SIZES[0][i] * R.VOXEL[i] for i in range(3)])
    assert bool((boxes[3, 3:6] > extent).all())                                 # a box larger than the grid
    assert float(boxes[4, 0] + boxes[4, 3:5].min() / 2) > float(origin[0] + extent[0] / 2)   # one partly outside it
    assert len(set(volumes.tolist())) == len(volumes)
    assert not A.near_decisions(SIZES, origin, (boxes, volumes, labels))
    *_, info = A.assign(SIZES, origin, boxes, volumes, labels, details=True)
    assert all(n < 27 for n in info[2][0]) and info[2][1] == 0                  # below the threshold at every level
    assert all(n >= 27 for n in info[3][0]) and info[3][1] == 2                 # above it at all levels
    box = gold["twelve:0:box_index"]
    assert (box == 1).any() and (box == 4).any()
    assert gold["no_valid:losses"].tolist() == [0.0, 0.0, 0.0]
    assert gold["valid_no_pos:losses"][2] > 0 and gold["valid_no_pos:losses"][:2].tolist() == [0.0, 0.0]
    assert len(gold["batch2:0:box_index"]) == len(gold["batch2:1:box_index"]) == 29200
    assert int(gold["sixty:0:box_index"].max()) >= 50
    for name in ("one", "twelve", "sixty", "batch2"):                           # no positive pair near a degenerate configuration
        assert not A.near_degenerate(*positive_pairs(gold, name), margin=float(gold["degenerate_margin"]))


@pytest.mark.parametrize("name", ["twelve", "sixty"])
def test_stand_in_iou_equals_exact_clipping(name):
    """diff_iou_rotated_3d in float64 = exact_iou's intersection (float64 Sutherland-Hodgman) times the z overlap over the union of
    the volumes, to float64 rounding, on the fixture's positive pairs."""
    gold = load_golden("g19_head_loss_arkit")
    pred, tgt = positive_pairs(gold, name)
    assert len(pred) > 50
    got = RI.diff_iou_rotated_3d(pred.double(), tgt.double()).numpy()
    got32 = RI.diff_iou_rotated_3d(pred, tgt).numpy()
    p, t = pred.double().numpy(), tgt.double().numpy()
    seen_overlap = 0
    for i in range(len(p)):
        bev = N.exact_iou(p[i], t[i])
        sa, sb = p[i][3] * p[i][4], t[i][3] * t[i][4]
        area = bev * (sa + sb) / (1 + bev)
        zo = max(min(p[i][2] + p[i][5] / 2, t[i][2] + t[i][5] / 2) - max(p[i][2] - p[i][5] / 2, t[i][2] - t[i][5] / 2), 0.0)
        inter = area * zo
        want = inter / (sa * p[i][5] + sb * t[i][5] - inter)
        assert abs(got[i] - want) <= 1e-12, (i, got[i], want)
        assert abs(got32[i] - want) <= 2e-5, (i, got32[i], want)
        seen_overlap += want > 0.01
    assert seen_overlap > 20


def test_stand_in_gradient_equals_central_differences():
    gold = load_golden("g19_head_loss_arkit")
    pred, tgt = positive_pairs(gold, "sixty")
    pred, tgt = pred[::9].double(), tgt[::9].double()
    keep = RI.diff_iou_rotated_3d(pred, tgt) > 0.01
    pred, tgt = pred[keep], tgt[keep]
    assert len(pred) >= 20
    x = pred.clone().requires_grad_(True)
    RI.diff_iou_rotated_3d(x, tgt).sum().backward()
    h = 1e-6
    for q in range(7):
        step = torch.zeros(7, dtype=torch.float64)
        step[q] = h
        fd = (RI.diff_iou_rotated_3d(pred + step, tgt) - RI.diff_iou_rotated_3d(pred - step, tgt)) / (2 * h)
        assert float((fd - x.grad[:, q]).abs().max()) <= 1e-6, (q, float((fd - x.grad[:, q]).abs().max()))
    assert float(x.grad.abs().max()) > 0.01


def test_dense_form_equals_restatement():
    c, r, k, v, origins, gts = A.batch(("five",), (77,), levels=((12, 10, 8), (6, 5, 4)), n_classes=3)
    trip = [A.gt_triplet(g) for g in gts]
    a, _ = A.loss_by_feat(c, r, k, v, trip, origins, 9, 4)
    b = A.dense_form_loss(c, r, k, v, trip, origins, 9, 4)
    for n in NAMES:
        assert abs(float(a[n].detach()) - float(b[n].detach())) <= 1e-5 * abs(float(b[n].detach())), n


# --------------------------------------------------------------------------------------------- the interface
ARKIT_MODEL = dict(type="MVSDet",
                   bbox_head=dict(type="ImVoxelHead_ARKit", n_classes=17, n_levels=3, n_channels=128, n_reg_outs=7,
                                  pts_assign_threshold=27, pts_center_threshold=18, prior_generator=dict(type="AlignedAnchor3DRangeGenerator")),
                   test_cfg=dict(nms_pre=1000, iou_thr=.25, score_thr=.01))


def test_head_from_config_builds_the_arkit_head():
    from mvsdet_amd import config
    kw = config.head_kwargs(dict(model=ARKIT_MODEL))
    assert kw["arkit_head"] is True and kw["n_reg_outs"] == 7 and kw["n_classes"] == 17 and kw["bbox_loss_weight"] == 1.0
    head = config.head_from_config(ARKIT_MODEL)
    assert head.arkit_head and head.conv_reg.out_channels == 7 and head.test_cfg["nms_pre"] == 1000
    assert (head.pts_assign_threshold, head.pts_center_threshold) == (27, 18)
    explicit = dict(ARKIT_MODEL, bbox_head=dict(ARKIT_MODEL["bbox_head"], bbox_loss=dict(type="RotatedIoU3DLoss", loss_weight=2.0)))
    assert config.head_kwargs(explicit)["bbox_loss_weight"] == 2.0
    without = {k: v for k, v in ARKIT_MODEL["bbox_head"].items() if k != "n_reg_outs"}
    assert config.head_kwargs(dict(ARKIT_MODEL, bbox_head=without))["n_reg_outs"] == 7
    with pytest.raises(ValueError, match="7 values"):
        config.head_kwargs(dict(ARKIT_MODEL, bbox_head=dict(ARKIT_MODEL["bbox_head"], n_reg_outs=6)))
    scannet = config.head_kwargs(dict(ARKIT_MODEL, bbox_head=dict(ARKIT_MODEL["bbox_head"], type="NerfDetHead", n_reg_outs=6,
                                                                   bbox_loss=dict(type="AxisAlignedIoULoss"))))
    assert scannet["arkit_head"] is False and scannet["n_reg_outs"] == 6


def test_the_three_refusals():
    from mvsdet_amd import config, ops
    from mvsdet_amd.head import NerfDetHeadConvs
    # 1. the ARKit head's loss on CPU maps: no CPU path, refused before any device work
    c, r, k, v, origins, gts = A.batch(("five",), (5,), levels=((4, 4, 4),), n_classes=3)
    head = NerfDetHeadConvs(n_classes=3, n_levels=1, n_channels=64, n_reg_outs=7, arkit_head=True)
    with pytest.raises(NotImplementedError, match="RotatedIoU3DLoss.*ROCm tensors only.*no CPU path"):
        head.loss_by_feat(c, r, k, v, gts, A.metas_for(origins))
    # 2. the ARKit head with the axis-aligned loss stays unimplemented
    bad = dict(ARKIT_MODEL, bbox_head=dict(ARKIT_MODEL["bbox_head"], bbox_loss=dict(type="AxisAlignedIoULoss")))
    with pytest.raises(NotImplementedError, match="computes 'RotatedIoU3DLoss' only"):
        config.head_kwargs(bad)
    # 3. the ScanNet head with the rotated loss, or with NerfDetHead's own default (the rotated loss)
    scannet = dict(ARKIT_MODEL["bbox_head"], type="NerfDetHead", n_reg_outs=6)
    with pytest.raises(ValueError, match="RotatedIoU3DLoss"):
        config.head_kwargs(dict(ARKIT_MODEL, bbox_head=dict(scannet, bbox_loss=dict(type="RotatedIoU3DLoss"))))
    with pytest.raises(ValueError, match="AxisAlignedIoULoss"):
        config.head_kwargs(dict(ARKIT_MODEL, bbox_head=scannet))
    with pytest.raises(ValueError, match="ImVoxelHead_ARKit"):
        config.head_kwargs(dict(ARKIT_MODEL, bbox_head=dict(scannet, type="FCAF3DHead")))
    # the box limit and the device are checked on shapes, before anything is launched
    with pytest.raises(ValueError, match="ASSIGN_MAX_BOXES"):
        ops.head_targets_rotated([(4, 4, 4)], [torch.zeros(3)], torch.zeros(1, ops.ASSIGN_MAX_BOXES + 1, 7), torch.zeros(1, 1, 2),
                                 torch.zeros(1, 1), torch.zeros(1, 1), torch.zeros(1), 27, 18)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_targets_rotated([(4, 4, 4)], [torch.zeros(3)], torch.zeros(1, 2, 7), torch.zeros(1, 2, 2), torch.zeros(1, 2),
                                 torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 27, 18)


def test_new_entries_check_their_arguments_before_launching():
    import ctypes
    import os
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    dims = (ctypes.c_int * 3)(4, 4, 4)
    f = lib.mvsdet_head_targets_rotated_f32
    assert f(dims, one, 1, 1, one, one, one, one, one, 1025, 27, 18, one, one, one, one, one, 1 << 30, None) == 1
    assert b"MVSDET_ASSIGN_MAX_BOXES" in lib.mvsdet_last_error()
    assert f(dims, one, 1, 1, one, None, one, one, one, 4, 27, 18, one, one, one, one, one, 1 << 30, None) == 1
    assert b"NULL" in lib.mvsdet_last_error()
    assert f(dims, one, 1, 1, one, one, one, one, one, 4, 27, 18, one, one, one, one, one, 8, None) == 2
    assert b"workspace" in lib.mvsdet_last_error()
    arr = (ctypes.c_void_p * 1)(4096)
    assert lib.mvsdet_head_loss_rotated_f32(arr, arr, arr, dims, one, one, 1, 1, 0, 4, 4, 4, one, one, one, 2.0, 0.25, one, one, one,
                                            1 << 30, None) == 1
    assert b"n_classes" in lib.mvsdet_last_error()
    assert lib.mvsdet_head_loss_rotated_backward_f32(arr, arr, arr, dims, one, one, 1, 1, 3, 4, 4, 4, one, one, one, 2.0, 0.25, None,
                                                     arr, arr, arr, None) == 1
    assert b"NULL" in lib.mvsdet_last_error()
