"""The head's training objective without a GPU: tests/head_loss_restated.py (the GPU tests' yardstick) against fixture G18 -- labels
and box choice equal, targets bit for bit, losses and gradients within 1e-6 relative -- and, under `-m refcheck`, against the
reference run live on fresh seeds; the C ABI declares the new entries; the Python layer's refusals come before any device work."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

import head_loss_restated as R

CASES = ("one", "twelve", "sixty", "no_valid", "valid_no_pos", "batch2")
NAMES = ("center_loss", "bbox_loss", "cls_loss")


def restated_case(gold, name):
    kinds, seeds = [str(k) for k in gold[f"{name}:kinds"]], [int(s) for s in gold[f"{name}:seeds"]]
    c, r, k, v, origins, gts = R.batch(kinds, seeds)
    maps = [t.requires_grad_(True) for t in c + r + k]
    losses, targets = R.loss_by_feat(c, r, k, v, [R.gt_triplet(g) for g in gts], origins, int(gold["pts_assign_threshold"]),
                                     int(gold["pts_center_threshold"]))
    (losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]).backward()
    return losses, targets, [m.grad for m in maps]


def check_targets(gold, name, b, labels, box_index, center_t, bbox_t):
    """labels and chosen box of every point equal; the targets' rows at assigned points bit for bit."""
    want = gold[f"{name}:{b}:labels"].astype(np.int64)
    assert np.array_equal(labels, want), name
    assert np.array_equal(box_index, gold[f"{name}:{b}:box_index"].astype(np.int64)), name
    assigned = np.nonzero(want >= 0)[0]
    assert np.array_equal(center_t[assigned].view(np.int32), gold[f"{name}:{b}:center_targets"].view(np.int32)), name
    assert np.array_equal(bbox_t[assigned].view(np.int32), gold[f"{name}:{b}:bbox_targets"].view(np.int32)), name


def check_gradients(gold, name, grads, n_levels, bar):
    """every stored element within `bar` of the map's largest absolute reference value; returns the largest deviation seen."""
    worst = 0.0
    for j, kind in enumerate(("center", "bbox", "cls")):
        for l in range(n_levels):
            g = grads[j * n_levels + l].detach().cpu().reshape(-1).numpy()
            idx, want = gold[f"{name}:grad:{kind}:{l}:index"], gold[f"{name}:grad:{kind}:{l}:values"]
            top = float(gold[f"{name}:grad:{kind}:{l}:sums"][2])
            dev = float(np.abs(g[idx] - want).max())
            if top == 0.0:
                assert dev == 0.0 and not g.any(), (name, kind, l)
                continue
            worst = max(worst, dev / top)
            assert dev <= bar * top, (name, kind, l, dev, top)
            s = gold[f"{name}:grad:{kind}:{l}:sums"]
            assert abs(float(g.astype(np.float64).sum()) - s[0]) <= 10 * bar * max(s[1], top), (name, kind, l)
    return worst


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_g18(name):
    gold = load_golden("g18_head_loss")
    losses, targets, grads = restated_case(gold, name)
    for b, t in enumerate(targets):
        check_targets(gold, name, b, *[x.numpy() for x in t])
    want = gold[f"{name}:losses"]
    for i, n in enumerate(NAMES):
        assert abs(float(losses[n].detach()) - float(want[i])) <= 1e-6 * abs(float(want[i])), (name, n, float(losses[n].detach()), float(want[i]))
    check_gradients(gold, name, grads, 3, 1e-6)


def test_g18_holds_the_cases_it_is_meant_to():
    gold = load_golden("g18_head_loss")
    assert "mmdet 3.x" in str(gold["stand_in"]) and "reduce_mean: identity" in str(gold["stand_in"])
    sizes = [tuple(s) for s in R.SCANNET_LEVELS]
    seed = int(gold["twelve:seeds"][0])
    *_, origin, gt = R.scene("twelve", seed)
    boxes, volumes, labels = R.gt_triplet(gt)
    *_, info = R.assign(sizes, origin, boxes, volumes, labels, details=True)
    assert all(n < 27 for n in info[2][0]) and info[2][1] == 0           # below the threshold at every level
    assert all(n >= 27 for n in info[3][0]) and info[3][1] == 2          # above it at all levels
    assert volumes[5] == volumes[6]                                        # equal volumes: the lower index wins where both apply
    box = gold["twelve:0:box_index"]
    assert (box == 5).any() and (box == 1).any()                           # the nested box takes points from box 0
    assert not R.near_decisions(sizes, origin, (boxes, volumes, labels))
    assert gold["no_valid:losses"].tolist() == [0.0, 0.0, 0.0]
    assert gold["valid_no_pos:losses"][2] > 0 and gold["valid_no_pos:losses"][:2].tolist() == [0.0, 0.0]
    assert len(gold["batch2:0:box_index"]) == len(gold["batch2:1:box_index"]) == 29200


def test_dense_form_equals_restatement():
    # the timing tool's baseline (the reference's form) computes what the restatement computes
    c, r, k, v, origins, gts = R.batch(("five",), (77,), levels=((12, 10, 8), (6, 5, 4)), n_classes=3)
    trip = [R.gt_triplet(g) for g in gts]
    a, _ = R.loss_by_feat(c, r, k, v, trip, origins, 9, 4)
    b = R.dense_form_loss(c, r, k, v, trip, origins, 9, 4)
    for n in NAMES:
        assert abs(float(a[n].detach()) - float(b[n].detach())) <= 1e-6 * abs(float(b[n].detach())), n


# --------------------------------------------------------------------------------------------- against the reference
@pytest.fixture(scope="module")
def reference_loss():
    sys.path.insert(0, GOLDEN)
    import make_goldens_g18 as g
    try:
        return g, g.load_reference_loss()
    except FileNotFoundError:
        pytest.skip("reference tree not mounted")


@pytest.mark.refcheck
@pytest.mark.parametrize("kinds,seed", [(("one",), 2101), (("twelve",), 2102), (("sixty",), 2103), (("five", "twelve"), 2104)])
def test_restatement_matches_reference_on_fresh_seeds(reference_loss, kinds, seed):
    g, RefLoss = reference_loss
    seeds = [seed + 11 * i for i in range(len(kinds))]
    ref_losses, scenes, ref_grads, _ = g.run_reference(RefLoss, kinds, seeds)
    c, r, k, v, origins, gts = R.batch(kinds, seeds)
    maps = [t.requires_grad_(True) for t in c + r + k]
    losses, targets = R.loss_by_feat(c, r, k, v, [R.gt_triplet(x) for x in gts], origins)
    (losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]).backward()
    for b, (t, sc) in enumerate(zip(targets, scenes)):
        near = R.near_decisions([tuple(s) for s in R.SCANNET_LEVELS], origins[b], R.gt_triplet(gts[b]))
        if near:   # a decision within rounding: both sides run the same float32 expressions on this CPU, so they still agree
            print(kinds, seeds, near[0])
        assert torch.equal(t[0], sc["labels"])
        a = t[0] >= 0
        assert torch.equal(t[2][a].view(torch.int32), sc["center_t"][a].view(torch.int32))
        assert torch.equal(t[3][a].view(torch.int32), sc["bbox_t"][a].view(torch.int32))
    for n in NAMES:
        assert abs(float(losses[n].detach()) - float(ref_losses[n].detach())) <= 1e-6 * abs(float(ref_losses[n].detach())), n
    for m, rg in zip(maps, ref_grads):
        assert float((m.grad - rg).abs().max()) <= 1e-6 * float(rg.abs().max()) or float(rg.abs().max()) == 0.0


@pytest.mark.refcheck
def test_g18_regenerates(reference_loss):
    g, RefLoss = reference_loss
    gold = load_golden("g18_head_loss")
    for name, kinds in g.CASES.items():
        seeds = [int(s) for s in gold[f"{name}:seeds"]]
        losses, scenes, _, _ = g.run_reference(RefLoss, kinds, seeds)
        for i, n in enumerate(NAMES):   # torch's sums depend on the thread count: to rounding, not to the bit
            want = float(gold[f"{name}:losses"][i])
            assert abs(float(losses[n].detach()) - want) <= 1e-6 * abs(want), (name, n)
        for b, sc in enumerate(scenes):
            assert np.array_equal(sc["labels"].numpy().astype(np.int8), gold[f"{name}:{b}:labels"]), name


# --------------------------------------------------------------------------------------------- the interface
def test_header_declares_the_new_entries():
    text = open(os.path.join(ROOT, "include", "mvsdet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn in ("mvsdet_head_targets_f32", "mvsdet_head_loss_f32", "mvsdet_head_loss_backward_f32",
               "mvsdet_head_targets_workspace_bytes", "mvsdet_head_loss_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % fn, text), fn
    m = re.search(r"#define\s+MVSDET_ASSIGN_MAX_BOXES\s+(\d+)", text)
    assert m and int(m.group(1)) >= 256
    from mvsdet_amd import ops
    assert ops.ASSIGN_MAX_BOXES == int(m.group(1))


def test_entries_check_their_arguments_before_launching():
    import ctypes
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    dims = (ctypes.c_int * 3)(4, 4, 4)
    assert lib.mvsdet_head_targets_workspace_bytes(2, 60) == 2 * 60 * 6 * 4 and lib.mvsdet_head_targets_workspace_bytes(2, 0) == 0
    assert lib.mvsdet_head_loss_workspace_bytes(2, 29200) == 2 * 115 * 24 and lib.mvsdet_head_loss_workspace_bytes(0, 5) == 0
    assert lib.mvsdet_head_targets_f32(dims, one, 1, 1, one, one, one, one, 1025, 27, 18, one, one, one, one, one, 1 << 30, None) == 1
    assert b"MVSDET_ASSIGN_MAX_BOXES" in lib.mvsdet_last_error()
    assert lib.mvsdet_head_targets_f32(dims, one, 1, 5, one, one, one, one, 4, 27, 18, one, one, one, one, one, 1 << 30, None) == 1
    assert b"levels" in lib.mvsdet_last_error()
    assert lib.mvsdet_head_targets_f32(dims, one, 1, 1, one, one, one, one, 4, 27, 18, one, one, one, one, one, 8, None) == 2
    assert b"workspace" in lib.mvsdet_last_error()
    assert lib.mvsdet_head_targets_f32(dims, one, 1, 1, None, one, one, one, 4, 27, 18, one, one, one, one, one, 1 << 30, None) == 1
    assert b"NULL" in lib.mvsdet_last_error()
    arr = (ctypes.c_void_p * 1)(4096)
    assert lib.mvsdet_head_loss_f32(arr, arr, arr, dims, one, one, 1, 1, 0, 4, 4, 4, one, one, one, 2.0, 0.25, one, one, one, 1 << 30,
                                    None) == 1
    assert b"n_classes" in lib.mvsdet_last_error()
    assert lib.mvsdet_head_loss_f32(arr, arr, arr, dims, one, one, 1, 1, 3, 4, 4, 4, one, one, one, 2.0, 0.25, one, one, one, 8, None) == 2
    assert lib.mvsdet_head_loss_backward_f32(arr, arr, arr, dims, one, one, 1, 1, 3, 4, 4, 4, one, one, one, 2.0, 0.25, None, arr, arr,
                                             arr, None) == 1
    assert b"NULL" in lib.mvsdet_last_error()


def test_loss_by_feat_has_the_reference_signature():
    from mvsdet_amd.head import NerfDetHeadConvs
    params = list(inspect.signature(NerfDetHeadConvs.loss_by_feat).parameters)
    assert params[:8] == ["self", "center_preds", "bbox_preds", "cls_preds", "valid_pred", "batch_gt_instances_3d", "batch_input_metas",
                          "batch_gt_instances_ignore"]
    head = NerfDetHeadConvs(n_classes=3, n_levels=1, n_channels=64)
    assert (head.pts_assign_threshold, head.pts_center_threshold) == (27, 18)


def _cpu_call(head, n_boxes=2):
    c, r, k, v, origins, gts = R.batch(("five",), (5,), levels=((4, 4, 4),), n_classes=3)
    if n_boxes != 5:
        t = torch.rand(n_boxes, 6) + 0.5
        gts = [R.GtInstances(R.DepthBoxes(t), torch.zeros(n_boxes, dtype=torch.int64))]
    return head.loss_by_feat(c, r, k, v, gts, R.metas_for(origins))


def test_refusals_come_before_any_device_work():
    from mvsdet_amd import ops
    from mvsdet_amd.head import NerfDetHeadConvs
    with pytest.raises(NotImplementedError, match="RotatedIoU3DLoss"):
        _cpu_call(NerfDetHeadConvs(n_classes=3, n_levels=1, n_channels=64, n_reg_outs=7, arkit_head=True))
    head = NerfDetHeadConvs(n_classes=3, n_levels=1, n_channels=64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _cpu_call(head)
    with pytest.raises(ValueError, match=f"ASSIGN_MAX_BOXES = {ops.ASSIGN_MAX_BOXES}"):
        _cpu_call(head, ops.ASSIGN_MAX_BOXES + 1)
    with pytest.raises(ValueError, match="ASSIGN_MAX_BOXES"):
        ops.head_targets([(4, 4, 4)], [torch.zeros(3)], torch.zeros(1, ops.ASSIGN_MAX_BOXES + 1, 6), torch.zeros(1, 1), torch.zeros(1, 1),
                         torch.zeros(1), 27, 18)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.head_targets([(4, 4, 4)], [torch.zeros(3)], torch.zeros(1, 2, 6), torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int64),
                         torch.zeros(1, dtype=torch.int32), 27, 18)


def test_head_from_config():
    from mvsdet_amd import config
    model = dict(type="MVSDet", bbox_head=dict(type="NerfDetHead", bbox_loss=dict(type="AxisAlignedIoULoss", loss_weight=2.0),
                                               n_classes=18, n_levels=3, n_channels=128, n_reg_outs=6, pts_assign_threshold=27,
                                               pts_center_threshold=18), test_cfg=dict(nms_pre=1000, iou_thr=.25, score_thr=.01))
    kw = config.head_kwargs(dict(model=model))
    assert kw["pts_assign_threshold"] == 27 and kw["pts_center_threshold"] == 18 and kw["bbox_loss_weight"] == 2.0
    assert kw["focal_gamma"] == 2.0 and kw["focal_alpha"] == 0.25 and kw["test_cfg"]["nms_pre"] == 1000
    head = config.head_from_config(model)
    assert head.n_classes == 18 and head.bbox_loss_weight == 2.0 and head.test_cfg["iou_thr"] == .25
    bad = dict(model, bbox_head=dict(model["bbox_head"], bbox_loss=dict(type="RotatedIoU3DLoss")))
    with pytest.raises(ValueError, match="RotatedIoU3DLoss"):
        config.head_kwargs(bad)
    with pytest.raises(ValueError, match="AxisAlignedIoULoss"):   # NerfDetHead's own default is the rotated loss
        config.head_kwargs(dict(model, bbox_head={k: v for k, v in model["bbox_head"].items() if k != "bbox_loss"}))
    with pytest.raises(ValueError, match="FocalLoss"):
        config.head_kwargs(dict(model, bbox_head=dict(model["bbox_head"], cls_loss=dict(type="mmdet.CrossEntropyLoss"))))
    with pytest.raises(NotImplementedError, match="RotatedIoU3DLoss"):
        config.head_kwargs(dict(model, bbox_head=dict(model["bbox_head"], type="ImVoxelHead_ARKit")))
