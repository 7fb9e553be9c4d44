"""The ARKit head's training objective on the GPU (csrc/assign.hip, the kernels instantiated for 7-value boxes):
ops.head_targets_rotated and NerfDetHeadConvs(arkit_head=True).loss_by_feat against fixture G19 (inputs rebuilt from the fixture's
seeds), against tests/head_loss_arkit_restated.py in float64 on shapes G19 does not hold, on planted degenerate pairs, without a host
synchronisation, with the same bits from run to run, and through one SGD step of neck + head.

G19's rotated IoU is tests/rotated_iou_restated.py: the mathematical function, not mmcv's rounding (mmcv's op has no CPU path).  What
these tests establish is "the true rotated IoU and its gradient, to the project's bar", not "mmcv's bits".

Bars (the project's, from G18): labels, chosen boxes and box targets bit for bit; centerness targets at positive points and each loss
within 1e-4 relative; gradients within 1e-4 of a map's largest absolute reference gradient.  test_loss_by_feat_equals_g19 prints
ours against the fixture's float32 and float64 results per case (run with -s); the table is in DESIGN.md 4.9 (measured again after
the z faces took ATen's tie routing and bce_logits ATen's log_sigmoid form: losses at most 2.1e-7 relative, gradients at most 7.7e-6
of a map's maximum, as before)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

import head_loss_arkit_restated as A
import head_loss_restated as R
from head_loss_planted import plant
from test_head_loss_arkit_host import CASES, NAMES, check_gradients, check_targets

pytestmark = pytest.mark.gpu


def _case(gold, name, dev):
    kinds, seeds = [str(k) for k in gold[f"{name}:kinds"]], [int(s) for s in gold[f"{name}:seeds"]]
    c, r, k, v, origins, gts = A.batch(kinds, seeds)
    to = lambda ts: [t.to(dev) for t in ts]  # noqa: E731
    return to(c), to(r), to(k), v.to(dev), origins, gts


def _targets(dev, sizes, origins, gts, assign_thr=27, center_thr=18):
    from mvsdet_amd import ops
    from mvsdet_amd.head import pad_ground_truth_rotated
    boxes, rot, volumes, labels, counts = pad_ground_truth_rotated(gts, dev)
    return ops.head_targets_rotated(sizes, origins, boxes, rot, volumes, labels, counts, assign_thr, center_thr)


def _head(**kw):
    from mvsdet_amd.head import NerfDetHeadConvs
    return NerfDetHeadConvs(n_classes=kw.pop("n_classes", 17), n_levels=kw.pop("n_levels", 3), n_channels=64, n_reg_outs=7,
                            arkit_head=True, **kw)


def _total(losses):
    return losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]


@pytest.mark.parametrize("name", CASES)
def test_head_targets_equal_g19(gpu, name):
    gold = load_golden("g19_head_loss_arkit")
    c, r, k, v, origins, gts = _case(gold, name, gpu)
    t = _targets(gpu, [tuple(x.shape[2:]) for x in c], origins, gts)
    assert t.bbox_targets.shape[-1] == 7
    for b in range(len(gts)):
        worst = check_targets(gold, name, b, t.labels[b].cpu().numpy(), t.box_index[b].cpu().numpy().astype(np.int64),
                              t.center_targets[b].cpu().numpy(), t.bbox_targets[b].cpu().numpy())
        print(f"G19 {name} scene {b} centerness targets: largest relative deviation {worst:.3g}")
        none = t.labels[b] < 0
        assert bool((t.center_targets[b][none] == -1).all()) and bool((t.box_index[b][none] == -1).all())


@pytest.mark.parametrize("name", CASES)
def test_loss_by_feat_equals_g19(gpu, name):
    """Fails on the parent commit with NotImplementedError."""
    gold = load_golden("g19_head_loss_arkit")
    c, r, k, v, origins, gts = _case(gold, name, gpu)
    maps = [t.requires_grad_(True) for t in c + r + k]
    losses = _head().loss_by_feat(c, r, k, v, gts, A.metas_for(origins))
    assert list(losses) == list(NAMES)
    _total(losses).backward()
    want, f64 = gold[f"{name}:losses"], gold[f"{name}:losses_f64"]
    for i, n in enumerate(NAMES):
        got = float(losses[n].detach())
        rel = abs(got - float(want[i])) / abs(float(want[i])) if want[i] else abs(got)
        rel64 = abs(got - f64[i]) / abs(f64[i]) if f64[i] else abs(got)
        ref_rel = abs(float(want[i]) - f64[i]) / abs(f64[i]) if f64[i] else 0.0
        print(f"G19 {name} {n}: ours {got:.9g} reference {float(want[i]):.9g} relative deviation {rel:.3g}, against float64 "
              f"{rel64:.3g} (reference fp32 against float64: {ref_rel:.3g})")
    worst = check_gradients(gold, name, [m.grad for m in maps], 3, float("inf"))
    print(f"G19 {name} gradients: largest deviation {worst:.3g} of a map's largest absolute reference value")
    for i, n in enumerate(NAMES):
        got = float(losses[n].detach())
        assert abs(got - float(want[i])) <= 1e-4 * abs(float(want[i])), (name, n, got, float(want[i]))
    check_gradients(gold, name, [m.grad for m in maps], 3, 1e-4)
    assert all(bool(torch.isfinite(m.grad).all()) for m in maps)


# ------------------------------------------------------------------- against the restatement in float64, other shapes
SHAPES = {
    # name: (levels, classes, scene kinds, pts_assign_threshold, pts_center_threshold)
    "l1_c1": (((12, 10, 8),), 1, ("five",), 9, 4),
    "l2_odd_c3_b2": (((13, 11, 7), (7, 5, 3)), 3, ("twelve", "one"), 9, 1),
    "l4_c40": (((16, 16, 8), (8, 8, 4), (4, 4, 2), (2, 2, 1)), 40, ("sixty",), 5, 0),
    "l3_c17_b4": (A.ARKIT_LEVELS, 17, ("sixty", "five", "one", "twelve"), 27, 18),
    "l1_topk_above_points": (((3, 2, 2),), 2, ("one",), 1, 18),     # pts_center_threshold + 1 > points: top-k takes them all
}


def _acceptable_seed(levels, n_classes, kinds, assign_thr, center_thr, seed):
    """The first seed from `seed` on whose scenes hang on no rounding (the fixture's conditions on the inputs)."""
    sizes = [tuple(s) for s in levels]
    for s in range(seed, seed + 200, 13):
        seeds = [s + 3 * i for i in range(len(kinds))]
        c, r, k, v, origins, gts = A.batch(kinds, seeds, levels, n_classes)
        if not any(A.near_decisions(sizes, o, A.gt_triplet(g), assign_thr, center_thr) for o, g in zip(origins, gts)):
            return seeds
    raise AssertionError("no acceptable seed")


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_restatement_on_other_shapes(gpu, name):
    levels, n_classes, kinds, assign_thr, center_thr = SHAPES[name]
    seeds = _acceptable_seed(levels, n_classes, kinds, assign_thr, center_thr, 2900)
    c, r, k, v, origins, gts = A.batch(kinds, seeds, levels, n_classes)
    L = len(levels)
    ref_maps = [t.double().requires_grad_(True) for t in c + r + k]
    want, want_t = A.loss_by_feat(ref_maps[:L], ref_maps[L:2 * L], ref_maps[2 * L:], v, [A.gt_triplet(g) for g in gts], origins,
                                  assign_thr, center_thr, dtype=torch.float64)
    _total(want).backward()
    maps = [t.to(gpu).requires_grad_(True) for t in c + r + k]
    head = _head(n_classes=n_classes, n_levels=L, pts_assign_threshold=assign_thr, pts_center_threshold=center_thr)
    got = head.loss_by_feat(maps[:L], maps[L:2 * L], maps[2 * L:], v.to(gpu), gts, A.metas_for(origins))
    _total(got).backward()
    got_t = _targets(gpu, [tuple(s) for s in levels], origins, gts, assign_thr, center_thr)
    for b, t in enumerate(want_t):
        assert torch.equal(got_t.labels[b].cpu(), t[0]) and torch.equal(got_t.box_index[b].cpu().long(), t[1])
        assert torch.equal(got_t.bbox_targets[b].cpu().view(torch.int32), t[3].view(torch.int32))
        a = t[0] >= 0
        if bool(a.any()):
            assert float(((got_t.center_targets[b].cpu()[a] - t[2][a]).abs() / t[2][a]).max()) <= 1e-4
    for n in NAMES:
        w = float(want[n].detach())
        assert abs(float(got[n].detach()) - w) <= 1e-4 * abs(w), (n, float(got[n].detach()), w)
    for m, rm in zip(maps, ref_maps):
        g = rm.grad if rm.grad is not None else torch.zeros_like(rm)
        top = float(g.abs().max())
        assert float((m.grad.cpu().double() - g).abs().max()) <= 1e-4 * top, top


# ------------------------------------------------------------------------------------------------ degenerate pairs
def _planted(gpu, pred, target, weight=0.7):
    """One positive point on a one-level 2x2x2 grid whose decoded box is `pred` (7,) against the target row `target` (7,), through
    ops.head_loss_rotated: (IoU, loss sum, gradient of the loss sum by the point's seven channels)."""
    from mvsdet_amd import ops
    levels = ((2, 2, 2),)
    origin = torch.tensor([1.05, 0.7, 0.3])                     # point 5 = (1.05, 0.54, 0.3)
    geom = ops.detect_level_geometry(levels, [origin]).to(gpu)
    pts = R.level_points(levels[0], 0, origin)
    i = 5
    p, pred, target = pts[i].double(), torch.tensor(pred, dtype=torch.float64), torch.tensor(target, dtype=torch.float64)
    c, s = math.cos(float(pred[6])), math.sin(float(pred[6]))
    sh = pred[:3] - p                                           # the shift in the predicted box's own frame
    sx, sy, sz = float(sh[0]) * c + float(sh[1]) * s, -float(sh[0]) * s + float(sh[1]) * c, float(sh[2])
    w, l, h = (float(x) for x in pred[3:6])
    d = torch.tensor([w / 2 - sx, w / 2 + sx, l / 2 - sy, l / 2 + sy, h / 2 - sz, h / 2 + sz, float(pred[6])])
    assert bool((d[:6] > 0).all())                              # the head's distances are exponentials
    sums, g = plant(gpu, geom, i, d, target, weight)
    assert abs(float(sums.weight_sum[0]) - weight) < 1e-6
    assert bool(torch.isfinite(g).all())
    loss = float(sums.bbox[0].detach())
    assert math.isfinite(loss)
    return 1.0 - loss / weight, loss, g[:, i], pts[i], d


B0 = [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.3]


def test_degenerate_pairs_are_finite_and_true(gpu):
    # identical boxes: loss 0 to 1e-6 absolute
    iou, loss, g, *_ = _planted(gpu, B0, B0)
    assert abs(loss) <= 1e-6
    # the same yaw, shifted along the box's own x axis by 0.5: the closed-form axis-aligned IoU 1.5 / (2 + 2 - 1.5)
    shifted = [B0[0] + 0.5 * math.cos(0.3), B0[1] + 0.5 * math.sin(0.3)] + B0[2:]
    iou, loss, g, *_ = _planted(gpu, B0, shifted)
    assert abs(iou - 1.5 / 2.5) <= 1e-5
    # axis-aligned, shifted in x, y and z
    a, b = [1.25, 0.75, 0.5, 2.0, 1.0, 1.0, 0.0], [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.0]
    inter = 1.75 * 0.75 * 0.75
    iou, loss, g, *_ = _planted(gpu, a, b)
    assert abs(iou - inter / (4.0 - inter)) <= 1e-5
    # one box inside the other (other yaw): the volume ratio, both ways
    inner = [1.1, 0.55, 0.3, 0.5, 0.4, 0.5, 1.2]
    for p, t in ((inner, B0), (B0, inner)):
        iou, loss, g, *_ = _planted(gpu, p, t)
        assert abs(iou - (0.5 * 0.4 * 0.5) / 2.0) <= 1e-5
    # disjoint: IoU 0, loss = w, no gradient
    iou, loss, g, *_ = _planted(gpu, B0, [7.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.9], weight=0.7)
    assert abs(iou) <= 1e-6 and abs(loss - 0.7) <= 1e-6 and not bool(g.any())
    # disjoint in z only
    iou, loss, g, *_ = _planted(gpu, B0, B0[:2] + [5.0] + B0[3:])
    assert abs(iou) <= 1e-6 and not bool(g.any())
    # touching along an edge: IoU 0
    iou, loss, g, *_ = _planted(gpu, [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.0], [3.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.0])
    assert abs(iou) <= 1e-6
    # yaw differing by exactly (float) pi / 2: the central 1 x 1 square of two crossed 2 x 1 rectangles
    iou, loss, g, *_ = _planted(gpu, B0[:6] + [0.3 + math.pi / 2], B0)
    assert abs(iou - 1.0 / 3.0) <= 1e-5
    iou, loss, g, *_ = _planted(gpu, [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, float(np.float32(math.pi / 2))], [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.0])
    assert abs(iou - 1.0 / 3.0) <= 1e-5
    # a square turned by pi / 2 is itself
    iou, loss, g, *_ = _planted(gpu, [1.0, 0.5, 0.25, 1.0, 1.0, 1.0, float(np.float32(math.pi / 2))], [1.0, 0.5, 0.25, 1.0, 1.0, 1.0, 0.0])
    assert abs(iou - 1.0) <= 1e-5
    # yaw differing by exactly (float) pi: the same rectangle
    for p in (B0[:6] + [0.3 + math.pi], B0[:6] + [0.3 - math.pi]):
        iou, loss, g, *_ = _planted(gpu, p, B0)
        assert abs(iou - 1.0) <= 1e-5
    iou, loss, g, *_ = _planted(gpu, [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, float(np.float32(math.pi))], [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.0])
    assert abs(iou - 1.0) <= 1e-5
    # a corner on an edge, a shared edge with the rest overlapping
    iou, loss, g, *_ = _planted(gpu, [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.0], [2.0, 0.5, 0.25, 2.0, 1.0, 1.0, 0.0])
    assert abs(iou - 1.0 / 3.0) <= 1e-5
    # ground truth of zero size: finite, IoU 0
    for t in (B0[:3] + [0.0, 1.0, 1.0, 0.3], B0[:3] + [0.0, 0.0, 0.0, 0.3], B0[:3] + [2.0, 1.0, 0.0, 0.3]):
        iou, loss, g, *_ = _planted(gpu, B0, t)
        assert abs(iou) <= 1e-6


def test_planted_gradient_equals_the_restatement(gpu):
    """value and gradient by the seven channels of a generic pair against autograd through the restatement in float64."""
    import rotated_iou_restated as RI
    pred, target = [1.2, 0.4, 0.35, 1.6, 0.9, 1.1, 0.8], [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, -0.4]   # no two z faces level
    iou, loss, g, p, d = _planted(gpu, pred, target, weight=1.0)
    x = d.double().view(1, 7).requires_grad_(True)
    want = RI.diff_iou_rotated_3d(A.pred_to_box(p.double().view(1, 3), x), torch.tensor([target], dtype=torch.float64))
    (1 - want).sum().backward()
    assert abs(iou - float(want.detach())) <= 1e-5 and float(want.detach()) > 0.2
    top = float(x.grad.abs().max())
    assert top > 0.01 and float((g.double() - x.grad[0]).abs().max()) <= 1e-4 * top


# ------------------------------------------------------------------------------------------------ behaviour
def test_no_host_synchronisation(gpu):
    gold = load_golden("g19_head_loss_arkit")
    c, r, k, v, origins, gts = _case(gold, "batch2", gpu)
    gts = [g.to(gpu) for g in gts]
    metas = A.metas_for(origins)
    head = _head()

    def step():
        maps = [t.detach().requires_grad_(True) for t in c + r + k]
        losses = head.loss_by_feat(maps[:3], maps[3:6], maps[6:], v, gts, metas)
        _total(losses).backward()
        return losses, maps

    step()   # warm: library load, allocator, pinned buffers
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses, maps = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert float(losses["bbox_loss"].detach()) > 0 and all(m.grad is not None for m in maps)


def test_two_runs_give_the_same_bits(gpu):
    gold = load_golden("g19_head_loss_arkit")
    c, r, k, v, origins, gts = _case(gold, "batch2", gpu)
    runs = []
    for _ in range(2):
        maps = [t.detach().clone().requires_grad_(True) for t in c + r + k]
        losses = _head().loss_by_feat(maps[:3], maps[3:6], maps[6:], v, gts, A.metas_for(origins))
        _total(losses).backward()
        runs.append([losses[n].detach() for n in NAMES] + [m.grad for m in maps])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_under_autocast_the_loss_computes_in_float32(gpu):
    gold = load_golden("g19_head_loss_arkit")
    c, r, k, v, origins, gts = _case(gold, "one", gpu)
    head = _head()
    plain = head.loss_by_feat(c, r, k, v, gts, A.metas_for(origins))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        amp = head.loss_by_feat(c, r, k, v, gts, A.metas_for(origins))
    for n in NAMES:
        assert amp[n].dtype == torch.float32 and torch.equal(amp[n], plain[n])


def test_head_from_config_trains_on_the_device(gpu):
    from mvsdet_amd import config
    from test_head_loss_arkit_host import ARKIT_MODEL
    head = config.head_from_config(ARKIT_MODEL)
    gold = load_golden("g19_head_loss_arkit")
    c, r, k, v, origins, gts = _case(gold, "twelve", gpu)
    maps = [t.requires_grad_(True) for t in c + r + k]
    losses = head.loss_by_feat(c, r, k, v, gts, A.metas_for(origins))
    _total(losses).backward()
    want = gold["twelve:losses"]
    for i, n in enumerate(NAMES):
        assert abs(float(losses[n].detach()) - float(want[i])) <= 1e-4 * abs(float(want[i]))
    assert all(m.grad is not None and bool(torch.isfinite(m.grad).all()) for m in maps) and float(maps[3].grad.abs().max()) > 0


def test_box_limit_and_empty_scene(gpu):
    from mvsdet_amd import ops
    levels = ((12, 12, 6), (6, 6, 3))
    for n_boxes in (0, ops.ASSIGN_MAX_BOXES):
        u = R._u((max(n_boxes, 1), 8), 2950 + n_boxes)[:n_boxes]
        ctr = torch.tensor([3.0, 3.0, 1.5]) + u[:, :3] * torch.tensor([0.9, 0.9, 0.5])
        size = 0.3 + 0.5 * (u[:, 3:6] + 1)
        tensor = torch.cat([ctr[:, :2], (ctr[:, 2] - size[:, 2] * 0.5).unsqueeze(1), size, u[:, 7:8] * math.pi], dim=1).float()
        gts = [R.GtInstances(A.RotatedDepthBoxes(tensor), ((u[:, 6] + 1) * 2).long().clamp(max=3))]
        c, r, k, v, origins, _ = A.batch(("one",), (2960,), levels, 4)
        maps = [t.to(gpu).requires_grad_(True) for t in c + r + k]
        head = _head(n_classes=4, n_levels=2, pts_assign_threshold=4, pts_center_threshold=2)
        got = head.loss_by_feat(maps[:2], maps[2:4], maps[4:], v.to(gpu), gts, A.metas_for(origins))
        _total(got).backward()
        assert all(bool(torch.isfinite(m.grad).all()) for m in maps)
        t = _targets(gpu, levels, origins, gts, 4, 2)
        if n_boxes == 0:
            assert int((t.labels >= 0).sum()) == 0 and float(got["center_loss"].detach()) == 0.0 == float(got["bbox_loss"].detach())
        else:
            assert int((t.labels >= 0).sum()) > 0 and int(t.box_index.max()) < n_boxes


def test_one_sgd_step_of_neck_and_arkit_head(gpu):
    """IndoorImVoxelNeck + NerfDetHeadConvs(arkit_head=True) on the HIP autograd route, loss_by_feat, backward, ten SGD steps: the
    summed loss falls and every parameter stays finite."""
    from mvsdet_amd.head import NerfDetHeadConvs
    from mvsdet_amd.neck import IndoorImVoxelNeck
    torch.manual_seed(0)
    neck = IndoorImVoxelNeck(256, 128, [1, 1, 1]).train()
    head = NerfDetHeadConvs(17, 3, 128, 7, arkit_head=True).train()
    head.init_weights()
    neck, head = neck.to(gpu), head.to(gpu)
    neck.autograd_route = head.autograd_route = "hip"
    levels = A.ARKIT_LEVELS
    *_, v, origins, gts = A.batch(("twelve",), (2972,), levels, 17)
    x = (0.5 * R._u((1, 256) + levels[0], 2973)).to(gpu)
    v, metas = v.to(gpu), A.metas_for(origins)
    params = list(neck.parameters()) + list(head.parameters())
    opt = torch.optim.SGD(params, lr=1e-3)
    totals = []
    for _ in range(10):
        for p in params:
            p.grad = None
        t = _total(head.loss_by_feat(*head(neck(x)), v, gts, metas))
        t.backward()
        assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in params)
        totals.append(float(t.detach()))
        opt.step()
    assert totals[-1] < totals[0], totals
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert head.conv_reg.weight.grad is not None and float(head.conv_reg.weight.grad[6].abs().max()) > 0   # the heading learns
