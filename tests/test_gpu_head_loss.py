"""The head's training objective on the GPU (csrc/assign.hip): ops.head_targets and NerfDetHeadConvs.loss_by_feat against fixture
G18 (the reference's results; inputs rebuilt from the fixture's seeds), against tests/head_loss_restated.py on shapes G18 does not
hold, without a host synchronisation, with the same bits from run to run, and through one SGD step of neck + head.

Deviations seen on an MI355X against G18 (bars: 1e-4 relative per loss, 1e-4 of a map's largest absolute reference gradient): losses
at most 3.1e-7 relative (the reference's own float32 result is up to 1.0e-7 from its float64 evaluation), gradients at most 4.3e-7 of
a map's maximum; targets bit for bit.  These are the figures of the kernels as they are now, measured again after iou_loss took
ATen's tie routing and bce_logits ATen's log_sigmoid form: both maxima are unchanged, one entry moved (case one's centre loss, from
0 to 7.0e-8).  test_loss_by_feat_equals_g18 prints them per case (run with -s); the table is in DESIGN.md 4.8."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

import head_loss_restated as R
from test_head_loss_host import CASES, NAMES, check_gradients, check_targets

pytestmark = pytest.mark.gpu


def _case(gold, name, dev):
    kinds, seeds = [str(k) for k in gold[f"{name}:kinds"]], [int(s) for s in gold[f"{name}:seeds"]]
    c, r, k, v, origins, gts = R.batch(kinds, seeds)
    to = lambda ts: [t.to(dev) for t in ts]  # noqa: E731
    return to(c), to(r), to(k), v.to(dev), origins, gts


def _targets(dev, sizes, origins, gts, assign_thr=27, center_thr=18):
    from mvsdet_amd import ops
    from mvsdet_amd.head import pad_ground_truth
    boxes, volumes, labels, counts = pad_ground_truth(gts, dev)
    return ops.head_targets(sizes, origins, boxes, volumes, labels, counts, assign_thr, center_thr)


def _head(**kw):
    from mvsdet_amd.head import NerfDetHeadConvs
    return NerfDetHeadConvs(n_classes=kw.pop("n_classes", 18), n_levels=kw.pop("n_levels", 3), n_channels=64, **kw)


@pytest.mark.parametrize("name", CASES)
def test_head_targets_equal_g18(gpu, name):
    gold = load_golden("g18_head_loss")
    c, r, k, v, origins, gts = _case(gold, name, gpu)
    t = _targets(gpu, [tuple(x.shape[2:]) for x in c], origins, gts)
    for b in range(len(gts)):
        check_targets(gold, name, b, t.labels[b].cpu().numpy(), t.box_index[b].cpu().numpy().astype(np.int64),
                      t.center_targets[b].cpu().numpy(), t.bbox_targets[b].cpu().numpy())


@pytest.mark.parametrize("name", CASES)
def test_loss_by_feat_equals_g18(gpu, name):
    gold = load_golden("g18_head_loss")
    c, r, k, v, origins, gts = _case(gold, name, gpu)
    maps = [t.requires_grad_(True) for t in c + r + k]
    losses = _head().loss_by_feat(c, r, k, v, gts, R.metas_for(origins))
    assert list(losses) == list(NAMES)
    (losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]).backward()
    want, f64 = gold[f"{name}:losses"], gold[f"{name}:losses_f64"]
    for i, n in enumerate(NAMES):
        got = float(losses[n].detach())
        rel = abs(got - float(want[i])) / abs(float(want[i])) if want[i] else abs(got)
        ref_rel = abs(float(want[i]) - f64[i]) / abs(f64[i]) if f64[i] else 0.0
        print(f"G18 {name} {n}: ours {got:.9g} reference {float(want[i]):.9g} relative deviation {rel:.3g} "
              f"(reference fp32 against float64: {ref_rel:.3g})")
    worst = check_gradients(gold, name, [m.grad for m in maps], 3, float("inf"))
    print(f"G18 {name} gradients: largest deviation {worst:.3g} of a map's largest absolute reference value")
    for i, n in enumerate(NAMES):
        got = float(losses[n].detach())
        assert abs(got - float(want[i])) <= 1e-4 * abs(float(want[i])), (name, n, got, float(want[i]))
    check_gradients(gold, name, [m.grad for m in maps], 3, 1e-4)


# ------------------------------------------------------------------------------- against the restatement, other shapes
SHAPES = {
    # name: (levels, classes, scene kinds, pts_assign_threshold, pts_center_threshold)
    "l1_c1": (((12, 10, 8),), 1, ("five",), 9, 4),
    "l2_odd_c3_b2": (((13, 11, 7), (7, 5, 3)), 3, ("twelve", "one"), 9, 1),
    "l4_c40": (((16, 16, 8), (8, 8, 4), (4, 4, 2), (2, 2, 1)), 40, ("sixty",), 5, 0),
    "l3_scannet_c18_b3": (R.SCANNET_LEVELS, 18, ("sixty", "five", "one"), 27, 18),
}


def _restated_and_ours(gpu, levels, n_classes, kinds, assign_thr, center_thr, seed, gts=None):
    c, r, k, v, origins, made = R.batch(kinds, [seed + 3 * i for i in range(len(kinds))], levels, n_classes)
    gts = made if gts is None else gts
    ref_maps = [t.clone().requires_grad_(True) for t in c + r + k]
    L = len(levels)
    want, want_t = R.loss_by_feat(ref_maps[:L], ref_maps[L:2 * L], ref_maps[2 * L:], v, [R.gt_triplet(g) for g in gts], origins,
                                  assign_thr, center_thr)
    (want["center_loss"] + want["bbox_loss"] + want["cls_loss"]).backward()
    maps = [t.to(gpu).requires_grad_(True) for t in c + r + k]
    head = _head(n_classes=n_classes, n_levels=L, pts_assign_threshold=assign_thr, pts_center_threshold=center_thr)
    got = head.loss_by_feat(maps[:L], maps[L:2 * L], maps[2 * L:], v.to(gpu), gts, R.metas_for(origins))
    (got["center_loss"] + got["bbox_loss"] + got["cls_loss"]).backward()
    got_t = _targets(gpu, [tuple(s) for s in levels], origins, gts, assign_thr, center_thr)
    return want, want_t, ref_maps, got, got_t, maps


def _check_against_restatement(want, want_t, ref_maps, got, got_t, maps):
    for b, t in enumerate(want_t):
        assert torch.equal(got_t.labels[b].cpu(), t[0]) and torch.equal(got_t.box_index[b].cpu().long(), t[1])
        assert torch.equal(got_t.center_targets[b].cpu().view(torch.int32), t[2].view(torch.int32))
        assert torch.equal(got_t.bbox_targets[b].cpu().view(torch.int32), t[3].view(torch.int32))
    for n in NAMES:
        w = float(want[n].detach())
        assert abs(float(got[n].detach()) - w) <= 1e-4 * abs(w), (n, float(got[n].detach()), w)
    for m, rm in zip(maps, ref_maps):
        top = float(rm.grad.abs().max())
        assert float((m.grad.cpu() - rm.grad).abs().max()) <= 1e-4 * top, top


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_restatement_on_other_shapes(gpu, name):
    levels, n_classes, kinds, assign_thr, center_thr = SHAPES[name]
    _check_against_restatement(*_restated_and_ours(gpu, levels, n_classes, kinds, assign_thr, center_thr, 2300))


@pytest.mark.parametrize("n_boxes", [0, 1, 256, 1024])
def test_box_counts_from_none_to_the_limit(gpu, n_boxes):
    from mvsdet_amd import ops
    assert ops.ASSIGN_MAX_BOXES == 1024
    levels = ((12, 12, 6), (6, 6, 3))
    u = R._u((max(n_boxes, 1), 7), 2400 + n_boxes)[:n_boxes]
    ctr = torch.tensor([3.0, 3.0, 1.5]) + u[:, :3] * torch.tensor([0.9, 0.9, 0.5])
    size = 0.3 + 0.5 * (u[:, 3:6] + 1)
    tensor = torch.cat([ctr[:, :2], (ctr[:, 2] - size[:, 2] * 0.5).unsqueeze(1), size], dim=1).float()
    gts = [R.GtInstances(R.DepthBoxes(tensor), ((u[:, 6] + 1) * 2).long().clamp(max=3))]
    res = _restated_and_ours(gpu, levels, 4, ("one",), 4, 2, 2410, gts)
    _check_against_restatement(*res)
    if n_boxes == 0:
        assert int((res[4].labels >= 0).sum()) == 0 and float(res[3]["center_loss"].detach()) == 0.0


def test_exact_centerness_ties_across_the_boundary_are_all_out(gpu):
    # a box centred on a grid point of an even-spaced grid: mirrored points share their centerness bit for bit.  With
    # pts_center_threshold = 1 the second largest value is one of such a group, and the whole group is out (strict >).
    levels = ((8, 8, 8),)
    origin = torch.tensor([0.0, 0.0, 0.0])
    pts = R.level_points(levels[0], 0, origin)
    centre = pts[4 * 64 + 4 * 8 + 4] + torch.tensor([0.08, 0.08, 0.1])    # the middle of a cell: eight nearest points tie
    tensor = torch.cat([centre[:2], centre[2:] - 0.5, torch.tensor([1.0, 1.0, 1.0])]).view(1, 6).float()
    gts = [R.GtInstances(R.DepthBoxes(tensor), torch.tensor([2]))]
    boxes, volumes, labels = R.gt_triplet(gts[0])
    for center_thr, expect_none in ((1, True), (0, True), (8, False)):
        *_, info = R.assign(levels, origin, boxes, volumes, labels, 4, center_thr, details=True)
        c, t = info[0][3], info[0][2]
        assert int((c == t).sum()) >= 2                                  # an exact tie at the boundary
        want = R.assign(levels, origin, boxes, volumes, labels, 4, center_thr)
        assert (int((want[0] >= 0).sum()) == 0) == expect_none
        got = _targets(gpu, levels, [origin], gts, 4, center_thr)
        assert torch.equal(got.labels[0].cpu(), want[0]) and torch.equal(got.box_index[0].cpu().long(), want[1])
        assert torch.equal(got.center_targets[0].cpu().view(torch.int32), want[2].view(torch.int32))


def test_c_abi_writes_nothing_outside_its_outputs(gpu):
    from mvsdet_amd import _lib, ops
    from mvsdet_amd.head import pad_ground_truth
    lib = _lib.load()
    levels = ((9, 7, 5), (5, 4, 3))
    c, r, k, v, origins, gts = R.batch(("five", "one"), (2501, 2502), levels, 3)
    B, L, C, P, PAD = 2, 2, 3, 9 * 7 * 5 + 5 * 4 * 3, 64
    dims = (ctypes.c_int * 6)(*[d for s in levels for d in s])
    geom = ops.detect_level_geometry(levels, origins).to(gpu)
    boxes, volumes, glabels, counts = pad_ground_truth(gts, gpu)
    G = int(boxes.shape[1])

    def canvas(n, dtype, fill):
        t = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=gpu)
        return t, t[PAD:PAD + n]

    sentinel = -12345.0
    cl, labels = canvas(B * P, torch.int64, -77)
    cb, box = canvas(B * P, torch.int32, -77)
    cc, center_t = canvas(B * P, torch.float32, sentinel)
    cx, bbox_t = canvas(B * P * 6, torch.float32, sentinel)
    cw, ws = canvas(int(lib.mvsdet_head_targets_workspace_bytes(B, G)), torch.uint8, 0x5a)
    stream = _lib.current_stream(gpu)
    _lib.check(lib.mvsdet_head_targets_f32(dims, _lib.ptr(geom), B, L, _lib.ptr(boxes), _lib.ptr(volumes), _lib.ptr(glabels),
                                           _lib.ptr(counts), G, 9, 4, _lib.ptr(labels), _lib.ptr(box), _lib.ptr(center_t),
                                           _lib.ptr(bbox_t), _lib.ptr(ws), ws.numel(), stream), "head_targets")
    want = [R.assign(levels, o, *R.gt_triplet(g), 9, 4) for o, g in zip(origins, gts)]
    assert torch.equal(labels.view(B, P).cpu(), torch.stack([w[0] for w in want]))
    assert torch.equal(bbox_t.view(B, P, 6).cpu().view(torch.int32), torch.stack([w[3] for w in want]).view(torch.int32))
    maps = [t.to(gpu).contiguous() for t in c + r + k]
    valid = v.to(gpu).float().contiguous()
    arr = ctypes.c_void_p * L
    ptrs = lambda ts: arr(*[t.data_ptr() for t in ts])  # noqa: E731
    cs, sums = canvas(B * 4, torch.float32, sentinel)
    cn, cnts = canvas(B * 2, torch.int32, -77)
    cw2, ws2 = canvas(int(lib.mvsdet_head_loss_workspace_bytes(B, P)), torch.uint8, 0x5a)
    _lib.check(lib.mvsdet_head_loss_f32(ptrs(maps[:L]), ptrs(maps[L:2 * L]), ptrs(maps[2 * L:]), dims, _lib.ptr(valid), _lib.ptr(geom),
                                        B, L, C, *levels[0], _lib.ptr(labels), _lib.ptr(center_t), _lib.ptr(bbox_t), 2.0, 0.25,
                                        _lib.ptr(sums), _lib.ptr(cnts), _lib.ptr(ws2), ws2.numel(), stream), "head_loss")
    grads = [canvas(m.numel(), torch.float32, sentinel) for m in maps]
    coef = torch.ones(B, 3, device=gpu)
    gp = lambda lo, hi: arr(*[g[1].data_ptr() for g in grads[lo:hi]])  # noqa: E731
    _lib.check(lib.mvsdet_head_loss_backward_f32(ptrs(maps[:L]), ptrs(maps[L:2 * L]), ptrs(maps[2 * L:]), dims, _lib.ptr(valid),
                                                 _lib.ptr(geom), B, L, C, *levels[0], _lib.ptr(labels), _lib.ptr(center_t),
                                                 _lib.ptr(bbox_t), 2.0, 0.25, _lib.ptr(coef), gp(0, L), gp(L, 2 * L), gp(2 * L, 3 * L),
                                                 stream), "head_loss_backward")
    torch.cuda.synchronize(gpu)
    for whole, fill in [(cl, -77), (cb, -77), (cc, sentinel), (cx, sentinel), (cs, sentinel), (cn, -77), (cw, 0x5a), (cw2, 0x5a)] + \
            [(g[0], sentinel) for g in grads]:
        assert bool((whole[:PAD] == fill).all()) and bool((whole[-PAD:] == fill).all())
    for g, _ in grads:
        assert not bool((g[PAD:-PAD] == sentinel).any())               # dense: every element of every map written
    assert not bool((sums == sentinel).any()) and int(cnts.view(B, 2)[:, 1].min()) >= 0


def test_no_host_synchronisation(gpu):
    gold = load_golden("g18_head_loss")
    c, r, k, v, origins, gts = _case(gold, "batch2", gpu)
    gts = [g.to(gpu) for g in gts]
    metas = R.metas_for(origins)
    head = _head()

    def step():
        maps = [t.detach().requires_grad_(True) for t in c + r + k]
        losses = head.loss_by_feat(maps[:3], maps[3:6], maps[6:], v, gts, metas)
        (losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]).backward()
        return losses, maps

    step()   # warm: library load, allocator, pinned buffers
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses, maps = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert float(losses["cls_loss"].detach()) > 0 and all(m.grad is not None for m in maps)


def test_two_runs_give_the_same_bits(gpu):
    gold = load_golden("g18_head_loss")
    c, r, k, v, origins, gts = _case(gold, "batch2", gpu)
    runs = []
    for _ in range(2):
        maps = [t.detach().clone().requires_grad_(True) for t in c + r + k]
        losses = _head().loss_by_feat(maps[:3], maps[3:6], maps[6:], v, gts, R.metas_for(origins))
        (losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]).backward()
        runs.append([losses[n].detach() for n in NAMES] + [m.grad for m in maps])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_under_autocast_the_loss_computes_in_float32(gpu):
    gold = load_golden("g18_head_loss")
    c, r, k, v, origins, gts = _case(gold, "one", gpu)
    head = _head()
    plain = head.loss_by_feat(c, r, k, v, gts, R.metas_for(origins))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        amp = head.loss_by_feat(c, r, k, v, gts, R.metas_for(origins))
    for n in NAMES:
        assert amp[n].dtype == torch.float32 and torch.equal(amp[n], plain[n])


def test_one_sgd_step_of_neck_and_head_and_ten_steps_falling(gpu):
    """IndoorImVoxelNeck + NerfDetHeadConvs on the HIP autograd route, loss_by_feat, backward: the parameter gradients against the
    same step with the restatement as the loss (torch's fp32 autograd on the same head maps) within G12b's bar for the bf16x3 route -- 1e-3 of each gradient tensor's scale element-wise, 1e-4 in norm -- and the
    summed loss falls over ten SGD steps."""
    from mvsdet_amd.head import NerfDetHeadConvs
    from mvsdet_amd.neck import IndoorImVoxelNeck
    torch.manual_seed(0)
    neck = IndoorImVoxelNeck(256, 128, [1, 1, 1]).train()   # the shipped neck and head at the ScanNet grid
    head = NerfDetHeadConvs(18, 3, 128, 6).train()
    head.init_weights()
    neck, head = neck.to(gpu), head.to(gpu)
    neck.autograd_route = head.autograd_route = "hip"
    levels = R.SCANNET_LEVELS
    *_, v, origins, gts = R.batch(("twelve",), (2602,), levels, 18)
    x = (0.5 * R._u((1, 256) + levels[0], 2603)).to(gpu)
    v, metas = v.to(gpu), R.metas_for(origins)
    params = [p for p in list(neck.parameters()) + list(head.parameters())]

    def total(losses):
        return losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]

    # ONE forward pass, both objectives on its head maps.  Two passes of the training-mode neck did not give the same maps on an
    # MI355X, and with the SAME loss their parameter gradients were 7e-2 of a tensor's scale apart on one layer
    # (down_layer_2.0.conv0), against 1e-5 between the two losses on one pass: only a shared pass compares the losses
    c, r, k = head(neck(x))
    ours = torch.autograd.grad(total(head.loss_by_feat(c, r, k, v, gts, metas)), params, retain_graph=True)
    restated, _ = R.loss_by_feat([t.cpu() for t in c], [t.cpu() for t in r], [t.cpu() for t in k], v.cpu(),
                                 [R.gt_triplet(g) for g in gts], origins)
    want = torch.autograd.grad(total(restated), params)
    for a, b in zip(ours, want):
        if float(b.abs().max()) == 0:   # the Scale of a level without a positive point
            assert not bool(a.any())
            continue
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())
        assert float((a - b).norm()) <= 1e-4 * float(b.norm())

    def run():
        for p in params:
            p.grad = None
        t = total(head.loss_by_feat(*head(neck(x)), v, gts, metas))
        t.backward()
        return float(t.detach())

    opt = torch.optim.SGD(params, lr=1e-3)
    totals = []
    for _ in range(10):
        totals.append(run())
        opt.step()
    assert totals[-1] < totals[0], totals
