"""csrc/assign.hip at its decisions and value edges: the scenes of tests/test_head_loss_edges_host.py (which proves, without a GPU,
that each one sits on the edge it claims) through the C entry points of the target assignment on a hand-built dyadic geometry, and
through ops.head_loss / ops.head_loss_rotated on hand-built targets.

Bars.  Assignment: labels, box index, centerness bits and box-target bits equal the restatement's, no tolerance (the kernel is the
reference's expression op for op).  Planted IoU pairs: 1e-6 absolute on the value and 1e-5 of the largest gradient component
against autograd through the restatements in float64 (exact inputs, a dozen float32 operations); an all-zero reference gradient
must be all zero.  Identical BEV rectangles are a degenerate pair of the vertex-gather restatement (shared edges: its gradient by
the BEV channels depends on the order of coincident vertices), so there the yardstick is the convention csrc/assign.hip's header
states, by autograd in float64 (H.shared_edges_reference: the value and the z channels are the restatement's, asserted in the host
module), with the same bars on all seven channels.  Saturated focal / BCE terms, per planted logit: float64 +- (4 x the float32
restatement's own deviation from float64 + 2 float32 ulp of the term); where 1 - p keeps fewer than 12 significant bits, between
the float64 evaluations of the formula at p and p -+ 2 ulp (where p + 2 ulp is clamped to 1, that end moved out by 2 float32 ulp:
the result is a float32, the end a float64 evaluation at p = 1); the class of a result (finite, inf, NaN) equals the float32
restatement's.  The tests print what they measure (run with -s); DESIGN.md 4.8 has the table.

Measured on an MI355X: targets bit for bit in all 24 cases; planted pairs at most 4.3e-8 on the value and 3.4e-7 of the largest
gradient component; the saturated terms track the float32 restatement (the kernel's deviation from float64 exceeds the
restatement's only below 3 ulp).  Two findings, fixed in csrc/assign.hip: a NaN class logit gave a finite focal term at gamma = 0
(0, 21.83, 87.34 at alpha 0, 0.25, 1 against NaN), and the centerness BCE of a confident logit was rounded to 0 (x = 30, target 1:
0 against 9.36e-14, 1.4e7 ulp of the term; x = 80: 0 against 1.8e-35)."""
import ctypes

import numpy as np
import pytest
import torch

import head_loss_restated as R
from head_loss_planted import plant
import test_head_loss_edges_host as H

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ assignment decisions
def _run_targets(gpu, case):
    """The case through mvsdet_head_targets[_rotated]_f32 with its hand-built geometry: host (labels, box, centerness, box targets)."""
    from mvsdet_amd import _lib
    lib = _lib.load()
    B, G, L = case.B, case.G, len(case.levels)
    P = sum(len(p) for p in case.points)
    w = 7 if case.rotated else 6
    dims = (ctypes.c_int * (3 * L))(*[d for s in case.levels for d in s])
    geom = case.geom.repeat(B, 1, 1).contiguous().to(gpu)
    boxes, volumes = case.boxes.contiguous().to(gpu), case.volumes.contiguous().to(gpu)
    glabels, counts = case.labels.contiguous().to(gpu), case.counts.to(gpu)
    labels = torch.full((B, P), -77, dtype=torch.int64, device=gpu)
    box = torch.full((B, P), -77, dtype=torch.int32, device=gpu)
    center_t = torch.full((B, P), -12345.0, device=gpu)
    bbox_t = torch.full((B, P, w), -12345.0, device=gpu)
    ws = torch.empty(int(lib.mvsdet_head_targets_workspace_bytes(B, G)), dtype=torch.uint8, device=gpu)
    tail = (_lib.ptr(volumes), _lib.ptr(glabels), _lib.ptr(counts), G, case.assign_thr, case.center_thr, _lib.ptr(labels), _lib.ptr(box),
            _lib.ptr(center_t), _lib.ptr(bbox_t), _lib.ptr(ws), ws.numel(), _lib.current_stream(gpu))
    if case.rotated:
        rot = case.rot.contiguous().to(gpu)
        rc = lib.mvsdet_head_targets_rotated_f32(dims, _lib.ptr(geom), B, L, _lib.ptr(boxes), _lib.ptr(rot), *tail)
    else:
        rc = lib.mvsdet_head_targets_f32(dims, _lib.ptr(geom), B, L, _lib.ptr(boxes), *tail)
    _lib.check(rc, "head_targets")
    torch.cuda.synchronize(gpu)
    return labels.cpu(), box.cpu().long(), center_t.cpu(), bbox_t.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def assigned(gpu):
    """Every case once: name -> the kernel's targets."""
    return {name: _run_targets(gpu, case) for name, case in H.CASES.items()}


@pytest.mark.parametrize("name", list(H.CASES))
def test_assignment_equals_the_restatement_bit_for_bit(assigned, name):
    case, got = H.CASES[name], assigned[name]
    for b in range(case.B):
        want = case.restated(b)
        assert torch.equal(got[0][b], want[0]), name
        assert torch.equal(got[1][b], want[1]), name
        assert torch.equal(_bits(got[2][b]), _bits(want[2])), name
        assert torch.equal(_bits(got[3][b]), _bits(want[3])), name


def test_a_face_moved_by_one_ulp_flips_exactly_its_plane(assigned):
    base = assigned["faces_base"][0][0] >= 0
    assert int(base.sum()) == 32
    for axis, side in H.MOVES:
        out, inn = assigned[f"face_{axis}{side}_out"][0][0] >= 0, assigned[f"face_{axis}{side}_in"][0][0] >= 0
        assert torch.equal(inn, base) and bool((out | ~base).all()) and int(out.sum()) - 32 in (8, 16)


def test_yaw_zero_on_the_rotated_route_equals_the_aligned_route(assigned):
    for a, r in (("pruning", "pruning_rotated_yaw0"), ("topk_boundary", "topk_boundary_rotated"), ("topk_all_stay", "topk_all_stay_rotated")):
        assert torch.equal(assigned[a][0], assigned[r][0]) and torch.equal(assigned[a][1], assigned[r][1])
    assert int((assigned["topk_above_points"][0] >= 0).sum()) == 32 > int((assigned["topk_above_points_rotated"][0] >= 0).sum()) > 0


def test_masked_volumes_padded_and_non_finite_rows_take_no_point(assigned):
    assert set(assigned["volume_mask"][1].unique().tolist()) == {-1, 4}
    pad = assigned["padded_rows"][1]
    assert set(pad[0].unique().tolist()) == {-1} and int(pad[1].max()) == 2 and set(pad[2].unique().tolist()) == {-1, 0}
    assert not bool((assigned["padded_rows"][0][0] >= 0).any())
    nf = assigned["non_finite_rows"][1][0]
    assert not any(g in H.NON_FINITE_BAD for g in nf.unique().tolist()) and int((nf >= 0).sum()) > 0
    assert bool((assigned["equal_volumes"][1][0][:256] <= 2).all())


# ------------------------------------------------------------------------------------------------ planted pairs
def _plant(gpu, d, target, weight=1.0):
    """One positive point (H.PLANT_INDEX of a 2x2x2 dyadic grid) with the predicted channels d (6: ops.head_loss, 7:
    ops.head_loss_rotated) against the target row: (loss sum / weight, its gradient by the point's channels)."""
    i = H.PLANT_INDEX
    geom = H.geometry(H.PLANT_LEVELS, H.PLANT_ORIGIN).view(1, 1, 6)
    assert H.points(H.PLANT_LEVELS, geom[0])[0][i].tolist() == list(H.PLANT_POINT)
    sums, g = plant(gpu, geom, i, d, target, weight)
    assert float(sums.weight_sum[0]) == weight
    return float(sums.bbox[0].detach()) / weight, g[:, i].double() / weight


def _compare(name, loss, grad, want_loss, want_grad):
    top = float(want_grad.abs().max())
    dev = float((grad - want_grad).abs().max())
    print(f"{name}: loss {loss:.9g} (float64 {want_loss:.9g}, off by {abs(loss - want_loss):.3g}); largest gradient component {top:.6g}, "
          f"gradient off by {dev:.3g} = {dev / top if top else 0:.3g} of it")
    assert abs(loss - want_loss) <= 1e-6, (name, loss, want_loss)
    assert dev <= 1e-5 * top, (name, grad.tolist(), want_grad.tolist())
    assert bool(torch.isfinite(grad).all())


@pytest.mark.parametrize("name", list(H.ALIGNED_PAIRS))
def test_aligned_iou_pairs_equal_autograd(gpu, name):
    """Before the tie routing followed ATen: identical boxes got the union's push without the overlap's pull (a non-zero gradient
    at loss 0), a tied corner lost the overlap's half, and touching boxes got no gradient at all."""
    corners, target, _, _ = H.ALIGNED_PAIRS[name]
    d = H.distances_to(corners)
    want_loss, want_grad, _ = H.aligned_reference(d, target)
    loss, grad = _plant(gpu, d, target, weight=0.5)
    _compare(name, loss, grad, want_loss, want_grad)


@pytest.mark.parametrize("bev", list(H.BEV_PAIRS))
@pytest.mark.parametrize("z", list(H.Z_PAIRS))
def test_rotated_iou_level_z_faces_equal_autograd(gpu, z, bev):
    """Identical BEV rectangles share all four edges, a degenerate pair of the vertex-gather restatement; there the yardstick is
    the convention csrc/assign.hip's header states (H.shared_edges_reference), all seven channels compared as everywhere."""
    d, t = H.rotated_pair(z, bev)
    want_loss, want_grad, _ = (H.shared_edges_reference if bev == "identical" else H.rotated_reference)(d, t)
    loss, grad = _plant(gpu, d, t, weight=0.5)
    _compare(f"{z} / {bev}", loss, grad, want_loss, want_grad)


# ------------------------------------------------------------------------------------------------ saturated terms
def _element_scene(gpu, positive, B=1):
    """One level of 32 points, C = 1: the planted class logits, the planted centre logits against their targets."""
    from mvsdet_amd import ops
    shape = (B, 1) + H.ELEMENT_LEVELS[0]
    cx, ct = H.center_maps()
    cls = H.class_logit_map().view(1, 1, 4, 4, 2).expand(shape).contiguous().to(gpu).requires_grad_(True)
    center = cx.view(1, 1, 4, 4, 2).expand(shape).contiguous().to(gpu).requires_grad_(True)
    bbox = torch.full((B, 6, 4, 4, 2), 0.375, device=gpu).requires_grad_(True)
    labels = torch.full((B, 32), 0 if positive else -1, dtype=torch.int64, device=gpu)
    geom = H.geometry(H.ELEMENT_LEVELS).view(1, 1, 6).repeat(B, 1, 1).to(gpu)
    bbox_t = torch.tensor([0.0, -3.0, 1.0, 3.0, 0.0, 3.0]).repeat(B, 32, 1).to(gpu)
    targets = ops.HeadTargets(labels, labels.int(), ct.repeat(B, 1).to(gpu), bbox_t, geom)
    return center, bbox, cls, targets


def _report(fails, what, x, got, bounds):
    lo, hi, f64, f32 = bounds
    got = got.double()
    u = torch.from_numpy(R.ulp(f64.float().nan_to_num(0.0, 0.0, 0.0).numpy())).double()
    for j in range(len(x)):
        ours, rest = float((got[j] - f64[j]).abs() / u[j]), float((f32[j] - f64[j]).abs() / u[j])
        print(f"{what} x={float(x[j]):g}: kernel {float(got[j]):.9g} float64 {float(f64[j]):.9g} float32 {float(f32[j]):.9g}; off by "
              f"{ours:.3g} ulp (float32 restatement {rest:.3g} ulp), allowed [{float(lo[j]):.9g}, {float(hi[j]):.9g}]")
        if int(H.kind(got[j])) != int(H.kind(f32[j])):
            fails.append((what, float(x[j]), "class", float(got[j]), float(f32[j])))
        elif int(H.kind(f64[j])) == 0 and not (float(lo[j]) <= float(got[j]) <= float(hi[j])):
            fails.append((what, float(x[j]), float(got[j]), float(lo[j]), float(hi[j])))


@pytest.mark.parametrize("positive", [True, False])
def test_saturated_focal_terms_per_element(gpu, positive):
    from mvsdet_amd import ops
    x = H.class_logit_map()[:len(H.CLASS_LOGITS)]
    n = len(x)
    onehot = torch.eye(32, device=gpu).view(32, 1, 1, 4, 4, 2)
    fails = []
    for gamma in H.GAMMAS:
        for alpha in H.ALPHAS:
            center, bbox, cls, targets = _element_scene(gpu, positive)
            with torch.no_grad():   # the forward kernels return sums: a valid mask of one voxel per launch isolates an element
                terms = torch.stack([ops.head_loss([center], [bbox], [cls], onehot[j], targets, gamma, alpha).cls[0] for j in range(32)])
            dense = ops.head_loss([center], [bbox], [cls], torch.ones(1, 1, 4, 4, 2, device=gpu), targets, gamma, alpha)
            dense.cls.sum().backward()
            tag = f"{'positive' if positive else 'background'} gamma={gamma} alpha={alpha}"
            _report(fails, f"focal term {tag}", x, terms.cpu()[:n], [b[:n] for b in H.focal_bounds(H.class_logit_map(), positive, gamma, alpha)])
            _report(fails, f"focal gradient {tag}", x, cls.grad.view(32).cpu()[:n],
                    [b[:n] for b in H.focal_bounds(H.class_logit_map(), positive, gamma, alpha, grad=True)])
    assert not fails, "\n".join(str(f) for f in fails)


def test_saturated_centerness_bce_per_element(gpu):
    from mvsdet_amd import ops
    cx, ct = H.center_maps()
    center, bbox, cls, targets = _element_scene(gpu, True)
    onehot = torch.eye(32, device=gpu).view(32, 1, 1, 4, 4, 2)
    with torch.no_grad():
        terms = torch.stack([ops.head_loss([center], [bbox], [cls], onehot[j], targets).center[0] for j in range(32)])
    ops.head_loss([center], [bbox], [cls], torch.ones(1, 1, 4, 4, 2, device=gpu), targets).center.sum().backward()
    value, grad = H.bce_bounds(cx, ct)
    fails = []
    tagged = torch.tensor([float(a) for a in cx])
    for j in range(32):
        print(f"pair {j}: logit {float(cx[j]):g} target {float(ct[j]):g}")
    _report(fails, "bce", tagged, terms.cpu(), value)
    _report(fails, "bce gradient", tagged, center.grad.view(32).cpu(), grad)
    assert not fails, "\n".join(str(f) for f in fails)


def test_gradient_maps_scale_exactly_with_the_coefficients(gpu):
    """Distinct coefficients per scene and per loss, a zero row among them: every gradient map is the unit-coefficient run's times
    the coefficient in float32, the same float32 value (NaN where that is NaN; a point taking no part is +0 whatever the sign).
    The box gradient is scaled by (coef * weight) in one factor, so its coefficients are powers of two, for which the order of the
    two multiplications cannot show."""
    from mvsdet_amd import ops
    coef = torch.tensor([[0.5, -2.0, 3.0], [-1.5, 0.25, 7.0], [0.0, 0.0, 0.0], [3.0, 0.5, -2.0]])
    runs = []
    for w in (torch.ones(4, 3), coef):
        center, bbox, cls, targets = _element_scene(gpu, True, B=4)
        labels = targets.labels.clone()
        labels[:, 16:] = -1
        targets = targets._replace(labels=labels, box_index=labels.int())
        sums = ops.head_loss([center], [bbox], [cls], torch.ones(4, 1, 4, 4, 2, device=gpu), targets)
        w = w.to(gpu)
        (sums.center * w[:, 0] + sums.bbox * w[:, 1] + sums.cls * w[:, 2]).sum().backward()
        runs.append([t.grad.cpu() for t in (center, bbox, cls)])
    for k, (unit, scaled) in enumerate(zip(*runs)):
        want = unit * coef[:, k].view(4, 1, 1, 1, 1)
        assert torch.equal(torch.isnan(want), torch.isnan(scaled))
        ok = ~torch.isnan(want)
        assert torch.equal(want[ok], scaled[ok]), k         # value for value; a point that takes no part is a plain +0, not coef * 0
        assert float(unit[ok].abs().max()) > 0
    assert not bool(runs[1][0][2].any()) and not bool(runs[1][1][2].any())     # the zero row


# ------------------------------------------------------------------------------------------------ valid mask
def test_valid_mask_rounds_half_to_even(gpu):
    from mvsdet_amd import ops
    v = H.valid_counts()
    want = R.upsampled_valid(v, H.VALID_LEVELS, 0)
    L = len(H.VALID_LEVELS)
    P = int(want.numel())
    mk = lambda c, val: [torch.full((1, c) + s, val, device=gpu).requires_grad_(True) for s in H.VALID_LEVELS]  # noqa: E731
    center, bbox, cls = mk(1, 0.0), mk(6, 0.5), mk(1, 0.0)
    labels = torch.full((1, P), -1, dtype=torch.int64, device=gpu)
    geom = H.geometry(H.VALID_LEVELS).view(1, L, 6).to(gpu)
    targets = ops.HeadTargets(labels, labels.int(), torch.zeros(1, P, device=gpu), torch.zeros(1, P, 6, device=gpu), geom)
    sums = ops.head_loss(center, bbox, cls, v.to(gpu), targets)
    assert int(sums.n_valid[0]) == int(want.sum()) and int(sums.n_pos[0]) == 0
    sums.cls.sum().backward()
    got = torch.cat([c.grad.reshape(-1) for c in cls]).cpu() != 0
    assert torch.equal(got, want)
