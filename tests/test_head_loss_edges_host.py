"""The planted scenes of tests/test_gpu_head_loss_edges.py and, for every one, the proof FROM THE RESTATEMENTS ALONE that it sits on
the edge it claims: a face distance that is 0 exactly, n[l] == pts_assign_threshold, n[best] == k, corners that tie bit for bit,
1 - sigmoid(x) == 0.  The GPU module imports the scenes from here, so the two cannot drift apart.  No GPU is needed here.

Exact arithmetic: voxel sizes 0.25 * 2^level, new origins multiples of 0.25, box centres and sizes multiples of 1/64 (1/512 for the
pair under the union's floor, which needs volumes below 1e-6), so that every face distance, corner and overlap is exact in float32
and in float64 and a tie in the kernel is a tie in the yardstick.  The assignment runs on a hand-built (B, L, 6) geometry handed to
the C entry points; the restatements take the same points through their `points` argument.

What the restatement does with non-finite live rows (asserted in test_non_finite_rows_take_nothing): a NaN centre or size makes
every face distance NaN, and NaN > 0 is false, so the box holds no point on any level; a +inf size makes every face distance +inf,
so the box holds every point, its centerness is inf / inf = NaN, the top-k boundary is NaN and no centerness is above a NaN.  All
three cases are expressible; none was dropped."""
import math

import numpy as np
import pytest
import torch

import head_loss_arkit_restated as A
import head_loss_restated as R
import rotated_iou_restated as RI

LEVELS2 = ((8, 8, 4), (4, 4, 2))
LEVELS4 = ((8, 8, 4), (4, 4, 2), (2, 2, 1), (1, 1, 1))   # ops.DETECT_MAX_LEVELS levels
ORIGIN = (0.5, -2.5, 1.5)                                # x 0.5 .. 2.25, y -2.5 .. -0.75, z 1.5 .. 2.25 at level 0
NAN, INF = float("nan"), float("inf")


def geometry(levels, origin=ORIGIN):
    """(L, 6) float32: voxel size 0.25 * 2^level and the new origin of every level."""
    return torch.tensor([[0.25 * 2 ** l] * 3 + list(origin) for l in range(len(levels))], dtype=torch.float32)


def points(levels, geom):
    """The levels' (N, 3) points as grid_point computes them: voxel * voxel size, rounded, + new origin, rounded."""
    out = []
    for s, g in zip(levels, geom):
        grid = torch.stack(torch.meshgrid([torch.arange(int(n)) for n in s], indexing="ij")).reshape(3, -1).t().float()
        out.append(grid * g[:3] + g[3:])
    return out


def box(lo, hi, yaw=None):
    """The (centre, size) row of the box with faces lo, hi; both must be exact in float32, or the faces would not be where asked."""
    row = [(a + b) / 2 for a, b in zip(lo, hi)] + [b - a for a, b in zip(lo, hi)]
    for v, a, b in zip(row[:3], lo, hi):
        d = b - a
        assert float(np.float32(v)) == v and float(np.float32(d)) == d, (lo, hi)
        assert float(np.float32(v) + np.float32(d) / np.float32(2)) == b and float(np.float32(v) - np.float32(d) / np.float32(2)) == a
    return row + ([] if yaw is None else [yaw])


def moved(lo, hi, axis, side, outward):
    """The faces with one of them moved by one float32 nextafter, away from the box (outward) or into it."""
    lo, hi = list(lo), list(hi)
    f = np.float32(hi[axis] if side else lo[axis])
    to = np.float32(INF if (side == 1) == outward else -INF)
    (hi if side else lo)[axis] = float(np.nextafter(f, to))
    return lo, hi


class Case:
    """A batch for the assignment: boxes per scene (rows of 6, or of 7 with yaw: the rotated route), padded to G rows."""

    def __init__(self, name, levels, scenes, assign_thr, center_thr, origin=ORIGIN, volumes=None, counts=None, rot=None):
        self.name, self.levels, self.assign_thr, self.center_thr = name, levels, assign_thr, center_thr
        self.geom = geometry(levels, origin)
        self.points = points(levels, self.geom)
        self.boxes = torch.tensor(scenes, dtype=torch.float32)              # (B, G, 6 | 7)
        self.B, self.G, width = self.boxes.shape
        self.rotated = width == 7
        b = self.boxes
        self.volumes = (b[..., 3] * b[..., 4] * b[..., 5]) if volumes is None else torch.tensor(volumes, dtype=torch.float32)
        self.labels = (torch.arange(self.G) % 3 + 1).repeat(self.B, 1)
        self.counts = torch.tensor([self.G] * self.B if counts is None else counts, dtype=torch.int32)
        if self.rotated:
            self.rot = torch.stack((torch.cos(b[..., 6]), torch.sin(b[..., 6])), dim=-1) if rot is None \
                else torch.tensor(rot, dtype=torch.float32)

    def restated(self, b, rows=None, details=False):
        """The restatement's targets of scene b from its live rows (or from `rows` of them)."""
        rows = list(range(int(self.counts[b]))) if rows is None else rows
        args = (self.levels, None, self.boxes[b][rows], self.volumes[b][rows], self.labels[b][rows], self.assign_thr, self.center_thr)
        if self.rotated:
            return A.assign(*args, details=details, points=self.points, rot=self.rot[b][rows])
        return R.assign(*args, details=details, points=self.points)

    def as_rotated(self, name):
        """The same boxes on the rotated route at yaw 0, (cos, sin) = (1, 0)."""
        rows = torch.cat((self.boxes, torch.zeros(self.B, self.G, 1)), dim=-1).tolist()
        return Case(name, self.levels, rows, self.assign_thr, self.center_thr, tuple(self.geom[0, 3:].tolist()),
                    self.volumes.tolist(), self.counts.tolist())


BASE_LO, BASE_HI = (1.0, -2.25, 1.5), (2.25, -1.0, 2.25)     # all six faces on grid planes: 32 points of level 0 inside, 4 of level 1
BASE = box(BASE_LO, BASE_HI)
WHOLE = box((-0.5, -3.5, 0.5), (3.5, 0.5, 3.5))               # holds every point of every level
MOVES = ((0, 1), (1, 0), (2, 1))                              # (axis, side): the faces whose centre lies a binade below the face
ALL_STAY = 400                                                # a pts_center_threshold above every count: no top-k cut


def _shift(row, by):
    return [row[i] + by[i] for i in range(3)] + row[3:]


def _cases():
    cs = [Case("faces_base", LEVELS2, [[BASE]], 5, ALL_STAY)]
    for axis, side in MOVES:
        for outward in (True, False):
            cs.append(Case(f"face_{axis}{side}_{'out' if outward else 'in'}", LEVELS2, [[box(*moved(BASE_LO, BASE_HI, axis, side, outward))]],
                           5, ALL_STAY))
    # n[1] == 4 == threshold (best = L - 1: no level below), n[1] == 3 (best 0), n[0] == 3 (the first level is below: max(-1, 0)),
    # n[0] == 4 with n[1] == 2
    cs.append(Case("assign_thr_l2", LEVELS2, [[BASE, box((0.75, -2.25, 1.75), (2.25, -1.75, 2.25)),
                                                box((0.75, -1.5625, 1.9375), (1.75, -1.4375, 2.0625)),
                                                box((0.75, -1.5625, 1.9375), (2.0, -1.4375, 2.0625))]], 4, ALL_STAY))
    # four levels: n[2] == 2 == threshold with n[3] == 1 (best 2), n[2] == 1 (best 1)
    cs.append(Case("assign_thr_l4", LEVELS4, [[box((0.25, -2.75, 1.25), (2.0, -2.0, 2.5)), box((0.25, -2.75, 1.25), (1.0, -2.0, 2.5))]],
                   2, ALL_STAY))
    cs.append(Case("topk_boundary", LEVELS2, [[BASE]], 5, 31))        # n[best] == 32 == pts_center_threshold + 1
    cs.append(Case("topk_all_stay", LEVELS2, [[BASE]], 5, 32))        # n[best] == 32 == pts_center_threshold
    cs.append(cs[-2].as_rotated("topk_boundary_rotated"))
    cs.append(cs[-2].as_rotated("topk_all_stay_rotated"))
    one = ((4, 4, 2),)
    cs.append(Case("topk_above_points", one, [[WHOLE]], 0, 40))       # 41 > P == 32 == n[best]: the aligned route keeps them all
    cs.append(cs[-1].as_rotated("topk_above_points_rotated"))         # the rotated route takes min(41, P) = 32: the smallest are out
    gx, gy, gz = 1.375, -1.625, 1.875                                 # the grid's middle
    out = [box((gx + s * 2.0 - 0.25, gy - 0.25, gz - 0.25), (gx + s * 2.0 + 0.25, gy + 0.25, gz + 0.25)) for s in (-1, 1)] + \
          [box((gx - 0.25, gy + s * 2.0 - 0.25, gz - 0.25), (gx + 0.25, gy + s * 2.0 + 0.25, gz + 0.25)) for s in (-1, 1)] + \
          [box((gx - 0.25, gy - 0.25, gz + s * 2.0 - 0.25), (gx + 0.25, gy + 0.25, gz + s * 2.0 + 0.25)) for s in (-1, 1)]
    past = [box((2.3125, -2.0, 1.625), (2.6875, -1.0, 2.125)), box((1.0, -2.9375, 1.625), (2.0, -2.5625, 2.125))]   # one voxel past the border
    straddle = [box((1.875, -1.375, 1.625), (2.875, -0.375, 2.625)), box((0.0, -3.0, 1.0), (0.875, -2.125, 1.875))]
    odd = [[gx, gy, gz, 64.0, 64.0, 64.0], [1.25, gy, gz, 0.0, 1.0, 0.5], [1.25, -1.5, 2.0, 0.0, 0.0, 0.0], [gx, gy, gz, 1.0, -0.5, 0.5]]
    cs.append(Case("pruning", LEVELS2, [out + past + straddle + odd + [BASE]], 4, 8))
    cs.append(cs[-1].as_rotated("pruning_rotated_yaw0"))
    far = (4096.5, -4098.5, 4097.5)
    by = [far[i] - ORIGIN[i] for i in range(3)]
    cs.append(Case("coarse_origin", LEVELS2, [[_shift(BASE, by), _shift(straddle[0], by), _shift(past[0], by)]], 4, 8, origin=far))
    q = float(np.float32(math.pi / 4))
    cs.append(Case("thin_rotated", LEVELS2, [[[gx, gy, gz, 1.5, 0.25, 0.5, q], [2.25, -1.0, 2.0, 3.0, 0.25, 0.5, q],
                                               [gx, gy, gz, 1.0, 0.75, 0.75, 0.5]]], 2, 3))
    h, p = float(np.float32(math.pi / 2)), float(np.float32(math.pi))
    cs.append(Case("quarter_turns", LEVELS2, [[[gx, gy, gz, 1.25, 0.75, 0.75, h], [1.5, -1.5, 1.875, 0.75, 1.25, 0.5, p]]], 4, 8,
                   rot=[[[0.0, 1.0], [-1.0, 0.0]]]))
    three = [box((0.75, -2.25, 1.5), (1.75, -1.25, 2.5)), box((1.0, -2.0, 1.5), (2.0, -1.0, 2.5)), box((1.25, -2.25, 1.5), (2.25, -1.25, 2.5))]
    cs.append(Case("equal_volumes", LEVELS2, [[three[2], three[0], three[1]]], 9, ALL_STAY, volumes=[[2.0, 2.0, 2.0]]))
    big = float(np.nextafter(np.float32(1e8), np.float32(INF)))
    cs.append(Case("volume_mask", LEVELS2, [[BASE, BASE, BASE, BASE, box((1.5, -2.25, 1.5), (2.5, -1.5, 2.5))]], 9, ALL_STAY,
                   volumes=[[1e8, big, INF, NAN, 0.75]]))
    junk = [gx, gy, gz, 64.0, 64.0, 64.0]
    nanrow = [NAN] * 6
    # the first scene has no box, the second G of them, the third one live row before its padding
    cs.append(Case("padded_rows", LEVELS2, [[junk, nanrow, junk], [three[0], BASE, three[1]], [BASE, nanrow, junk]], 4, 8,
                   volumes=[[1e-9, NAN, 1e-9], [1.0, 0.5, 1.0], [1.0, NAN, 1e-9]], counts=[0, 3, 1]))
    bad = [[NAN, gy, gz, 1.0, 1.0, 1.0], [gx, gy, gz, 1.0, NAN, 1.0], [gx, gy, gz, INF, INF, INF]]
    cs.append(Case("non_finite_rows", LEVELS2, [[three[0], bad[0], BASE, bad[1], bad[2], three[1]]], 4, 8,
                   volumes=[[1.0, 0.25, 0.5, 0.25, 0.25, 1.0]]))
    return cs


CASES = {c.name: c for c in _cases()}
NON_FINITE_BAD = (1, 3, 4)


def _n_best(case, g, b=0):
    n, best, t, c = case.restated(b, details=True)[4][g][:4]
    return n, best, t, c


def _inside0(case):
    """The level-0 points the scene's only box takes (no top-k cut, level 0 the best)."""
    labels = case.restated(0)[0]
    return labels[:len(case.points[0])] >= 0


# ------------------------------------------------------------------------------------------------ assignment premises
def test_every_case_is_dyadic():
    for c in CASES.values():
        assert bool(((c.geom * 4) == (c.geom * 4).round()).all())
        live = torch.cat([c.boxes[b, :int(c.counts[b]), :6] for b in range(c.B)])
        fin = live[torch.isfinite(live)]
        assert bool(((fin * 64) == (fin * 64).round()).all()) or c.name.startswith("face_")     # the nextafter faces are not


def test_faces_on_grid_planes():
    base = CASES["faces_base"]
    d = R.face_distances(base.points[0], base.boxes[0, 0])
    for q in range(6):
        assert int((d[:, q] == 0).sum()) > 0                    # every face passes through grid points: distance 0 exactly
    inside = _inside0(base)
    assert int(inside.sum()) == 32 and not bool(inside[(d == 0).any(-1)].any())      # strict > 0: they are outside
    for axis, side in MOVES:
        plane = (d[:, 2 * axis + side] == 0) & (torch.cat((d[:, :2 * axis + side], d[:, 2 * axis + side + 1:]), 1).min(-1)[0] > 0)
        assert int(plane.sum()) in (8, 16)
        assert torch.equal(_inside0(CASES[f"face_{axis}{side}_out"]), inside | plane)     # exactly that plane's points flip
        assert torch.equal(_inside0(CASES[f"face_{axis}{side}_in"]), inside)


def test_assign_threshold_boundaries():
    c = CASES["assign_thr_l2"]
    ns = [_n_best(c, g)[:2] for g in range(4)]
    assert ns[0] == ([32, 4], 1) and ns[0][0][1] == c.assign_thr                      # no level is below: best = L - 1
    assert ns[1][0][1] == c.assign_thr - 1 and ns[1][0][0] >= c.assign_thr and ns[1][1] == 0
    assert ns[2][0][0] == c.assign_thr - 1 and ns[2][1] == 0                          # the first level is below: max(0 - 1, 0)
    assert ns[3][0][0] == c.assign_thr and ns[3][0][1] < c.assign_thr and ns[3][1] == 0
    assert c.G == 4
    c = CASES["assign_thr_l4"]
    (n0, b0), (n1, b1) = (_n_best(c, g)[:2] for g in range(2))
    assert n0[2] == c.assign_thr and n0[3] == 1 and b0 == 2 and min(n0[:2]) >= c.assign_thr
    assert n1[2] == c.assign_thr - 1 and b1 == 1 and min(n1[:2]) >= c.assign_thr


def test_topk_boundaries():
    for name in ("topk_boundary", "topk_boundary_rotated"):
        c = CASES[name]
        n, best, t, cn = _n_best(c, 0)
        assert n[best] == c.center_thr + 1 == 32 and t == float(cn.min())            # the smallest candidates are the boundary
        assert int((cn == t).sum()) == 8                                             # and tie eight ways: all of them are out
        assert int((c.restated(0)[0] >= 0).sum()) == 24
    for name in ("topk_all_stay", "topk_all_stay_rotated"):
        c = CASES[name]
        n, best, t, cn = _n_best(c, 0)
        assert n[best] == c.center_thr == 32 and t == -1.0 and int((c.restated(0)[0] >= 0).sum()) == 32
    c, r = CASES["topk_above_points"], CASES["topk_above_points_rotated"]
    assert c.center_thr + 1 > 32 == _n_best(c, 0)[0][0] and _n_best(c, 0)[2] == -1.0 and int((c.restated(0)[0] >= 0).sum()) == 32
    n, best, t, cn = _n_best(r, 0)
    assert n[best] == 32 and t == float(cn.min()) and 0 < int((r.restated(0)[0] >= 0).sum()) < 32     # min(.., P) decides


def test_pruning_scene_and_yaw0():
    c = CASES["pruning"]
    ns = [_n_best(c, g)[0] for g in range(c.G)]
    assert all(n == [0, 0] for n in ns[:8])                       # outside on six sides, one voxel past two borders
    assert ns[8][0] > 0 and ns[9][0] > 0                          # straddling the border
    assert ns[10] == [256, 32]                                    # the whole grid several times over
    assert ns[11] == ns[12] == ns[13] == [0, 0]                   # zero size on one axis, on all (AT a grid point), negative size
    assert bool((R.face_distances(c.points[0], c.boxes[0, 12]) == 0).all(-1).any())
    assert ns[14] == [32, 4]
    r = CASES["pruning_rotated_yaw0"]
    a, b = c.restated(0), r.restated(0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int((a[0] >= 0).sum()) > 0
    f = CASES["coarse_origin"]
    assert [_n_best(f, g)[0] for g in range(3)] == [ns[14], ns[8], ns[6]]             # the same counts 4096 m away
    assert float(torch.cat(f.points).abs().min()) > 4096
    d = R.face_distances(f.points[0], f.boxes[0, 0])
    assert all(int((d[:, q] == 0).sum()) > 0 for q in range(6))


def test_rotated_footprints_and_quarter_turns():
    c = CASES["thin_rotated"]
    ex = c.rot[0, :, 0].abs() * c.boxes[0, :, 3] + c.rot[0, :, 1].abs() * c.boxes[0, :, 4]
    assert float(ex[0]) > 4 * 0.25 and float(ex[0]) < 2.0         # the hull is far wider than the box and fits the 2 m grid
    assert float(c.boxes[0, 1, 0] + ex[1] / 2) > 2.25 + 0.5       # the second is clipped by the border
    ns = [_n_best(c, g)[0] for g in range(3)]
    assert all(0 < n[0] < 60 for n in ns) and int((c.restated(0)[0] >= 0).sum()) > 0
    qt = CASES["quarter_turns"]
    assert qt.rot.tolist() == [[[0.0, 1.0], [-1.0, 0.0]]]
    d = A.face_distances(qt.points[0], qt.boxes[0, 0], qt.rot[0, 0])
    assert int((d == 0).any(-1).sum()) > 0 and int((qt.restated(0)[0] >= 0).sum()) > 0          # faces on grid planes, exactly


def test_volume_rules():
    c = CASES["equal_volumes"]
    labels, arg, *_ = c.restated(0)
    ins = [R.face_distances(torch.cat(c.points), c.boxes[0, g]).min(-1)[0] > 0 for g in range(3)]
    all3 = ins[0] & ins[1] & ins[2] & (torch.arange(len(arg)) < 256)
    assert int(all3.sum()) > 0 and bool((arg[all3] == 0).all()) and bool((arg[ins[1] & ins[2] & ~ins[0] & (arg >= 0)] == 1).all())
    c = CASES["volume_mask"]
    assert float(c.volumes[0, 0]) == 1e8 and float(c.volumes[0, 1]) > 1e8
    labels, arg, *_ = c.restated(0)
    assert set(arg.tolist()) == {-1, 4}
    only = (R.face_distances(torch.cat(c.points), c.boxes[0, 0]).min(-1)[0] > 0) & (arg < 0)
    assert int(only.sum()) > 0                                    # points inside the four masked boxes alone keep -1


def test_padded_rows_show_nowhere():
    c = CASES["padded_rows"]
    assert c.counts.tolist() == [0, c.G, 1] and c.G == 3
    assert int((c.restated(0)[0] >= 0).sum()) == 0
    assert int(c.restated(1)[1].max()) == 2 and set(c.restated(2)[1].tolist()) == {-1, 0}
    pts = torch.cat(c.points)
    for b, g in ((0, 0), (0, 2), (2, 2)):                           # a padded tiny-volume box that holds the whole grid
        assert bool((R.face_distances(pts, c.boxes[b, g]).min(-1)[0] > 0).all()) and float(c.volumes[b, g]) < float(c.volumes[2, 0])


def test_non_finite_rows_take_nothing():
    c = CASES["non_finite_rows"]
    pts = torch.cat(c.points)
    assert not bool((R.face_distances(pts, c.boxes[0, 1]).min(-1)[0] > 0).any())     # NaN centre: never inside
    assert not bool((R.face_distances(pts, c.boxes[0, 3]).min(-1)[0] > 0).any())     # NaN size: never inside
    d = R.face_distances(pts, c.boxes[0, 4])
    assert bool((d.min(-1)[0] > 0).all()) and bool(torch.isnan(R.centerness_of(d)).all())   # +inf size: inside everywhere, inf / inf
    n, best, t, cn = _n_best(c, 4)
    assert math.isnan(t) and not bool((cn > t).any())
    full = c.restated(0)
    good = [g for g in range(c.G) if g not in NON_FINITE_BAD]
    clean = c.restated(0, rows=good)
    assert not any(g in NON_FINITE_BAD for g in full[1].tolist())
    remap = torch.tensor(good + [-1])
    assert torch.equal(full[1], remap[clean[1]]) and int((full[1] >= 0).sum()) > 0
    for a, b in zip(full[2:4], clean[2:4]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------- planted pairs, aligned IoU
PLANT_LEVELS = ((2, 2, 2),)
PLANT_ORIGIN = (1.0, 0.0, 0.25)
PLANT_INDEX = 5                                                  # voxel (1, 0, 1): the point (1.25, 0.0, 0.5)
PLANT_POINT = (1.25, 0.0, 0.5)
T6 = (1.0, -0.5, 0.25, 2.0, 0.5, 0.75)
S, H = 1 / 256, 1 / 512
# name: (predicted corners, target corners, tied corners, axes with rb - lt == 0)
ALIGNED_PAIRS = {
    "generic": ((0.75, -0.25, 0.125, 1.75, 1.0, 0.625), T6, 0, 0),
    "pred_inside": ((1.125, -0.375, 0.375, 1.5, 0.25, 0.625), T6, 0, 0),
    "target_inside": ((0.5, -1.0, 0.0, 2.5, 1.0, 1.0), T6, 0, 0),
    "disjoint_x": ((2.5, -0.25, 0.125, 3.0, 1.0, 0.625), T6, 0, 0),
    "identical": (T6, T6, 6, 0),
    "one_corner": ((1.0, -0.25, 0.125, 1.75, 1.0, 0.625), T6, 1, 0),
    "two_corners": ((1.0, -0.25, 0.125, 1.75, 0.5, 0.625), T6, 2, 0),
    "three_corners": ((1.0, -0.25, 0.25, 1.75, 0.5, 0.625), T6, 3, 0),
    "touch_face": ((0.5, -0.25, 0.125, 1.0, 1.0, 0.625), T6, 0, 1),
    "touch_edge": ((0.5, 0.5, 0.125, 1.0, 1.0, 0.625), T6, 0, 2),
    "negative_extent": ((1.5, -0.25, 0.125, 1.25, 1.0, 0.625), T6, 0, 0),
    "under_the_floor": ((1.25, 0.0, 0.5, 1.25 + S, S, 0.5 + S), (1.25 + H, H, 0.5 + H, 1.25 + S + H, S + H, 0.5 + S + H), 0, 0),
}


def distances_to(corners, point=PLANT_POINT):
    """The six predicted distances whose decoded box (_bbox_pred_to_bbox) has these corners, float32."""
    a, p = corners, point
    return torch.tensor([p[0] - a[0], a[3] - p[0], p[1] - a[1], a[4] - p[1], p[2] - a[2], a[5] - p[2]], dtype=torch.float32)


def aligned_reference(d, target, point=PLANT_POINT):
    """(1 - IoU, its gradient by the six distances) by autograd through head_loss_restated.aligned_iou in float64."""
    x = d.double().clone().requires_grad_(True)
    p = torch.tensor(point, dtype=torch.float64)
    pred = torch.stack((p[0] - x[0], p[1] - x[2], p[2] - x[4], p[0] + x[1], p[1] + x[3], p[2] + x[5])).view(1, 6)
    loss = (1 - R.aligned_iou(pred, torch.tensor([target], dtype=torch.float32).double())).sum()
    loss.backward()
    return float(loss.detach()), x.grad.clone(), pred.detach()[0]


@pytest.mark.parametrize("name", list(ALIGNED_PAIRS))
def test_aligned_pairs_sit_where_they_claim(name):
    corners, target, ties, touches = ALIGNED_PAIRS[name]
    d = distances_to(corners)
    p32 = torch.tensor(PLANT_POINT)
    pred32 = torch.stack((p32[0] - d[0], p32[1] - d[2], p32[2] - d[4], p32[0] + d[1], p32[1] + d[3], p32[2] + d[5]))
    loss, grad, pred = aligned_reference(d, target)
    t = torch.tensor(target, dtype=torch.float32).double()
    assert torch.equal(pred32.double(), pred) and torch.equal(pred, torch.tensor(corners, dtype=torch.float64))   # exact in float32
    assert int((pred == t).sum()) == ties
    gap = torch.min(pred[3:], t[3:]) - torch.max(pred[:3], t[:3])
    assert int((gap == 0).sum()) == touches
    vol = lambda b: float((b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]))  # noqa: E731
    un0 = vol(pred) + vol(t) - float(gap.clamp(min=0).prod())
    if name == "under_the_floor":
        assert 0 < un0 < 0.5e-6 and float(gap.min()) > 0 and abs(loss - (1 - H ** 3 / 1e-6)) < 1e-9
    else:
        assert un0 > 1e-3
    if name == "negative_extent":
        assert float(d[0] + d[1]) < 0
    if name in ("disjoint_x", "negative_extent"):
        assert loss == 1.0 and not bool(grad.any())
    if name in ("identical", "touch_edge"):
        # identical boxes: the halves of the overlap's pull cancel the union's push exactly; an edge: two factors of the overlap are 0
        assert not bool(grad.any())
    elif ties or touches:
        assert bool(grad.any()) and math.isfinite(loss)


def test_ties_split_in_halves_and_touches_pull():
    """ATen's rules, from autograd itself: identical boxes pull with half the overlap's gradient on all six corners (the union's
    part cancels it to exactly zero loss gradient only where IoU' = 0, which it is not), and touching boxes are drawn together."""
    _, g, _ = aligned_reference(distances_to(T6), T6)
    # d iou / d a_hi = (1/un + ov/un^2) * 0.5 * oth - ov/un^2 * oth with ov == un == V: (2/V) * 0.5 * oth - oth / V = 0
    assert float(g.abs().max()) == 0.0
    _, g, _ = aligned_reference(distances_to(ALIGNED_PAIRS["touch_face"][0]), T6)
    assert float(g[1]) < 0 and not bool(g[[0, 2, 3, 4, 5]].any())          # only the touching face is pulled, towards the target
    x = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    torch.max(x, torch.zeros(1, dtype=torch.float64)).sum().backward()
    assert float(x.grad) == 0.5
    y = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    y.clamp(min=0).sum().backward()
    assert float(y.grad) == 1.0


# ------------------------------------------------------------------------------------------- planted pairs, rotated IoU
# name: (d4, d5 of the prediction, the target's centre z); the target is 0.5 high, the point's z is 0.5
Z_PAIRS = {"tops_level": (0.125, 0.25, 0.5), "bottoms_level": (0.25, 0.125, 0.5), "both_level": (0.25, 0.25, 0.5),
           "touching": (0.25, 0.5, 1.25)}
BEV_PAIRS = {"generic": ((0.5, 0.375, 0.25, 0.5, 0.5), (1.3125, 0.0625, 1.0, 0.75, -0.25)),
             "identical": ((0.5, 0.5, 0.375, 0.375, 0.0), (1.25, 0.0, 1.0, 0.75, 0.0))}


def rotated_pair(zname, bevname):
    """(the seven predicted channels, the target row (7,)), float32."""
    d4, d5, cz = Z_PAIRS[zname]
    (d0, d1, d2, d3, yaw), (tx, ty, tw, tl, tyaw) = BEV_PAIRS[bevname]
    return torch.tensor([d0, d1, d2, d3, d4, d5, yaw]), torch.tensor([tx, ty, cz, tw, tl, 0.5, tyaw])


def rotated_reference(d, target, point=PLANT_POINT):
    """(1 - IoU3D, its gradient by the seven channels) by autograd through rotated_iou_restated in float64."""
    x = d.double().view(1, 7).clone().requires_grad_(True)
    pred = A.pred_to_box(torch.tensor([point], dtype=torch.float64), x)
    loss = (1 - RI.diff_iou_rotated_3d(pred, target.double().view(1, 7))).sum()
    loss.backward()
    return float(loss.detach()), x.grad[0].clone(), pred.detach()[0]


def shared_edges_reference(d, target, point=PLANT_POINT):
    """The same for identical BEV rectangles, where the vertex-gather restatement is degenerate (all four edges are shared: its
    gradient by the BEV channels depends on the order of coincident vertices), by autograd in float64 through the convention
    csrc/assign.hip's header states.  An edge of the prediction that lies on a parallel edge of the target with the same outward
    normal counts in full, and the target's edge on it never: the intersection is the prediction's own rectangle.  Its area is w *
    l and moves with the prediction's sizes alone (the derivative towards a smaller prediction, which the overlap follows); a shift
    or a turn does not change it to first order (the shared edges' normals, and their moments about their midpoints, cancel).  The
    z overlap and the composition are diff_iou_rotated_3d's own, with ATen's ties."""
    x = d.double().view(1, 7).clone().requires_grad_(True)
    pred, t = A.pred_to_box(torch.tensor([point], dtype=torch.float64), x)[0], target.double()
    assert torch.equal(pred.detach()[[0, 1, 3, 4, 6]], t[[0, 1, 3, 4, 6]])        # the convention's premise: the same rectangle
    area = pred[3] * pred[4]
    z_overlap = (torch.min(pred[2] + pred[5] * 0.5, t[2] + t[5] * 0.5) - torch.max(pred[2] - pred[5] * 0.5, t[2] - t[5] * 0.5)).clamp(min=0.)
    inter = area * z_overlap
    loss = 1 - inter / (pred[3] * pred[4] * pred[5] + t[3] * t[4] * t[5] - inter)
    loss.backward()
    return float(loss.detach()), x.grad[0].clone(), pred.detach()


@pytest.mark.parametrize("z", list(Z_PAIRS))
def test_shared_edges_convention_agrees_with_the_restatement_where_that_is_defined(z):
    """The value, and the gradient by the two z channels (which the coincident vertices do not enter), are the vertex-gather
    restatement's; the BEV channels are the convention's: equal pulls on both faces of an axis (no shift), none on the heading."""
    d, t = rotated_pair(z, "identical")
    loss, grad, _ = shared_edges_reference(d, t)
    want_loss, want_grad, _ = rotated_reference(d, t)
    assert abs(loss - want_loss) <= 1e-15 and float((grad - want_grad)[4:6].abs().max()) <= 1e-15
    assert float(grad[0]) == float(grad[1]) and float(grad[2]) == float(grad[3]) and float(grad[6]) == 0.0
    if z == "touching":
        assert not bool(grad[:4].any())                             # no z overlap: the BEV area carries no gradient
    elif z == "both_level":
        assert loss == 0.0 and not bool(grad[4:6].any())            # the same box: the z halves cancel the union's push
        assert float(grad[:4].max()) < 0                            # the BEV edges count in full: a one-sided derivative, not 0
    else:
        assert float(grad[:4].abs().min()) > 0


@pytest.mark.parametrize("bev", list(BEV_PAIRS))
@pytest.mark.parametrize("z", list(Z_PAIRS))
def test_rotated_pairs_have_level_z_faces(z, bev):
    d, t = rotated_pair(z, bev)
    loss, grad, pred = rotated_reference(d, t)
    hi_a, lo_a, hi_b, lo_b = (float(v) for v in (pred[2] + pred[5] / 2, pred[2] - pred[5] / 2, t[2] + t[5] / 2, t[2] - t[5] / 2))
    f = np.float32
    az = f(PLANT_POINT[2]) + (f(d[5]) - f(d[4])) / f(2)
    assert float(az + (f(d[4]) + f(d[5])) * f(0.5)) == hi_a and float(az - (f(d[4]) + f(d[5])) * f(0.5)) == lo_a    # exact in float32
    assert (hi_a == hi_b) == (z in ("tops_level", "both_level")) and (lo_a == lo_b) == (z in ("bottoms_level", "both_level"))
    assert (hi_a == lo_b) == (z == "touching")
    assert math.isfinite(loss) and bool(torch.isfinite(grad).all())
    if z == "touching":
        assert loss == 1.0 and float(grad[4:6].abs().max()) > 0     # clamp(min=0) passes the gradient at 0: the boxes are drawn together
    elif (z, bev) == ("both_level", "identical"):
        assert loss == 0.0                                          # the same box
    else:
        assert 0 < loss < 1
    if bev == "identical":
        assert torch.equal(pred[[0, 1, 3, 4, 6]], t.double()[[0, 1, 3, 4, 6]])


# ------------------------------------------------------------------------------------------- saturated focal and BCE terms
CLASS_LOGITS = [0.0] + [s * v for v in (1e-3, 5.0, 12.0, 16.0, 17.0, 30.0, 88.0, 89.0, 100.0, INF) for s in (1, -1)] + [NAN]
GAMMAS, ALPHAS = (0.0, 1.5, 2.0), (0.0, 0.25, 1.0)
CENTER_LOGITS = [0.0] + [s * v for v in (5.0, 30.0, 80.0) for s in (1, -1)]
CENTER_TARGETS = [1e-30, 0.5, 1.0]
ELEMENT_LEVELS = ((4, 4, 2),)                                    # one level of 32 points
BAND_BITS = 12


def class_logit_map():
    x = torch.zeros(32)
    x[:len(CLASS_LOGITS)] = torch.tensor(CLASS_LOGITS)
    return x


def center_maps():
    """(logits (32,), targets (32,)): every logit with every target, 21 planted elements; the rest 0 against 0.5."""
    x, t = torch.zeros(32), torch.full((32,), 0.5)
    pairs = [(a, b) for a in CENTER_LOGITS for b in CENTER_TARGETS]
    x[:len(pairs)] = torch.tensor([a for a, _ in pairs])
    t[:len(pairs)] = torch.tensor([b for _, b in pairs])
    return x, t


def focal_of_p(p, positive, gamma, alpha, grad=False):
    """The reference's term (or mmcv's backward) as a function of p = sigmoid(x) alone, float64: what the band rule evaluates."""
    tiny = float(np.finfo(np.float32).tiny)
    p = p.double().clamp(0, 1)
    lp, lq = torch.log(p.clamp(min=tiny)), torch.log((1 - p).clamp(min=tiny))
    if not grad:
        return -alpha * (1 - p).pow(gamma) * lp if positive else -(1 - alpha) * p.pow(gamma) * lq
    return -alpha * (1 - p).pow(gamma) * (1 - p - gamma * p * lp) if positive else -(1 - alpha) * p.pow(gamma) * (gamma * (1 - p) * lq - p)


def in_band(x):
    """Where 1 - p keeps fewer than BAND_BITS significant bits in float32 (p = sigmoid(x) >= 0.5, spacing 2^-24): the formula is
    ill-conditioned by itself there, p == 1 included."""
    q = 1 - torch.sigmoid(x.float())
    return (x > 0) & (q < 2.0 ** (BAND_BITS - 24)) & torch.isfinite(x)


def focal_bounds(x, positive, gamma, alpha, grad=False):
    """Per planted logit (lo, hi, f64, f32): the interval the kernel's value must lie in and the two yardstick columns.  Outside
    the band: float64 +- (4 x |float32 restatement - float64| + 2 float32 ulp of the term).  Inside: between the float64
    evaluations of the formula at p, p - 2 ulp and p + 2 ulp of the float32 p.  Where p + 2 ulp is clamped to 1, and only there,
    the end of the interval that this evaluation sets is moved out by 2 float32 ulp of the term: the kernel's result is a float32,
    and that end IS the float64 value at p = 1 (-log(FLT_MIN) = 87.33654475 against float32's 87.33654785), which no float32
    computation of the formula at p = 1 lies inside."""
    tgt = torch.zeros(len(x), dtype=torch.int64) if positive else torch.full((len(x),), -1, dtype=torch.int64)
    fn = R.focal_grads if grad else R.focal_terms
    f32 = fn(x.view(-1, 1), tgt, gamma, alpha)[:, 0].double()
    f64 = fn(x.double().view(-1, 1), tgt, gamma, alpha)[:, 0]
    tol = 4 * (f32 - f64).abs() + 2 * torch.from_numpy(R.ulp(f64.float().nan_to_num(0.0, 0.0, 0.0).numpy())).double()
    lo, hi = f64 - tol, f64 + tol
    p = torch.sigmoid(x)
    u = torch.from_numpy(np.spacing(p.numpy())).double()
    ev = torch.stack([focal_of_p(p.double() + k * u, positive, gamma, alpha, grad) for k in (-2, 0, 2)])
    band = in_band(x)
    clamped = p.double() + 2 * u >= 1
    two = 2 * torch.from_numpy(R.ulp(ev[2].float().nan_to_num(0.0, 0.0, 0.0).numpy())).double()
    blo, bhi = ev.min(0)[0], ev.max(0)[0]
    blo, bhi = torch.where(clamped & (ev[2] == blo), blo - two, blo), torch.where(clamped & (ev[2] == bhi), bhi + two, bhi)
    return torch.where(band, blo, lo), torch.where(band, bhi, hi), f64, f32


def bce_bounds(x, t):
    """(lo, hi, f64, f32) of binary_cross_entropy_with_logits per element, and the same of its gradient sigmoid(x) - t."""
    bce = lambda a, b: torch.nn.functional.binary_cross_entropy_with_logits(a, b, reduction="none")  # noqa: E731
    out = []
    for fn in (bce, lambda a, b: torch.sigmoid(a) - b):
        f32, f64 = fn(x, t).double(), fn(x.double(), t.double())
        tol = 4 * (f32 - f64).abs() + 2 * torch.from_numpy(R.ulp(f64.float().numpy())).double()
        out.append((f64 - tol, f64 + tol, f64, f32))
    return out


def kind(v):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    v = v.double()
    return torch.isposinf(v) * 1 + torch.isneginf(v) * 2 + torch.isnan(v) * 3


def test_saturation_premises():
    f = np.float32
    assert len(CLASS_LOGITS) == 22 and len(CENTER_LOGITS) * len(CENTER_TARGETS) == 21
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(f(89.0))) and np.isfinite(np.exp(f(88.0)))            # expf overflows between 88 and 89
    s = lambda v: float(torch.sigmoid(torch.tensor([v]))[0])  # noqa: E731
    assert 1 - s(17.0) == 0 and 1 - s(30.0) == 0 and 1 - s(16.0) > 0                 # 1 - p rounds to 0
    assert s(-89.0) == 0 or s(-89.0) < float(np.finfo(f).tiny)                        # p underflows below the floor of the logarithm
    assert s(-100.0) == 0 and 0 < s(-88.0) < float(np.finfo(f).tiny)
    assert in_band(torch.tensor(CLASS_LOGITS)).tolist() == [v in (12.0, 16.0, 17.0, 30.0, 88.0, 89.0, 100.0) for v in CLASS_LOGITS]
    x = torch.tensor([-100.0])
    assert float(R.focal_terms(x.view(1, 1), torch.tensor([-1]), 0.0, 0.25)) == 0.0   # pow(0, 0) = 1, times log(1) = 0
    assert float(R.focal_terms(x.view(1, 1), torch.tensor([0]), 0.0, 0.25)) == pytest.approx(0.25 * 87.3365, rel=1e-6)
    assert float(torch.tensor(0.0).pow(0.0)) == 1.0


def test_focal_grads_is_the_derivative_away_from_the_floor():
    x = torch.tensor([0.0, 1e-3, -1e-3, 5.0, -5.0, 12.0, -12.0, 30.0], dtype=torch.float64).view(-1, 1).requires_grad_(True)
    for tgt in (0, -1):
        for gamma in GAMMAS:
            for alpha in ALPHAS:
                t = torch.full((8,), tgt)
                g, = torch.autograd.grad(R.focal_terms(x, t, gamma, alpha).sum(), x)
                want = R.focal_grads(x.detach(), t, gamma, alpha)
                assert float((g - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-30) + 1e-300
                assert torch.equal(focal_of_p(torch.sigmoid(x.detach()[:, 0]), tgt == 0, gamma, alpha, True), want[:, 0])


def test_bounds_are_well_formed():
    x = class_logit_map()
    for positive in (True, False):
        for gamma in GAMMAS:
            for alpha in ALPHAS:
                for grad in (False, True):
                    lo, hi, f64, f32 = focal_bounds(x, positive, gamma, alpha, grad)
                    assert torch.equal(kind(f64), kind(f32))                       # the two columns agree in class
                    fin = kind(f64) == 0
                    assert bool((lo[fin] <= hi[fin]).all()) and bool(((f32[fin] >= lo[fin]) & (f32[fin] <= hi[fin])).all())
    cx, ct = center_maps()
    for lo, hi, f64, f32 in bce_bounds(cx, ct):
        assert bool(torch.isfinite(f64).all()) and bool((lo <= f32).all()) and bool((f32 <= hi).all())


# ------------------------------------------------------------------------------------------- valid mask at the boundary
VALID_LEVELS = ((8, 8, 4), (4, 4, 2), (3, 5, 3))                 # the mask's own resolution, exactly half, a non-integer ratio


def valid_counts():
    """(1, 1, 8, 8, 4) view counts in {0..3}: x pairs (0,1), (1,2), (2,3), (3,0) in the low-y half (half resolution: 0.5, 1.5, 2.5,
    1.5), (1,0), (0,0), (3,2), (0,3) halved again by an empty high-y quarter."""
    v = torch.zeros(1, 1, 8, 8, 4)
    v[0, 0, :, :4] = torch.tensor([0.0, 1, 1, 2, 2, 3, 3, 0]).view(8, 1, 1)
    v[0, 0, :, 4:6] = torch.tensor([1.0, 0, 0, 0, 3, 2, 0, 3]).view(8, 1, 1)
    return v


def test_valid_mask_lands_on_the_rounding_boundary():
    v = valid_counts()
    assert set(v.unique().tolist()) == {0.0, 1.0, 2.0, 3.0}
    half = torch.nn.Upsample(size=VALID_LEVELS[1], mode="trilinear")(v)
    assert {0.5, 1.5, 2.5} <= set(half.unique().tolist())
    want = R.upsampled_valid(v, VALID_LEVELS, 0)
    m1 = want[256:288].view(4, 4, 2)
    assert not bool(m1[0, :2].any()) and bool(m1[1, :2].all()) and bool(m1[2, :2].all())      # 0.5 -> 0 (half to even), 1.5 -> 2, 2.5 -> 2
    assert 0 < int(want[288:].sum()) < 45
