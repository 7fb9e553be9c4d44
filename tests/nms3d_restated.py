"""mmcv's nms3d (mmcv 2.1.0, the OpenPCDet-derived iou3d kernel) restated in float32 NumPy, one operation per rounding, and an
exact float64 polygon-clipping IoU to judge it by.  The restatement is the yardstick of the rotated detection kernels
(csrc/detect.hip: rot_prep, box_overlap, rot_iou) and the nms3d stand-in of tests/golden/make_goldens_g16.py.

Boxes are (x, y, z, dx, dy, dz, heading); z and dz are unused (bird's-eye view).  iou_bev(a, b) = overlap / fmaxf(sa + sb - overlap,
1e-8) with sa = dx * dy.  overlap: the rotated corners, every edge-edge crossing (a's edge i against b's edge j), then b's corner k
inside a and a's corner k inside b (|r| < half size + 1e-2 in the other box's frame), their centroid, a bubble sort by atan2 about
it and the shoelace sum about the first point."""
import numpy as np

F = np.float32
MARGIN = F(1e-2)
EPS = F(1e-8)
NPTS = 25   # 16 crossings + 8 corners at the most, one spare slot for the vectorised writes


def prep(boxes):
    """Per box: centre, size, the four rotated corners and cos / sin of -heading (rot_prep)."""
    with np.errstate(all="ignore"):
        return _prep(np.asarray(boxes, F).reshape(-1, 7))


def _prep(b):
    x, y, dx, dy, h = b[:, 0], b[:, 1], b[:, 3], b[:, 4], b[:, 6]
    hx, hy = dx / F(2), dy / F(2)
    x1, y1, x2, y2 = x - hx, y - hy, x + hx, y + hy
    ax = np.stack([x1, x2, x2, x1], 1)
    ay = np.stack([y1, y1, y2, y2], 1)
    c, s = np.cos(h)[:, None], np.sin(h)[:, None]
    ux, uy = ax - x[:, None], ay - y[:, None]
    px = (ux * c - uy * s) + x[:, None]
    py = (ux * s + uy * c) + y[:, None]
    return dict(x=x, y=y, dx=dx, dy=dy, px=px, py=py, cn=np.cos(-h), sn=np.sin(-h))


def _cross(p1x, p1y, p2x, p2y, p0x, p0y):
    return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y)


def _in_box(b, x, y):
    rx = (x - b["x"]) * b["cn"] + (y - b["y"]) * -b["sn"]
    ry = (x - b["x"]) * b["sn"] + (y - b["y"]) * b["cn"]
    return (np.abs(rx) < b["dx"] / F(2) + MARGIN) & (np.abs(ry) < b["dy"] / F(2) + MARGIN)


def _take(g, idx):
    return {k: v[idx] for k, v in g.items()}


def overlap_pairs(a, b):
    """box_overlap of the paired rows of two prep() dicts of equal length."""
    m = len(a["x"])
    qx, qy = np.zeros((m, NPTS), F), np.zeros((m, NPTS), F)
    cnt = np.zeros(m, np.int64)
    sx, sy = np.zeros(m, F), np.zeros(m, F)
    rows = np.arange(m)

    def add(flag, ox, oy):
        nonlocal sx, sy, cnt
        qx[rows, cnt] = np.where(flag, ox, qx[rows, cnt])
        qy[rows, cnt] = np.where(flag, oy, qy[rows, cnt])
        sx = np.where(flag, sx + ox, sx)
        sy = np.where(flag, sy + oy, sy)
        cnt = cnt + flag

    for i in range(4):
        p0x, p0y, p1x, p1y = a["px"][:, i], a["py"][:, i], a["px"][:, (i + 1) % 4], a["py"][:, (i + 1) % 4]
        for j in range(4):
            q0x, q0y, q1x, q1y = b["px"][:, j], b["py"][:, j], b["px"][:, (j + 1) % 4], b["py"][:, (j + 1) % 4]
            rect = ((np.fmin(p0x, p1x) <= np.fmax(q0x, q1x)) & (np.fmin(q0x, q1x) <= np.fmax(p0x, p1x))
                    & (np.fmin(p0y, p1y) <= np.fmax(q0y, q1y)) & (np.fmin(q0y, q1y) <= np.fmax(p0y, p1y)))
            s1 = _cross(q0x, q0y, p1x, p1y, p0x, p0y)
            s2 = _cross(p1x, p1y, q1x, q1y, p0x, p0y)
            s3 = _cross(p0x, p0y, q1x, q1y, q0x, q0y)
            s4 = _cross(q1x, q1y, p1x, p1y, q0x, q0y)
            flag = rect & (s1 * s2 > 0) & (s3 * s4 > 0)
            s5 = _cross(q1x, q1y, p1x, p1y, p0x, p0y)
            a0, b0, c0 = p0y - p1y, p1x - p0x, p0x * p1y - p1x * p0y
            a1, b1, c1 = q0y - q1y, q1x - q0x, q0x * q1y - q1x * q0y
            D = a0 * b1 - a1 * b0
            far = np.abs(s5 - s1) > EPS
            ox = np.where(far, (s5 * q0x - s1 * q1x) / (s5 - s1), (b0 * c1 - b1 * c0) / D)
            oy = np.where(far, (s5 * q0y - s1 * q1y) / (s5 - s1), (a1 * c0 - a0 * c1) / D)
            add(flag, ox, oy)
    for k in range(4):
        add(_in_box(a, b["px"][:, k], b["py"][:, k]), b["px"][:, k], b["py"][:, k])
        add(_in_box(b, a["px"][:, k], a["py"][:, k]), a["px"][:, k], a["py"][:, k])
    top = int(cnt.max()) if m else 0
    area = np.zeros(m, F)
    if top >= 2:
        cx, cy = sx / cnt.astype(F), sy / cnt.astype(F)
        ang = np.arctan2(qy[:, :top] - cy[:, None], qx[:, :top] - cx[:, None]).astype(F)
        qx, qy = qx[:, :top].copy(), qy[:, :top].copy()
        for j in range(top - 1):
            for i in range(top - j - 1):
                sw = (i < cnt - j - 1) & (ang[:, i] > ang[:, i + 1])
                if sw.any():
                    for arr in (ang, qx, qy):
                        t = arr[sw, i].copy()
                        arr[sw, i] = arr[sw, i + 1]
                        arr[sw, i + 1] = t
        for k in range(top - 1):
            ax, ay = qx[:, k] - qx[:, 0], qy[:, k] - qy[:, 0]
            bx, by = qx[:, k + 1] - qx[:, 0], qy[:, k + 1] - qy[:, 0]
            area = np.where(k < cnt - 1, area + (ax * by - ay * bx), area)
    return np.abs(area) / F(2)


def far_apart(a, b, slack=F(0.1)):
    """Pairs whose overlap is 0 for certain (the corners lie within half a diagonal of their centre): a wide version of the
    kernels' early exit, to skip the full path in long walks.  NaN / inf distances are never far."""
    ra = F(0.5) * np.sqrt(a["dx"] * a["dx"] + a["dy"] * a["dy"])
    rb = F(0.5) * np.sqrt(b["dx"] * b["dx"] + b["dy"] * b["dy"])
    reach = (ra + rb + slack) + F(1e-3) * (np.abs(a["x"]) + np.abs(a["y"]) + np.abs(b["x"]) + np.abs(b["y"]) + ra + rb)
    ex, ey = b["x"] - a["x"], b["y"] - a["y"]
    return ex * ex + ey * ey > reach * reach


def iou_pairs(a, b, skip_far=True):
    """iou_bev of the paired rows of two prep() dicts (a first)."""
    with np.errstate(all="ignore"):
        ov = np.zeros(len(a["x"]), F)
        near = ~far_apart(a, b) if skip_far else np.ones(len(a["x"]), bool)
        if near.any():
            ov[near] = overlap_pairs(_take(a, near), _take(b, near))
        sa, sb = a["dx"] * a["dy"], b["dx"] * b["dy"]
        return ov / np.fmax((sa + sb) - ov, EPS)


def bev_iou(boxes_a, boxes_b, skip_far=False):
    """(n, m) iou_bev of every pair (ops.bev_iou_rotated's restatement)."""
    a, b = prep(boxes_a), prep(boxes_b)
    n, m = len(a["x"]), len(b["x"])
    ia, ib = np.repeat(np.arange(n), m), np.tile(np.arange(m), n)
    return iou_pairs(_take(a, ia), _take(b, ib), skip_far).reshape(n, m)


def score_order(scores):
    """Visiting order: score descending, NaN first (either sign), -0 equal to +0, ties by lower index."""
    s = np.asarray(scores, F)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), -np.where(nan, F(0), s), ~nan))


def nms3d(boxes, scores, thresh, visit=None):
    """mmcv's nms3d: the kept indices in pick order.  `visit(i, js, iou)` sees every (kept i, still alive later js) step."""
    g = prep(boxes)
    t = F(thresh)
    order = score_order(scores)
    picks = []
    while order.size:
        i, rest = order[0], order[1:]
        picks.append(int(i))
        if rest.size == 0:
            break
        iou = iou_pairs(_take(g, np.full(rest.size, i)), _take(g, rest))
        if visit is not None:
            visit(i, rest, iou)
        order = rest[~(iou > t)]
    return np.array(picks, dtype=np.int64)


# ------------------------------------------------------------------------------------------- exact geometry
def _rect64(box):
    x, y, dx, dy, h = (float(v) for v in (box[0], box[1], box[3], box[4], box[6]))
    c, s = np.cos(h), np.sin(h)
    pts = []
    for ux, uy in ((-dx / 2, -dy / 2), (dx / 2, -dy / 2), (dx / 2, dy / 2), (-dx / 2, dy / 2)):
        pts.append((x + ux * c - uy * s, y + ux * s + uy * c))
    return pts


def _clip(poly, a, b):
    """Sutherland-Hodgman: the part of poly left of the directed line a -> b."""
    out = []
    side = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])  # noqa: E731
    for k in range(len(poly)):
        p, q = poly[k], poly[(k + 1) % len(poly)]
        sp, sq = side(p), side(q)
        if sp >= 0:
            out.append(p)
        if (sp >= 0) != (sq >= 0):
            t = sp / (sp - sq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def _area(poly):
    return 0.5 * abs(sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1]
                         for k in range(len(poly)))) if len(poly) >= 3 else 0.0


def exact_iou(box_a, box_b):
    """The true BEV IoU of two rotated rectangles in float64 (positive sizes), by clipping a against b."""
    pa, pb = _rect64(box_a), _rect64(box_b)
    ccw = lambda p: p if _signed(p) >= 0 else p[::-1]  # noqa: E731
    poly, clipper = ccw(pa), ccw(pb)
    for k in range(4):
        if not poly:
            break
        poly = _clip(poly, clipper[k], clipper[(k + 1) % 4])
    inter = _area(poly)
    sa, sb = float(box_a[3]) * float(box_a[4]), float(box_b[3]) * float(box_b[4])
    return inter / max(sa + sb - inter, 1e-8)


def _signed(p):
    return sum(p[k][0] * p[(k + 1) % 4][1] - p[(k + 1) % 4][0] * p[k][1] for k in range(4))


def corner_in_margin_band(box_a, box_b):
    """True if a corner of one box lies within the 1e-2 margin band around the other's boundary (where the restated overlap
    counts a corner that is outside, by design)."""
    for u, v in ((box_a, box_b), (box_b, box_a)):
        c, s = np.cos(-float(v[6])), np.sin(-float(v[6]))
        for px, py in _rect64(u):
            rx = (px - float(v[0])) * c - (py - float(v[1])) * s
            ry = (px - float(v[0])) * s + (py - float(v[1])) * c
            ex, ey = abs(rx) - float(v[3]) / 2, abs(ry) - float(v[4]) / 2
            if max(ex, ey) > -2e-2 and max(ex, ey) < 2e-2:
                return True
    return False
