"""The rotated 3-D IoU of RotatedIoU3DLoss as plain torch: the stand-in for mmcv.ops.diff_iou_rotated_3d in fixture G19 and the
yardstick of tests/test_gpu_head_loss_arkit.py.  It is THE MATHEMATICAL FUNCTION, NOT MMCV'S ROUNDING: the exact area of the
intersection of the two rectangles, differentiable by autograd, in float32 or float64.  mmcv's compiled sort_vertices op has no CPU
path and none of its text is at hand, so nothing here can be compared with mmcv's own float32 result.

The construction is the public one mmcv's op follows (and unlike the HIP kernel's, which clips edges by parameter interval and never
builds a vertex list): the candidates are the 4 + 4 corners and the 16 pairwise edge intersections; a corner counts where it lies
inside the other rectangle, an intersection where both parameters lie inside (0, 1); the valid vertices are ordered by angle about
their mean and summed by the shoelace formula.  Mask and order carry no gradient; the gathered vertices do.  The 3-D IoU is composed
as projects/TR3D/tr3d/rotated_iou_loss.py:23-37 shows: intersection area * z overlap over the union of the volumes.

Boxes are (x, y, z, dx, dy, dz, yaw), rows paired one to one.  Away from degenerate pairs (a corner on an edge, parallel
overlapping edges) the value is exact to rounding; tests/nms3d_restated.exact_iou (float64 Sutherland-Hodgman) is the independent
check of it (tests/test_head_loss_arkit_host.py)."""
import torch


def corners(box):
    """(N, 4, 2) corners, counter-clockwise, of (N, 5) rectangles (x, y, dx, dy, yaw)."""
    x4 = box.new_tensor([0.5, -0.5, -0.5, 0.5]) * box[:, 2:3]
    y4 = box.new_tensor([0.5, 0.5, -0.5, -0.5]) * box[:, 3:4]
    c, s = torch.cos(box[:, 4:5]), torch.sin(box[:, 4:5])
    return torch.stack((box[:, 0:1] + x4 * c - y4 * s, box[:, 1:2] + x4 * s + y4 * c), dim=-1)


def _edge_intersections(c1, c2):
    """(N, 16, 2) points and (N, 16) mask: edge i of c1 with edge j of c2, both parameters strictly inside (0, 1)."""
    p1, p2 = c1[:, :, None, :], torch.roll(c1, -1, dims=1)[:, :, None, :]
    p3, p4 = c2[:, None, :, :], torch.roll(c2, -1, dims=1)[:, None, :, :]
    d12, d34, d13 = p1 - p2, p3 - p4, p1 - p3
    den = d12[..., 0] * d34[..., 1] - d12[..., 1] * d34[..., 0]
    ok = den != 0
    den = torch.where(ok, den, torch.ones_like(den))
    t = (d13[..., 0] * d34[..., 1] - d13[..., 1] * d34[..., 0]) / den
    u = -(d12[..., 0] * d13[..., 1] - d12[..., 1] * d13[..., 0]) / den
    mask = ok & (t > 0) & (t < 1) & (u > 0) & (u < 1)
    pts = p1 + t.unsqueeze(-1) * (p2 - p1)
    n = c1.shape[0]
    return pts.reshape(n, 16, 2), mask.reshape(n, 16)


def _inside(points, rect):
    """(N, 4) mask: points (N, 4, 2) inside (boundary included) the rectangles with corners rect (N, 4, 2)."""
    a, b, d = rect[:, 0:1], rect[:, 1:2], rect[:, 3:4]
    ab, ad, am = b - a, d - a, points - a
    pab = (ab * am).sum(-1) / (ab * ab).sum(-1).clamp(min=torch.finfo(points.dtype).tiny)
    pad = (ad * am).sum(-1) / (ad * ad).sum(-1).clamp(min=torch.finfo(points.dtype).tiny)
    return (pab >= 0) & (pab <= 1) & (pad >= 0) & (pad <= 1)


def intersection_area(c1, c2):
    """(N,) area of the intersection of the convex quadrilaterals c1, c2 (N, 4, 2), with autograd to both."""
    pts, mask = _edge_intersections(c1, c2)
    verts = torch.cat((c1, c2, pts), dim=1)                                   # (N, 24, 2)
    mask = torch.cat((_inside(c1, c2), _inside(c2, c1), mask), dim=1)         # (N, 24)
    with torch.no_grad():
        cnt = mask.sum(1, keepdim=True).clamp(min=1)
        mean = (verts * mask.unsqueeze(-1)).sum(1, keepdim=True) / cnt.unsqueeze(-1)
        rel = verts - mean
        ang = torch.atan2(rel[..., 1], rel[..., 0])
        ang = torch.where(mask, ang, torch.full_like(ang, float("inf")))       # the vertices that do not count go last
        order = torch.argsort(ang, dim=1)
        first = order[:, :1]
        k = mask.sum(1, keepdim=True)
        take = torch.where(torch.arange(24, device=verts.device).view(1, -1) < k, order, first.expand(-1, 24))
    poly = torch.gather(verts, 1, take.unsqueeze(-1).expand(-1, -1, 2))        # valid vertices in order, then the first repeated
    nxt = torch.roll(poly, -1, dims=1)
    twice = (poly[..., 0] * nxt[..., 1] - nxt[..., 0] * poly[..., 1]).sum(1)
    return torch.where(mask.sum(1) >= 3, twice.abs() / 2, torch.zeros_like(twice))


def diff_iou_rotated_3d(box1, box2):
    """(N,) rotated 3-D IoU of the paired rows of box1, box2 (N, 7) = (x, y, z, dx, dy, dz, yaw)."""
    if box1.shape[0] == 0:
        return box1.new_zeros((0,))
    area = intersection_area(corners(box1[:, [0, 1, 3, 4, 6]]), corners(box2[:, [0, 1, 3, 4, 6]]))
    zmax1, zmin1 = box1[:, 2] + box1[:, 5] * 0.5, box1[:, 2] - box1[:, 5] * 0.5
    zmax2, zmin2 = box2[:, 2] + box2[:, 5] * 0.5, box2[:, 2] - box2[:, 5] * 0.5
    z_overlap = (torch.min(zmax1, zmax2) - torch.max(zmin1, zmin2)).clamp(min=0.)
    inter = area * z_overlap
    union = box1[:, 3] * box1[:, 4] * box1[:, 5] + box2[:, 3] * box2[:, 4] * box2[:, 5] - inter
    return inter / union


def degeneracy(box1, box2):
    """How close each pair is to a degenerate configuration, in float64: (|sin(2 (yaw1 - yaw2))|, the least distance of a corner of
    one rectangle to an edge SEGMENT of the other).  Both (N,)."""
    b1, b2 = box1.double(), box2.double()
    c1, c2 = corners(b1[:, [0, 1, 3, 4, 6]]), corners(b2[:, [0, 1, 3, 4, 6]])

    def seg_dist(p, q):   # corners p (N, 4, 2) to the edges of q: (N,) minimum
        a, b = q[:, None, :, :], torch.roll(q, -1, dims=1)[:, None, :, :]
        ab, ap = b - a, p[:, :, None, :] - a
        t = ((ap * ab).sum(-1) / (ab * ab).sum(-1).clamp(min=1e-300)).clamp(0, 1)
        return (ap - t.unsqueeze(-1) * ab).norm(dim=-1).reshape(p.shape[0], -1).min(1)[0]

    return torch.sin(2 * (b1[:, 6] - b2[:, 6])).abs(), torch.min(seg_dist(c1, c2), seg_dist(c2, c1))
