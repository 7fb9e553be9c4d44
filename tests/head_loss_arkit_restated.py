"""Restatement of ImVoxelHead_ARKit's target assignment and losses (nerfdet_head.py:779-900, 1016-1185) in torch on the CPU, box by
box: the rotated sibling of tests/head_loss_restated.py, which it reuses for everything the two heads share (points, centerness,
focal loss, maps, valid mask, LCG scenes).  The rotated IoU is tests/rotated_iou_restated.py.  The yardstick of
tests/test_gpu_head_loss_arkit.py on shapes fixture G19 does not hold, checked against G19 by tests/test_head_loss_arkit_host.py.

Also here, because the generator of G19, the tests and tools/head_loss_timing.py share them: the rotated scenes made from LCG seeds
(`scene`, `batch`), the conditions a scene must meet to go into the fixture (`near_decisions`, `near_degenerate`), and
`dense_form_loss`, the same objective in the reference's FORM (points x boxes tensors, boolean indexing, host reads) on any device.

Face distances rotate point - centre by -yaw with cos / sin from torch.cos / torch.sin of the ground truth, as rotation_3d_in_axis
does; the reference sums the rotation in an einsum, whose last bit may differ from the two-product sum here, so centerness targets
agree to rounding, labels wherever no decision hangs on that bit (the fixture's conditions)."""
import math

import numpy as np
import torch

import head_loss_restated as R
import rotated_iou_restated as RI

ARKIT_LEVELS = R.SCANNET_LEVELS
FLOAT_MAX = R.FLOAT_MAX
EPS = R.EPS
DEGENERATE_MARGIN = 1e-5   # |sin(2 (yaw_p - yaw_t))|, and metres between a corner of one rectangle and an edge of the other


def face_distances(p, b, rot=None):
    """ImVoxelHead_ARKit._get_face_distances of points (N, 3) to ONE box (7,) = (cx, cy, cz, dx, dy, dz, yaw): (N, 6).
    rot = (cos(yaw), sin(yaw)) handed in (as the kernels take them) instead of torch.cos / torch.sin of -yaw."""
    c, s = (torch.cos(-b[6]), torch.sin(-b[6])) if rot is None else (rot[0], -rot[1])
    sx, sy, sz = p[:, 0] - b[0], p[:, 1] - b[1], p[:, 2] - b[2]
    q = torch.stack((b[0] + (sx * c + sy * -s), b[1] + (sx * s + sy * c), b[2] + sz), dim=-1)
    return R.face_distances(q, b)


def assign(sizes, origin, boxes, volumes, labels, pts_assign_threshold=27, pts_center_threshold=18, details=False, points=None,
           rot=None):
    """Targets of one scene: labels (P,) int64 (-1: none), box_index (P,) int64 (-1), center_targets (P,) (-1 where no box),
    bbox_targets (P, 7) = the chosen box (zero where no box).  boxes (G, 7) = cat(gravity_center, size, yaw).
    points: the levels' (N, 3) points handed in instead of level_points; rot (G, 2): every box's (cos, sin) handed in."""
    pts = [R.level_points(s, l, origin) for l, s in enumerate(sizes)] if points is None else list(points)
    fd = lambda p, g: face_distances(p, boxes[g], None if rot is None else rot[g])  # noqa: E731
    offs = np.cumsum([0] + [len(p) for p in pts])
    P, L, G = int(offs[-1]), len(sizes), int(boxes.shape[0])
    vmin = torch.full((P,), FLOAT_MAX)
    arg = torch.full((P,), -1, dtype=torch.int64)
    center_t = torch.full((P,), -1.0)
    info = []
    k = min(pts_center_threshold + 1, P)
    for g in range(G):
        ins = [fd(p, g).min(-1)[0] > 0 for p in pts]
        n = [int(m.sum()) for m in ins]
        best = L - 1
        for l in range(L):
            if n[l] < pts_assign_threshold:
                best = max(l - 1, 0)
                break
        cand = torch.nonzero(ins[best]).squeeze(1)
        c = R.centerness_of(fd(pts[best][cand], g))
        t = torch.topk(c, k).values[-1] if len(c) >= k else torch.tensor(-1.0)
        keep = c > t
        idx = cand[keep] + int(offs[best])
        win = volumes[g] < vmin[idx]          # strict: an earlier box of the same volume keeps the point
        vmin[idx[win]] = volumes[g]
        arg[idx[win]] = g
        center_t[idx[win]] = c[keep][win]
        info.append((n, best, float(t), c, idx))
    out_labels = torch.full((P,), -1, dtype=torch.int64)
    bbox_t = torch.zeros(P, 7)
    pos = torch.nonzero(arg >= 0).squeeze(1)
    if len(pos):
        out_labels[pos] = labels[arg[pos]]
        bbox_t[pos] = boxes[arg[pos]]
    res = (out_labels, arg, center_t, bbox_t)
    return res + (info,) if details else res


def pred_to_box(points, d):
    """_bbox_pred_to_bbox (nerfdet_head.py:1029-1055): points (n, 3), d (n, 7) -> (n, 7)."""
    c, s = torch.cos(d[:, 6]), torch.sin(d[:, 6])
    sx, sy, sz = (d[:, 1] - d[:, 0]) / 2, (d[:, 3] - d[:, 2]) / 2, (d[:, 5] - d[:, 4]) / 2
    return torch.stack((points[:, 0] + (sx * c - sy * s), points[:, 1] + (sx * s + sy * c), points[:, 2] + sz,
                        d[:, 0] + d[:, 1], d[:, 2] + d[:, 3], d[:, 4] + d[:, 5], d[:, 6]), dim=-1)


def scene_losses(center, bbox, cls, valid, points, targets, gamma=2.0, alpha=0.25, weights=(1.0, 1.0, 1.0)):
    """(center_loss, bbox_loss, cls_loss) of one scene from the flattened maps; any float dtype."""
    labels, _, center_t, bbox_t = targets
    dt = center.dtype
    pos = (labels >= 0) & valid
    n_pos = max(float(pos.sum()), 1.0)
    navg = float(np.float32(n_pos) + np.float32(EPS)) if dt == torch.float32 else n_pos + EPS
    cls_loss = R.focal_terms(cls[valid], labels[valid], gamma, alpha).sum() / navg
    ct = center_t[pos].to(dt)
    center_loss = torch.nn.functional.binary_cross_entropy_with_logits(center[pos], ct, reduction="none").sum() / navg
    iou = RI.diff_iou_rotated_3d(pred_to_box(points[pos].to(dt), bbox[pos]), bbox_t[pos].to(dt))
    bbox_loss = ((1 - iou) * ct).sum() / (ct.sum() + EPS)
    return center_loss * weights[0], bbox_loss * weights[1], cls_loss * weights[2]


def loss_by_feat(center_preds, bbox_preds, cls_preds, valid_pred, gts, origins, pts_assign_threshold=27, pts_center_threshold=18,
                 gamma=2.0, alpha=0.25, weights=(1.0, 1.0, 1.0), dtype=None):
    """dict(center_loss, bbox_loss, cls_loss) (batch means, with autograd) and the per-scene targets.  gts: per scene (boxes (G, 7),
    volumes (G,), labels (G,)).  dtype=torch.float64: the losses evaluated in float64 on the float32 targets."""
    sizes = [tuple(int(v) for v in c.shape[2:]) for c in center_preds]
    per, all_targets = [], []
    for b, (gt, origin) in enumerate(zip(gts, origins)):
        targets = assign(sizes, origin, gt[0], gt[1], gt[2], pts_assign_threshold, pts_center_threshold)
        all_targets.append(targets)
        center, bbox, cls = R.flatten_maps(center_preds, bbox_preds, cls_preds, b)
        if dtype is not None:
            center, bbox, cls = center.to(dtype), bbox.to(dtype), cls.to(dtype)
        points = torch.cat([R.level_points(s, l, origin) for l, s in enumerate(sizes)])
        per.append(scene_losses(center, bbox, cls, R.upsampled_valid(valid_pred, sizes, b), points, targets, gamma, alpha, weights))
    names = ("center_loss", "bbox_loss", "cls_loss")
    return {n: torch.mean(torch.stack([p[i] for p in per])) for i, n in enumerate(names)}, all_targets


def dense_form_loss(center_preds, bbox_preds, cls_preds, valid_pred, gts, origins, pts_assign_threshold=27, pts_center_threshold=18,
                    gamma=2.0, alpha=0.25):
    """The same losses in the reference's form, on the maps' device: per scene (P, G, 6) face distances in the boxes' frames,
    (P, G) masks, topk over all points, boolean indexing with its host reads, the restated rotated IoU.  G >= 1."""
    dev = center_preds[0].device
    sizes = [tuple(int(v) for v in c.shape[2:]) for c in center_preds]
    L = len(sizes)
    per = []
    for b, (gt, origin) in enumerate(zip(gts, origins)):
        boxes, volumes, glabels = (t.to(dev) for t in gt)
        pts = [R.level_points(s, l, origin).to(dev) for l, s in enumerate(sizes)]
        scales = torch.cat([p.new_tensor(l).expand(len(p)) for l, p in enumerate(pts)])
        points = torch.cat(pts)
        P, G = len(points), len(boxes)
        eb = boxes.expand(P, G, 7)
        ep = points.unsqueeze(1).expand(P, G, 3)
        c, s = torch.cos(-boxes[:, 6]), torch.sin(-boxes[:, 6])
        sh = ep - eb[..., :3]
        q = torch.stack((eb[..., 0] + (sh[..., 0] * c + sh[..., 1] * -s), eb[..., 1] + (sh[..., 0] * s + sh[..., 1] * c),
                         eb[..., 2] + sh[..., 2]), dim=-1)
        d = torch.stack((q[..., 0] - eb[..., 0] + eb[..., 3] / 2, eb[..., 0] + eb[..., 3] / 2 - q[..., 0],
                         q[..., 1] - eb[..., 1] + eb[..., 4] / 2, eb[..., 1] + eb[..., 4] / 2 - q[..., 1],
                         q[..., 2] - eb[..., 2] + eb[..., 5] / 2, eb[..., 2] + eb[..., 5] / 2 - q[..., 2]), dim=-1)
        inside = d.min(-1)[0] > 0
        n = torch.stack([torch.sum(inside[scales == l], dim=0) for l in range(L)])
        low = n < pts_assign_threshold
        lower = (torch.argmax(low.int(), dim=0) - 1).clamp(min=0)
        best = torch.where(torch.all(~low, dim=0), torch.full_like(lower, L - 1), lower)
        at_best = best.unsqueeze(0).expand(P, G) == scales.unsqueeze(1).expand(P, G)
        cn = torch.sqrt(d[..., :2].min(-1)[0] / d[..., :2].max(-1)[0] * d[..., 2:4].min(-1)[0] / d[..., 2:4].max(-1)[0]
                        * d[..., 4:].min(-1)[0] / d[..., 4:].max(-1)[0])
        cn = torch.where(inside & at_best, cn, torch.full_like(cn, -1))
        top = cn > torch.topk(cn, min(pts_center_threshold + 1, P), dim=0).values[-1].unsqueeze(0)
        vol = torch.where(inside & at_best & top, volumes.expand(P, G), torch.full((P, G), FLOAT_MAX, device=dev))
        vmin, arg = vol.min(dim=1)
        labels = torch.where(vmin == FLOAT_MAX, torch.full_like(glabels[arg], -1), glabels[arg])
        center_t = cn[torch.arange(P, device=dev), arg]
        bbox_t = boxes[arg]
        center, bbox, cls = R.flatten_maps(center_preds, bbox_preds, cls_preds, b)
        valid = R.upsampled_valid(valid_pred, sizes, b)
        pos_inds = torch.nonzero(torch.logical_and(labels >= 0, valid)).squeeze(1)
        n_pos = max(float(len(pos_inds)), 1.0) + EPS                                   # host read 1
        if torch.any(valid):                                                           # host read 2
            cls_loss = R.focal_terms(cls[valid], labels[valid], gamma, alpha).sum() / n_pos
        else:
            cls_loss = cls[valid].sum()
        if len(pos_inds) > 0:
            ct = center_t[pos_inds]
            center_loss = torch.nn.functional.binary_cross_entropy_with_logits(center[pos_inds], ct, reduction="none").sum() / n_pos
            pred = pred_to_box(points[pos_inds], bbox[pos_inds])
            if not torch.any(ct > 0):                                                  # host read 3
                bbox_loss = pred.sum() * ct.sum()
            else:
                bbox_loss = ((1 - RI.diff_iou_rotated_3d(pred, bbox_t[pos_inds])) * ct).sum() / (ct.sum() + EPS)
        else:
            center_loss, bbox_loss = center[pos_inds].sum(), bbox[pos_inds].sum()
        per.append((center_loss, bbox_loss, cls_loss))
    names = ("center_loss", "bbox_loss", "cls_loss")
    return {n: torch.mean(torch.stack([p[i] for p in per])) for i, n in enumerate(names)}


# ---------------------------------------------------------------------------------------------------------------------- scenes
class RotatedDepthBoxes(R.DepthBoxes):
    """What loss_by_feat reads of mmdet3d's DepthInstance3DBoxes with yaw (x, y, bottom z, dx, dy, dz, yaw)."""
    with_yaw = True

    def to(self, device):
        return RotatedDepthBoxes(self.tensor.to(device))


def gt_triplet(gt):
    """(boxes (G, 7), volumes, labels) as ImVoxelHead_ARKit._get_targets reads them (nerfdet_head.py:1130-1134)."""
    b = gt.bboxes_3d
    return torch.cat((b.gravity_center, b.tensor[:, 3:7]), dim=1), b.volume, gt.labels_3d


SCENE_KINDS = R.SCENE_KINDS


def scene(kind, seed, levels=ARKIT_LEVELS, n_classes=17):
    """One rotated scene from its seed: head_loss_restated.scene's maps, valid counts and boxes; a seventh bbox channel (the
    predicted heading), a yaw for every box over the whole circle, and in kind "twelve" yaws near 0, pi / 2 and pi, a box larger
    than the grid and one partly outside it (no two boxes of equal volume: size[6] is changed)."""
    centers, bboxes, clss, valid, origin, gt = R.scene(kind, seed, levels, n_classes)
    tensor, labels = gt.bboxes_3d.tensor.clone(), gt.labels_3d
    G = tensor.shape[0]
    yaw = R._u((G,), seed * 10 + 7) * math.pi
    if kind == "twelve":
        tensor[6, 3:6] = tensor[6, 3:6] * torch.tensor([0.9, 1.1, 1.05])
        tensor[4, 2] += 0.013   # head_loss_restated centres box 4 on the origin's z: mirrored points would tie in centerness
        yaw[7], yaw[8], yaw[9], yaw[10] = 1e-3, math.pi / 2 + 2e-3, math.pi - 1.5e-3, -math.pi / 2 - 1e-3
    if kind == "valid_no_pos":
        yaw = yaw * 0.2
    tensor = torch.cat([tensor, yaw.view(-1, 1).float()], dim=1)
    heads = []
    for lvl, size in enumerate(levels):
        h = (1.7 * R._u((1, 1) + tuple(size), 100 * (lvl + 1) + seed * 10 + 6)).float()
        heads.append(torch.cat([bboxes[lvl], h], dim=1).contiguous())
    return centers, heads, clss, valid, origin, R.GtInstances(RotatedDepthBoxes(tensor), labels)


def batch(kinds, seeds, levels=ARKIT_LEVELS, n_classes=17):
    scenes = [scene(k, s, levels, n_classes) for k, s in zip(kinds, seeds)]
    cat = lambda j: [torch.cat([sc[j][lvl] for sc in scenes]) for lvl in range(len(levels))]  # noqa: E731
    return cat(0), cat(1), cat(2), torch.cat([sc[3] for sc in scenes]), [sc[4] for sc in scenes], [sc[5] for sc in scenes]


metas_for = R.metas_for


def near_decisions(sizes, origin, gt, pts_assign_threshold=27, pts_center_threshold=18):
    """Reasons a scene's assignment could hang on rounding: a face distance within 4 ulp (of its operands' scale) of 0; a candidate's
    centerness within 4 ulp of its box's boundary value other than the boundary point itself; the pts_center_threshold-th and the
    next centerness of a box on its best level closer than 1e-5 relative; a point two boxes of equal volume both claim."""
    boxes, volumes, labels = gt
    why = []
    *_, info = assign(sizes, origin, boxes, volumes, labels, pts_assign_threshold, pts_center_threshold, details=True)
    pts = torch.cat([R.level_points(s, l, origin) for l, s in enumerate(sizes)])
    claimed = {}
    for g in range(len(boxes)):
        d = face_distances(pts, boxes[g]).numpy()
        scale = np.maximum(np.abs(pts.numpy()).max(), float(boxes[g, :6].abs().max()) * 1.5)
        if (np.abs(d) <= 4 * R.ulp(scale)).any():
            why.append(f"box {g}: a face distance within 4 ulp of 0")
        _, _, t, c, idx = info[g]
        if t >= 0:
            close = np.abs(c.numpy() - np.float32(t)) <= 4 * R.ulp(t)
            if int(close.sum()) != 1:
                why.append(f"box {g}: {int(close.sum())} centerness values within 4 ulp of the boundary")
            top = np.sort(c.numpy().astype(np.float64))[::-1]
            k = pts_center_threshold
            if k >= 1 and len(top) > k and (top[k - 1] - top[k]) < 1e-5 * top[k - 1]:
                why.append(f"box {g}: the {k}-th and the next centerness are {top[k - 1] - top[k]:.3g} apart")
        for i in idx.tolist():
            for h in claimed.get(i, []):
                if float(volumes[h]) == float(volumes[g]):
                    why.append(f"point {i}: boxes {h} and {g} of equal volume")
            claimed.setdefault(i, []).append(g)
    return why


def near_degenerate(pred_boxes, target_boxes, margin=DEGENERATE_MARGIN):
    """Reasons a positive pair is closer to a degenerate configuration than `margin`."""
    if len(pred_boxes) == 0:
        return []
    s, dist = RI.degeneracy(pred_boxes, target_boxes)
    why = []
    if bool((s < margin).any()):
        why.append(f"a pair with |sin 2(yaw_p - yaw_t)| = {float(s.min()):.3g}")
    if bool((dist < margin).any()):
        why.append(f"a pair with a corner {float(dist.min()):.3g} m from an edge")
    return why
