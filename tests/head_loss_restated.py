"""Restatement of NerfDetHead's target assignment and losses (nerfdet_head.py:152-257, 473-562) in torch on the CPU, box by box,
without the reference's points x boxes x 6 tensors: the yardstick of tests/test_gpu_head_loss.py on shapes fixture G18 does not
hold, checked against G18 (and under `-m refcheck` against the reference run live) by tests/test_head_loss_host.py.

Also here, because the generator of G18, the tests and tools/head_loss_timing.py share them: the scenes made from LCG seeds
(`scene`, `batch`), and `dense_form_loss`, the same computation in the reference's FORM (points x boxes tensors, boolean indexing,
three host reads per scene) on any device -- the baseline the timing tool runs on the GPU.

The element-wise float32 expressions are the reference's, operand for operand, so targets agree bit for bit; sums are taken in
another order, so losses and gradients agree to rounding.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from lcg import lcg_uniform  # noqa: E402

VOXEL = (.16, .16, .2)
SCANNET_LEVELS = ((40, 40, 16), (20, 20, 8), (10, 10, 4))
FLOAT_MAX = 1e8
EPS = float(torch.finfo(torch.float32).eps)   # mmdet 3.x weight_reduce_loss: loss.sum() / (avg_factor + eps)


def _u(shape, seed):
    return torch.from_numpy(lcg_uniform(int(np.prod(shape)), seed)).reshape(shape)


# ------------------------------------------------------------------------------------------------------------------- geometry
def level_points(size, level, origin):
    """get_points of one level, flattened x-major: (N, 3) float32."""
    n = torch.tensor(list(size))
    vs = torch.tensor(VOXEL) * (2 ** level)
    new_origin = origin - n / 2. * vs
    grid = torch.stack(torch.meshgrid([torch.arange(int(s)) for s in size], indexing="ij"))
    pts = grid * vs.view(3, 1, 1, 1) + new_origin.view(3, 1, 1, 1)
    return pts.reshape(3, -1).transpose(0, 1).contiguous()


def face_distances(p, b):
    """_get_face_distances of points (N, 3) to ONE box (6,) = (cx, cy, cz, dx, dy, dz): (N, 6)."""
    return torch.stack((p[:, 0] - b[0] + b[3] / 2, b[0] + b[3] / 2 - p[:, 0], p[:, 1] - b[1] + b[4] / 2, b[1] + b[4] / 2 - p[:, 1],
                        p[:, 2] - b[2] + b[5] / 2, b[2] + b[5] / 2 - p[:, 2]), dim=-1)


def ieee_sqrt(x):
    """The correctly rounded float32 square root: through float64 (53 >= 2 * 24 + 2 bits, so the second rounding cannot differ).
    torch.sqrt on a CPU build with MKL's vector maths is within an ulp but not correctly rounded (6 values in 1000 differ from
    numpy's); torch on the GPU, numpy and the HIP kernels all round correctly."""
    return x.double().sqrt().to(x.dtype) if x.dtype == torch.float32 else torch.sqrt(x)


def centerness_of(d):
    x, y, z = d[:, [0, 1]], d[:, [2, 3]], d[:, [4, 5]]
    c = x.min(dim=-1)[0] / x.max(dim=-1)[0] * y.min(dim=-1)[0] / y.max(dim=-1)[0] * z.min(dim=-1)[0] / z.max(dim=-1)[0]
    return ieee_sqrt(c)


# ------------------------------------------------------------------------------------------------------------------ assignment
def assign(sizes, origin, boxes, volumes, labels, pts_assign_threshold=27, pts_center_threshold=18, details=False, points=None):
    """Targets of one scene: labels (P,) int64 (-1: none), box_index (P,) int64 (-1), center_targets (P,), bbox_targets (P, 6) (zero
    where no box).  boxes (G, 6) = cat(gravity_center, size), volumes (G,), labels (G,).  Equal volumes: the lowest box index.
    points: the levels' (N, 3) points handed in (a hand-built geometry) instead of level_points(size, level, origin)."""
    pts = [level_points(s, l, origin) for l, s in enumerate(sizes)] if points is None else list(points)
    offs = np.cumsum([0] + [len(p) for p in pts])
    P, L, G = int(offs[-1]), len(sizes), int(boxes.shape[0])
    vmin = torch.full((P,), FLOAT_MAX)
    arg = torch.full((P,), -1, dtype=torch.int64)
    info = []
    for g in range(G):
        ins = [face_distances(p, boxes[g]).min(-1)[0] > 0 for p in pts]
        n = [int(m.sum()) for m in ins]
        best = L - 1
        for l in range(L):
            if n[l] < pts_assign_threshold:
                best = max(l - 1, 0)
                break
        cand = torch.nonzero(ins[best]).squeeze(1)
        c = centerness_of(face_distances(pts[best][cand], boxes[g]))
        k = pts_center_threshold + 1
        t = torch.topk(c, k).values[-1] if len(c) >= k else torch.tensor(-1.0)
        idx = cand[c > t] + int(offs[best])
        win = volumes[g] < vmin[idx]          # strict: an earlier box of the same volume keeps the point
        vmin[idx[win]] = volumes[g]
        arg[idx[win]] = g
        info.append((n, best, float(t), c))
    allp = torch.cat(pts)
    out_labels = torch.full((P,), -1, dtype=torch.int64)
    center_t = torch.zeros(P)
    bbox_t = torch.zeros(P, 6)
    pos = torch.nonzero(arg >= 0).squeeze(1)
    if len(pos):
        b = boxes[arg[pos]]
        p = allp[pos]
        d = torch.stack((p[:, 0] - b[:, 0] + b[:, 3] / 2, b[:, 0] + b[:, 3] / 2 - p[:, 0], p[:, 1] - b[:, 1] + b[:, 4] / 2,
                         b[:, 1] + b[:, 4] / 2 - p[:, 1], p[:, 2] - b[:, 2] + b[:, 5] / 2, b[:, 2] + b[:, 5] / 2 - p[:, 2]), dim=-1)
        out_labels[pos] = labels[arg[pos]]
        center_t[pos] = centerness_of(d)
        bbox_t[pos] = torch.stack((p[:, 0] - d[:, 0], p[:, 1] - d[:, 2], p[:, 2] - d[:, 4], p[:, 0] + d[:, 1], p[:, 1] + d[:, 3],
                                   p[:, 2] + d[:, 5]), dim=-1)
    res = (out_labels, arg, center_t, bbox_t)
    return res + (info,) if details else res


# ---------------------------------------------------------------------------------------------------------------------- losses
def focal_terms(x, target, gamma=2.0, alpha=0.25):
    """mmcv's sigmoid focal loss per (point, class): x (n, C) logits, target (n,) with -1 = background everywhere."""
    tiny = torch.finfo(torch.float32).tiny
    p = torch.sigmoid(x)
    pos = target.view(-1, 1) == torch.arange(x.shape[1], device=x.device).view(1, -1)
    term_p = -alpha * (1 - p).pow(gamma) * torch.log(p.clamp(min=tiny))
    term_n = -(1 - alpha) * p.pow(gamma) * torch.log((1 - p).clamp(min=tiny))
    return torch.where(pos, term_p, term_n)


def focal_grads(x, target, gamma=2.0, alpha=0.25):
    """d focal_terms / d x as mmcv's sigmoid focal loss hands it back (its backward is the closed form by p = sigmoid(x), with the
    same floor under the logarithm, not autograd through the clamp): the same shape and dtype as x."""
    tiny = torch.finfo(torch.float32).tiny
    p = torch.sigmoid(x)
    pos = target.view(-1, 1) == torch.arange(x.shape[1], device=x.device).view(1, -1)
    grad_p = -alpha * (1 - p).pow(gamma) * (1 - p - gamma * p * torch.log(p.clamp(min=tiny)))
    grad_n = -(1 - alpha) * p.pow(gamma) * (gamma * (1 - p) * torch.log((1 - p).clamp(min=tiny)) - p)
    return torch.where(pos, grad_p, grad_n)


def aligned_iou(a, b):
    """axis_aligned_bbox_overlaps_3d(is_aligned=True) (iou3d_calculator.py:281-323): (n, 6) x (n, 6) -> (n,)."""
    area1 = (a[:, 3] - a[:, 0]) * (a[:, 4] - a[:, 1]) * (a[:, 5] - a[:, 2])
    area2 = (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])
    wh = (torch.min(a[:, 3:], b[:, 3:]) - torch.max(a[:, :3], b[:, :3])).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1] * wh[:, 2]
    union = torch.max(area1 + area2 - overlap, overlap.new_tensor([1e-6]))
    return overlap / union


def flatten_maps(center_preds, bbox_preds, cls_preds, b):
    """Scene b's maps as the reference flattens them: (P,), (P, 6), (P, C)."""
    flat = lambda ms: torch.cat([m[b].permute(1, 2, 3, 0).reshape(-1, m.shape[1]) for m in ms])  # noqa: E731
    return flat(center_preds)[:, 0], flat(bbox_preds), flat(cls_preds)


def upsampled_valid(valid_pred, sizes, b):
    return torch.cat([torch.nn.Upsample(size=tuple(s), mode="trilinear")(valid_pred[b:b + 1].float()).round().bool().reshape(-1)
                      for s in sizes])


def scene_losses(center, bbox, cls, valid, points, targets, gamma=2.0, alpha=0.25, weights=(1.0, 1.0, 1.0)):
    """(center_loss, bbox_loss, cls_loss) of one scene from the flattened maps, the valid mask (P,), the points (P, 3) and the
    targets (labels, box_index, center_targets, bbox_targets); any float dtype (the float64 evaluation uses it too)."""
    labels, _, center_t, bbox_t = targets
    dt = center.dtype
    pos = (labels >= 0) & valid
    n_pos = max(float(pos.sum()), 1.0)
    navg = float(np.float32(n_pos) + np.float32(EPS)) if dt == torch.float32 else n_pos + EPS
    cls_loss = focal_terms(cls[valid], labels[valid], gamma, alpha).sum() / navg
    ct = center_t[pos].to(dt)
    center_loss = torch.nn.functional.binary_cross_entropy_with_logits(center[pos], ct, reduction="none").sum() / navg
    p, d = points[pos].to(dt), bbox[pos]
    pred = torch.stack((p[:, 0] - d[:, 0], p[:, 1] - d[:, 2], p[:, 2] - d[:, 4], p[:, 0] + d[:, 1], p[:, 1] + d[:, 3],
                        p[:, 2] + d[:, 5]), dim=-1)
    bbox_loss = ((1 - aligned_iou(pred, bbox_t[pos].to(dt))) * ct).sum() / (ct.sum() + EPS)
    return center_loss * weights[0], bbox_loss * weights[1], cls_loss * weights[2]


def loss_by_feat(center_preds, bbox_preds, cls_preds, valid_pred, gts, origins, pts_assign_threshold=27, pts_center_threshold=18,
                 gamma=2.0, alpha=0.25, weights=(1.0, 1.0, 1.0), dtype=None):
    """dict(center_loss, bbox_loss, cls_loss) (batch means, with autograd) and the per-scene targets.  gts: per scene (boxes (G, 6),
    volumes (G,), labels (G,)).  dtype=torch.float64: the losses evaluated in float64 on the float32 targets."""
    sizes = [tuple(int(v) for v in c.shape[2:]) for c in center_preds]
    per, all_targets = [], []
    for b, (gt, origin) in enumerate(zip(gts, origins)):
        targets = assign(sizes, origin, gt[0], gt[1], gt[2], pts_assign_threshold, pts_center_threshold)
        all_targets.append(targets)
        center, bbox, cls = flatten_maps(center_preds, bbox_preds, cls_preds, b)
        if dtype is not None:
            center, bbox, cls = center.to(dtype), bbox.to(dtype), cls.to(dtype)
        points = torch.cat([level_points(s, l, origin) for l, s in enumerate(sizes)])
        per.append(scene_losses(center, bbox, cls, upsampled_valid(valid_pred, sizes, b), points, targets, gamma, alpha, weights))
    names = ("center_loss", "bbox_loss", "cls_loss")
    return {n: torch.mean(torch.stack([p[i] for p in per])) for i, n in enumerate(names)}, all_targets


def dense_form_loss(center_preds, bbox_preds, cls_preds, valid_pred, gts, origins, pts_assign_threshold=27, pts_center_threshold=18,
                    gamma=2.0, alpha=0.25):
    """The same losses in the reference's form, on the maps' device: per scene (P, G, 6) face distances, (P, G) masks, topk over
    all points, boolean indexing and its three host reads (len(pos_inds), any(valid), any(weight > 0)).  G >= 1."""
    dev = center_preds[0].device
    sizes = [tuple(int(v) for v in c.shape[2:]) for c in center_preds]
    L = len(sizes)
    per = []
    for b, (gt, origin) in enumerate(zip(gts, origins)):
        boxes, volumes, glabels = (t.to(dev) for t in gt)
        pts = [level_points(s, l, origin).to(dev) for l, s in enumerate(sizes)]
        scales = torch.cat([p.new_tensor(l).expand(len(p)) for l, p in enumerate(pts)])
        points = torch.cat(pts)
        P, G = len(points), len(boxes)
        eb = boxes.expand(P, G, 6)
        ep = points.unsqueeze(1).expand(P, G, 3)
        d = torch.stack((ep[..., 0] - eb[..., 0] + eb[..., 3] / 2, eb[..., 0] + eb[..., 3] / 2 - ep[..., 0],
                         ep[..., 1] - eb[..., 1] + eb[..., 4] / 2, eb[..., 1] + eb[..., 4] / 2 - ep[..., 1],
                         ep[..., 2] - eb[..., 2] + eb[..., 5] / 2, eb[..., 2] + eb[..., 5] / 2 - ep[..., 2]), dim=-1)
        inside = d.min(-1)[0] > 0
        n = torch.stack([torch.sum(inside[scales == l], dim=0) for l in range(L)])
        low = n < pts_assign_threshold
        extra = torch.arange(L, 0, -1, device=dev).unsqueeze(1).expand(L, G)
        lower = (torch.argmax(low.int() * extra, dim=0) - 1).clamp(min=0)
        best = torch.where(torch.all(~low, dim=0), torch.full_like(lower, L - 1), lower)
        at_best = best.unsqueeze(0).expand(P, G) == scales.unsqueeze(1).expand(P, G)
        c = torch.sqrt(d[..., :2].min(-1)[0] / d[..., :2].max(-1)[0] * d[..., 2:4].min(-1)[0] / d[..., 2:4].max(-1)[0]
                       * d[..., 4:].min(-1)[0] / d[..., 4:].max(-1)[0])
        c = torch.where(inside & at_best, c, torch.full_like(c, -1))
        top = c > torch.topk(c, pts_center_threshold + 1, dim=0).values[-1].unsqueeze(0)
        vol = torch.where(inside & at_best & top, volumes.expand(P, G), torch.full((P, G), FLOAT_MAX, device=dev))
        vmin, arg = vol.min(dim=1)
        labels = torch.where(vmin == FLOAT_MAX, torch.full_like(glabels[arg], -1), glabels[arg])
        dsel = d[torch.arange(P, device=dev), arg]
        center_t = torch.sqrt(dsel[:, :2].min(-1)[0] / dsel[:, :2].max(-1)[0] * dsel[:, 2:4].min(-1)[0] / dsel[:, 2:4].max(-1)[0]
                              * dsel[:, 4:].min(-1)[0] / dsel[:, 4:].max(-1)[0])
        bbox_t = torch.stack((points[:, 0] - dsel[:, 0], points[:, 1] - dsel[:, 2], points[:, 2] - dsel[:, 4],
                              points[:, 0] + dsel[:, 1], points[:, 1] + dsel[:, 3], points[:, 2] + dsel[:, 5]), dim=-1)
        center, bbox, cls = flatten_maps(center_preds, bbox_preds, cls_preds, b)
        valid = upsampled_valid(valid_pred, sizes, b)
        pos_inds = torch.nonzero(torch.logical_and(labels >= 0, valid)).squeeze(1)
        n_pos = max(float(len(pos_inds)), 1.0) + EPS                                   # host read 1
        if torch.any(valid):                                                           # host read 2
            cls_loss = focal_terms(cls[valid], labels[valid], gamma, alpha).sum() / n_pos
        else:
            cls_loss = cls[valid].sum()
        if len(pos_inds) > 0:
            ct = center_t[pos_inds]
            center_loss = torch.nn.functional.binary_cross_entropy_with_logits(center[pos_inds], ct, reduction="none").sum() / n_pos
            p, dd = points[pos_inds], bbox[pos_inds]
            pred = torch.stack((p[:, 0] - dd[:, 0], p[:, 1] - dd[:, 2], p[:, 2] - dd[:, 4], p[:, 0] + dd[:, 1], p[:, 1] + dd[:, 3],
                                p[:, 2] + dd[:, 5]), dim=-1)
            if not torch.any(ct > 0):                                                  # host read 3
                bbox_loss = (pred * ct.unsqueeze(1)).sum()
            else:
                bbox_loss = ((1 - aligned_iou(pred, bbox_t[pos_inds])) * ct).sum() / (ct.sum() + EPS)
        else:
            center_loss, bbox_loss = center[pos_inds].sum(), bbox[pos_inds].sum()
        per.append((center_loss, bbox_loss, cls_loss))
    names = ("center_loss", "bbox_loss", "cls_loss")
    return {n: torch.mean(torch.stack([p[i] for p in per])) for i, n in enumerate(names)}


# ---------------------------------------------------------------------------------------------------------------------- scenes
class DepthBoxes:
    """What loss_by_feat reads of mmdet3d's DepthInstance3DBoxes (origin (.5, .5, 0): x, y, bottom z, dx, dy, dz): `tensor`,
    `gravity_center` = the bottom centre raised by half the height, `volume` = dx * dy * dz."""

    def __init__(self, tensor):
        self.tensor = tensor

    def __len__(self):
        return int(self.tensor.shape[0])

    @property
    def device(self):
        return self.tensor.device

    @property
    def gravity_center(self):
        t = self.tensor
        return torch.cat([t[:, :2], (t[:, 2] + t[:, 5] * 0.5).unsqueeze(1)], dim=1)

    @property
    def volume(self):
        return self.tensor[:, 3] * self.tensor[:, 4] * self.tensor[:, 5]

    def to(self, device):
        return DepthBoxes(self.tensor.to(device))


class GtInstances:
    def __init__(self, bboxes_3d, labels_3d):
        self.bboxes_3d, self.labels_3d = bboxes_3d, labels_3d

    def to(self, device):
        return GtInstances(self.bboxes_3d.to(device), self.labels_3d.to(device))


def gt_triplet(gt):
    """(boxes (G, 6), volumes, labels) as _get_targets reads them (nerfdet_head.py:497-500)."""
    b = gt.bboxes_3d
    return torch.cat((b.gravity_center, b.tensor[:, 3:6]), dim=1), b.volume, gt.labels_3d


SCENE_KINDS = ("one", "twelve", "sixty", "no_valid", "valid_no_pos", "five")


def scene_boxes(kind, seed, origin, n_classes, extent):
    """Depth-box tensor (G, 6) and labels (G,) of a planted room around `origin`; extent = the level-0 grid's size in metres."""
    ex = torch.tensor(extent)
    G = {"one": 1, "twelve": 12, "sixty": 60, "no_valid": 5, "valid_no_pos": 4, "five": 5}[kind]
    u = _u((G, 8), seed * 10 + 2)
    size = 0.35 + 0.55 * (u[:, 3:6] + 1) * torch.tensor([1.0, 1.0, 0.6])
    ctr = origin + u[:, :3] * ex * torch.tensor([0.42, 0.42, 0.35])
    if kind == "valid_no_pos":   # every box in the low-x half; the valid voxels are in the high-x half
        ctr[:, 0] = origin[0] - ex[0] * (0.15 + 0.1 * (u[:, 0] + 1))
        size[:, 0] = size[:, 0].clamp(max=0.5)
    if kind == "twelve":
        size[1] = size[0] * 0.45                       # nested in box 0: the least volume decides
        ctr[1] = ctr[0] + 0.05
        size[2] = torch.tensor([0.21, 0.19, 0.23])     # below pts_assign_threshold at every level
        size[3] = ex * 1.2                             # passes the threshold at all levels, and reaches outside the grid
        ctr[3] = origin + torch.tensor([0.03, -0.02, 0.01])
        ctr[4] = origin + ex * torch.tensor([0.47, 0.1, 0.0])   # partly outside the grid
        size[4] = torch.tensor([1.3, 1.1, 0.9])
        size[6] = size[5]                              # two overlapping boxes of equal volume: the lower index wins
        ctr[6] = ctr[5] + torch.tensor([0.11, -0.07, 0.04])
    labels = ((u[:, 6] + 1) * 0.5 * n_classes).long().clamp(max=n_classes - 1)
    tensor = torch.cat([ctr[:, :2], (ctr[:, 2] - size[:, 2] * 0.5).unsqueeze(1), size], dim=1).float()
    return tensor, labels


def scene(kind, seed, levels=SCANNET_LEVELS, n_classes=18):
    """One scene from its seed: (center, bbox, cls) lists over the levels of (1, c, X, Y, Z) float32, valid counts (1, 1) + level 0,
    origin (3,), GtInstances."""
    origin = (torch.tensor([3.0, 3.0, 1.5]) + _u((3,), seed * 10) * torch.tensor([0.5, 0.5, 0.2])).float()
    extent = [levels[0][i] * VOXEL[i] for i in range(3)]
    vshape = (1, 1) + tuple(levels[0])
    uv = _u(vshape, seed * 10 + 1)
    if kind == "no_valid":
        valid = torch.zeros(vshape)
    elif kind == "valid_no_pos":
        valid = torch.zeros(vshape)
        valid[:, :, (3 * levels[0][0]) // 4:] = 2.0
    else:
        valid = torch.floor((uv + 1) * 2.0)            # 0 .. 3 views
    centers, bboxes, clss = [], [], []
    for lvl, size in enumerate(levels):
        s = 100 * (lvl + 1) + seed * 10
        size = tuple(size)
        centers.append((2.0 * _u((1, 1) + size, s + 3)).float().contiguous())
        bboxes.append((0.15 + 0.5 * (2 ** lvl) * (_u((1, 6) + size, s + 4) + 1)).float().contiguous())
        clss.append((3.5 * _u((1, n_classes) + size, s + 5) - 3.0).float().contiguous())
    tensor, labels = scene_boxes(kind, seed, origin, n_classes, extent)
    return centers, bboxes, clss, valid, origin, GtInstances(DepthBoxes(tensor), labels)


def batch(kinds, seeds, levels=SCANNET_LEVELS, n_classes=18):
    scenes = [scene(k, s, levels, n_classes) for k, s in zip(kinds, seeds)]
    cat = lambda j: [torch.cat([sc[j][lvl] for sc in scenes]) for lvl in range(len(levels))]  # noqa: E731
    return cat(0), cat(1), cat(2), torch.cat([sc[3] for sc in scenes]), [sc[4] for sc in scenes], [sc[5] for sc in scenes]


def metas_for(origins):
    return [{"lidar2img": {"origin": o.numpy().astype(np.float32)}} for o in origins]


def ulp(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.spacing(np.maximum(x, np.float32(1e-30)))


def near_decisions(sizes, origin, gt, pts_assign_threshold=27, pts_center_threshold=18):
    """Reasons a scene's assignment could hang on rounding: a face distance within 4 ulp (of its operands' scale) of 0, or a
    candidate's centerness within 4 ulp of its box's boundary value t[g] other than the boundary point itself."""
    boxes, volumes, labels = gt
    why = []
    *_, info = assign(sizes, origin, boxes, volumes, labels, pts_assign_threshold, pts_center_threshold, details=True)
    pts = torch.cat([level_points(s, l, origin) for l, s in enumerate(sizes)])
    for g in range(len(boxes)):
        d = face_distances(pts, boxes[g]).numpy()
        scale = np.maximum(np.abs(pts.numpy()).max(), float(boxes[g].abs().max()) * 1.5)
        if (np.abs(d) <= 4 * ulp(scale)).any():
            why.append(f"box {g}: a face distance within 4 ulp of 0")
        _, _, t, c = info[g]
        if t >= 0:
            close = np.abs(c.numpy() - np.float32(t)) <= 4 * ulp(t)
            if int(close.sum()) != 1:
                why.append(f"box {g}: {int(close.sum())} centerness values within 4 ulp of the boundary")
    return why
