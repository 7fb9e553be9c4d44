"""The ScanNet head's predict_by_feat (nerfdet_head.py:21-34, 301-420, 564-628) restated in float32 torch on the CPU, the yardstick
of the detection kernels at any level count, level shape and class count (a helper module: nothing here is collected).

predict() follows the reference op for op: nn.Upsample(trilinear) of the view counts, .round().bool(); cls.sigmoid() *
center.sigmoid() * valid; max over the classes (first argmax); the top nms_pre of a level; get_points and the box decode;
score > score_thr; the greedy walk of test_detect_host.nms_restated over the levels' candidates; the conversion to centre and size.
Where the reference leaves an order open it takes the kernels' convention: top-k by score descending (NaN largest), then voxel
index; a level's candidates in voxel order, the levels concatenated level-major; equal scores in the walk by that candidate index.
A scene with more than DETECT_MAX_CANDIDATES survivors is reported as the kernels report it: count -n, no boxes.

near_decisions() lists what could flip under an ulp of sigmoid / exp between two devices (G15's screen, make_goldens_g15.py, for
any levels and classes): an upsampled view count within 1e-5 of 0.5 but not 0.5, a max-score within 1e-5 of score_thr, a level's
top-k boundary within 1e-5, equal survivor scores (the reference's argsort leaves their order open), a same-class IoU of the walk
within 1e-4 of iou_thr."""
import numpy as np
import torch

from test_detect_host import nms_restated

VOXEL = (.16, .16, .2)
DETECT_MAX_CANDIDATES = 16384


def get_points(size, level, origin):
    """get_points of one level, (X*Y*Z, 3) float32, as the reference's _get_points computes it."""
    n_voxels = torch.tensor(list(size))
    voxel_size = torch.tensor(VOXEL) * (2 ** level)
    points = torch.stack(torch.meshgrid([torch.arange(s) for s in size], indexing="ij"))
    new_origin = origin - n_voxels / 2. * voxel_size
    return (points * voxel_size.view(3, 1, 1, 1) + new_origin.view(3, 1, 1, 1)).reshape(3, -1).transpose(0, 1)


def topk_ids(ms, k):
    """Indices of the k largest of ms (NaN largest, equal values by lower index), in ascending (voxel) order."""
    s = ms.numpy()
    nan = np.isnan(s)
    order = np.lexsort((np.arange(len(s)), -np.where(nan, np.float32(0), s), ~nan))
    return np.sort(order[:k])


def level_scores(c, k, vm):
    """(N, C) scores and the (N,) max-score and first argmax of one scene's level."""
    C = k.shape[0]
    scores = k.permute(1, 2, 3, 0).reshape(-1, C).sigmoid() * c.permute(1, 2, 3, 0).reshape(-1, 1).sigmoid() \
        * vm.permute(1, 2, 3, 0).reshape(-1, 1)
    a = scores.numpy()
    lab = np.argmax(a, axis=1)            # the first maximum; a NaN counts as the maximum (the first NaN)
    return scores, torch.from_numpy(a[np.arange(len(a)), lab]), torch.from_numpy(lab.astype(np.int64))


def upsampled_valid(valid_pred, sizes):
    """nn.Upsample(size, trilinear)(valid_pred) per level, before .round().bool()."""
    return [torch.nn.Upsample(size=tuple(s), mode="trilinear")(valid_pred.float()) for s in sizes]


def candidates(center_preds, bbox_preds, cls_preds, valid_pred, b, origin, nms_pre, ups=None):
    """Scene b's candidates, level-major and in voxel order within a level: boxes (n, 6), scores (n,), labels (n,) and the per-level
    (max-scores, top-k ids) that chose them."""
    sizes = [tuple(x.shape[-3:]) for x in center_preds]
    ups = ups if ups is not None else upsampled_valid(valid_pred, sizes)
    boxes, scores, labels, levels = [], [], [], []
    for lvl, size in enumerate(sizes):
        vm = ups[lvl][b].round().bool()
        _, ms, lab = level_scores(center_preds[lvl][b], cls_preds[lvl][b], vm)
        ids = topk_ids(ms, nms_pre) if len(ms) > nms_pre > 0 else np.arange(len(ms))
        levels.append((ms, ids))
        ids = torch.from_numpy(ids)
        point = get_points(size, lvl, origin)[ids]
        bp = bbox_preds[lvl][b].permute(1, 2, 3, 0).reshape(-1, 6)[ids]
        boxes.append(torch.stack([point[:, 0] - bp[:, 0], point[:, 1] - bp[:, 2], point[:, 2] - bp[:, 4],
                                  point[:, 0] + bp[:, 1], point[:, 1] + bp[:, 3], point[:, 2] + bp[:, 5]], -1))
        scores.append(ms[ids])
        labels.append(lab[ids])
    return torch.cat(boxes), torch.cat(scores), torch.cat(labels), levels


def predict(center_preds, bbox_preds, cls_preds, valid_pred, origins, nms_pre, score_thr, iou_thr):
    """Per scene a dict: boxes (n, 6) float32 (cx, cy, cz, dx, dy, dz), scores (n,), labels (n,) int64, count n in pick order; or
    count -m and empty arrays when m > DETECT_MAX_CANDIDATES boxes pass score_thr.  Maps: per level (B, 1|6|C, X, Y, Z) float32 CPU
    tensors; valid_pred (B, 1, VX, VY, VZ); origins: B float32 (3,) tensors."""
    sizes = [tuple(x.shape[-3:]) for x in center_preds]
    ups = upsampled_valid(valid_pred, sizes)
    out = []
    with torch.no_grad():
        for b in range(valid_pred.shape[0]):
            bx, sc, lb, _ = candidates(center_preds, bbox_preds, cls_preds, valid_pred, b, origins[b], nms_pre, ups)
            keep = sc > score_thr
            bx, sc, lb = bx[keep], sc[keep], lb[keep]
            if len(sc) > DETECT_MAX_CANDIDATES:
                out.append(dict(count=-len(sc), boxes=np.zeros((0, 6), np.float32), scores=np.zeros(0, np.float32),
                                labels=np.zeros(0, np.int64)))
                continue
            ids = torch.from_numpy(nms_restated(bx.numpy(), sc.numpy(), lb.numpy(), iou_thr))
            bx = bx[ids]
            bx = torch.stack(((bx[:, 0] + bx[:, 3]) / 2., (bx[:, 1] + bx[:, 4]) / 2., (bx[:, 2] + bx[:, 5]) / 2.,
                              bx[:, 3] - bx[:, 0], bx[:, 4] - bx[:, 1], bx[:, 5] - bx[:, 2]), dim=1)
            out.append(dict(count=len(ids), boxes=bx.numpy(), scores=sc[ids].numpy(), labels=lb[ids].numpy()))
    return out


def near_decisions(center_preds, bbox_preds, cls_preds, valid_pred, origins, nms_pre, score_thr, iou_thr):
    """Reasons a result could flip under an ulp of sigmoid / exp (empty: none); see the module's docstring."""
    sizes = [tuple(x.shape[-3:]) for x in center_preds]
    ups = upsampled_valid(valid_pred, sizes)
    why = []
    for lvl, u in enumerate(ups):
        if (((u - 0.5).abs() < 1e-5) & (u != 0.5)).any():
            why.append(f"level {lvl}: an upsampled view count near 0.5")
    with torch.no_grad():
        for b in range(valid_pred.shape[0]):
            bx, sc, lb, levels = candidates(center_preds, bbox_preds, cls_preds, valid_pred, b, origins[b], nms_pre, ups)
            for lvl, (ms, ids) in enumerate(levels):
                m = ms.double()
                if ((m - score_thr).abs() <= 1e-5 * abs(score_thr)).any():
                    why.append(f"scene {b} level {lvl}: a max-score at score_thr")
                if len(m) > nms_pre > 0:
                    srt = m[~m.isnan()].sort(descending=True).values
                    k = nms_pre - int(m.isnan().sum())
                    if 0 < k < len(srt) and float(srt[k - 1]) > score_thr and \
                            abs(float(srt[k - 1] - srt[k])) <= 1e-5 * abs(float(srt[k - 1])):   # else neither survives
                        why.append(f"scene {b} level {lvl}: top-k boundary")
            keep = sc > score_thr
            bx, sc, lb = bx[keep].double().numpy(), sc[keep].numpy(), lb[keep].numpy()
            if len(np.unique(sc)) != len(sc):
                why.append(f"scene {b}: equal survivor scores")
            if not 0 < len(sc) <= DETECT_MAX_CANDIDATES:
                continue
            order = nms_restated(bx.astype(np.float32), sc, lb, iou_thr)
            # every same-class IoU the walk evaluates between a picked box and a later one, in float64
            area = (bx[:, 3] - bx[:, 0]) * (bx[:, 4] - bx[:, 1]) * (bx[:, 5] - bx[:, 2])
            rank = np.empty(len(sc), np.int64)
            srt = np.lexsort((np.arange(len(sc)), -sc))
            rank[srt] = np.arange(len(sc))
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                for i in order:
                    j = np.nonzero((rank > rank[i]) & (lb == lb[i]))[0]
                    if len(j) == 0:
                        continue
                    lo, hi = np.maximum(bx[i, :3], bx[j, :3]), np.minimum(bx[i, 3:], bx[j, 3:])
                    inter = np.prod(np.maximum(hi - lo, 0), axis=1)
                    iou = inter / (area[i] + area[j] - inter)
                    if (np.abs(iou - iou_thr) < 1e-4).any():
                        why.append(f"scene {b}: an IoU at iou_thr")
                        break
    return why


# ------------------------------------------------------------------------------------------------------------ inputs
def random_maps(sizes, valid_shape, C, B, seed, cls_bias=-4.5):
    """General head maps from a seed (torch's CPU generator): per level center (B,1,...), bbox (B,6,...) > 0 and cls (B,C,...)
    logits, view counts 0..4 (B,1,*valid_shape) and B float32 origins, as G15's random scenes are drawn."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(shape, generator=g) * 2 - 1  # noqa: E731
    centers = [2.0 * u(B, 1, *s) for s in sizes]
    bboxes = [0.05 + 0.1 * (u(B, 6, *s) + 1) for s in sizes]
    clss = [3.5 * u(B, C, *s) + cls_bias for s in sizes]
    valid = torch.floor((u(B, 1, *valid_shape) + 1) * 2.5)
    origins = [(torch.tensor([3.0, 3.0, 1.5]) + u(3) * torch.tensor([.5, .5, .2])).float() for _ in range(B)]
    return centers, bboxes, clss, valid, origins


RAGGED = ((21, 19, 8), (11, 10, 4), (6, 5, 2), (3, 3, 1))     # against a 41x37x15 valid volume: no ratio is an integer
# family (a): name -> (level sizes, valid volume, classes, scenes, nms_pre, cls_bias, seed); seeds with no near decision
CASES_A = {
    "l1_c18": (((40, 40, 16),), (40, 40, 16), 18, 1, 1000, -4.5, 101),
    "l4_ragged_c40_b3_pre440": (RAGGED, (41, 37, 15), 40, 3, 440, -4.5, 103),
    "l4_ragged_c1_pre439": (RAGGED, (41, 37, 15), 1, 1, 439, -4.5, 104),
    "l4_ragged_c2_b3_pre441": (RAGGED, (41, 37, 15), 2, 3, 441, -4.5, 106),
    "l2_larger_than_valid_c2_pre0": (((43, 39, 17), (11, 10, 4)), (41, 37, 15), 2, 1, 0, -7.5, 100),
    "l2_larger_than_valid_c18_b3_pre1": (((43, 39, 17), (11, 10, 4)), (41, 37, 15), 18, 3, 1, -4.5, 101),
    "l3_scannet_c40_b3_pre1000": (((40, 40, 16), (20, 20, 8), (10, 10, 4)), (40, 40, 16), 40, 3, 1000, -4.5, 102),
}
SCORE_THR, IOU_THR = 0.01, 0.25


def case_a(name):
    sizes, vshape, C, B, nms_pre, bias, seed = CASES_A[name]
    return random_maps(sizes, vshape, C, B, seed, bias), nms_pre
