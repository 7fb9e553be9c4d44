"""mmdet3d's indoor_eval (eval_det_cls + average_precision + the dict assembly, indoor_eval.py:8-302) restated in NumPy / float64
without its walk over box objects, and BaseInstance3DBoxes.overlaps (base_box3d.py:496-590) from exact float64 geometry rounded to
float32.  The yardstick of csrc/evalmap.hip and the `overlaps` stand-in of tests/golden/make_goldens_g21.py.

Boxes are the box classes' rows (x, y, bottom z, dx, dy, dz, yaw).  A scene is a dict: boxes (n,7) float32, scores (n) float32,
labels (n) int64, gt_boxes (g,7) float32, gt_labels (g) int64.

The restated walk: the index jmax of a detection's best box (first of equal IoUs, strict >) does not depend on the threshold, and
the reference never falls back to a second-best box; so a detection is a true positive at t exactly when iou_max > t and it is the
first, in visiting order, of the detections with the same (scene, jmax) and iou_max > t.  Visiting order: score descending, NaN
last (np.argsort(-confidence)); equal scores by (scene, row), where the reference's unstable argsort leaves the order open."""
import numpy as np

from nms3d_restated import exact_iou

F = np.float32


def iou3d(a, b):
    """(n, m) float32: overlaps(a, b) of boxes (n,7) and (m,7), every operation in float64 on the float32 inputs."""
    a, b = np.asarray(a, F).reshape(-1, 7).astype(np.float64), np.asarray(b, F).reshape(-1, 7).astype(np.float64)
    out = np.zeros((len(a), len(b)), np.float64)
    for i, p in enumerate(a):
        for j, q in enumerate(b):
            oh = max(min(p[2] + p[5], q[2] + q[5]) - max(p[2], q[2]), 0.0)
            pw, pl, qw, ql = max(p[3], 1e-4), max(p[4], 1e-4), max(q[3], 1e-4), max(q[4], 1e-4)
            if p[6] == 0.0 and q[6] == 0.0:
                ox = min(p[0] + pw / 2, q[0] + qw / 2) - max(p[0] - pw / 2, q[0] - qw / 2)
                oy = min(p[1] + pl / 2, q[1] + ql / 2) - max(p[1] - pl / 2, q[1] - ql / 2)
                area = max(ox, 0.0) * max(oy, 0.0)
            else:
                pb, qb = (p[0], p[1], 0, pw, pl, 0, p[6]), (q[0], q[1], 0, qw, ql, 0, q[6])
                iou2d = exact_iou(pb, qb)
                area = iou2d * (pw * pl + qw * ql) / (1 + iou2d)    # the reference's own recovery of the intersection
            ov = area * oh
            out[i, j] = ov / max(p[3] * p[4] * p[5] + q[3] * q[4] * q[5] - ov, 1e-8)
    return out.astype(F)


def visiting_order(scores, scene, row):
    s = np.asarray(scores, F).astype(np.float64)
    nan = np.isnan(s)
    return np.lexsort((row, scene, np.where(nan, 0.0, -s), nan))


def average_precision(recall, precision):
    """average_precision(mode='area') of one row."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([0.0], precision, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    ind = np.where(mrec[1:] != mrec[:-1])[0]
    with np.errstate(invalid="ignore"):
        return F(np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1]))


def match(scenes, iou_fn=iou3d):
    """One row per detection in feeding order: (label, score, scene, row, slot, iou_max, second) -- slot = (scene, j) of the best
    ground-truth box as a global index over the scenes' boxes in order (-1: none), second = the runner-up IoU (-inf: none) -- and
    the label order of the reference's dicts, {label: npos}."""
    rows, first, npos = [], {}, {}
    base = 0
    for sid, sc in enumerate(scenes):
        labels, gl = np.asarray(sc["labels"]).reshape(-1), np.asarray(sc["gt_labels"]).reshape(-1)
        for i, lab in enumerate(labels):
            first.setdefault(int(lab), len(first))
            npos.setdefault(int(lab), 0)
            js = np.nonzero(gl == lab)[0]
            best, jbest, second = -np.inf, -1, -np.inf
            if len(js):
                v = iou_fn(np.asarray(sc["boxes"], F)[i:i + 1], np.asarray(sc["gt_boxes"], F)[js])[0]
                for j, x in zip(js, v):
                    if x > best:
                        second, best, jbest = best, x, int(j)
                    elif x > second:
                        second = x
            rows.append((int(lab), F(sc["scores"][i]), sid, i, base + jbest if jbest >= 0 else -1, F(best), F(second)))
        for lab in gl:
            first.setdefault(int(lab), len(first))
            npos[int(lab)] = npos.get(int(lab), 0) + 1
        base += len(gl)
    return rows, sorted(first, key=first.get), npos


def evaluate(scenes, thresholds, iou_fn=iou3d):
    """{label: dict(npos, ndet, index (record index in visiting order), tp (T,nd) bool, recall (T,nd), precision (T,nd), ap (T,)
    float32)} in the order of the reference's dicts; a label without predictions has ndet 0 and empty arrays."""
    rows, order, npos = match(scenes, iou_fn)
    out = {}
    for lab in order:
        idx = np.array([k for k, r in enumerate(rows) if r[0] == lab], np.int64)
        T = len(thresholds)
        if len(idx) == 0:
            out[lab] = dict(npos=npos[lab], ndet=0, index=idx, tp=np.zeros((T, 0), bool), recall=np.zeros((T, 0)),
                            precision=np.zeros((T, 0)), ap=np.zeros(T, F))
            continue
        sel = [rows[k] for k in idx]
        vis = visiting_order([r[1] for r in sel], [r[2] for r in sel], [r[3] for r in sel])
        idx = idx[vis]
        slot = np.array([rows[k][4] for k in idx])
        iou = np.array([rows[k][5] for k in idx], F)
        tp = np.zeros((T, len(idx)), bool)
        rec, pre, ap = np.zeros((T, len(idx))), np.zeros((T, len(idx))), np.zeros(T, F)
        for t, thr in enumerate(thresholds):
            above = iou > F(thr)
            seen = set()
            for k in np.nonzero(above)[0]:
                if slot[k] not in seen:
                    seen.add(slot[k])
                    tp[t, k] = True
            ctp, cfp = np.cumsum(tp[t].astype(np.float64)), np.cumsum((~tp[t]).astype(np.float64))
            with np.errstate(invalid="ignore", divide="ignore"):
                rec[t] = ctp / float(npos[lab])
            pre[t] = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
            ap[t] = average_precision(rec[t], pre[t])
        out[lab] = dict(npos=npos[lab], ndet=len(idx), index=idx, tp=tp, recall=rec, precision=pre, ap=ap)
    return out


def assemble(labels, ap, rec_last, ndet, thresholds, label2cat):
    """indoor_eval's ret_dict (:266-289) from per-label values: labels in the dicts' order, ap[t][k] float32, rec_last[t][k]
    float64, ndet[k].  A label without predictions contributes the reference's float64 zeros(1), the others float32 arrays of one
    value: the dtype in which np.mean rounds mAP follows from that."""
    ret = {}
    for t, thr in enumerate(thresholds):
        aps = [np.zeros(1) if ndet[k] == 0 else np.array([ap[t][k]], F) for k in range(len(labels))]
        recs = [np.float64(0.0) if ndet[k] == 0 else np.float64(rec_last[t][k]) for k in range(len(labels))]
        for k, lab in enumerate(labels):
            ret[f"{label2cat[lab]}_AP_{thr:.2f}"] = float(aps[k][0])
        ret[f"mAP_{thr:.2f}"] = float(np.mean(aps))
        for k, lab in enumerate(labels):
            ret[f"{label2cat[lab]}_rec_{thr:.2f}"] = float(recs[k])
        ret[f"mAR_{thr:.2f}"] = float(np.mean(recs))
    return ret


def indoor_eval(scenes, thresholds, label2cat, iou_fn=iou3d):
    ev = evaluate(scenes, thresholds, iou_fn)
    labels = list(ev)
    ap = [[ev[l]["ap"][t] for l in labels] for t in range(len(thresholds))]
    rec = [[ev[l]["recall"][t][-1] if ev[l]["ndet"] else 0.0 for l in labels] for t in range(len(thresholds))]
    return assemble(labels, ap, rec, [ev[l]["ndet"] for l in labels], thresholds, label2cat)
