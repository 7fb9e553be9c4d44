"""G21 (tests/golden/make_goldens_g21.py) as the scene lists of tests/indoor_eval_restated.py, and what the reference stored for
them; shared by test_indoor_eval_host.py and test_gpu_indoor_eval.py."""
import functools

import numpy as np

import indoor_eval_restated as R
from conftest import load_golden

CASES = ("scannet", "arkit")


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("g21_indoor_eval")


def scenes_of(case):
    g = golden()
    out = []
    for s in range(len(g[f"{case}_counts"])):
        n, m = int(g[f"{case}_counts"][s]), int(g[f"{case}_gt_counts"][s])
        out.append(dict(boxes=g[f"{case}_boxes"][s, :n], scores=g[f"{case}_scores"][s, :n], labels=g[f"{case}_labels"][s, :n],
                        gt_boxes=g[f"{case}_gt_boxes"][s, :m], gt_labels=g[f"{case}_gt_labels"][s, :m]))
    return out


def thresholds_of(case):
    return tuple(float(v) for v in golden()[f"{case}_thresholds"])


def label2cat_of(case):
    return {i: str(v) for i, v in enumerate(golden()[f"{case}_label2cat"])}


def ret_dict_of(case):
    g = golden()
    return dict(zip((str(k) for k in g[f"{case}_ret_keys"]), (float(v) for v in g[f"{case}_ret_values"])))


def reference_flags(case, t, label):
    """True-positive flags of the reference's walk, from the precision it returned: tp_cum = precision * (tp + fp)."""
    p = golden()[f"{case}_precision_{t}_{label}"]
    cum = np.rint(p * np.arange(1, len(p) + 1)).astype(np.int64)
    return np.diff(np.concatenate(([0], cum))).astype(bool)


@functools.lru_cache(maxsize=None)
def restated(case):
    """R.evaluate of the case, computed once and shared (read only)."""
    return R.evaluate(scenes_of(case), thresholds_of(case))


def same_or_both_nan(a, b, tol=0.0):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


def random_scenes(seed, counts, n_gt, n_labels=1, thresholds=(0.25, 0.5), margin=1e-4):
    """Yaw-0 scenes with counts[s] detections (jittered copies of ground-truth boxes) and n_gt boxes each.  Scores are pairwise
    distinct (a permutation); a detection whose IoUs miss the margins of margins_ok is drawn again."""
    g = np.random.default_rng(seed)
    f = np.float32
    total = int(sum(counts))
    scores = ((g.permutation(total) + 1) / f(total + 1)).astype(f)
    out, at = [], 0
    for nd in counts:
        gb = np.zeros((n_gt, 7), f)
        gb[:, :2], gb[:, 2], gb[:, 3:6] = g.uniform(-2, 2, (n_gt, 2)), g.uniform(0, 1, n_gt), g.uniform(0.5, 1.5, (n_gt, 3))
        gl = g.integers(0, n_labels, n_gt).astype(np.int64)
        src = g.integers(0, n_gt, nd)
        db = np.zeros((nd, 7), f)
        todo = np.arange(nd)
        while len(todo):
            db[todo] = gb[src[todo]]
            db[todo, :3] += g.normal(0, 0.15, (len(todo), 3)).astype(f)
            db[todo, 3:6] *= g.uniform(0.8, 1.25, (len(todo), 3)).astype(f)
            sc = dict(boxes=db, scores=scores[at:at + nd], labels=gl[src], gt_boxes=gb, gt_labels=gl)
            todo = np.array([i for i in todo if not margins_ok([{**sc, "boxes": db[i:i + 1], "scores": sc["scores"][i:i + 1],
                                                                  "labels": sc["labels"][i:i + 1]}], thresholds, margin)], np.int64)
        out.append(dict(boxes=db, scores=scores[at:at + nd], labels=gl[src], gt_boxes=gb, gt_labels=gl))
        at += nd
    return out


def margins_ok(scenes, thresholds, margin=1e-4):
    """The conditions of G21 on random inputs: distinct scores inside a label, iou_max `margin` off every threshold, the two
    largest IoUs of a detection `margin` apart (or both exactly 0)."""
    rows, _, _ = R.match(scenes)
    for lab in {r[0] for r in rows}:
        sc = [r[1] for r in rows if r[0] == lab]
        if len(set(sc)) != len(sc):
            return False
    for r in rows:
        best, second = float(r[5]), float(r[6])
        if np.isfinite(best) and any(abs(best - t) < margin for t in thresholds):
            return False
        if np.isfinite(second) and best - second < margin and not (best == 0.0 and second == 0.0):
            return False
    return True
