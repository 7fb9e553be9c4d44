"""G21: mmdet3d's indoor_eval on two small random detection sets -> tests/golden/g21_indoor_eval.npz (arrays and key lists only).

The generator executes the reference's own mmdet3d/evaluation/functional/indoor_eval.py where it lies (MVSDET_REFERENCE; nothing of
it is stored), with three stand-ins for what is not installed, each named in the fixture's `stand_in` entry:
  * mmengine.logging.print_log: drops the table;
  * terminaltables.AsciiTable: holds the rows, `.table` is their plain join;
  * ONE box class (tensor, __len__, __getitem__, new_box, convert_to, classmethod overlaps) whose `overlaps` is
    tests/indoor_eval_restated.iou3d: BaseInstance3DBoxes.overlaps from exact float64 geometry, rounded to float32 -- the
    mathematical function, NOT mmcv's box_iou_rotated rounding (mmcv is not installed; the distance to its float32 result is unknown).

Cases (each at its first seed that meets the conditions below; the seed is recorded):
  scannet: 18 labels, yaw 0, 12 scenes with 0-9 boxes and 0-60 detections;
  arkit:   17 labels, yaws over the whole circle, the same sizes.
Each holds a label with ground truth and no prediction, a scene without boxes of a predicted label, a scene with no detections and
two overlapping boxes of one label; the ARKit case also a label predicted without ground truth anywhere (NaN AP, NaN mAP and mAR).

Conditions on the random inputs, asserted here, so that no detection is left out of a comparison with float32 device arithmetic:
scores pairwise distinct inside a label; every iou_max at least 1e-4 from both thresholds (1e-4 = ten times the 1e-5 the device IoU is
allowed against exact geometry); the two largest IoUs of a detection at least 1e-4 apart -- except where both are exactly 0 (the
detection's column range or height range is disjoint from both boxes: below every positive threshold whichever index is kept).

Stored per case <c>: <c>_boxes (S,N,7), <c>_scores, <c>_labels, <c>_counts, <c>_gt_boxes (S,G,7), <c>_gt_labels, <c>_gt_counts,
<c>_thresholds, <c>_label2cat, <c>_ret_keys / <c>_ret_values (ret_dict in order), <c>_label_order (the dicts' label order),
<c>_ap (T,L) and per (threshold t, label l) <c>_recall_<t>_<l>, <c>_precision_<t>_<l> of eval_map_recall, <c>_seed."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import indoor_eval_restated as R  # noqa: E402

REF_ROOT = os.environ.get("MVSDET_REFERENCE", "/root/reference")
THRESHOLDS = (0.25, 0.5)
S, NMAX, GMAX = 12, 60, 9
STAND_IN = ("mmengine.logging.print_log: no-op; terminaltables.AsciiTable: rows joined as text; box class: one stand-in with "
            "tensor / __len__ / __getitem__ / new_box / convert_to and overlaps = tests/indoor_eval_restated.iou3d (exact float64 "
            "geometry rounded to float32: the mathematical function, not mmcv's box_iou_rotated rounding)")


class Box:
    def __init__(self, tensor):
        self.tensor = torch.as_tensor(tensor, dtype=torch.float32).reshape(-1, 7)

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, i):
        return Box(self.tensor[i].reshape(-1, 7))

    def new_box(self, data):
        return Box(data)

    def convert_to(self, dst, rt_mat=None):
        return self

    @classmethod
    def overlaps(cls, boxes1, boxes2, mode="iou"):
        return torch.from_numpy(R.iou3d(boxes1.tensor.numpy(), boxes2.tensor.numpy()))


def load_reference_indoor_eval():
    path = os.path.join(REF_ROOT, "mmdet3d", "evaluation", "functional", "indoor_eval.py")
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    saved = {k: sys.modules.get(k) for k in ("mmengine", "mmengine.logging", "terminaltables")}
    me, ml, tt = types.ModuleType("mmengine"), types.ModuleType("mmengine.logging"), types.ModuleType("terminaltables")
    ml.print_log = lambda *a, **k: None
    me.logging = ml

    class AsciiTable:
        def __init__(self, data):
            self.table = "\n".join(" ".join(map(str, r)) for r in data)

    tt.AsciiTable = AsciiTable
    sys.modules.update({"mmengine": me, "mmengine.logging": ml, "terminaltables": tt})
    try:
        spec = importlib.util.spec_from_file_location("ref_indoor_eval", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def make_scenes(n_labels, rotated, seed, with_ghost):
    """Ground truth drawn from the labels 0 .. n_labels-3 (label n_labels-3 never predicted, label n_labels-2 predicted only,
    label n_labels-1 unused); detections = jittered copies of ground-truth boxes, some under another label, plus stray boxes."""
    g = np.random.default_rng(seed)
    f = np.float32
    n_used = n_labels - 3
    lonely_gt, ghost = n_labels - 3, n_labels - 2
    weights = 1.0 / (1 + np.arange(n_used))
    weights /= weights.sum()
    scenes = []
    for sid in range(S):
        ng = int(g.integers(0, GMAX + 1)) if sid not in (3, 7) else (0 if sid == 3 else GMAX)
        nd = int(g.integers(0, NMAX + 1)) if sid not in (5, 7) else (0 if sid == 5 else NMAX)
        gl = g.choice(n_used, size=ng, p=weights).astype(np.int64)
        if sid == 7:
            gl[0] = lonely_gt
            gl[1], gl[2] = 0, 0
        gb = np.zeros((ng, 7), f)
        gb[:, :2] = g.uniform(-3, 3, (ng, 2))
        gb[:, 2] = g.uniform(0, 1, ng)
        gb[:, 3:6] = g.uniform(0.4, 1.6, (ng, 3))
        if ng > 2 and sid == 7:
            gb[2, :3] = gb[1, :3] + f(0.3)          # two boxes of one label that overlap: the runner-up IoU is not 0
        if rotated:
            gb[:, 6] = g.uniform(-np.pi, np.pi, ng)
        db, dl = np.zeros((nd, 7), f), np.zeros(nd, np.int64)
        for i in range(nd):
            kind = g.uniform()
            if ng and kind < 0.75:
                j = int(g.integers(ng))
                db[i] = gb[j]
                db[i, :3] += g.normal(0, 0.18, 3)
                db[i, 3:6] *= g.uniform(0.75, 1.3, 3)
                if rotated:
                    db[i, 6] += g.normal(0, 0.25)
                dl[i] = gl[j] if kind < 0.65 else g.integers(n_used)
                if gl[j] == lonely_gt:
                    dl[i] = 0
            else:
                db[i, :2] = g.uniform(-3, 3, 2)
                db[i, 2] = g.uniform(0, 1)
                db[i, 3:6] = g.uniform(0.4, 1.6, 3)
                if rotated:
                    db[i, 6] = g.uniform(-np.pi, np.pi)
                dl[i] = ghost if with_ghost and g.uniform() >= 0.9 else g.integers(n_used)
        if sid == 7 and with_ghost:
            dl[0] = ghost
        scenes.append(dict(boxes=db.astype(f), scores=g.uniform(0.01, 1, nd).astype(f), labels=dl, gt_boxes=gb.astype(f),
                           gt_labels=gl))
    return scenes


def conditions_hold(scenes):
    rows, _, _ = R.match(scenes)
    for lab in {r[0] for r in rows}:
        sc = [r[1] for r in rows if r[0] == lab]
        if len(set(sc)) != len(sc):
            return False
    for r in rows:
        best, second = float(r[5]), float(r[6])
        if np.isfinite(best) and any(abs(best - t) < 1e-4 for t in THRESHOLDS):
            return False
        if np.isfinite(second) and best - second < 1e-4 and not (best == 0.0 and second == 0.0):
            return False
    return True


def case_has_the_planted_features(scenes, with_ghost):
    det = {int(l) for s in scenes for l in s["labels"]}
    gt = {int(l) for s in scenes for l in s["gt_labels"]}
    lonely = bool(gt - det) and bool(det - gt) == with_ghost
    no_det = any(len(s["labels"]) == 0 and len(s["gt_labels"]) > 0 for s in scenes)
    missing = any(set(map(int, s["labels"])) - set(map(int, s["gt_labels"])) for s in scenes)
    rows, _, _ = R.match(scenes)
    runner_up = any(np.isfinite(r[6]) and r[6] > 0 for r in rows)
    return lonely and no_det and missing and runner_up


def run_reference(mod, scenes, label2cat):
    captured = {}
    inner = mod.eval_map_recall

    def spy(pred, gt, ovthresh=None):
        captured["out"] = inner(pred, gt, ovthresh)
        return captured["out"]

    mod.eval_map_recall = spy
    try:
        gt_annos = [dict(gt_bboxes_3d=Box(s["gt_boxes"]), gt_labels_3d=s["gt_labels"]) for s in scenes]
        dt_annos = [dict(bboxes_3d=Box(s["boxes"]), scores_3d=torch.from_numpy(s["scores"]), labels_3d=torch.from_numpy(s["labels"]))
                    for s in scenes]
        with np.errstate(invalid="ignore", divide="ignore"):
            ret = mod.indoor_eval(gt_annos, dt_annos, list(THRESHOLDS), label2cat)
    finally:
        mod.eval_map_recall = inner
    return ret, captured["out"]


def main():
    mod = load_reference_indoor_eval()
    out = dict(stand_in=np.array(STAND_IN))
    for name, n_labels, rotated in (("scannet", 18, False), ("arkit", 17, True)):   # the ARKit case holds the NaN label
        make = lambda s: make_scenes(n_labels, rotated, s, rotated)  # noqa: E731
        seed = next(s for s in range(1000) if conditions_hold(sc := make(s))
                    and case_has_the_planted_features(sc, rotated))
        scenes = make(seed)
        assert conditions_hold(scenes) and case_has_the_planted_features(scenes, rotated)
        label2cat = {i: f"{name}{i:02d}" for i in range(n_labels)}
        ret, (rec, prec, ap) = run_reference(mod, scenes, label2cat)
        # the restatement, on the CPU, against the reference alone: every value of ret_dict, NaN included
        mine = R.indoor_eval(scenes, THRESHOLDS, label2cat)
        assert list(mine) == list(ret), "key order"
        for k in ret:
            assert (np.isnan(ret[k]) and np.isnan(mine[k])) or abs(ret[k] - mine[k]) <= 2.0 ** -24, (k, ret[k], mine[k])
        assert np.isnan(ret["mAP_0.25"]) == rotated
        pad = lambda rows, w, dt: np.stack([np.concatenate([np.asarray(r, dt).reshape((-1,) + w),  # noqa: E731
                                                            np.zeros((m - len(r),) + w, dt)]) for r in rows])
        m = NMAX
        out[f"{name}_boxes"] = pad([s["boxes"] for s in scenes], (7,), np.float32)
        out[f"{name}_scores"] = pad([s["scores"] for s in scenes], (), np.float32)
        out[f"{name}_labels"] = pad([s["labels"] for s in scenes], (), np.int64)
        out[f"{name}_counts"] = np.array([len(s["labels"]) for s in scenes], np.int32)
        m = GMAX
        out[f"{name}_gt_boxes"] = pad([s["gt_boxes"] for s in scenes], (7,), np.float32)
        out[f"{name}_gt_labels"] = pad([s["gt_labels"] for s in scenes], (), np.int64)
        out[f"{name}_gt_counts"] = np.array([len(s["gt_labels"]) for s in scenes], np.int32)
        out[f"{name}_thresholds"] = np.array(THRESHOLDS, np.float64)
        out[f"{name}_label2cat"] = np.array([label2cat[i] for i in range(n_labels)])
        out[f"{name}_ret_keys"] = np.array(list(ret))
        out[f"{name}_ret_values"] = np.array(list(ret.values()), np.float64)
        order = list(ap[0].keys())
        out[f"{name}_label_order"] = np.array(order, np.int64)
        out[f"{name}_ap"] = np.array([[float(ap[t][l][0]) for l in order] for t in range(len(THRESHOLDS))], np.float64)
        for t in range(len(THRESHOLDS)):
            for l in order:
                out[f"{name}_recall_{t}_{l}"] = np.asarray(rec[t][l], np.float64)
                out[f"{name}_precision_{t}_{l}"] = np.asarray(prec[t][l], np.float64)
        out[f"{name}_seed"] = np.array(seed)
        nd = int(out[f"{name}_counts"].sum())
        print(name, "seed", seed, "detections", nd, "boxes", int(out[f"{name}_gt_counts"].sum()), "labels", len(order),
              "mAP", ret["mAP_0.25"], "mAR", ret["mAR_0.25"])
    path = os.path.join(HERE, "g21_indoor_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
