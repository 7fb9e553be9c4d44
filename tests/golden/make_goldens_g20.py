#!/usr/bin/env python3
"""Generate tests/golden/g20_depth_diag.npz by RUNNING THE REFERENCE (build container only: needs the reference tree).

G20: the gt_depth branch of the reference's `backproject_Weigh` (mvsdet.py:1435-1484), unmodified, on the inputs of fixture G5 (ScanNet-
like and ARKit-like; loaded from g5_backproject_*.npz, not stored again).  Two inputs are new, neither is stored:

  depth_mean  (N,h,w)      sum_j est_depth * est_dens / sum_j est_dens of G5's three candidates, formed in float64 and rounded to fp32
                           (`depth_mean_of`) -- the branch takes any depth map here; the detector hands it the depth expectation.
  gt_depth    (N,239,320)  tests/depth_diag_planted.py: a smooth surface near the first candidate plus LCG noise, two zero rectangles
                           per view, the LAST view all zeros; then single pixels moved until the margins below hold.  The moved
                           pixels are stored (`bumps`), so the tests rebuild the map from the seed and that list.

Stored per case: gap_all and rmse as the reference returns them; what it prints per view (:1480: orig_gap - new_gap, n_reduce, gap_i,
5 decimals), parsed; the number of views it skipped (:1464); the margins -- also ASSERTED here: no original_valid voxel has z within
1e-4 of g -+ vz, no resized value lies in (0, 1e-5).  The volume and valid returned beside them are checked to be bit-identical to
G5's (the branch does not touch them).

    python tests/golden/make_goldens_g20.py
"""
import contextlib
import io
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import depth_diag_planted as planted  # noqa: E402
from depth_diag_restated import margins, resize_aten_cpu  # noqa: E402

GT_HW = (239, 320)
SEEDS = {"scannet": 2001, "arkit": 2002}
LINE = re.compile(r"orig_gap - new_gap: (-?[\d.]+|nan), reduce (-?\d+) voxels, weight_gap vs gt: (-?[\d.]+|nan)")


def depth_mean_of(g5):
    ed, en = g5["est_depth"].astype(np.float64), g5["est_dens"].astype(np.float64)
    return ((ed * en).sum(1) / en.sum(1)).astype(np.float32)


def base_gt_of(g5, tag):
    N = g5["est_depth"].shape[0]
    return planted.base_gt(g5["est_depth"][:, 0], GT_HW[0], GT_HW[1], SEEDS[tag], zero_view=N - 1)


def run(tag):
    from _ref_loader import load_reference
    ref, _ = load_reference()
    g5 = np.load(os.path.join(HERE, f"g5_backproject_{tag}.npz"))
    h, w = int(g5["img_shape"][0] // 4), int(g5["img_shape"][1] // 4)
    vz = float(g5["voxel_size"][-1])
    N = g5["est_depth"].shape[0]
    gt = base_gt_of(g5, tag)
    bumps = planted.plant(gt, g5["x"], g5["y"], g5["z"], h, w, vz)
    g = resize_aten_cpu(gt, h, w)
    win, pos = margins(g5["x"], g5["y"], g5["z"], g, vz)
    assert win > planted.WINDOW_MARGIN and pos > planted.POSITIVE_MARGIN, (win, pos)
    feat = torch.from_numpy(g5["feature"])[:, :, :h, :w]
    ed = torch.from_numpy(g5["est_depth"]).reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)      # mvsdet.py:484,495
    en = torch.from_numpy(g5["est_dens"]).reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)
    dm = torch.from_numpy(depth_mean_of(g5))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        volume, valid, gap_all, rmse = ref.backproject_Weigh(feat, torch.from_numpy(g5["points"]), torch.from_numpy(g5["projection"]),
                                                             ed, [float(v) for v in g5["voxel_size"]], en,
                                                             gt_depth=torch.from_numpy(gt), depth_mean=dm)
    assert np.array_equal(volume.numpy(), g5["volume"]) and np.array_equal(valid.numpy(), g5["valid"])
    lines = [m.groups() for m in map(LINE.search, out.getvalue().splitlines()) if m]
    printed = np.array([[float(a), float(b), float(c)] for a, b, c in lines], np.float64)
    n_skipped = N - len(lines)
    assert n_skipped == int((g5["valid"].reshape(N, -1).sum(1) < 1).sum())
    print(tag, "gap_all", float(gap_all), "rmse", float(rmse), "views printed", len(lines), "skipped", n_skipped, "window margin", win,
          "smallest positive", pos, "bumps", len(bumps))
    return dict(gap_all=np.float32(gap_all), rmse=np.float32(rmse), printed=printed, n_skipped=np.int64(n_skipped),
                window_margin=np.float64(win), positive_margin=np.float64(pos), bumps=bumps.astype(np.int32),
                gt_seed=np.int64(SEEDS[tag]), gt_hw=np.array(GT_HW), zero_view=np.int64(N - 1))


if __name__ == "__main__":
    torch.set_num_threads(4)
    arrs = dict(torch_version=np.array(torch.__version__), generator=np.array("tests/golden/make_goldens_g20.py"))
    for tag in SEEDS:
        for k, v in run(tag).items():
            arrs[f"{tag}:{k}"] = np.asarray(v)
    path = os.path.join(HERE, "g20_depth_diag.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}  {os.path.getsize(path)} bytes")
