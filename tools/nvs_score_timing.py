"""The view-synthesis scores of one scene at the test shape (2 target views of 239x320 with a rendered depth): ops.nvsmetric.nvs_score on
csrc/nvsmetric.hip beside the reference's sequence restated with torch and scipy on the same box -- per view the squared error
reduced on the device and read back for PSNR, both images copied to the host (`.cpu().numpy()`) and structural_similarity's
uniform_filter form in float32 there (tests/nvs_score_restated.py; skimage itself is not installed), the whole squared depth error
copied to the host for its mean (save_rendered_img.py:21-44, 178-235).  The picture writing is left out of both.

  hip        one nvs_score call per scene; HIP events around the calls (device time per scene), and wall clock of a call followed by
             the read-back of its three numbers, which is what integration.patch_reference_nvs_scores does per scene
  reference  wall clock of the restated sequence, one process; the usable cores are reported beside it

Also counted, for one scene of each: device kernels (torch.profiler) and host synchronisations (torch's sync debug mode).  The two are
checked against each other first.  The text goes to --out (default profiles/nvs_score_timing.txt) and to stdout.

    python tools/nvs_score_timing.py [--out FILE] [--rounds N]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nvs_score_restated as R  # noqa: E402
from mvsdet_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nvs_score_timing.txt"))
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda:0")
N_TGT, H, W = 2, 239, 320
sc = R.scene(N_TGT, H, W, seed=5)
pred, gt, pred_depth, gt_depth = (torch.from_numpy(sc[k]).to(dev) for k in ("pred", "gt", "pred_depth", "gt_depth"))


def hip_device_only():
    return ops.nvsmetric.nvs_score(None, pred, gt, pred_depth, gt_depth)[1]


def hip():
    return hip_device_only().cpu().tolist()


def reference():
    """save_rendered_img_Image + save_rendered_depth as the reference runs them, without the pictures."""
    p, g = pred.permute(0, 2, 3, 1), gt.permute(0, 2, 3, 1)
    psnr_total, ssim_total, rmse = 0, 0, 0
    for v in range(N_TGT):
        mse = ((p[v] - g[v]) ** 2).mean()
        psnr_total += (-10.0 * torch.log(mse) / np.log(10.0)).cpu().numpy()
        a, b = p[v].cpu().numpy(), g[v].cpu().numpy()
        ssim_total += np.array([R.ssim_plane_filter(a[..., c], b[..., c], np.float32) for c in range(3)]).mean()
    for v in range(N_TGT):
        rmse += np.mean(((pred_depth[v] - gt_depth[v]) ** 2).cpu().numpy())
    return [float(psnr_total / N_TGT), float(ssim_total / N_TGT), float(rmse / N_TGT)]


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        return len(names), names
    except Exception as exc:   # a build without device tracing: report that, time anyway
        return None, [f"not counted: {type(exc).__name__}: {exc}"]


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return sum("synchroniz" in str(x.message) for x in seen)


lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


ours, theirs = hip(), reference()
say(f"{N_TGT} target views of {H}x{W} with depth: {N_TGT * 3 * (H - 6) * (W - 6)} windows of 7x7, "
    f"workspace {ops.nvsmetric.workspace_bytes(N_TGT, H, W, True)} bytes")
for n, a, b in zip(("psnr", "ssim", "rmse"), ours, theirs):
    say(f"    {n}: HIP (float64) {a!r}, the reference's float32 sequence {b!r}, difference {abs(a - b):.3g}")
    assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), "the two disagree"
for _ in range(3):
    hip()
torch.cuda.synchronize()
ms = []
for _ in range(args.rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        hip_device_only()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1) / 50)
say(f"ops.nvsmetric.nvs_score, device time by HIP events: median {statistics.median(ms):.4f} ms, min {min(ms):.4f} ms per scene")
for name, fn, steps in (("ops.nvsmetric.nvs_score and the read-back of its three numbers (HIP)", hip, 50), ("the reference's sequence (torch + scipy)", reference, 5)):
    for _ in range(2):
        fn()
    wall = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        wall.append((time.perf_counter() - t0) * 1e3 / steps)
    syncs = count_syncs(fn)
    n_kernels, names = count_kernels(fn)
    say(f"{name}: wall clock median {statistics.median(wall):.3f} ms, min {min(wall):.3f} ms per scene; {syncs} host synchronisation(s); "
        f"{n_kernels if n_kernels is not None else '?'} device kernels and copies")
    for n in [n for n in names if "nvs_" in n]:
        say(f"        {n[:150]}")
say(f"host: {len(os.sched_getaffinity(0))} usable cores, the reference's sequence uses one thread")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
