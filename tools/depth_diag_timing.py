"""ops.depth_diagnostics at the reference-true shape (40 views, 59x80 maps, the 40x40x16 grid, ground truth 239x320) beside the
same branch of backproject_Weigh (mvsdet.py:1435-1481) written as the ATen operations the reference runs -- a Python loop over the
views with boolean-mask indexing and, per view, the three device-to-host reads of its print -- on the same GPU.  HIP events, median
and minimum of 7 rounds (50 calls of the operator, 5 of the ATen branch per round).  The two are checked against each other first."""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvsdet_amd import ops, synthetic  # noqa: E402
from mvsdet_amd.hotpath import MVSDetHotPath  # noqa: E402

dev = torch.device("cuda:0")
N, C, D, hw, VZ = 40, 32, 12, (60, 80), 0.2
hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D, topk=3)
scene = synthetic.Scene(N, C, D, hw, seed=5)
out = hp.forward_scene(scene.features.to(dev), scene.img_meta, cost_logits=synthetic.make_cost_logits(N, D, hw, seed=5, sharp=2.0).to(dev))
geo = out["geometry"]
est_depth, est_dens, depth_mean = out["est_depth"], out["est_densities"], out["depth_coding"][:, 0]
h, w = geo.height, geo.width
g = torch.Generator(device=dev)
g.manual_seed(5)
gt = F.interpolate(est_depth[:, :1], size=(239, 320), mode="nearest")[:, 0] + 0.03 * torch.randn(N, 239, 320, device=dev, generator=g)
gt[:, 40:70, 100:140] = 0.0
gt[-1] = 0.0


def hip():
    return ops.depth_diagnostics(geo.points, geo.projection, est_depth, est_dens, depth_mean, gt, VZ)


# what the branch reads from the function around it (mvsdet.py:1384-1430), made once and not timed
pts = geo.points.reshape(1, 3, -1).expand(N, 3, -1)
q = torch.bmm(geo.projection, torch.cat((pts, torch.ones_like(pts[:, :1])), dim=1))
x, y, z = (q[:, 0] / q[:, 2]).round().long(), (q[:, 1] / q[:, 2]).round().long(), q[:, 2]
original_valid = (x >= 0) & (y >= 0) & (x < w) & (y < h) & (z > 0)
weight, valid = ops.backproject_weigh(torch.ones(N, 1, h, w, device=dev), geo.points, geo.projection, est_depth, est_dens, VZ)


def aten():
    with torch.no_grad():
        gr = F.interpolate(gt.unsqueeze(1), size=(h, w), mode="bilinear").squeeze(1)
        m = gr > 0
        rmse = torch.mean((depth_mean[m] - gr[m]) ** 2)
        gaps = []
        for i in range(N):
            if torch.sum(valid[i]) < 1:
                continue
            ov = original_valid[i]
            gi = gr[i, y[i, ov], x[i, ov]]
            gv = ov.clone()
            gv[ov] = (z[i, ov] > gi - VZ) & (z[i, ov] < gi + VZ)
            gap_i = torch.mean((gv[ov].float() - weight[i, 0, ov]) ** 2)
            gaps.append(gap_i)
            orig_gap = torch.mean((gv.float() - ov.float()) ** 2)
            new_gap = torch.mean((gv.float() - valid[i].float()) ** 2)
            "{:.5f} {} {:.5f}".format(orig_gap - new_gap, torch.sum(ov) - torch.sum(valid[i]), gap_i)   # the line the reference prints
        return sum(gaps) / len(gaps), rmse


a, b = hip()[0].cpu(), torch.stack(aten()).cpu()
print(f"gap_all, rmse: operator {a.tolist()}  ATen branch {b.tolist()}")
assert torch.allclose(a, b, rtol=1e-4, atol=0), "the two branches disagree"
for name, fn, reps in (("depth_diagnostics (HIP, 3 launches)", hip, 50), ("the branch as ATen operations", aten, 5)):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    print(f"{name} {N} views x {h}x{w}, {geo.points.numel() // 3} voxels, gt 239x320: median {statistics.median(ms):.4f} ms, min {min(ms):.4f} ms")
