#!/usr/bin/env python3
"""Generate tests/golden/g17_lifting_grads.npz by RUNNING THE REFERENCE under autograd (build container only: needs the
reference tree).

G17: the lifting block's backward as the reference computes it.  An instance of the reference's `MVSDet` runs its own
`extract_feat` (mvsdet.py:336-698) with grad enabled and ray_batch=None.  The 2-D backbone hands out LCG feature maps (a leaf
with requires_grad); `cost_regularization` is a stand-in that returns a leaf (N, 2, D, Hf, Wf) logits tensor, LCG-made with a
gain so the depth distribution is peaked (the cost network's own backward is G12's business); `neck_3d` is a pass-through, so
the returned volume is the view mean of :509-515.  prob_volume, off_pred, est_depth / est_densities and the depth expectation
are recorded by wrappers that call the reference's own sample_depth_prob / compute_avg_depth (:266, :298).  One statement is
restated: the opacity of :582, `torch.max(prob_volume, dim=1)[0]`, which sits in the NVS branch (inline_restated=1).

Loss: <R_v, volume_mean> + <R_dc, depth_coding> + <R_p, prob_volume> + <R_o, max(prob_volume, 1)[0][:, :h, :w]>, the
cotangents LCG-made from stored seeds.  Cotangents that sit on a discrete decision within fp32 noise of its threshold are
zeroed, so the reference gradient is well posed everywhere (`decisions`, the logic of test_g13_chain._decisions plus the
window's argmax gap and the opacity's top-1 gap); the masks are stored.  Stored: seeds, cameras, d loss / d logits and
d loss / d features (float32), the forward outputs the checks need, the masks, and the scale of each path's gradient.

Shapes.  No committed file may exceed 1 MiB, so the maps are 16 x 20 (15 x 20 after the crop) instead of the shipped 60 x 80:
the two gradients are dense, and at 60 x 80 the logits' alone would take 2.8 MB.  Views, channels (C = 40: one full and one
partial slab of the packed maps), planes and the shipped 40 x 40 x 16 voxel grid are kept.

    python tests/golden/make_goldens_g17.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from lcg import lcg_uniform  # noqa: E402

FEAT_HW = (16, 20)
N_VOXELS, VOXEL_SIZE = [40, 40, 16], [0.16, 0.16, 0.2]
COST_GAIN, OFF_GAIN = 6.0, 2.0
GAP = 1e-4      # a ranking / argmax / top-1 is decided when the competing probabilities are further apart than this
WINDOW = 3e-4   # a depth-window test is decided when |z - d_j| is further than this (metres) from the window's edge
ROUND = 1e-3    # a projection rounding is decided when the position is further than this (pixels) from a .5 tie
CASES = {
    "scannet": dict(N=6, C=40, D=12, near_far=(0.2, 5.0), pvi=False,
                    seeds=dict(camera_seed=171, feature_seed=1701, logits_seed=1702, cot_seed=1703)),
    "arkit": dict(N=4, C=40, D=12, near_far=(0.5, 5.5), pvi=True,
                  seeds=dict(camera_seed=172, feature_seed=1721, logits_seed=1722, cot_seed=1723)),
}


def inputs(case):
    """-> meta, features (N,C,Hf,Wf), logits (N,2,D,Hf,Wf), cotangents {v, dc, p, o} (unmasked), all from the seeds."""
    from mvsdet_amd import synthetic
    c = CASES[case]
    s = c["seeds"]
    N, C, D = c["N"], c["C"], c["D"]
    Hf, Wf = FEAT_HW
    meta = synthetic.make_img_meta(N, FEAT_HW, seed=s["camera_seed"], per_view_intrinsics=c["pvi"])
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    feat = torch.from_numpy(lcg_uniform(N * C * Hf * Wf, s["feature_seed"])).reshape(N, C, Hf, Wf)
    logits = torch.from_numpy(lcg_uniform(N * 2 * D * Hf * Wf, s["logits_seed"])).reshape(N, 2, D, Hf, Wf)
    logits = logits * torch.tensor([COST_GAIN, OFF_GAIN]).view(1, 2, 1, 1, 1)
    V = int(np.prod(N_VOXELS))
    r = torch.from_numpy(lcg_uniform(C * V + N * h * w + N * D * Hf * Wf + N * h * w, s["cot_seed"]))
    sizes = [C * V, N * h * w, N * D * Hf * Wf, N * h * w]
    parts = torch.split(r, sizes)
    cots = dict(v=parts[0].reshape(C, *N_VOXELS), dc=parts[1].reshape(N, 1, h, w), p=parts[2].reshape(N, D, Hf, Wf),
                o=parts[3].reshape(N, h, w))
    return meta, feat, logits, cots


def decisions(prob, est_depth, est_dens, projection, points, vz, h, w):
    """(decided voxels (V,), clear pixels (N,h,w), decided opacity pixels (N,h,w)) in float64 from the reference's fp32
    outputs: a voxel is decided when, in every view that sees it, the projection's rounding, the top-3 ranking at its pixel,
    the open depth window and the argmax among the matching candidates all hold with a margin above fp32 noise."""
    prob = np.asarray(prob, np.float64)
    srt = np.sort(prob, axis=1)[:, ::-1]
    clear = ((srt[:, :3] - srt[:, 1:4]).min(axis=1) > GAP)[:, :h, :w]
    opa_ok = ((srt[:, 0] - srt[:, 1]) > GAP)[:, :h, :w]
    pts = np.asarray(points, np.float64).reshape(3, -1)
    P = np.asarray(projection, np.float64)
    q = np.einsum("nij,jv->niv", P[:, :, :3], pts) + P[:, :, 3:]
    z = q[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = q[:, 0] / z, q[:, 1] / z
    xr, yr = np.rint(x), np.rint(y)
    inside = (xr >= 0) & (xr < w) & (yr >= 0) & (yr < h) & (z > 0)
    near_image = (x > -1) & (x < w) & (y > -1) & (y < h) & (z > -1e-3)
    tie = (np.abs(np.abs(x - np.floor(x)) - 0.5) < ROUND) | (np.abs(np.abs(y - np.floor(y)) - 0.5) < ROUND) | (np.abs(z) < 1e-3)
    undecided = near_image & tie
    xi, yi = np.clip(xr, 0, w - 1).astype(int), np.clip(yr, 0, h - 1).astype(int)
    ed = np.asarray(est_depth, np.float64)
    en = np.asarray(est_dens, np.float64)
    pn = en / en.sum(axis=1, keepdims=True)
    for i in range(len(ed)):
        dj = ed[i][:, yi[i], xi[i]]
        margin = np.abs(np.abs(z[i][None] - dj) - vz).min(axis=0)
        match = np.abs(z[i][None] - dj) < vz
        cand = np.where(match, pn[i][:, yi[i], xi[i]], -1.0)
        top2 = np.sort(cand, axis=0)[::-1][:2]
        argmax_tie = (top2[1] >= 0) & ((top2[0] - top2[1]) < GAP)
        undecided[i] |= inside[i] & ((margin < WINDOW) | ~clear[i][yi[i], xi[i]] | argmax_tie)
    return ~undecided.any(axis=0), clear, opa_ok


def run_reference(case):
    """The reference's extract_feat under autograd -> dict of the fixture's arrays."""
    from _ref_loader import load_reference
    ref, _ = load_reference()
    MVSDet = ref.MVSDet
    c = CASES[case]
    N, C, D = c["N"], c["C"], c["D"]
    nf = c["near_far"]
    meta, feat0, logits0, cots = inputs(case)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    feat = feat0.clone().requires_grad_(True)
    logits = logits0.clone().requires_grad_(True)

    det = MVSDet.__new__(MVSDet)                     # the reference class; its __init__ needs mmengine's registry
    torch.nn.Module.__init__(det)
    det.backbone = lambda img: feat
    det.neck = lambda x: [x]
    det.head_2d = None
    det.n_voxels, det.voxel_size, det.near_far_range, det.topk = N_VOXELS, VOXEL_SIZE, list(nf), 3
    det.gs_cfg = SimpleNamespace(num_monocular_samples=D)
    det.depth_interval = (nf[1] - nf[0]) / D         # mvsdet.py:221-225
    det.depth_values = np.arange(nf[0], nf[1], det.depth_interval, dtype=np.float32)
    assert len(det.depth_values) == D
    det.cost_regularization = lambda variance: logits
    det.neck_3d = lambda x: x
    det.eval()

    rec = {}

    def sample_depth_prob(prob_volume, off_pred, topk=3):
        rec["prob"], rec["off"] = prob_volume, off_pred
        rec["est_depth"], rec["est_dens"] = MVSDet.sample_depth_prob(det, prob_volume, off_pred, topk=topk)
        return rec["est_depth"], rec["est_dens"]

    def compute_avg_depth(prob_volume, off_pred):
        rec["avg_depth"] = MVSDet.compute_avg_depth(det, prob_volume, off_pred)
        return rec["avg_depth"]

    det.sample_depth_prob, det.compute_avg_depth = sample_depth_prob, compute_avg_depth
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        res = det.extract_feat({"imgs": torch.zeros(1, N, 3, 4 * FEAT_HW[0], 4 * FEAT_HW[1])}, [SimpleNamespace(metainfo=meta)],
                               "test")
    finally:
        torch.Tensor.cuda = real_cuda
    volume, valid = res[0][0], res[1][0]
    assert tuple(volume.shape) == (C, *N_VOXELS)
    prob = rec["prob"]
    depth_coding = rec["avg_depth"][:, :h, :w].unsqueeze(1)
    opacity = torch.max(prob, dim=1)[0][:, :h, :w]                      # mvsdet.py:582 (restated)
    projection = MVSDet._compute_projection(meta, 4, None)
    points = ref.get_points(n_voxels=torch.tensor(N_VOXELS), voxel_size=torch.tensor(VOXEL_SIZE),
                            origin=torch.tensor(meta["lidar2img"]["origin"]))
    est_depth = rec["est_depth"][:, :, :h, :w].detach()
    est_dens = rec["est_dens"][:, :, :h, :w].detach()
    decided, clear, opa_ok = decisions(prob.detach().numpy(), est_depth.numpy(), est_dens.numpy(), projection.numpy(),
                                       points.numpy(), VOXEL_SIZE[-1], h, w)
    Rv = cots["v"] * torch.from_numpy(decided).view(1, *N_VOXELS).float()
    Ro = cots["o"] * torch.from_numpy(opa_ok).float()
    terms = [(volume * Rv).sum(), (depth_coding * cots["dc"]).sum(), (prob * cots["p"]).sum(), (opacity * Ro).sum()]
    # each path's share of d loss / d logits (and the volume's of d loss / d features): non-trivial on every path
    path_scales = []
    for t in terms:
        gl, = torch.autograd.grad(t, (logits,), retain_graph=True)
        path_scales.append(float(gl.abs().max()))
    gf_volume, = torch.autograd.grad(terms[0], (feat,), retain_graph=True)
    g_logits, g_feat = torch.autograd.grad(sum(terms), (logits, feat))
    out = dict(
        extrinsic=np.array(meta["lidar2img"]["extrinsic"]), intrinsic=np.array(meta["lidar2img"]["intrinsic"]),
        origin=meta["lidar2img"]["origin"], img_shape=np.array(meta["img_shape"]), ori_shape=np.array(meta["ori_shape"]),
        near_far=np.array(nf, dtype=np.float64), n_voxels=np.array(N_VOXELS), voxel_size=np.array(VOXEL_SIZE, dtype=np.float64),
        feature_shape=np.array(feat.shape), logits_gains=np.array([COST_GAIN, OFF_GAIN], dtype=np.float32),
        **{k: np.int64(v) for k, v in c["seeds"].items()},
        grad_logits=g_logits.numpy(), grad_features=g_feat.numpy(),
        path_scale_logits=np.array(path_scales), path_scale_features_volume=np.float64(gf_volume.abs().max()),
        prob=prob.detach().numpy(), est_depth=est_depth.numpy(), est_dens=est_dens.numpy(), projection=projection.numpy(),
        valid_count=valid.detach().long().numpy().reshape(-1),
        decided_voxels=decided, clear_pixels=clear, opacity_decided=opa_ok)
    return out


def build():
    """-> {"<case>:<key>": array} for every case, plus the flags."""
    out = dict(inline_restated=np.int64(1), feat_hw=np.array(FEAT_HW), torch_version=np.array(torch.__version__),
               generator=np.array("tests/golden/make_goldens_g17.py"))
    for case in CASES:
        for k, v in run_reference(case).items():
            out[f"{case}:{k}"] = np.asarray(v)
    return out


if __name__ == "__main__":
    torch.set_num_threads(4)
    arrs = build()
    path = os.path.join(HERE, "g17_lifting_grads.npz")
    np.savez_compressed(path, **arrs)
    for case in CASES:
        d = arrs[f"{case}:decided_voxels"]
        print(case, "undecided voxels", int((~d).sum()), "of", d.size, "non-empty", int((arrs[f"{case}:valid_count"] > 0).sum()),
              "unclear pixels", float(1 - arrs[f"{case}:clear_pixels"].mean()), "path scales", arrs[f"{case}:path_scale_logits"],
              float(arrs[f"{case}:path_scale_features_volume"]))
    print(f"wrote {path}  {os.path.getsize(path) / 2 ** 20:.3f} MiB")
