#!/usr/bin/env python3
"""Generate tests/golden/g25_photo_loss.npz by RUNNING THE REFERENCE on the CPU (build container only: needs the reference tree).

G25: the reference's photometric consistency term, unmodified: mvs_models/homography.py (inverse_warping, compute_reconstr_loss),
MVSDet.photometric_loss (mvsdet.py:845-874) and MVSDet.warp_img (:701-768), the methods unbound with a SimpleNamespace as `self`.
homography.py hard-codes `.cuda()`; inside this process only, and only for the duration of a call, torch.Tensor.cuda is rebound to
the identity.

Cases (cameras rotate about all three axes and have per-view translations):
  tiny          B=2, 5x7, C=3
  small         B=3, 12x16, per-view intrinsics (the K_left-for-both quirk shows), image amplitude 3: both smooth-L1 branches
  ref_true      N=12 views, ref_id of 10, neighbor_ids k=2, a (12,1,60,81) depth whose padding row and column are NaN, the 59x80 crop;
                images stored as uint8 (value / 255)
  behind        part of the frustum has p2 < 0: the mask follows the formula
  lastrow       coordinates that land with y0 = H-1 (valid, both row taps on the last row)
  simple        compute_reconstr_loss(simple=True) on a 6x9 map (L and its gradient; loss_pc is that of simple=False)
  two_scenes, three_scenes   the minimum over scenes (tiny-sized scenes, every scene wins pixels)
  warp_img      MVSDet.warp_img itself: N=5, 24x32 images -> 6x8, randperm fixed by the seed (stored: ref_id)
Stored per case: the inputs, warped, mask, L, loss_pc, d loss_pc / d depth from the reference's autograd, and `dist_*`: the distances
between the reference's numbers and tests/photo_loss_restated.py in float64 (the tests' bars are 4 x these).

ASSERTED here on every case (depths are moved in steps of 1/64 m, reference pixels in steps of 1/256, until they hold): every mask
decision >= 1e-3 px from its threshold; every coordinate within a pixel of the image >= 1e-4 px from an integer; |p2| >= 1e-2; no
||d| - 1| < 1e-4 in any smooth-L1 term; competing L_i >= 1e-5 apart (relative); the reference's mask equals the restatement's.

    python tests/golden/make_goldens_g25.py
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import photo_loss_restated as R  # noqa: E402
from lcg import lcg_uniform  # noqa: E402

F32 = np.float32


@contextlib.contextmanager
def cuda_is_identity():
    keep = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = keep


def rot(a):
    cx, cy, cz = np.cos(a)
    sx, sy, sz = np.sin(a)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_views(N, h, w, seed, ang=0.06, shift=0.12, per_view_k=False, extra=None):
    """(N,4,4) world-to-camera and (4,4) | (N,4,4) feature-level intrinsics."""
    u = lcg_uniform(N * 12, seed).reshape(N, 12).astype(np.float64)
    w2c = np.tile(np.eye(4), (N, 1, 1))
    K = np.tile(np.eye(4), (N, 1, 1))
    for i in range(N):
        w2c[i, :3, :3] = rot(ang * u[i, :3] + (0 if extra is None else extra[i][0]))
        w2c[i, :3, 3] = shift * u[i, 3:6] + (0 if extra is None else extra[i][1])
        s = 1.0 + (0.15 * u[i, 6] if per_view_k else 0.0)
        K[i, 0, 0], K[i, 1, 1] = 0.85 * w * s, 0.85 * w * s * (1.0 + (0.05 * u[i, 7] if per_view_k else 0.0))
        K[i, 0, 2] = (w - 1) / 2 + (0.7 * u[i, 8] if per_view_k else 0.3)
        K[i, 1, 2] = (h - 1) / 2 + (0.7 * u[i, 9] if per_view_k else -0.2)
        K[i, 0, 1] = 0.01 * u[i, 10] if per_view_k else 0.0
    return w2c.astype(F32), (K if per_view_k else K[0]).astype(F32)


def make_depth(B, h, w, seed, base=2.2):
    u = lcg_uniform(B * 4 + B * h * w, seed).astype(np.float64)
    par, noise = u[:B * 4].reshape(B, 4), u[B * 4:].reshape(B, h, w)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    d = base + 0.6 * np.sin(2.0 * x[None] + 3 * par[:, 0, None, None]) * np.cos(1.5 * y[None] + 3 * par[:, 1, None, None]) + 0.08 * noise
    return (np.round(d * 64) / 64).astype(F32)


def make_images(N, h, w, C, seed, amp=1.0, noise_amp=0.2):
    """Smooth colour plus noise in [0, amp], in steps of amp / 255."""
    u = lcg_uniform(N * C * 3 + N * h * w * C, seed).astype(np.float64)
    par, noise = u[:N * C * 3].reshape(N, 1, 1, C, 3), u[N * C * 3:].reshape(N, h, w, C)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    v = 0.5 + 0.3 * np.sin(5 * x[None, :, :, None] * (1 + par[..., 0]) + 3 * par[..., 1]) * np.cos(4 * y[None, :, :, None] + 3 * par[..., 2])
    q = np.clip(np.round((v + noise_amp * noise) * 255), 0, 255)
    return q.astype(np.uint8), (q.astype(F32) / F32(255) * F32(amp)).astype(F32)


def packed(w2c, K, ids):
    N = w2c.shape[0]
    Kn = np.broadcast_to(K, (N, 4, 4)) if K.ndim == 2 else K
    return np.stack([w2c, Kn], axis=1)[ids][:, :, :3, :].astype(F32).copy()


def settle_depth(left, right, depth, tag):
    """Move single depths in steps of 1/64 m until the margins hold; returns the depth and the margins."""
    depth = depth.copy()
    B, h, w = depth.shape
    for it in range(400):
        x, y, _, _, p2 = R.project(left, right, depth)
        with np.errstate(all="ignore"):
            border = np.minimum(np.minimum(np.abs(x), np.abs(x - (w - 1))), np.minimum(np.abs(y), np.abs(y - h)))
            near = (x > -1) & (x < w) & (y > -1) & (y < h + 1)
            integer = np.where(near, np.minimum(np.abs(x - np.round(x)), np.abs(y - np.round(y))), 1.0)
            bad = (np.abs(p2) < 1e-2) | (border < 1e-3) | (integer < 1e-4) | ~np.isfinite(x) | ~np.isfinite(y)
        if not bad.any():
            return depth, dict(border=float(border.min()), integer=float(integer.min()), p2=float(np.abs(p2).min()), moved=it)
        depth[bad] += F32(1 / 64)
    raise AssertionError(f"{tag}: margins do not settle")


def settle_ref(img, left, right, depth, ref, simple, tag):
    """Move single reference pixels in steps of 1/256 until no smooth-L1 argument is within 1e-4 of +-1."""
    ref = ref.copy()
    for it in range(100):
        warped, mask, _ = R.inverse_warping(img, left, right, depth)
        d0, dxs, dys = R.compute_reconstr_loss(warped, ref, mask, simple)[3]
        bad = np.zeros(ref.shape, bool)
        bad |= np.abs(np.abs(d0) - 1) < 1e-4
        if not simple:
            bx, by = np.abs(np.abs(dxs) - 1) < 1e-4, np.abs(np.abs(dys) - 1) < 1e-4
            bad[:, :, 1:] |= bx
            bad[:, :, :-1] |= bx
            bad[:, 1:] |= by
            bad[:, :-1] |= by
        bad &= mask.astype(bool)
        if not bad.any():
            gap = min([float(np.abs(np.abs(v) - 1).min()) for v in ((d0,) if simple else (d0, dxs, dys)) if v.size])
            assert gap >= 1e-4, (tag, gap)
            return ref, gap
        ref[bad] += F32(1 / 256)
    raise AssertionError(f"{tag}: smooth-L1 margins do not settle")


def run_reference(ref_mod, homo, scenes, simple=False):
    """scenes: list of (img, left, right, depth (B,h,w), ref) -> per scene warped, mask, L, grad; and loss_pc."""
    leaves, warped, masks, refs, Ls = [], [], [], [], []
    with cuda_is_identity():
        for img, left, right, depth, rf in scenes:
            d = torch.from_numpy(depth).unsqueeze(1).clone().requires_grad_(True)
            wv, mv = homo.inverse_warping(torch.from_numpy(img), torch.from_numpy(left), torch.from_numpy(right), d)
            leaves.append(d)
            warped.append(wv)
            masks.append(mv)
            refs.append(torch.from_numpy(rf))
            Ls.append(homo.compute_reconstr_loss(wv, refs[-1], mv, simple=simple))
        loss = ref_mod.MVSDet.photometric_loss(types.SimpleNamespace(), warped, masks, refs)["loss_pc"]
        grads = torch.autograd.grad(loss, leaves, retain_graph=True)
        gL = [torch.autograd.grad(L, d, retain_graph=True)[0] for L, d in zip(Ls, leaves)]
    return ([w.detach().numpy() for w in warped], [m.detach().numpy() for m in masks], [L.detach().numpy().astype(F32) for L in Ls],
            [g.squeeze(1).numpy() for g in grads], loss.detach().numpy().astype(F32), [g.squeeze(1).numpy() for g in gL])


def distances(arrs, tag, warped, mask, L, grad, loss, gL, img, left, right, depth, rf, simple, share=None):
    """Reference against the float64 restatement, stored as the tests' yardstick."""
    r = R.loss_and_depth_grad(img, left, right, depth, rf, simple)
    assert np.array_equal(r["mask"] != 0, mask != 0), f"{tag}: the reference's mask differs from the restatement's"
    m = (mask != 0)[..., 0]
    mag = np.maximum(r["aux"]["mag"], 1e-30)
    with np.errstate(all="ignore"):
        arrs[f"{tag}:dist_warped_in"] = np.float64(np.abs(warped - r["warped"])[m].max()) if m.any() else np.float64(0)
        arrs[f"{tag}:dist_warped_out"] = np.float64(np.nanmax((np.abs(warped - r["warped"]) / mag)[~m])) if (~m).any() else np.float64(0)
    arrs[f"{tag}:dist_L"] = np.float64(abs(float(L) - float(r["L"])) / abs(float(r["L"])))
    gref = r["grad"] / (r["wins"][0] / mask.size)      # d L / d depth
    arrs[f"{tag}:dist_gL"] = np.float64(np.abs(gL - gref).max() / np.abs(gref).max())
    assert np.all(gL[~m] == 0), tag
    if share is None:                                  # a single scene: loss_pc and its gradient too (always of simple=False)
        if simple:
            r = R.loss_and_depth_grad(img, left, right, depth, rf, False)
        arrs[f"{tag}:dist_loss_pc"] = np.float64(abs(float(loss) - float(r["loss_pc"])) / abs(float(r["loss_pc"])))
        arrs[f"{tag}:dist_grad"] = np.float64(np.abs(grad - r["grad"]).max() / np.abs(r["grad"]).max())
        assert np.all(grad[~m] == 0), tag
    print(f"{tag}: mask {int(m.sum())}/{m.size}  L {float(L)!r}  |grad|max {np.abs(gL).max():.3g}  " +
          "  ".join(f"{k.split(':')[1]} {float(v):.2e}" for k, v in arrs.items() if k.startswith(tag + ":dist_")))
    return r


def single_case(ref_mod, homo, arrs, tag, img, left, right, depth, rf, simple=False, store_img=True):
    depth, margins = settle_depth(left, right, depth, tag)
    rf, gap = settle_ref(img, left, right, depth, rf, simple, tag)
    warped, mask, L, grad, loss, gL = run_reference(ref_mod, homo, [(img, left, right, depth, rf)], simple)
    print(f"{tag}: margins {margins}, smallest ||d| - 1| {gap:.3g}")
    if store_img:
        arrs[f"{tag}:img"], arrs[f"{tag}:ref"] = img, rf
    arrs[f"{tag}:left_cam"], arrs[f"{tag}:right_cam"], arrs[f"{tag}:depth"] = left, right, depth
    arrs[f"{tag}:warped"], arrs[f"{tag}:mask"], arrs[f"{tag}:L"], arrs[f"{tag}:gL"] = warped[0], mask[0], L[0], gL[0]
    arrs[f"{tag}:loss_pc"], arrs[f"{tag}:grad"], arrs[f"{tag}:simple"] = loss, grad[0], np.int64(simple)
    r = distances(arrs, tag, warped[0], mask[0], L[0], grad[0], loss, gL[0], img, left, right, depth, rf, simple)
    return dict(img=img, left=left, right=right, depth=depth, ref=rf, r=r, mask=mask[0], args=r["args"])


def pair_case(ref_mod, homo, arrs, tag, B, h, w, seed, C=3, amp=1.0, per_view_k=False, extra=None, ang=0.06, shift=0.12, simple=False,
              base=2.2, depth=None):
    w2c, K = make_views(2 * B, h, w, seed, ang, shift, per_view_k, extra)
    left, right = packed(w2c, K, np.arange(B)), packed(w2c, K, np.arange(B, 2 * B))
    img = make_images(B, h, w, C, seed + 1, amp)[1]
    rf = make_images(B, h, w, C, seed + 2, amp)[1]
    depth = make_depth(B, h, w, seed + 3, base) if depth is None else depth
    return single_case(ref_mod, homo, arrs, tag, img, left, right, depth, rf, simple)


def multi_case(ref_mod, homo, arrs, tag, n, B, h, w, seed):
    scenes = []
    for i in range(n):
        w2c, K = make_views(2 * B, h, w, seed + 10 * i, shift=0.1 + 0.25 * i)
        left, right = packed(w2c, K, np.arange(B)), packed(w2c, K, np.arange(B, 2 * B))
        img, rf = make_images(B, h, w, 3, seed + 10 * i + 1)[1], make_images(B, h, w, 3, seed + 10 * i + 2)[1]
        depth, _ = settle_depth(left, right, make_depth(B, h, w, seed + 10 * i + 3), f"{tag}[{i}]")
        rf, _ = settle_ref(img, left, right, depth, rf, False, f"{tag}[{i}]")
        scenes.append((img, left, right, depth, rf))
    warped, mask, L, grad, loss, gL = run_reference(ref_mod, homo, scenes)
    Lf = np.array([float(v) for v in L])
    order = np.sort(Lf)
    assert np.all(np.diff(order) / order[1:] >= 1e-5), (tag, Lf)
    res = [R.loss_and_depth_grad(*s) for s in scenes]
    loss64, g64, wins, L64 = R.photometric_loss([r["warped"] for r in res], [r["mask"] for r in res], [s[4] for s in scenes])
    assert np.all(wins > 0), (tag, wins)
    arrs[f"{tag}:n"], arrs[f"{tag}:loss_pc"], arrs[f"{tag}:wins"] = np.int64(n), loss, wins
    arrs[f"{tag}:dist_loss_pc"] = np.float64(abs(float(loss) - float(loss64)) / abs(float(loss64)))
    total = mask[0].size
    for i, s in enumerate(scenes):
        t = f"{tag}[{i}]"
        for k, v in zip(("img", "left_cam", "right_cam", "depth", "ref"), s):
            arrs[f"{t}:{k}"] = v
        arrs[f"{t}:warped"], arrs[f"{t}:mask"], arrs[f"{t}:L"], arrs[f"{t}:grad"], arrs[f"{t}:gL"] = warped[i], mask[i], L[i], grad[i], gL[i]
        distances(arrs, t, warped[i], mask[i], L[i], grad[i], loss, gL[i], *s, False, share=wins[i] / total)
        g64_depth = res[i]["grad"] / (res[i]["wins"][0] / total) * (wins[i] / total)
        arrs[f"{t}:dist_grad"] = np.float64(np.abs(grad[i] - g64_depth).max() / np.abs(g64_depth).max())
    print(f"{tag}: loss_pc {float(loss)!r} wins {wins.tolist()} L {Lf.tolist()} dist {float(arrs[f'{tag}:dist_loss_pc']):.2e}")


if __name__ == "__main__":
    from _ref_loader import load_reference
    torch.set_num_threads(4)
    ref_mod, _ = load_reference()
    homo = sys.modules["refpkg.mvs_models.homography"]
    arrs = dict(torch_version=np.array(torch.__version__), generator=np.array("tests/golden/make_goldens_g25.py"))

    pair_case(ref_mod, homo, arrs, "tiny", 2, 5, 7, 2501)
    c = pair_case(ref_mod, homo, arrs, "small", 3, 12, 16, 2502, amp=3.0, per_view_k=True)
    a = np.concatenate([np.abs(v).ravel() for v in c["args"]])
    assert (a > 1).sum() > 10 and (a < 1).sum() > 10, "small: both smooth-L1 branches"
    # behind: the right cameras stand 4 m ahead, inside a scene whose depth runs from 1.5 m (left) to 6.5 m (right): the near part lies
    # behind them and projects through the sign flip of x = p0 / p2
    extra = [(np.zeros(3), np.zeros(3))] * 2 + [(np.zeros(3), np.array([0.0, 0.0, -4.0 - 0.3 * i])) for i in range(2)]
    ramp = make_depth(2, 8, 10, 2533, 0.0) * F32(0.25) + (1.5 + 5.0 * np.linspace(0, 1, 10))[None, None, :]
    c = pair_case(ref_mod, homo, arrs, "behind", 2, 8, 10, 2503, extra=extra, depth=(np.round(ramp * 64) / 64).astype(F32))
    assert (c["r"]["aux"]["p2"] < 0).sum() > 8 and (c["r"]["aux"]["p2"] > 0).sum() > 8, "behind: both signs of p2"
    print("behind: p2 < 0 at", int((c["r"]["aux"]["p2"] < 0).sum()), "pixels, of them in the mask", int(((c["r"]["aux"]["p2"] < 0) & (c["mask"][..., 0] != 0)).sum()))
    # lastrow: the right cameras sit higher, the picture moves down by one to two rows
    extra = [(np.zeros(3), np.zeros(3))] * 2 + [(np.zeros(3), np.array([0.0, 0.35 + 0.1 * i, 0.0])) for i in range(2)]
    c = pair_case(ref_mod, homo, arrs, "lastrow", 2, 7, 9, 2504, extra=extra, ang=0.01, shift=0.02)
    on_last = (np.floor(c["r"]["aux"]["y"]) == 6) & (c["mask"][..., 0] != 0)
    assert on_last.sum() >= 4, "lastrow: masked pixels with y0 = H-1"
    print("lastrow: masked pixels with y0 = H-1:", int(on_last.sum()))
    pair_case(ref_mod, homo, arrs, "simple", 2, 6, 9, 2505, simple=True)
    multi_case(ref_mod, homo, arrs, "two_scenes", 2, 2, 5, 7, 2510)
    multi_case(ref_mod, homo, arrs, "three_scenes", 3, 2, 5, 7, 2540)

    # ref_true: the scene form.  The reference sees the gathered tensors; the fixture keeps the scene and the indices.
    N, h, w = 12, 59, 80
    w2c, K = make_views(N, h, w, 2506, ang=0.05, shift=0.1)
    u = lcg_uniform(N * 2, 2507)
    nbr = np.stack([(np.arange(N) + 1 + (np.abs(u[:N]) * 3).astype(int)) % N, (np.arange(N) + 5) % N], axis=1).astype(np.int64)
    ref_id = np.array([7, 2, 11, 0, 5, 9, 3, 10, 1, 6], np.int64)
    src_id = nbr[ref_id, 0]
    img_u8, imgs = make_images(N, h, w, 3, 2508, noise_amp=0.05)
    left, right = packed(w2c, K, ref_id), packed(w2c, K, src_id)
    depth_all = make_depth(N, h, w, 2509)
    c = single_case(ref_mod, homo, arrs, "ref_true", imgs[src_id], left, right, depth_all[ref_id], imgs[ref_id].copy(), store_img=False)
    assert np.array_equal(c["ref"], imgs[ref_id]), "ref_true: the reference images are the scene's own (in [0,1] no term reaches 1)"
    depth_all[ref_id] = c["depth"]
    pad = np.full((N, 1, 60, 81), np.nan, F32)
    pad[:, 0, :h, :w] = depth_all
    for k in ("left_cam", "right_cam", "depth", "gL"):      # gL: loss_pc's gradient is the same map times mean(mask)
        del arrs[f"ref_true:{k}"]
    arrs["ref_true:imgs_u8"], arrs["ref_true:w2c"], arrs["ref_true:K"], arrs["ref_true:depth_pad"] = img_u8, w2c, K, pad
    arrs["ref_true:neighbor_ids"], arrs["ref_true:ref_id"] = nbr, ref_id

    # warp_img itself
    N, h, w = 5, 6, 8
    w2c, K = make_views(N, h, w, 2520, ang=0.05, shift=0.1)
    K4 = K.copy()
    nbr = np.stack([(np.arange(N) + 2) % N, (np.arange(N) + 1) % N], axis=1).astype(np.int64)
    big = np.ascontiguousarray(make_images(N, 4 * h, 4 * w, 3, 2521)[1].transpose(0, 3, 1, 2))
    small = torch.nn.functional.interpolate(torch.from_numpy(big), scale_factor=0.25, mode="bilinear").permute(0, 2, 3, 1).numpy()
    torch.manual_seed(2522)
    ref_id = torch.randperm(N)[:min(10, N)].numpy()
    src_id = nbr[ref_id, 0]
    left, right = packed(w2c, K, ref_id), packed(w2c, K, src_id)
    depth_all = make_depth(N, h, w, 2523)
    depth_all[ref_id], margins = settle_depth(left, right, depth_all[ref_id], "warp_img")
    torch.manual_seed(2522)
    with cuda_is_identity():
        d = torch.from_numpy(depth_all).unsqueeze(1).clone().requires_grad_(True)
        wv, mv, chosen = ref_mod.MVSDet.warp_img(types.SimpleNamespace(), torch.from_numpy(big), torch.from_numpy(nbr), torch.from_numpy(w2c),
                                                 torch.from_numpy(K4), d)
        loss = ref_mod.MVSDet.photometric_loss(types.SimpleNamespace(), [wv], [mv], [chosen])["loss_pc"]
        L = homo.compute_reconstr_loss(wv, chosen, mv, simple=False)
        grad = torch.autograd.grad(loss, d, retain_graph=True)[0].squeeze(1).numpy()
        gL = torch.autograd.grad(L, d)[0].squeeze(1).numpy()
    assert np.array_equal(chosen.numpy(), small[ref_id])
    arrs["warp_img:imgs"], arrs["warp_img:neighbor_ids"], arrs["warp_img:w2c"], arrs["warp_img:K"] = big, nbr, w2c, K4
    arrs["warp_img:depth"], arrs["warp_img:ref_id"], arrs["warp_img:chosen"] = depth_all, ref_id, chosen.numpy()
    arrs["warp_img:warped"], arrs["warp_img:mask"], arrs["warp_img:loss_pc"], arrs["warp_img:grad"] = wv.detach().numpy(), mv.numpy(), loss.detach().numpy().astype(F32), grad
    arrs["warp_img:L"] = L.detach().numpy().astype(F32)
    r = distances(arrs, "warp_img", wv.detach().numpy(), mv.numpy(), arrs["warp_img:L"], grad[ref_id], arrs["warp_img:loss_pc"], gL[ref_id],
                  small[src_id], left, right, depth_all[ref_id], small[ref_id], False)
    gap = min(float(np.abs(np.abs(v) - 1).min()) for v in r["args"])
    assert gap >= 1e-4, ("warp_img", gap)
    print(f"warp_img: ref_id {ref_id.tolist()} margins {margins}")

    path = os.path.join(HERE, "g25_photo_loss.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}  {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)
