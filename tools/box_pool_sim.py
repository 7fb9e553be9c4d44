#!/usr/bin/env python3
"""CPU restatement (numpy, no library, no GPU) of the sweep geometry kernel's corner fast path and of its two run policies
(csrc/sweep_kernel.h: plane_sweep_coords_kernel), for K = 2 neighbours and 32x4 tiles:

  slot policy    every neighbour owns one LDS slot of `cap` texels; runs of planes whose union box fits the slot share it
  pooled policy  the two slots are one pool of 2*(cap + 8) - 8 texels; over planes on which the other neighbour has no footprint
                 a run's union box may grow to the pool (a WIDE box, kept at the pool's base); a wide run always refills, and
                 the other neighbour's next staged plane refills too

and what they cost a (view, tile) block of the slab kernel that sweeps all planes: stall events (planes on which at least one
neighbour refills its box), staged and gathered footprints, texels moved by the refills.

Footprints the kernel hands to its exact per-pixel scan (a denominator changing sign over the tile, a non-finite position) are
scanned here per pixel too.  Positions are computed in float32 with the kernel's order of operations (a fused multiply-add is
restated in float64 and rounded once), so boxes agree with the kernel's except where a position lies within rounding of a texel
border.

Usage: python tools/box_pool_sim.py [workload ...] [--seeds 1000,1001,1002] [--cap 312]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TW, TH, PAD = 32, 4, 8
f32 = np.float32
EMPTY = np.array([1, 0, 1, 0], np.int64)


def scene_cameras(n_views, hw, seed, per_view_K, near_far, num_depth, stride=4):
    """mvsdet.py:407-450 on the host (hotpath._host_geometry without the library): proj_rel (N,K,4,4), depth (N,D), float32."""
    import torch
    from mvsdet_amd import functional as F_, synthetic
    meta = synthetic.make_img_meta(n_views, hw, seed=seed, per_view_intrinsics=per_view_K)
    w2c = torch.tensor(np.array(meta["lidar2img"]["extrinsic"]))
    K = torch.tensor(np.array(meta["lidar2img"]["intrinsic"]))
    ratio = meta["ori_shape"][0] / (meta["img_shape"][0] / stride)
    K_feat = K.clone()
    if K_feat.dim() == 2:
        K_feat[:2] /= ratio
    else:
        K_feat[:, :2] /= ratio
    n = w2c.shape[0]
    c2w = w2c.inverse()
    nbr = F_.get_nearest_pose_ids(c2w, c2w, min(2, n - 1), maskself=True)
    ref_proj, nei = F_.collect_proj(w2c, K_feat, nbr)
    inv_ref = torch.inverse(ref_proj)
    proj_rel = torch.stack([torch.matmul(p, inv_ref) for p in nei], dim=1)
    interval = (float(near_far[1]) - float(near_far[0])) / num_depth
    depth = np.arange(float(near_far[0]), float(near_far[1]), interval, dtype=np.float32)
    return proj_rel.numpy().astype(np.float32), np.tile(depth[None], (n, 1)), int(hw[0]), int(hw[1])   # the sweep runs on the maps' own shape


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _positions(P, x, y, d, H, W):
    """sample_ray + sample_at: P (...,16), x, y, d broadcastable float32 -> (ix, iy, Z)."""
    rx = _fma(P[..., 1], y, P[..., 0] * x) + P[..., 2]
    ry = _fma(P[..., 5], y, P[..., 4] * x) + P[..., 6]
    rz = _fma(P[..., 9], y, P[..., 8] * x) + P[..., 10]
    X = rx * d + P[..., 3]
    Y = ry * d + P[..., 7]
    Z = rz * d + P[..., 11]
    with np.errstate(all="ignore"):
        px, py = X / Z, Y / Z
        gx = px / f32((W - 1) * 0.5) - f32(1)
        gy = py / f32((H - 1) * 0.5) - f32(1)
        ix = _fma(gx + f32(1), np.broadcast_to(f32(W * 0.5), gx.shape), np.broadcast_to(f32(-0.5), gx.shape))
        iy = _fma(gy + f32(1), np.broadcast_to(f32(H * 0.5), gy.shape), np.broadcast_to(f32(-0.5), gy.shape))
    return ix, iy, Z


def _exact_box(P, d, x0, y0, H, W):
    """The wave-wide scan of one (tile, plane, neighbour): bounding box of the taps inside the image."""
    xs, ys = np.meshgrid(np.arange(x0, min(x0 + TW, W)), np.arange(y0, min(y0 + TH, H)))
    ix, iy, _ = _positions(P, xs.astype(f32).ravel(), ys.astype(f32).ravel(), f32(d), H, W)
    with np.errstate(all="ignore"):
        fx, fy = np.floor(ix), np.floor(iy)
    x0in, x1in = (fx >= 0) & (fx <= W - 1), (fx >= -1) & (fx <= W - 2)
    y0in, y1in = (fy >= 0) & (fy <= H - 1), (fy >= -1) & (fy <= H - 2)
    ok = (x0in | x1in) & (y0in | y1in)
    if not ok.any():
        return EMPTY
    cx = np.clip(np.nan_to_num(fx[ok], nan=-1.0, posinf=W - 1, neginf=-1.0), -1, W - 1).astype(np.int64)
    cy = np.clip(np.nan_to_num(fy[ok], nan=-1.0, posinf=H - 1, neginf=-1.0), -1, H - 1).astype(np.int64)
    return np.array([np.where(x0in[ok], cx, cx + 1).min(), np.where(x1in[ok], cx + 1, cx).max(),
                     np.where(y0in[ok], cy, cy + 1).min(), np.where(y1in[ok], cy + 1, cy).max()], np.int64)


def footprint_boxes(proj, depth, H, W):
    """-> boxes (N, tiles, K, D, 4) int64 [x0, x1, y0, y1]; an empty footprint is (1, 0, 1, 0)."""
    N, K = proj.shape[:2]
    D = depth.shape[1]
    tiles_x, tiles_y = (W + TW - 1) // TW, (H + TH - 1) // TH
    tx0 = (np.arange(tiles_x * tiles_y) % tiles_x) * TW
    ty0 = (np.arange(tiles_x * tiles_y) // tiles_x) * TH
    xa, xb = tx0, np.minimum(tx0 + TW, W) - 1
    ya, yb = ty0, np.minimum(ty0 + TH, H) - 1
    P = proj.reshape(N, 1, K, 1, 1, 16).astype(f32)
    d = depth.reshape(N, 1, 1, D, 1).astype(f32)
    cx = np.stack([xa, xb, xa, xb], -1).astype(f32).reshape(1, -1, 1, 1, 4)
    cy = np.stack([ya, ya, yb, yb], -1).astype(f32).reshape(1, -1, 1, 1, 4)
    ix, iy, Z = _positions(P, cx, cy, d, H, W)            # (N, tiles, K, D, 4 corners)
    ok = np.isfinite(Z).all(-1) & np.isfinite(ix).all(-1) & np.isfinite(iy).all(-1) & ((Z > 0).all(-1) | (Z < 0).all(-1))
    with np.errstate(all="ignore"):
        ux0, ux1 = np.floor(ix.min(-1) - f32(1e-3)), np.floor(ix.max(-1) + f32(1e-3)) + 1
        uy0, uy1 = np.floor(iy.min(-1) - f32(1e-3)), np.floor(iy.max(-1) + f32(1e-3)) + 1
    fx0, fx1 = np.maximum(ux0, 0), np.minimum(ux1, W - 1)
    fy0, fy1 = np.maximum(uy0, 0), np.minimum(uy1, H - 1)
    out = ~(ok & (fx1 >= fx0) & (fy1 >= fy0))
    boxes = np.stack([fx0, fx1, fy0, fy1], -1)
    boxes = np.where(out[..., None], EMPTY.astype(np.float64), np.nan_to_num(boxes)).astype(np.int64)
    for n, t, j, dd in zip(*np.nonzero(~ok)):               # the kernel's exact scan
        boxes[n, t, j, dd] = _exact_box(proj[n, j].reshape(16).astype(f32), depth[n, dd], tx0[t], ty0[t], H, W)
    return boxes


def _area(b):
    return np.maximum(b[..., 1] - b[..., 0] + 1, 0) * np.maximum(b[..., 3] - b[..., 2] + 1, 0)


def _walk(b, other_live, cap, pool):
    """The greedy run pass of one neighbour for B blocks at once.  b (B, D, 4).  -> final boxes (B, D, 4), staged (B, D),
    refill (B, D) before the pooled policy's forced refills."""
    B, D, _ = b.shape
    area = _area(b)
    live = area > 0
    planes = np.arange(D)
    lo = np.maximum.accumulate(np.where(other_live, planes[None], -1), axis=1)   # last plane <= d where the other is live
    run_id = -np.ones((B, D), np.int64)
    run_box = np.zeros((B, D + 1, 4), np.int64)
    cur = np.zeros(B, np.int64)
    nrun = np.zeros(B, np.int64)
    first = np.zeros(B, np.int64)
    open_ = np.zeros(B, bool)
    u = np.zeros((B, 4), np.int64)
    rows = np.arange(B)
    for d in range(D):
        bd, lv = b[:, d], live[:, d]
        cap_b = np.where(lo[:, d] < d, pool, cap)
        fits = lv & (area[:, d] <= cap_b) & (cap > 0)
        c = np.stack([np.minimum(u[:, 0], bd[:, 0]), np.maximum(u[:, 1], bd[:, 1]),
                      np.minimum(u[:, 2], bd[:, 2]), np.maximum(u[:, 3], bd[:, 3])], -1)
        ac = _area(c)
        ext = fits & open_ & ((ac <= cap) | ((ac <= pool) & (lo[:, d] < first)))
        u[ext] = c[ext]
        run_id[ext, d] = cur[ext]
        close = lv & ~ext & open_
        run_box[rows[close], cur[close]] = u[close]
        open_[close] = False
        start = fits & ~ext
        cur[start] = nrun[start]
        nrun[start] += 1
        first[start] = d
        u[start] = bd[start]
        run_id[start, d] = cur[start]
        open_[start] = True
    run_box[rows[open_], cur[open_]] = u[open_]
    staged = run_id >= 0
    rid = np.where(staged, run_id, 0)
    final = np.where(staged[..., None], run_box[rows[:, None], rid], b)
    prev = np.concatenate([np.full((B, 1, 4), -1, np.int64), run_box[:, :-1]], 1)      # run 0 differs from the empty slot
    differs = (_area(run_box) > cap) | (run_box != prev).any(-1)
    seen = np.concatenate([-np.ones((B, 1), np.int64), np.maximum.accumulate(run_id, axis=1)[:, :-1]], 1)
    refill = staged & (run_id > seen) & differs[rows[:, None], rid]
    return final, staged, refill


def run_policy(boxes, cap, pooled):
    """boxes (B, 2, D, 4) -> dict of final boxes (B, 2, D, 4), live / staged / refill (B, 2, D) under the slot or pooled policy."""
    pool = 2 * (cap + PAD) - PAD if pooled else cap
    live = _area(boxes) > 0
    fin, st, rf = zip(*[_walk(boxes[:, j], live[:, 1 - j], cap, pool) for j in (0, 1)])
    fin, st, rf = np.stack(fin, 1), np.stack(st, 1), np.stack(rf, 1)
    if pooled:   # the other neighbour's first staged plane after a wide staged plane refills
        wide = st & (_area(fin) > cap)
        for j in (0, 1):
            carry = np.zeros(boxes.shape[0], bool)
            for d in range(boxes.shape[2]):
                s = st[:, j, d]
                rf[:, j, d] |= s & carry
                carry = (carry & ~s) | wide[:, 1 - j, d]
    return dict(boxes=fin, live=live, staged=st, refill=rf)


def summarize(r):
    B = r["boxes"].shape[0]
    events = (r["refill"].any(1)).sum()
    return dict(blocks=B, events_per_block=events / B, refills=int(r["refill"].sum()), staged=int(r["staged"].sum()),
                gathered=int((r["live"] & ~r["staged"]).sum()), live=int(r["live"].sum()),
                texels_per_block=float((_area(r["boxes"]) * r["refill"]).sum() / B),
                wide=int((r["staged"] & (_area(r["boxes"]) > r.get("cap", 1 << 30))).sum()))


def simulate(proj, depth, H, W, cap=312):
    boxes = footprint_boxes(proj, depth, H, W)
    b = boxes.reshape(-1, *boxes.shape[2:])
    out = {}
    for name, pooled in (("slot", False), ("pooled", True)):
        r = run_policy(b, cap, pooled)
        r["cap"] = cap
        out[name] = summarize(r)
    return out


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["scannet_40v_64d_120x160"])
    ap.add_argument("--seeds", default="1000,1001,1002")
    ap.add_argument("--cap", type=int, default=312)
    a = ap.parse_args()
    for name in a.workloads:
        w = bench.WORKLOADS[name]
        tot = {}
        for seed in [int(s) for s in a.seeds.split(",")]:
            proj, depth, H, W = scene_cameras(w["N"], (w["H"], w["W"]), seed, w["per_view_K"], w["near_far"], w["D"])
            if proj.shape[1] != 2:
                raise SystemExit("K = 2 only")
            for pol, s in simulate(proj, depth, H, W, a.cap).items():
                t = tot.setdefault(pol, {k: 0 for k in s})
                for k, v in s.items():
                    t[k] += v
        n = len(a.seeds.split(","))
        for pol, t in tot.items():
            print(f"{name} {pol:6s}: stall events / block {t['events_per_block'] / n:.2f}, refills / staged {t['refills'] / max(t['staged'], 1):.3f}, "
                  f"staged {t['staged']} gathered {t['gathered']} of {t['live']} live footprints (wide staged {t['wide']}), "
                  f"texels DMA-ed / block {t['texels_per_block'] / n:.0f}")


if __name__ == "__main__":
    main()
