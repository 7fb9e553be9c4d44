"""The reference's photometric consistency term, restated in NumPy with analytic gradients; shared by make_goldens_g25.py,
test_photo_loss_host.py and test_gpu_photo_loss.py.

  inverse_warping       mvs_models/homography.py:6-201   img (B,h,w,C), left_cam / right_cam (B,2,3,4), depth (B,1,h,w) | (B,h,w)
  compute_reconstr_loss mvs_models/homography.py:204-225
  photometric_loss      mvsdet.py:845-874
  warp_img              mvsdet.py:701-768 (everything after the resize: the selection of images, cameras and depth)

`dtype=np.float64` is the mathematical function of the fp32 inputs; `dtype=np.float32` follows the reference's fp32 operation
order (every intermediate rounded where torch rounds it; the 3x3 inverse and the small matrix products are then formed in
float64 and rounded once, which is where a LAPACK inverse and this differ by an ulp or two).
"""
import numpy as np


def pixel_grid(n, dtype):
    """homography.py:68-77: (linspace(-1,1,n) + 1) * 0.5 * (n-1).  torch.linspace in fp32 fills from both ends symmetrically:
    start + i*step below the middle, end - (n-1-i)*step from it on (ATen's vectorised kernel may round the last bit differently)."""
    if dtype == np.float64:
        return np.arange(n, dtype=np.float64)
    f = np.float32
    step = f((f(1.0) - f(-1.0)) / f(max(n - 1, 1)))
    i = np.arange(n)
    lin = np.where(i < n // 2, f(-1.0) + step * i.astype(f), f(1.0) - step * (n - 1 - i).astype(f)).astype(f)
    if n == 1:
        lin = np.array([-1.0], f)
    return ((lin + f(1.0)) * f(0.5) * f(n - 1)).astype(f)


def pair_geometry(left_cam, right_cam, dtype=np.float64):
    """K_left^-1 (B,3,3) and K_left [R_right R_left^T | t_right - R_rel t_left] (B,3,4): the LEFT intrinsics on both sides."""
    L, R = np.asarray(left_cam, np.float64), np.asarray(right_cam, np.float64)
    K = L[:, 1, :3, :3]
    Rl, tl, Rr, tr = L[:, 0, :3, :3], L[:, 0, :3, 3:4], R[:, 0, :3, :3], R[:, 0, :3, 3:4]
    Rrel = Rr @ Rl.transpose(0, 2, 1)
    T = np.concatenate([Rrel, tr - Rrel @ tl], axis=2)
    return np.linalg.inv(K).astype(dtype), (K @ T).astype(dtype)


def project(left_cam, right_cam, depth, dtype=np.float64):
    """-> x, y (B,h,w) in source pixels (after the normalise / denormalise round trip), and what the gradient needs."""
    depth = np.asarray(depth)
    if depth.ndim == 4:
        depth = depth[:, 0]
    B, h, w = depth.shape
    Kinv, P = pair_geometry(left_cam, right_cam, dtype)
    d = depth.astype(dtype)
    xg = pixel_grid(w, dtype)[None, None, :]
    yg = pixel_grid(h, dtype)[None, :, None]
    G = lambda M, i, j: M[:, i, j][:, None, None]   # noqa: E731
    r = [G(Kinv, i, 0) * xg + G(Kinv, i, 1) * yg + G(Kinv, i, 2) for i in range(3)]
    c = [ri * d for ri in r]
    p = [G(P, i, 0) * c[0] + G(P, i, 1) * c[1] + G(P, i, 2) * c[2] + G(P, i, 3) for i in range(3)]
    z = p[2] + dtype(1e-10)
    with np.errstate(all="ignore"):
        wm1, hm1 = dtype(w - 1), dtype(h - 1)
        x = (((p[0] / z) / wm1 * dtype(2.0) - dtype(1.0)) + dtype(1.0)) * wm1 / dtype(2.0)
        y = (((p[1] / z) / hm1 * dtype(2.0) - dtype(1.0)) + dtype(1.0)) * hm1 / dtype(2.0)
        q = [G(P, i, 0) * r[0] + G(P, i, 1) * r[1] + G(P, i, 2) * r[2] for i in range(3)]
        dx = (q[0] - (p[0] / z) * q[2]) / z
        dy = (q[1] - (p[1] / z) * q[2]) / z
    return x, y, dx, dy, p[2]


def sample(img, x, y):
    """_bilinear_sample (homography.py:118-201) at absolute coordinates -> warped, mask (B,h,w,1), d warped / dx, d warped / dy
    (B,h,w,C), and sum |w_i tap_i| (B,h,w,C)."""
    dtype = x.dtype.type
    img = np.asarray(img).astype(dtype)
    B, h, w, C = img.shape
    with np.errstate(all="ignore"):
        fx, fy = np.floor(x), np.floor(y)
        mask = (fx >= 0) & (fx + 1 <= w - 1) & (fy >= 0) & (fy <= h - 1)
        cl = lambda v, hi: np.nan_to_num(np.clip(v, 0, hi), nan=0.0)   # noqa: E731
        x0, x1, y0, y1 = cl(fx, w - 1), cl(fx + 1, w - 1), cl(fy, h - 1), cl(fy + 1, h - 1)
        ax, ay = (x1.astype(dtype) - x)[..., None], (y1.astype(dtype) - y)[..., None]
    bi = np.arange(B)[:, None, None]
    x0, x1, y0, y1 = (v.astype(np.int64) for v in (x0, x1, y0, y1))
    a, b, c, d = img[bi, y0, x0], img[bi, y1, x0], img[bi, y0, x1], img[bi, y1, x1]
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        wa, wb, wc, wd = ax * ay, ax * (one - ay), (one - ax) * ay, (one - ax) * (one - ay)
        warped = wa * a + wb * b + wc * c + wd * d
        mag = np.abs(wa * a) + np.abs(wb * b) + np.abs(wc * c) + np.abs(wd * d)
        gx = ay * (c - a) + (one - ay) * (d - b)
        gy = ax * (b - a) + (one - ax) * (d - c)
    return warped, mask[..., None].astype(dtype), gx, gy, mag


def inverse_warping(img, left_cam, right_cam, depth, dtype=np.float64):
    """-> warped (B,h,w,C), mask (B,h,w,1), and aux = dict(dwarped (B,h,w,C): d warped / d depth, mag, x, y, p2)."""
    x, y, dx, dy, p2 = project(left_cam, right_cam, depth, dtype)
    warped, mask, gx, gy, mag = sample(img, x, y)
    with np.errstate(all="ignore"):
        dw = gx * dx[..., None] + gy * dy[..., None]
    return warped, mask, dict(dwarped=dw, mag=mag, x=x, y=y, p2=p2)


def _sl1(d):
    a = np.abs(d)
    return np.where(a < 1, d.dtype.type(0.5) * a * a, a - d.dtype.type(0.5))


def compute_reconstr_loss(warped, ref, mask, simple=True, dtype=np.float64):
    """-> L, terms (3), d L / d warped (B,h,w,C), and the smooth-L1 arguments of the three terms (for the margin checks)."""
    warped, ref, mask = (np.asarray(v).astype(dtype) for v in (warped, ref, mask))
    wm, rm = warped * mask, ref * mask
    d0 = wm - rm
    dxs = (wm[:, :, 1:] - wm[:, :, :-1]) - (rm[:, :, 1:] - rm[:, :, :-1])
    dys = (wm[:, 1:] - wm[:, :-1]) - (rm[:, 1:] - rm[:, :-1])
    mean = lambda v: (np.sum(_sl1(v).astype(np.float64)) / v.size).astype(dtype) if v.size else dtype(np.nan)   # noqa: E731
    t = [mean(d0), dtype(0.0) if simple else mean(dxs), dtype(0.0) if simple else mean(dys)]
    half = dtype(0.5)
    L = t[0] if simple else half * t[0] + half * (t[1] + t[2])
    g = np.clip(d0, -1, 1) * ((1.0 if simple else 0.5) / d0.size)
    if not simple:
        if dxs.size:
            cx = np.clip(dxs, -1, 1) * (0.5 / dxs.size)
            g[:, :, 1:] += cx
            g[:, :, :-1] -= cx
        if dys.size:
            cy = np.clip(dys, -1, 1) * (0.5 / dys.size)
            g[:, 1:] += cy
            g[:, :-1] -= cy
    return L, np.array(t, dtype), (g * mask).astype(dtype), (d0, dxs, dys)


def photometric_select(L, masks, dtype=np.float64):
    """L (n), masks (n,B,h,w,1) -> loss_pc, wins (n) int64: ties to the lower scene."""
    L = np.asarray(L, dtype)
    masks = np.asarray(masks).astype(dtype)
    v = L.reshape((-1,) + (1,) * (masks.ndim - 1)) + dtype(1e4) * (dtype(1.0) - masks)
    best = np.argmin(v, axis=0)                     # the first minimum
    keep = np.min(v, axis=0) < dtype(1e4)
    wins = np.array([int(np.sum((best == i) & keep)) for i in range(len(L))], np.int64)
    total = masks[0].size
    return dtype(np.sum(wins * L.astype(np.float64)) / total), wins


def photometric_loss(warped_list, mask_list, ref_list, dtype=np.float64, simple=False):
    """-> loss_pc, [d loss_pc / d warped_i], wins, [L_i]."""
    res = [compute_reconstr_loss(w, r, m, simple, dtype) for w, r, m in zip(warped_list, ref_list, mask_list)]
    L = [r[0] for r in res]
    loss, wins = photometric_select(L, np.stack([np.asarray(m) for m in mask_list]), dtype)
    total = np.asarray(mask_list[0]).size
    return loss, [r[2] * (wins[i] / total) for i, r in enumerate(res)], wins, L


def scene_cameras(ref_w2c, ref_feat_intrinsic, neighbor_ids, ref_id):
    """warp_img (mvsdet.py:731-739): packed (B,2,3,4) cameras of the chosen views and of their FIRST neighbours, and those ids."""
    w2c, K = np.asarray(ref_w2c, np.float32), np.asarray(ref_feat_intrinsic, np.float32)
    N = w2c.shape[0]
    Kn = np.broadcast_to(K, (N, 4, 4)) if K.ndim == 2 else K
    full = np.stack([w2c, Kn], axis=1)[:, :, :3, :]
    ref_id = np.asarray(ref_id, np.int64)
    src_id = np.asarray(neighbor_ids, np.int64)[ref_id, 0]
    return full[ref_id], full[src_id], src_id


def loss_and_depth_grad(img, left_cam, right_cam, depth, ref, simple=False, dtype=np.float64):
    """One scene end to end -> dict(warped, mask, L, terms, loss_pc, grad (B,h,w) = d loss_pc / d depth, aux, args)."""
    warped, mask, aux = inverse_warping(img, left_cam, right_cam, depth, dtype)
    L, terms, gw, args = compute_reconstr_loss(warped, ref, mask, simple, dtype)
    loss, wins = photometric_select([L], mask[None], dtype)
    with np.errstate(all="ignore"):
        prod = np.where(gw != 0, gw * aux["dwarped"], 0)
    grad = np.sum(prod, axis=-1) * (wins[0] / mask.size)
    return dict(warped=warped, mask=mask, L=L, terms=terms, loss_pc=loss, grad=grad.astype(dtype), gw=gw, aux=aux, args=args, wins=wins)


# ------------------------------------------------------------------------------------------- fixture G25 (tests/golden/make_goldens_g25.py)
SINGLE_CASES = ["tiny", "small", "ref_true", "behind", "lastrow", "simple", "warp_img"]
MULTI_CASES = [("two_scenes", 2), ("three_scenes", 3)]


def g25_case(g, tag):
    """One scene of G25 in the packed form -> dict(img, left_cam, right_cam, depth (B,h,w), ref, simple, warped, mask, L, loss_pc, grad,
    dist_*); the scene forms (ref_true, warp_img) also keep their own inputs (`scene`)."""
    c = {k.split(":", 1)[1]: g[k] for k in g.files if k.startswith(tag + ":")}
    c["simple"] = bool(c.get("simple", 0))
    if tag == "ref_true":
        imgs = (c["imgs_u8"].astype(np.float32) / np.float32(255)).astype(np.float32)
        c["scene"] = dict(imgs=imgs, w2c=c["w2c"], K=c["K"], neighbor_ids=c["neighbor_ids"], ref_id=c["ref_id"], depth_pad=c["depth_pad"])
        left, right, src_id = scene_cameras(c["w2c"], c["K"], c["neighbor_ids"], c["ref_id"])
        c.update(img=imgs[src_id], ref=imgs[c["ref_id"]], left_cam=left, right_cam=right, depth=c["depth_pad"][c["ref_id"], 0, :59, :80],
                 src_id=src_id)
    elif tag == "warp_img":
        left, right, src_id = scene_cameras(c["w2c"], c["K"], c["neighbor_ids"], c["ref_id"])
        small = c["chosen"][np.argsort(c["ref_id"])] if len(c["ref_id"]) == c["imgs"].shape[0] else None
        c["scene"] = dict(imgs=c["imgs"], w2c=c["w2c"], K=c["K"], neighbor_ids=c["neighbor_ids"], ref_id=c["ref_id"], depth=c["depth"])
        c.update(img=small[src_id], ref=c["chosen"], left_cam=left, right_cam=right, depth=c["depth"][c["ref_id"]],
                 grad_all=c["grad"], grad=c["grad"][c["ref_id"]], src_id=src_id)
    return c


def bar(dist, scale=1.0):
    """4 x the distance the generator measured between the reference and the float64 restatement (two fp32 evaluations with different
    operation orders may each sit that far from float64, on either side), floor 1e-6, times the quantity's scale."""
    return max(4.0 * float(dist), 1e-6) * float(scale)


def check_against(c, warped, mask, L, loss_pc, grad, other, what, simple_loss_pc=True):
    """The issue's comparisons of one scene's numbers with `other` = dict(warped, mask, L, loss_pc, grad, mag) -- G25 or the restatement.
    Prints each figure before it asserts."""
    m = (np.asarray(other["mask"]) != 0)[..., 0]
    assert np.array_equal(np.asarray(mask) != 0, np.asarray(other["mask"]) != 0), f"{what}: masks differ"
    scale = float(np.abs(c["img"]).max())
    d_in = float(np.abs(warped - other["warped"])[m].max()) if m.any() else 0.0
    with np.errstate(all="ignore"):
        d_out = float(np.nanmax((np.abs(warped - other["warped"]) / np.maximum(other["mag"], 1e-30))[~m])) if (~m).any() else 0.0
    d_L = abs(float(L) - float(other["L"])) / abs(float(other["L"]))
    gmax = float(np.abs(other["grad"]).max())
    d_g = float(np.abs(grad - other["grad"]).max()) / gmax
    line = (f"{what}: warped in {d_in:.2e} (bar {bar(c['dist_warped_in'] / scale, scale):.2e})  out {d_out:.2e} (bar {bar(c['dist_warped_out']):.2e})  "
            f"L {d_L:.2e} (bar {bar(c['dist_L']):.2e})  grad {d_g:.2e} of max {gmax:.3g} (bar {bar(c['dist_grad']):.2e})")
    if loss_pc is not None:
        d_pc = abs(float(loss_pc) - float(other["loss_pc"])) / abs(float(other["loss_pc"]))
        line += f"  loss_pc {d_pc:.2e} (bar {bar(c['dist_loss_pc']):.2e})"
    print(line)
    assert d_in <= bar(c["dist_warped_in"] / scale, scale), what
    assert d_out <= bar(c["dist_warped_out"]), what
    assert d_L <= bar(c["dist_L"]), what
    assert d_g <= bar(c["dist_grad"]), what
    assert np.all(np.asarray(grad)[~m] == 0), f"{what}: the gradient outside the mask is not exactly 0"
    if loss_pc is not None:
        assert d_pc <= bar(c["dist_loss_pc"]), what
