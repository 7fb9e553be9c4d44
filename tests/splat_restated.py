"""The Gaussian rasteriser of csrc/splat.hip restated in torch on the CPU, vectorised over pixels, in float64 or
float32, differentiable by autograd (the 0.99 cap straight-through), with the margin of every decision it takes.

    cameras(...)   the front of cuda_splatting.py::render_cuda: what it hands the rasteriser per view, float64 -> (V,40) float32
    render(...)    image (V,3,H,W), per-Gaussian margins (V,G), the smallest per-(pixel, Gaussian) margin of every pixel (V,H,W)

Nothing here is taken from the kernels: the formulas are the issue's, written a second time.
"""
import math

import numpy as np
import torch

TILE = 16
CAM = 40
NEAR_Z = 0.2
ALPHA_MIN = 1.0 / 255.0
ALPHA_CAP = 0.99
T_STOP = 1e-4

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431, -0.6690465435572892,
      0.47308734787878004, -1.7701307697799304, 0.6258357354491761)


def sh_basis(d, n):
    """(..., 3) unit directions -> (..., n) basis values, n in {1, 4, 9, 16, 25}: degrees 0..3 as published, degree 4 in the same sign
    convention (odd |m| negative)."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = [C0 * torch.ones_like(x)]
    if n > 1:
        out += [-C1 * y, C1 * z, -C1 * x]
    if n > 4:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        out += [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if n > 9:
        out += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    if n > 16:
        out += [C4[0] * xy * (xx - yy), C4[1] * yz * (3 * xx - yy), C4[2] * xy * (7 * zz - 1), C4[3] * yz * (7 * zz - 3),
                C4[4] * (35 * zz * zz - 30 * zz + 3), C4[5] * xz * (7 * zz - 3), C4[6] * (xx - yy) * (7 * zz - 1),
                C4[7] * xz * (xx - 3 * yy), C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    assert len(out) == n
    return torch.stack(out, dim=-1)


def cameras(extrinsics, intrinsics, near, far, scale_invariant=True, dtype=np.float32):
    """cuda_splatting.py:66-90 and projection.py::get_fov for V views: numpy float32 in -> (V,40) float32: the transposed view matrix,
    the transposed full projection, tan(fov/2) x and y, the camera position, the scale; the reference's fp32 scaling steps, then
    float64, rounded once (dtype=np.float64: not rounded)."""
    e = np.asarray(extrinsics, np.float32).copy()
    k = np.asarray(intrinsics, np.float32)
    near, far = np.asarray(near, np.float32), np.asarray(far, np.float32)
    V = e.shape[0]
    scale = (np.float32(1) / near) if scale_invariant else np.ones(V, np.float32)
    if scale_invariant:
        e[:, :3, 3] = e[:, :3, 3] * scale[:, None]
        near, far = near * scale, far * scale
    out = np.zeros((V, CAM), np.float64)
    for v in range(V):
        E = e[v].astype(np.float64)
        E[3] = (0, 0, 0, 1)
        ki = np.linalg.inv(k[v].astype(np.float64))

        def ray(x, y):
            r = ki @ np.array([x, y, 1.0])
            return r / np.linalg.norm(r)
        tanx = math.tan(0.5 * math.acos(float(ray(0, 0.5) @ ray(1, 0.5))))
        tany = math.tan(0.5 * math.acos(float(ray(0.5, 0) @ ray(0.5, 1))))
        n, f = float(near[v]), float(far[v])
        P = np.zeros((4, 4))
        P[0, 0], P[1, 1], P[3, 2] = 1 / tanx, 1 / tany, 1.0
        P[2, 2], P[2, 3] = f / (f - n), -(f * n) / (f - n)
        view = np.linalg.inv(E).T
        out[v, :16] = view.reshape(-1)
        out[v, 16:32] = (view @ P.T).reshape(-1)
        out[v, 32], out[v, 33] = tanx, tany
        out[v, 34:37] = e[v, :3, 3]
        out[v, 37] = scale[v]
    return out.astype(dtype)


def preprocess(means, covs, sh, opac, cam, H, W, use_sh=True):
    """One view.  Tensors of one dtype; cam (40).  -> dict of per-Gaussian quantities, the cull mask and the decision margins."""
    dt = means.dtype
    cam = cam.to(dt)
    VM, PM = cam[:16].view(4, 4), cam[16:32].view(4, 4)
    tanx, tany, campos, s = cam[32], cam[33], cam[34:37], cam[37]
    m = means * s
    t = m @ VM[:3, :3] + VM[3, :3]
    hom = m @ PM[:3, :] + PM[3, :]
    tz = t[:, 2]
    ok = tz > NEAR_Z
    tz_safe = torch.where(ok, tz, torch.ones_like(tz))
    pw = 1.0 / (hom[:, 3] + 1e-7)
    S = covs * (s * s)
    iu = torch.triu_indices(3, 3, device=means.device)
    up = S[:, iu[0], iu[1]]                                  # the upper triangle only
    Sig = torch.zeros_like(S)
    Sig[:, iu[0], iu[1]] = up
    Sig = Sig + torch.triu(Sig, 1).transpose(1, 2)
    limx, limy = 1.3 * tanx, 1.3 * tany
    rx, ry = t[:, 0] / tz_safe, t[:, 1] / tz_safe
    txc = torch.clamp(rx, -limx, limx) * tz_safe
    tyc = torch.clamp(ry, -limy, limy) * tz_safe
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz_safe, zero, -(fx * txc) / (tz_safe * tz_safe)], -1),
                     torch.stack([zero, fy / tz_safe, -(fy * tyc) / (tz_safe * tz_safe)], -1)], 1)      # (G,2,3)
    M = J @ VM[:3, :3].T                                      # J W_rot
    cov2 = M @ Sig @ M.transpose(1, 2)
    a, b, c = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    ok = ok & (det != 0)
    det_safe = torch.where(det != 0, det, torch.ones_like(det))
    conic = torch.stack([c / det_safe, -b / det_safe, a / det_safe], -1)
    mid = 0.5 * (a + c)
    lam = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    r3 = 3.0 * torch.sqrt(lam)
    radius = torch.ceil(r3)
    px = ((hom[:, 0] * pw + 1.0) * W - 1.0) * 0.5
    py = ((hom[:, 1] * pw + 1.0) * H - 1.0) * 0.5
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    q = torch.stack([(px - radius) / TILE, (px + radius + (TILE - 1)) / TILE, (py - radius) / TILE, (py + radius + (TILE - 1)) / TILE], -1)
    q = q.detach()
    rect = torch.stack([torch.clamp(torch.trunc(q[:, 0]), 0, gx), torch.clamp(torch.trunc(q[:, 1]), 0, gx),
                        torch.clamp(torch.trunc(q[:, 2]), 0, gy), torch.clamp(torch.trunc(q[:, 3]), 0, gy)], -1).long()
    ok = ok & ((rect[:, 1] - rect[:, 0]) * (rect[:, 3] - rect[:, 2]) > 0)
    if use_sh:
        d = m - campos
        d = d / torch.sqrt((d * d).sum(-1, keepdim=True))
        raw = (sh * sh_basis(d, sh.shape[-1])[:, None, :]).sum(-1) + 0.5         # (G,3)
        colour = torch.clamp(raw, min=0.0)
    else:
        raw = torch.ones_like(sh[:, :, 0])        # no clamp on precomputed colours: nothing to decide
        colour = sh[:, :, 0]
    # decision margins (detached): each is |value - threshold| in the unit named
    with torch.no_grad():
        frac = lambda x: torch.minimum(x - torch.floor(x), torch.ceil(x) - x)    # distance to the nearest integer  # noqa: E731
        # truncation then the clamp to [0, grid]: the result changes at the integers 1 .. grid only
        grid = torch.tensor([gx, gx, gy, gy], dtype=dt, device=means.device)
        qm = (q - torch.minimum(torch.clamp(torch.round(q), min=1.0), grid)).abs() * TILE
        margins = dict(z=(tz - NEAR_Z).abs() / NEAR_Z, radius=frac(r3), rect=qm.min(-1).values,
                       tan=torch.minimum((rx.abs() - limx).abs() / limx, (ry.abs() - limy).abs() / limy),
                       colour=raw.abs().min(-1).values)
    return dict(ok=ok, depth=tz, px=px, py=py, conic=conic, colour=colour, rect=rect, radius=radius, margins=margins)


def render(means, covs, sh, opac, cams, bg, H, W, dtype=torch.float64, use_sh=True):
    """V views of one Gaussian set.  means (G,3), covs (G,3,3), sh (G,3,d), opac (G), cams (V,40), bg (V,3): tensors (leaves may
    require grad; they are cast to `dtype` inside autograd).  -> image (V,3,H,W), info dict:
      gauss  {name: (V,G)} per-Gaussian margins;  ok (V,G) not culled;  pixel (V,H,W) the smallest relative per-(pixel, Gaussian) margin;
      keys (V) (Gaussian, tile) pairs;  stopped (V,H,W) the pixel hit the early stop;  n_contrib (V,H,W)."""
    means, covs, sh, opac = means.to(dtype), covs.to(dtype), sh.to(dtype), opac.to(dtype)
    cams, bg = torch.as_tensor(cams), torch.as_tensor(bg).to(dtype)
    V = cams.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    X, Y = xs.to(dtype), ys.to(dtype)
    tx, ty = xs // TILE, ys // TILE
    images, gauss, oks, pixel, keys, stopped, ncontrib = [], [], [], [], [], [], []
    for v in range(V):
        p = preprocess(means, covs, sh, opac, cams[v], H, W, use_sh)
        ok = p["ok"]
        idx = torch.nonzero(ok).flatten()
        order = idx[torch.sort(p["depth"][idx].detach(), stable=True).indices]
        T = torch.ones((H, W), dtype=dtype)
        C = torch.zeros((3, H, W), dtype=dtype)
        done = torch.zeros((H, W), dtype=torch.bool)
        pm = torch.full((H, W), 1.0, dtype=torch.float64)
        count = torch.zeros((H, W), dtype=torch.long)
        last = torch.zeros((H, W), dtype=torch.long)
        r = p["rect"]
        keys.append(int(((r[:, 1] - r[:, 0]) * (r[:, 3] - r[:, 2]))[ok].sum()))
        for g in order.tolist():
            x0, x1, y0, y1 = r[g].tolist()
            live = (tx >= x0) & (tx < x1) & (ty >= y0) & (ty < y1) & ~done
            if not bool(live.any()):
                continue
            count = count + live.long()
            dx, dy = p["px"][g] - X, p["py"][g] - Y
            A, B, Cc = p["conic"][g]
            power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
            raw = opac[g] * torch.exp(power)
            alpha = raw + (torch.clamp(raw, max=ALPHA_CAP) - raw).detach()           # the cap passes the gradient through
            c1 = live & ~(power > 0)
            c2 = c1 & ~(alpha < ALPHA_MIN)
            Tn = T * (1.0 - alpha)
            stop = c2 & (Tn < T_STOP)
            c3 = c2 & ~stop
            with torch.no_grad():
                one = torch.ones((H, W), dtype=torch.float64)
                m_alpha = torch.where(c1, (alpha.double() / ALPHA_MIN - 1.0).abs(), one)
                m_T = torch.where(c2, (Tn.double() / T_STOP - 1.0).abs(), one)
                m_cap = torch.where(c2, (raw.double() / ALPHA_CAP - 1.0).abs(), one)
                pm = torch.minimum(pm, torch.minimum(m_alpha, torch.minimum(m_T, m_cap)))
            w = torch.where(c3, alpha * T, torch.zeros_like(T))
            # a pixel that skips the Gaussian takes nothing from it: not colour * 0, which a NaN colour would turn into NaN
            C = C + torch.where(c3, p["colour"][g][:, None, None] * w, torch.zeros_like(C))
            T = torch.where(c3, Tn, T)
            last = torch.where(c3, count, last)
            done = done | stop
        images.append(C + T * bg[v][:, None, None])
        gauss.append(p["margins"])
        oks.append(ok)
        pixel.append(pm)
        stopped.append(done)
        ncontrib.append(last)
    info = dict(gauss={k: torch.stack([g[k] for g in gauss]) for k in gauss[0]}, ok=torch.stack(oks), pixel=torch.stack(pixel), keys=keys,
                stopped=torch.stack(stopped), n_contrib=torch.stack(ncontrib))
    return torch.stack(images), info


def bar(x64, x32, got_scale=None):
    """The comparison bar of 4.12 / 4.15 for a quantity x: elementwise max(1e-4 |x| + 1.25e-6 max|x|, 4 x the float32 restatement's own
    distance from float64), the latter as its largest element."""
    x64, x32 = np.asarray(x64, np.float64), np.asarray(x32, np.float64)
    top = float(np.abs(x64).max()) if x64.size else 0.0
    own = float(np.abs(x32 - x64).max()) if x64.size else 0.0
    return np.maximum(1e-4 * np.abs(x64) + 1.25e-6 * top, 4.0 * own), own
