"""float64 yardsticks of the FPN's gradients for the tests (a helper, not collected).

The yardstick is torch's CPU float64 autograd: of single F.conv2d / F.interpolate calls for the kernels, of `fpn_restated.level0_64`
for the module's chain.  tests/test_fpn_grad_host.py pins it against the hand-written sums below (`*_sum`), so the yardstick is
neither the code under test nor one formula trusted twice.  Everything here runs on the CPU; tensors from a device are brought over.

    dW[o,c,dy,dx] = sum_{n,y,x} gy[n,o,y,x] x[n,c,y+dy-1,x+dx-1]       (zero outside; 1x1: the centre tap alone)
    dx[n,c,y,x]   = sum_{o,dy,dx} g[n,o,y-dy+1,x-dx+1] w[o,c,dy,dx]
    up^T(g)[yt,xt] = sum of g over the pixels whose nearest source (ATen's float32 index) is (yt,xt)
"""
import torch
import torch.nn.functional as F

import fpn_restated as R


def _d(t):
    return t.detach().double().cpu()


def dw64(gy, x, taps):
    """Weight gradient of F.conv2d(x, w, padding=k//2) for the output gradient gy: (Cout,C,k,k) in float64."""
    gy, x = _d(gy), _d(x)
    k = 3 if taps == 9 else 1
    w = torch.zeros(gy.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.conv2d(x, w, padding=k // 2), w, gy)[0]


def dx64(g, w):
    """Input gradient of F.conv2d(x, w, padding=k//2) for the output gradient g: (N,C,H,W) in float64; w (Cout,C,k,k) or (Cout,C)."""
    g, w = _d(g), _d(w)
    if w.dim() == 2:
        w = w.view(w.shape[0], w.shape[1], 1, 1)
    x = torch.zeros(g.shape[0], w.shape[1], g.shape[2], g.shape[3], dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.conv2d(x, w, padding=w.shape[2] // 2), x, g)[0]


def up_t(g, size):
    """ATen's backward of F.interpolate(top, size=g.shape[2:], mode='nearest') in g's own dtype, on the CPU: (N,C,*size)."""
    g = g.detach().cpu()
    top = torch.zeros(g.shape[0], g.shape[1], size[0], size[1], dtype=g.dtype, requires_grad=True)
    return torch.autograd.grad(F.interpolate(top, size=g.shape[2:], mode="nearest"), top, g)[0]


def up_t64(g, size):
    return up_t(_d(g), size)


def three_term_dw64(gy, x, taps):
    """The three products the weight-gradient kernel multiplies, summed in float64: gy_hi x_hi + gy_hi x_mid + gy_mid x_hi."""
    gh, gm = R.split_bf16(gy.detach().cpu())
    xh, xm = R.split_bf16(x.detach().cpu())
    return dw64(gh, xh, taps) + dw64(gh, xm, taps) + dw64(gm, xh, taps)


def three_term_dx64(g, w):
    gh, gm = R.split_bf16(g.detach().cpu())
    wh, wm = R.split_bf16(w.detach().cpu())
    return dx64(gh, wh) + dx64(gh, wm) + dx64(gm, wh)


def mag_dw64(gy, x, taps):
    return dw64(gy.detach().abs(), x.detach().abs(), taps)


def mag_dx64(g, w):
    return dx64(g.detach().abs(), w.detach().abs())


# ------------------------------------------------------------------------------------------- the hand-written sums (the pins)
def dw_sum(gy, x, taps):
    gy, x = _d(gy), _d(x)
    H, W = gy.shape[2:]
    if taps == 1:
        return torch.einsum("nohw,nchw->oc", gy, x).view(gy.shape[1], x.shape[1], 1, 1)
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(gy.shape[1], x.shape[1], 3, 3, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            out[:, :, dy, dx] = torch.einsum("nohw,nchw->oc", gy, xp[:, :, dy:dy + H, dx:dx + W])
    return out


def dx_sum(g, w):
    g, w = _d(g), _d(w)
    if w.dim() == 2:
        return torch.einsum("oc,nohw->nchw", w, g)
    if w.shape[2] == 1:
        return torch.einsum("oc,nohw->nchw", w[:, :, 0, 0], g)
    H, W = g.shape[2:]
    gp = F.pad(g, (1, 1, 1, 1))
    out = torch.zeros(g.shape[0], w.shape[1], H, W, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):   # g at (y - dy + 1, x - dx + 1) = padded (y + 2 - dy, x + 2 - dx)
            out += torch.einsum("oc,nohw->nchw", w[:, :, dy, dx], gp[:, :, 2 - dy:2 - dy + H, 2 - dx:2 - dx + W])
    return out


def up_t_sum(g, size):
    g = _d(g)
    iy, ix = R.nearest_index(g.shape[2], size[0]), R.nearest_index(g.shape[3], size[1])
    rows = torch.zeros(g.shape[0], g.shape[1], size[0], g.shape[3], dtype=torch.float64).index_add_(2, iy, g)
    return torch.zeros(g.shape[0], g.shape[1], size[0], size[1], dtype=torch.float64).index_add_(3, ix, rows)


def preimage_size(hw, size):
    """(Ht,Wt) element counts of the pre-images of the gather (H,W) <- size."""
    return up_t_sum(torch.ones(1, 1, hw[0], hw[1]), size)[0, 0]


# ------------------------------------------------------------------------------------------- the module's chain
def _ulp(v):
    return v.abs() * 2.0 ** -23


def chain_grads64(stages, sd, r):
    """float64 autograd of sum(level0_64(stages, sd) * r): ({i: d stage i}, {key: d parameter})."""
    xs = [_d(s).requires_grad_(True) for s in stages]
    ps = {k: _d(v).requires_grad_(True) for k, v in sd.items() if k.startswith("lateral_convs.") or k.startswith("fpn_convs.0.")}
    out = R.level0_64(xs, ps)
    keys = sorted(ps)
    grads = torch.autograd.grad((out * _d(r)).sum(), xs + [ps[k] for k in keys])
    return list(grads[:len(xs)]), dict(zip(keys, grads[len(xs):]))


def l0_and_its_bound(stages, sd):
    """L0 in float64 and the per-element bound on the HIP forward's L0 (tests/test_gpu_fpn.py's chain test): each lateral's own
    CUT mag, summed down the pyramid through the exact gather, one float32 ulp per epilogue addition."""
    lat, e = None, None
    for i in range(len(stages) - 1, -1, -1):
        w, b = sd[f"lateral_convs.{i}.conv.weight"], sd[f"lateral_convs.{i}.conv.bias"]
        own = R.conv64(stages[i], w, b)
        ei = R.CUT * R.mag64(stages[i], w)
        if lat is None:
            lat, e = own, ei + _ulp(own)
        else:
            lat = own + R.gather_nearest(lat, own.shape[2:])
            e = ei + R.gather_nearest(e, own.shape[2:]) + _ulp(own) + _ulp(lat)
    return lat, e


def chain_bounds64(stages, sd, r):
    """Per-element bounds on the HIP backward of sum(out * r) against `chain_grads64`, propagated down the chain in float64:
        every product    its own CUT (mag + what the incoming bound adds to mag)
        gL0              CUT mag of conv3x3(|r|, |w3'|), one ulp for the epilogue's addition
        gL_i             the incoming bound pushed through up^T, plus n 2^-24 up^T(|gL_{i-1}|) for the n-term float32 sum
        dx_i             the incoming bound pushed through |W_i|^T, one ulp for the epilogue's addition
        dW_i, db_i       sum of the incoming bound times |x_i| (times 1); db: K 2^-24 sum|gL_i| for the float32 sum
        dW3              sum |r| e0 with the forward bound e0 on L0; db3: K 2^-24 sum|r|
    -> ({i: bound on d stage i}, {key: bound on d parameter})."""
    n = len(stages)
    r = _d(r)
    w3 = _d(sd["fpn_convs.0.conv.weight"])
    l0, e0 = l0_and_its_bound([_d(s) for s in stages], {k: _d(v) for k, v in sd.items()})
    K0 = r.shape[0] * r.shape[2] * r.shape[3]
    pb = {}
    cross = dw64(r.abs(), e0, 9)
    pb["fpn_convs.0.conv.weight"] = R.CUT * (mag_dw64(r, l0, 9) + cross) + cross
    pb["fpn_convs.0.conv.bias"] = K0 * 2.0 ** -24 * r.abs().sum((0, 2, 3))
    gl = dx64(r, w3)
    e = R.CUT * mag_dx64(r, w3) + _ulp(gl)
    xb = []
    for i in range(n):
        x, w = _d(stages[i]), _d(sd[f"lateral_convs.{i}.conv.weight"])
        if i > 0:
            size = x.shape[2:]
            npre = preimage_size(gl.shape[2:], size)
            e = up_t64(e, size) + npre * 2.0 ** -24 * up_t64(gl.abs(), size)
            gl = up_t64(gl, size)
        K = x.shape[0] * x.shape[2] * x.shape[3]
        through = dx64(e, w.abs())
        dxi = dx64(gl, w)
        xb.append(R.CUT * (mag_dx64(gl, w) + through) + through + _ulp(dxi))
        cross = dw64(e, x.abs(), 1)
        pb[f"lateral_convs.{i}.conv.weight"] = R.CUT * (mag_dw64(gl, x, 1) + cross) + cross
        pb[f"lateral_convs.{i}.conv.bias"] = e.sum((0, 2, 3)) + K * 2.0 ** -24 * (gl.abs() + e).sum((0, 2, 3))
    return xb, pb
