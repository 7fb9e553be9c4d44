"""float64 restatement of one bottleneck's backward and of a net's, for the ResNet gradient tests (a helper, not collected).

With W' = scale (.) W (the fp32 values the kernels split), g = dL/dout and the SAVED activations a, b, out given as inputs:

    gz  = gate(g, out)                        gate(v, y) = where(y <= 0, 0, v): torch.relu's gradient rule on the saved output
    dW3 = scale3 (.) (gz b^T)                 gb = gate(W3'^T gz, b)
    dW2 = scale2 (.) dw3x3_s(gb, a)           ga = gate(convT3x3_s(gb; W2'), a)
    dW1 = scale1 (.) (ga x^T)                 dx = W1'^T ga + ( gz | spread_s(Wd'^T gz) )
    dWd = scaled (.) (gz x[.., s y, s x]^T)

The gates are inputs: imposing the HIP forward's own activations removes ReLU flips from the comparison, so no case is ever excluded.
`conv_dx64` / `conv_dw64` are the two sums written per tap with strided slices; tests/test_resnet_grad_host.py pins them against scalar
loops and the whole chain against torch's float64 autograd.  Everything runs wherever its tensors live.

Bounds, in the manner of fpn_grad_restated.chain_bounds64, per element with mag = the same sum over absolute values:
    every product   CUT (mag + what the incoming bound adds to mag), plus the incoming bound pushed through |W'| (or times |activation|)
    an epilogue's addition, autograd's sum of two gradients, the rows' scale: one float32 ulp each
    a gate          passes the bound where it passes the value, zero elsewhere
"""
import torch
import torch.nn.functional as F

from fpn_restated import ACC, CUT, split_bf16  # noqa: F401

EPS = 1e-5


def out_size(h, s):
    return (h - 1) // s + 1


def gate64(v, y):
    """torch.relu's gradient rule on the saved output y: 0 where y <= 0 (0.0, -0.0, negatives), v elsewhere (positives, inf, NaN)."""
    return torch.where(y <= 0, torch.zeros_like(v), v)


def conv_dx64(g, w, stride, size):
    """Input gradient of F.conv2d(x, w, None, stride, k // 2) at an input of `size` for the output gradient g, float64:
    dx[n,c,s yo+dy-p,s xo+dx-p] += w[o,c,dy,dx] g[n,o,yo,xo]."""
    g, w = g.double(), w.double()
    k, p = w.shape[2], w.shape[2] // 2
    H, W = size
    ho, wo = g.shape[2:]
    buf = torch.zeros(g.shape[0], w.shape[1], H + 2 * p + stride, W + 2 * p + stride, dtype=torch.float64, device=g.device)
    for dy in range(k):
        for dx in range(k):
            buf[:, :, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride] += torch.einsum("oc,nohw->nchw", w[:, :, dy, dx], g)
    return buf[:, :, p:p + H, p:p + W]


def conv_dw64(gy, x, k, stride):
    """Weight gradient of F.conv2d(x, w, None, stride, k // 2) for the output gradient gy, float64:
    dW[o,c,dy,dx] = sum gy[n,o,yo,xo] x[n,c,s yo+dy-p,s xo+dx-p], zero outside."""
    gy, x = gy.double(), x.double()
    p = k // 2
    ho, wo = gy.shape[2:]
    xp = F.pad(x, (p, p + stride, p, p + stride))
    out = torch.zeros(gy.shape[1], x.shape[1], k, k, dtype=torch.float64, device=gy.device)
    for dy in range(k):
        for dx in range(k):
            out[:, :, dy, dx] = torch.einsum("nohw,nchw->oc", gy, xp[:, :, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride])
    return out


def three_term_dx64(g, w, stride, size):
    """The three products the input-gradient kernels multiply, summed in float64."""
    gh, gm = split_bf16(g)
    wh, wm = split_bf16(w)
    return conv_dx64(gh, wh, stride, size) + conv_dx64(gh, wm, stride, size) + conv_dx64(gm, wh, stride, size)


def three_term_dw64(gy, x, k, stride):
    gh, gm = split_bf16(gy)
    xh, xm = split_bf16(x)
    return conv_dw64(gh, xh, k, stride) + conv_dw64(gh, xm, k, stride) + conv_dw64(gm, xh, k, stride)


def spread64(t, stride, size):
    """(yo, xo) -> (s yo, s xo) of a zero map of `size`."""
    if stride == 1:
        return t
    out = torch.zeros(t.shape[0], t.shape[1], size[0], size[1], dtype=t.dtype, device=t.device)
    out[:, :, ::stride, ::stride] = t
    return out


# ------------------------------------------------------------------------------------------- scalar loops (the pins)
def convT3x3_s2_loops(gb, w, H, W):
    """The stride-2 transposed 3x3 by its parity rule, scalar loops: input pixel (y, x) takes the taps with y + 1 - dy and x + 1 - dx even
    and the output pixel in range."""
    gb, w = gb.double(), w.double()
    N, O, Ho, Wo = gb.shape
    C = w.shape[1]
    out = torch.zeros(N, C, H, W, dtype=torch.float64)
    taps = torch.zeros(H, W, dtype=torch.int64)
    for y in range(H):
        for x in range(W):
            for dy in range(3):
                for dx in range(3):
                    if (y + 1 - dy) % 2 or (x + 1 - dx) % 2:
                        continue
                    yo, xo = (y + 1 - dy) // 2, (x + 1 - dx) // 2
                    if 0 <= yo < Ho and 0 <= xo < Wo:
                        taps[y, x] += 1
                        out[:, :, y, x] += gb[:, :, yo, xo] @ w[:, :, dy, dx]
    return out, taps


def dw_s2_loops(gy, x, k):
    gy, x = gy.double(), x.double()
    N, O, Ho, Wo = gy.shape
    C, H, W = x.shape[1:]
    p = k // 2
    out = torch.zeros(O, C, k, k, dtype=torch.float64)
    for dy in range(k):
        for dx in range(k):
            for yo in range(Ho):
                for xo in range(Wo):
                    y, xx = 2 * yo + dy - p, 2 * xo + dx - p
                    if 0 <= y < H and 0 <= xx < W:
                        out[:, :, dy, dx] += gy[:, :, yo, xo].t() @ x[:, :, y, xx]
    return out


# ------------------------------------------------------------------------------------------- one bottleneck
def _ulp(v):
    return v.abs() * 2.0 ** -23


def scale32(sd, name, eps=EPS):
    """The BatchNorm's scale in float32, the module's own expression: weight / sqrt(running_var + eps)."""
    return sd[name + ".weight"].float() / torch.sqrt(sd[name + ".running_var"].float() + eps)


def folded(sd, conv, bn):
    """(W' as the fp32 product the kernels split, in float64; scale in float64)."""
    s = scale32(sd, bn)
    return (sd[conv + ".weight"].float() * s.view(-1, 1, 1, 1)).double(), s.double()


def block_backward64(x, a, b, out, g, sd, name, stride, eg=None):
    """One block's backward in float64 with its bounds.  x, a, b, out = the SAVED activations (values and gates), g = dL/dout, eg = the
    bound on the kernel's g (None: exact) -> (grads, bounds), dicts with "x", "conv1", "conv2", "conv3" and, with the branch,
    "downsample"."""
    x, a, b, out, g = (t.double() for t in (x, a, b, out, g))
    eg = torch.zeros_like(g) if eg is None else eg
    down = name + ".downsample.0.weight" in sd
    w1, s1 = folded(sd, name + ".conv1", name + ".bn1")
    w2, s2 = folded(sd, name + ".conv2", name + ".bn2")
    w3, s3 = folded(sd, name + ".conv3", name + ".bn3")
    grads, bounds = {}, {}

    def dw(key, gy, ey, act, k, s, scale):
        raw = conv_dw64(gy, act, k, s)
        cross = conv_dw64(ey, act.abs(), k, s)
        eraw = CUT * (conv_dw64(gy.abs(), act.abs(), k, s) + cross) + cross
        sc = scale.view(-1, 1, 1, 1)
        grads[key] = sc * raw
        bounds[key] = sc.abs() * eraw + _ulp(sc * raw) + 2.0 ** -23 * sc.abs() * eraw

    def dx(gy, ey, w, s, size):
        through = conv_dx64(ey, w.abs(), s, size)
        val = conv_dx64(gy, w, s, size)
        return val, CUT * (conv_dx64(gy.abs(), w.abs(), s, size) + through) + through

    gz, ez = gate64(g, out), gate64(eg, out)
    dw("conv3", gz, ez, b, 1, 1, s3)
    gb, eb = dx(gz, ez, w3, 1, b.shape[2:])
    gb, eb = gate64(gb, b), gate64(eb, b)
    dw("conv2", gb, eb, a, 3, stride, s2)
    ga, ea = dx(gb, eb, w2, stride, a.shape[2:])
    ga, ea = gate64(ga, a), gate64(ea, a)
    dw("conv1", ga, ea, x, 1, 1, s1)
    main, emain = dx(ga, ea, w1, 1, x.shape[2:])
    if down:
        wd, sdn = folded(sd, name + ".downsample.0", name + ".downsample.1")
        dw("downsample", gz, ez, x, 1, stride, sdn)
        res, eres = dx(gz, ez, wd, 1, gz.shape[2:])
        res, eres = spread64(res, stride, x.shape[2:]), spread64(eres, stride, x.shape[2:])
    else:
        res, eres = gz, ez
    grads["x"] = main + res
    bounds["x"] = emain + eres + _ulp(main + res) + 2.0 ** -23 * (emain + eres)
    return grads, bounds


def net_backward64(blocks, Rs, sd):
    """The backward of sum_k (C_k . R_k) through a list of blocks, last block first.  blocks = [(name, stride, x, a, b, out, k or
    None)], k = the index of the stage C_k this block's output is (None: an inner block); Rs = the R_k -> ({name: grads}, {name: bounds})
    of `block_backward64`, the gradient arriving at a block being autograd's float32 sum of R_k and the next block's dx."""
    g = eg = None
    all_g, all_b = {}, {}
    for name, stride, x, a, b, out, k in reversed(blocks):
        if k is not None:
            r = Rs[k].double()
            if g is None:
                g, eg = r, torch.zeros_like(r)
            else:
                g, eg = g + r, eg + _ulp(g + r)
        grads, bounds = block_backward64(x, a, b, out, g, sd, name, stride, eg)
        all_g[name], all_b[name] = grads, bounds
        g, eg = grads["x"], bounds["x"]
    return all_g, all_b
