"""float64 restatements of the 2-D feature pyramid for the FPN tests (a helper, not collected).

mmdet is not installed here, so the yardstick is the builder's reading of mmdet.models.necks.FPN in the shipped configuration
(in_channels=[256,512,1024,2048], out_channels=256, num_outs=4, start_level=0, no add_extra_convs, no norm, no activation,
upsample_cfg=dict(mode='nearest')), written out in torch:

    laterals[i] = lat_i(inputs[i])                                              1x1 convolution with bias
    for i = top .. 1: laterals[i-1] += F.interpolate(laterals[i], size=laterals[i-1].shape[2:], mode='nearest')
    outs[i] = fpn_conv_i(laterals[i])                                           3x3 convolution, padding 1, with bias
"""
import torch
import torch.nn.functional as F


def make_params(channels, cout, seed, scale=1.0):
    """Random weights with mmdet's state-dict keys (under no prefix): lateral_convs.{i}.conv.*, fpn_convs.{i}.conv.*."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, c in enumerate(channels):
        sd[f"lateral_convs.{i}.conv.weight"] = torch.randn(cout, c, 1, 1, generator=g) * scale / c ** 0.5
        sd[f"lateral_convs.{i}.conv.bias"] = torch.randn(cout, generator=g) * 0.1
        sd[f"fpn_convs.{i}.conv.weight"] = torch.randn(cout, cout, 3, 3, generator=g) * scale / (9 * cout) ** 0.5
        sd[f"fpn_convs.{i}.conv.bias"] = torch.randn(cout, generator=g) * 0.1
    return sd


def make_stages(n, channels, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, c, h, w, generator=g) for c, (h, w) in zip(channels, sizes)]


def nearest_index(out_size, in_size):
    """ATen's source index of mode='nearest' by size, in float32: min((int)floorf(dst * ((float)in / (float)out)), in - 1)."""
    scale = torch.tensor(float(in_size), dtype=torch.float32) / torch.tensor(float(out_size), dtype=torch.float32)
    dst = torch.arange(out_size, dtype=torch.float32)
    return torch.clamp(torch.floor(dst * scale).to(torch.int64), max=in_size - 1)


def nearest_index_integer(out_size, in_size):
    """The integer form dst * in / out, which is NOT what ATen computes."""
    return (torch.arange(out_size, dtype=torch.int64) * in_size) // out_size


def gather_nearest(top, size):
    """top (N,C,Ht,Wt) -> (N,C,H,W) through `nearest_index` (exact: a gather)."""
    iy, ix = nearest_index(size[0], top.shape[2]), nearest_index(size[1], top.shape[3])
    return top[:, :, iy][:, :, :, ix]


def fpn_full64(stages, sd):
    """The stock module's four outputs in float64."""
    n = len(stages)
    lat = [F.conv2d(s.double(), sd[f"lateral_convs.{i}.conv.weight"].double(), sd[f"lateral_convs.{i}.conv.bias"].double())
           for i, s in enumerate(stages)]
    for i in range(n - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
    return [F.conv2d(lat[i], sd[f"fpn_convs.{i}.conv.weight"].double(), sd[f"fpn_convs.{i}.conv.bias"].double(), padding=1)
            for i in range(n)]


def level0_64(stages, sd, want_laterals=False):
    """Level 0 only, in float64: the chain L3 -> L2 -> L1 -> L0 -> conv3x3, the gather through `gather_nearest`."""
    top = None
    for i in range(len(stages) - 1, -1, -1):
        lat = F.conv2d(stages[i].double(), sd[f"lateral_convs.{i}.conv.weight"].double(), sd[f"lateral_convs.{i}.conv.bias"].double())
        top = lat if top is None else lat + gather_nearest(top, lat.shape[2:])
    out = F.conv2d(top, sd["fpn_convs.0.conv.weight"].double(), sd["fpn_convs.0.conv.bias"].double(), padding=1)
    return (out, top) if want_laterals else out


def split_bf16(t):
    """fp32 -> (hi, mid) bfloat16 pieces: hi = bf16(t), mid = bf16(t - hi), both round-to-nearest-even; t - hi is exact."""
    hi = t.to(torch.bfloat16)
    mid = (t - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, mid


def conv64(x, w, bias=None, padding=0):
    """F.conv2d(x, w, bias, padding=padding) in float64, written as one matrix product per tap so that it runs wherever the tensors
    live (a device's float64 convolution may not exist; its float64 matrix product does)."""
    x, w = x.double(), w.double()
    k = w.shape[2]
    if padding:
        x = F.pad(x, (padding,) * 4)
    h, wd = x.shape[2] - k + 1, x.shape[3] - k + 1
    out = torch.zeros((x.shape[0], w.shape[0], h, wd), dtype=torch.float64, device=x.device)
    for dy in range(k):
        for dx in range(k):
            out += torch.einsum("oc,nchw->nohw", w[:, :, dy, dx], x[:, :, dy:dy + h, dx:dx + wd])
    return out if bias is None else out + bias.double().view(1, -1, 1, 1)


def three_term_conv64(x, w, **kw):
    """float64 convolution of the pieces the kernels multiply: x_hi w_hi + x_hi w_mid + x_mid w_hi (every product exact in float64)."""
    xh, xm = split_bf16(x)
    wh, wm = split_bf16(w)
    return conv64(xh, wh, **kw) + conv64(xh, wm, **kw) + conv64(xm, wh, **kw)


def mag64(x, w, **kw):
    """conv(|x|, |w|) per element in float64: the size of the summed products."""
    return conv64(x.abs(), w.abs(), **kw)


ACC = 4e-7              # fp32 accumulation of exact products, relative to mag (tests/test_gpu_bf16.py)
CUT = 3 * 2.0 ** -16    # the dropped terms, worst case, relative to mag


class StandInConv:
    def __init__(self, weight, bias):
        self.conv = torch.nn.Conv2d(weight.shape[1], weight.shape[0], weight.shape[2], padding=weight.shape[2] // 2)
        with torch.no_grad():
            self.conv.weight.copy_(weight)
            self.conv.bias.copy_(bias)


class StandInFPN:
    """An object with mmdet's attribute layout: lateral_convs[i].conv, fpn_convs[i].conv."""

    def __init__(self, sd, n_levels):
        self.lateral_convs = [StandInConv(sd[f"lateral_convs.{i}.conv.weight"], sd[f"lateral_convs.{i}.conv.bias"]) for i in range(n_levels)]
        self.fpn_convs = [StandInConv(sd[f"fpn_convs.{i}.conv.weight"], sd[f"fpn_convs.{i}.conv.bias"]) for i in range(n_levels)]
