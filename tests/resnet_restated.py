"""float64 restatements of the bottleneck ResNet with frozen BatchNorm for the backbone tests (a helper, not collected).

mmdet and torchvision are not installed here, so the yardstick is the builder's reading of ResNet v1.5 (style='pytorch'), written out
in torch:

    stem(img)  = maxpool(3, stride 2, pad 1)( relu( bn1( conv 7x7, stride 2, pad 3 (img) ) ) )
    bottleneck(x; planes p, stride s, downsample?):
        a = relu(bn1(conv1x1(x)));  b = relu(bn2(conv3x3(a, stride s, pad 1)));  c = bn3(conv1x1(b))
        id = bn_d(conv1x1(x, stride s)) if downsample else x;  out = relu(c + id)
    bn(y) = y * scale + shift, scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale

Parameters travel as a state-dict with torchvision's keys under no prefix.  Everything runs wherever its tensors live: the
convolutions are one matrix product per tap (`conv64`), so the references can be made on the device.
"""
import torch
import torch.nn.functional as F
from torch import nn

from fpn_restated import ACC, CUT, split_bf16  # noqa: F401  (the project's bounds; re-exported for the tests)

EPS = 1e-5
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def out_size(h, s):
    return (h - 1) // s + 1


# ------------------------------------------------------------------------------------------------------------ parameters
def _conv_w(g, cout, cin, k, gain=1.0):
    return torch.randn(cout, cin, k, k, generator=g) * gain / (k * k * cin) ** 0.5


def _bn(g, sd, name, c):
    """Running statistics that are NOT the defaults: var in [0.5, 2], a nonzero mean."""
    sd[name + ".weight"] = 0.5 + torch.rand(c, generator=g)
    sd[name + ".bias"] = torch.randn(c, generator=g) * 0.1
    sd[name + ".running_mean"] = torch.randn(c, generator=g) * 0.2 + 0.05
    sd[name + ".running_var"] = 0.5 + 1.5 * torch.rand(c, generator=g)
    sd[name + ".num_batches_tracked"] = torch.tensor(7)


def make_block_params(sd, g, name, cin, p, downsample):
    sd[name + ".conv1.weight"] = _conv_w(g, p, cin, 1, 1.4)
    _bn(g, sd, name + ".bn1", p)
    sd[name + ".conv2.weight"] = _conv_w(g, p, p, 3, 1.4)
    _bn(g, sd, name + ".bn2", p)
    sd[name + ".conv3.weight"] = _conv_w(g, 4 * p, p, 1, 0.7)
    _bn(g, sd, name + ".bn3", 4 * p)
    if downsample:
        sd[name + ".downsample.0.weight"] = _conv_w(g, 4 * p, cin, 1)
        _bn(g, sd, name + ".downsample.1", 4 * p)


def make_params(planes, depths, seed, stem=64):
    """A seeded state-dict of a bottleneck ResNet: `planes[i]`, `depths[i]` per layer, the first block of each with a downsample."""
    g = torch.Generator().manual_seed(seed)
    sd = {"conv1.weight": _conv_w(g, stem, 3, 7, 1.4)}
    _bn(g, sd, "bn1", stem)
    c = stem
    for li, (p, d) in enumerate(zip(planes, depths)):
        for bi in range(d):
            make_block_params(sd, g, f"layer{li + 1}.{bi}", c, p, bi == 0)
            c = 4 * p
    return sd


class StandInBottleneck(nn.Module):
    def __init__(self, cin, p, stride, downsample):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, p, 1, bias=False), nn.BatchNorm2d(p)
        self.conv2, self.bn2 = nn.Conv2d(p, p, 3, stride=stride, padding=1, bias=False), nn.BatchNorm2d(p)
        self.conv3, self.bn3 = nn.Conv2d(p, 4 * p, 1, bias=False), nn.BatchNorm2d(4 * p)
        self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * p, 1, stride=stride, bias=False), nn.BatchNorm2d(4 * p)) if downsample else None

    def forward(self, x):
        a = torch.relu(self.bn1(self.conv1(x)))
        a = torch.relu(self.bn2(self.conv2(a)))
        c = self.bn3(self.conv3(a))
        return torch.relu(c + (x if self.downsample is None else self.downsample(x)))


class StandInResNet(nn.Module):
    """nn.Conv2d / nn.BatchNorm2d under torchvision's attribute names; forward(img) -> (c2, c3, c4, c5)."""

    def __init__(self, planes=(64, 128, 256, 512), depths=(3, 4, 6, 3), strides=(1, 2, 2, 2), stem=64):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(3, stem, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(stem)
        c = stem
        for li, (p, d, s) in enumerate(zip(planes, depths, strides)):
            blocks = [StandInBottleneck(c if bi == 0 else 4 * p, p, s if bi == 0 else 1, bi == 0) for bi in range(d)]
            setattr(self, f"layer{li + 1}", nn.Sequential(*blocks))
            c = 4 * p
        self.n_layers = len(planes)

    def forward(self, img):
        x = F.max_pool2d(torch.relu(self.bn1(self.conv1(img))), 3, 2, 1)
        outs = []
        for li in range(self.n_layers):
            x = getattr(self, f"layer{li + 1}")(x)
            outs.append(x)
        return tuple(outs)


def stand_in(planes, depths, seed, strides=(1, 2, 2, 2), stem=64):
    """(the module in eval mode with the seeded parameters, its state-dict)."""
    sd = make_params(planes, depths, seed, stem)
    net = StandInResNet(planes, depths, strides[:len(planes)], stem)
    net.load_state_dict(sd)
    return net.eval(), sd


# ------------------------------------------------------------------------------------------------------------ float64
def conv64(x, w, stride=1, padding=0):
    """F.conv2d(x, w, None, stride, padding) in float64 as one matrix product per tap (a device's float64 convolution may not exist;
    its float64 matrix product does)."""
    x, w = x.double(), w.double()
    k = w.shape[2]
    if padding:
        x = F.pad(x, (padding,) * 4)
    h, wd = (x.shape[2] - k) // stride + 1, (x.shape[3] - k) // stride + 1
    out = torch.zeros((x.shape[0], w.shape[0], h, wd), dtype=torch.float64, device=x.device)
    for dy in range(k):
        for dx in range(k):
            out += torch.einsum("oc,nchw->nohw", w[:, :, dy, dx],
                                x[:, :, dy:dy + stride * (h - 1) + 1:stride, dx:dx + stride * (wd - 1) + 1:stride])
    return out


def unfold_matrix(wmat, cout, k):
    """The folded (ceil128(Cout), k k Cin) tap-major matrix back as a (Cout,Cin,k,k) weight (the zero rows dropped)."""
    return wmat[:cout].reshape(cout, k, k, -1).permute(0, 3, 1, 2)


def three_term_conv64(x, wfold, stride=1, padding=0):
    """float64 convolution of the pieces the kernels multiply, `wfold` = the FOLDED fp32 weight (Cout,Cin,k,k):
    x_hi w_hi + x_hi w_mid + x_mid w_hi (every product exact in float64)."""
    xh, xm = split_bf16(x)
    wh, wm = split_bf16(wfold)
    return conv64(xh, wh, stride, padding) + conv64(xh, wm, stride, padding) + conv64(xm, wh, stride, padding)


def mag64(x, wfold, shift, residual=None, stride=1, padding=0):
    """conv(|x|, |w'|) + |shift| + |residual| per element in float64: the size of everything the kernel sums."""
    m = conv64(x.abs(), wfold.abs(), stride, padding) + shift.double().abs().view(1, -1, 1, 1)
    return m if residual is None else m + residual.double().abs()


def affine64(sd, name, eps=EPS):
    w, b, mean, var = (sd[f"{name}.{k}"].double() for k in BN_KEYS)
    scale = w / torch.sqrt(var + eps)
    return scale, b - mean * scale


def _layer(x, bx, sd, conv, bn, stride, padding, residual=None, bres=None, relu=True):
    """One layer in float64 and, where bx (the bound on the kernel's input error) is given, the bound on its output error:
    conv(bx, |w'|) + CUT * mag [+ bres], mag taken at |x| + bx (and |residual| + bres): what the kernel really summed."""
    scale, shift = affine64(sd, bn)
    wf = sd[conv + ".weight"].double() * scale.view(-1, 1, 1, 1)
    y = conv64(x, wf, stride, padding) + shift.view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual
    bound = None
    if bx is not None:
        mag = conv64(x.abs() + bx, wf.abs(), stride, padding) + shift.abs().view(1, -1, 1, 1)
        bound = conv64(bx, wf.abs(), stride, padding)
        if residual is not None:
            mag = mag + residual.abs() + bres
            bound = bound + bres
        bound = bound + CUT * mag
    return (torch.relu(y) if relu else y), bound         # the bound passes through ReLU unchanged (1-Lipschitz)


def _block(x, bx, sd, name, stride):
    down = name + ".downsample.0.weight" in sd
    identity, bid = x.double(), bx
    if down:
        identity, bid = _layer(x, bx, sd, name + ".downsample.0", name + ".downsample.1", stride, 0, relu=False)
    a, ba = _layer(x, bx, sd, name + ".conv1", name + ".bn1", 1, 0)
    a, ba = _layer(a, ba, sd, name + ".conv2", name + ".bn2", stride, 1)
    return _layer(a, ba, sd, name + ".conv3", name + ".bn3", 1, 0, residual=identity, bres=bid)


def bottleneck64(x, sd, name, stride):
    return _block(x, None, sd, name, stride)[0]


def bottleneck_bounds64(x, sd, name, stride, bx=None):
    """(out, bound) of one block whose input the kernel has to within bx (None: exactly)."""
    return _block(x, torch.zeros_like(x, dtype=torch.float64) if bx is None else bx, sd, name, stride)


def _depths(sd):
    depths = []
    while f"layer{len(depths) + 1}.0.conv1.weight" in sd:
        li, d = len(depths) + 1, 0
        while f"layer{li}.{d}.conv1.weight" in sd:
            d += 1
        depths.append(d)
    return depths


def stem64(img, sd, want_bound=False):
    """The stem in float64; its bound: CUT * mag of the 7x7 (a float32 convolution of 147 products errs by far less), carried
    through ReLU unchanged and through the max-pool as the window's largest bound."""
    scale, shift = affine64(sd, "bn1")
    wf = sd["conv1.weight"].double() * scale.view(-1, 1, 1, 1)
    y = torch.relu(conv64(img, wf, 2, 3) + shift.view(1, -1, 1, 1))
    s = F.max_pool2d(y, 3, 2, 1)
    if not want_bound:
        return s
    mag = conv64(img.abs(), wf.abs(), 2, 3) + shift.abs().view(1, -1, 1, 1)
    return s, F.max_pool2d(CUT * mag, 3, 2, 1)


def _stages(s, bs, sd, strides):
    outs = []
    for li, d in enumerate(_depths(sd)):
        for bi in range(d):
            s, bs = _block(s, bs, sd, f"layer{li + 1}.{bi}", strides[li] if bi == 0 else 1)
        outs.append((s, bs))
    return outs


def stages64(img, sd, strides=(1, 2, 2, 2), from_stem=False):
    """(c2, c3, c4, c5) in float64 from the image, or from the stem's map."""
    return tuple(o for o, _ in _stages(img.double() if from_stem else stem64(img, sd), None, sd, strides))


def chain_bounds64(img, sd, strides=(1, 2, 2, 2), from_stem=False):
    """[(c_i in float64, the propagated bound on the HIP route's error in it)]: per layer B_out = conv(B_in, |w'|) + CUT * mag,
    plus B_residual at the sum, unchanged through ReLU."""
    if from_stem:
        s, bs = img.double(), torch.zeros_like(img, dtype=torch.float64)
    else:
        s, bs = stem64(img, sd, want_bound=True)
    return _stages(s, bs, sd, strides)
