"""The 2-D backbone's kernels (csrc/fpn.hip, fpn_bwd.hip, resnet.hip, resnet_bwd.hip) where their first tests did not reach:

A. the four weight-gradient kernels in their steady state: runs of four and more tiles per block that cross from one view into the next,
   a ragged last run, and the workload's own run length (38 tiles);
B. ResNet-50's own widths, every kernel alone against the two tight bounds: two to sixteen row blocks, reductions up to 2304 terms;
C. the value range, which is fp32's: an exact power-of-two scaling far outside fp16's range commutes bit for bit, the largest value two
   bf16 pieces hold comes out as itself, fp32 subnormals come out finite;
D. non-finite inputs: NaN, +inf and the finite 0x7f7f8000 (which rounds to an infinite hi piece) turn exactly the receptive field of the
   planted element into NaN and leave every other bit as it was; in the weight gradients they stay in their row or column.

The bounds are the project's (tests/fpn_restated.py), per element with mag = the same sum over absolute values in float64:
    |kernel - three-term restatement| <= ACC mag = 4e-7 mag      asserted: every reduction here has at most 2304 terms
    |kernel - float64|                <= CUT mag = 3 2^-16 mag   the dropped terms, worst case
Integer-valued operands that fit one bf16 piece with sums below 2^24 are compared bit for bit.  The float64 references are the
restatement modules' sums (`resnet_grad_restated.conv_dw64` / `conv_dx64`, `resnet_restated.conv64`; stride 1 is the FPN's operation),
computed once per case on the device.

Worst |error| / bound measured on MI355X: see DESIGN 4.21 - 4.23 (the rows "long runs" and "ResNet-50 widths")."""
import math

import pytest
import torch
import torch.nn.functional as F

import fpn_restated as FR
import resnet_grad_restated as G
import resnet_restated as R

pytestmark = pytest.mark.gpu

ACC_TERMS = 2304                    # the longest reduction ACC is asserted at
DW_TILE = (2, 16)                   # output pixels of a weight-gradient tile, both strides (ops.fpn.DW_TILE, ops.resnet.DW_S2_TILE)
TILE3 = {1: (8, 16), 2: (4, 16)}    # output pixels of the 3x3 kernels' tile per stride
WORST = {}                          # section -> worst |error| / bound of the random cases, printed with every line


def _within(section, name, got, want, bound):
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[section] = max(WORST.get(section, 0.0), ratio)
    print(f"[{section}] {name}: max |error| / bound = {ratio:.3e}, max |error| = {float(err.max()):.3e}; worst of [{section}] so far {WORST[section]:.3e}")
    assert bool((err <= bound).all()), f"{name}: max |error| / bound = {ratio}"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rand(shape, seed, gpu):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(gpu)


def _ints(lo, hi, shape, seed, gpu):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float().to(gpu)


def _f32(bits, gpu=None):
    """The float32 with this bit pattern."""
    t = torch.tensor([bits if bits < 1 << 31 else bits - (1 << 32)], dtype=torch.int32).view(torch.float32)[0]
    return t if gpu is None else t.to(gpu)


# ======================================================================== A. weight gradients in long runs across views
# kernel, taps, (N, C, Cout, H, W) of x, (tiles, tiles per split, splits), terms of the reduction
RUNS = [("fpn", 9, (3, 512, 512, 6, 40), (27, 4, 7), 720),
        ("fpn", 1, (3, 512, 512, 10, 35), (33, 5, 7), 1050),
        ("s2", 1, (3, 512, 512, 10, 70), (27, 4, 7), 525),
        ("s2", 9, (3, 512, 512, 10, 70), (27, 4, 7), 525),
        ("s2", 1, (3, 512, 512, 11, 69), (27, 4, 7), 630),
        ("s2", 9, (3, 512, 512, 11, 69), (27, 4, 7), 630)]
# two views of a whole 60 x 80 OUTPUT map at the workload's own run length
LONG = [("fpn", 9, (2, 512, 512, 60, 80)), ("fpn", 1, (2, 512, 512, 60, 80)), ("s2", 1, (2, 512, 512, 120, 160)),
        ("s2", 9, (2, 512, 512, 120, 160))]
LONG_PLAN, LONG_TERMS = (300, 38, 8), 9600
GY_MAX, X_MAX = 4, 3                # the integer operands: exact in one bf16 piece


def _run_id(c):
    return f"{c[0]}-{c[1]}tap-{'x'.join(str(v) for v in c[2])}"


def _stride(kernel):
    return 2 if kernel == "s2" else 1


def _gy_shape(kernel, shape):
    N, C, cout, H, W = shape
    s = _stride(kernel)
    return (N, cout, G.out_size(H, s), G.out_size(W, s))


def _plan(kernel, taps, shape):
    from mvsdet_amd import ops
    return (ops.resnet if kernel == "s2" else ops.fpn).weight_grad_plan(taps, *shape)


def _c_splits(kernel, taps, shape):
    from mvsdet_amd import _lib
    lib = _lib.load()
    return (lib.mvsdet_resnet_dw_s2_splits if kernel == "s2" else lib.mvsdet_fpn_dw_splits)(taps, *shape)


def _crossing_runs(plan, views):
    """The runs [s per, s per + per) whose first and last tile lie in different views (the tiles are view-major)."""
    tiles, per, splits = plan
    tpv = tiles // views
    return [s for s in range(splits) if (s * per) // tpv != (min(s * per + per, tiles) - 1) // tpv]


def _check_plan(kernel, taps, shape, plan, terms, min_run):
    """What keeps a case what its name says; pure arithmetic and the C query, no device."""
    assert DW_TILE == (2, 16)
    assert _plan(kernel, taps, shape) == plan
    assert _c_splits(kernel, taps, shape) == plan[2]
    tiles, per, splits = plan
    assert tiles % shape[0] == 0 and per >= min_run and splits > 1
    assert _crossing_runs(plan, shape[0]), "no run crosses a view boundary"
    gy = _gy_shape(kernel, shape)
    assert gy[0] * gy[2] * gy[3] == terms
    assert GY_MAX * X_MAX * terms < 2 ** 24                   # every partial sum of the integer operands is exact in fp32


def test_plans_and_constants():
    """No device: the plan tuples (the Python restatement and the C query), the run-crossing condition, a ragged last run, the integer
    sums' ceilings, the asserted three-term bound's reach, and the largest value two bf16 pieces hold."""
    from mvsdet_amd import ops
    assert ops.fpn.DW_TILE == DW_TILE and ops.resnet.DW_S2_TILE == DW_TILE
    assert ops.resnet.CONV3X3_TILE == TILE3[1] and ops.resnet.CONV3X3_S2_TILE == TILE3[2]
    for kernel, taps, shape, plan, terms in RUNS:
        _check_plan(kernel, taps, shape, plan, terms, min_run=4)
        assert plan[0] % plan[1] != 0 and terms <= ACC_TERMS   # the last run is ragged; ACC is asserted
        assert GY_MAX * X_MAX * terms <= 12 * 1050
    for kernel, taps, shape in LONG:
        _check_plan(kernel, taps, shape, LONG_PLAN, LONG_TERMS, min_run=8)
        assert _gy_shape(kernel, shape)[2:] == (60, 80) and GY_MAX * X_MAX * LONG_TERMS == 115200
    assert _bits(TWO_PIECE_MAX.view(1)).item() == 0x7f7f7f80
    hi, mid = ops.split_bf16(TWO_PIECE_MAX)
    assert bool(torch.isfinite(hi.float())) and hi.double() + mid.double() == TWO_PIECE_MAX.double()
    nxt = (_bits(TWO_PIECE_MAX.view(1)) + 1).view(torch.float32)[0]          # one ulp more no longer fits
    h2, m2 = ops.split_bf16(nxt)
    assert h2.double() + m2.double() != nxt.double()
    h3, _ = ops.split_bf16(_f32(0x7f7f8000))
    assert bool(torch.isinf(h3.float()))                                      # the tie rounds to even: an infinite hi


def _dw(kernel, gy, x, taps):
    from mvsdet_amd import ops
    return ops.fpn.weight_grad(gy, x, taps) if kernel == "fpn" else ops.resnet.weight_grad(gy, x, taps, 2)


def _check_dw(section, name, got, gy, x, taps, stride):
    k = 3 if taps == 9 else 1
    mag = G.conv_dw64(gy.abs(), x.abs(), k, stride)
    assert gy.shape[0] * gy.shape[2] * gy.shape[3] <= ACC_TERMS
    _within(section + " three-term", name, got, G.three_term_dw64(gy, x, k, stride), FR.ACC * mag)
    _within(section + " float64", name, got, G.conv_dw64(gy, x, k, stride), FR.CUT * mag)


@pytest.mark.parametrize("case", RUNS, ids=_run_id)
def test_weight_grad_runs_across_views(gpu, case):
    """Runs of four (five) tiles, at least one of which starts in one view and ends in the next, and a ragged last run.  Integer operands
    are bit-exact against float64 -- a tile dropped, doubled or taken from the wrong view is a whole integer -- also with the views in
    another order; random operands hold both bounds, with the views permuted too, and give the same bits on a second call."""
    kernel, taps, shape, plan, terms = case
    _check_plan(kernel, taps, shape, plan, terms, min_run=4)
    N, C, cout, H, W = shape
    stride, k = _stride(kernel), 3 if taps == 9 else 1
    gshape, xshape = _gy_shape(kernel, shape), (N, C, H, W)
    perm = torch.tensor([2, 0, 1], device=gpu)
    section = f"A {'fpn' if kernel == 'fpn' else 'resnet s2'} dw{taps}"
    # 1. integers
    gyi, xi = _ints(-GY_MAX, GY_MAX, gshape, 11 + H + taps, gpu), _ints(-X_MAX, X_MAX, xshape, 12 + W + taps, gpu)
    got = _dw(kernel, gyi, xi, taps)
    want = G.conv_dw64(gyi, xi, k, stride)
    assert got.shape == (cout, C, k, k) and float(want.abs().max()) > 0
    assert torch.equal(got.double(), want)
    assert _same_bits(_dw(kernel, gyi[perm].contiguous(), xi[perm].contiguous(), taps), got)      # 4. the views in another order
    # 2. random operands, 3. the same bits again, 4. permuted: within both bounds (the order of the sum moves with the views)
    gy, x = _rand(gshape, 13 + H + taps, gpu), _rand(xshape, 14 + W + taps, gpu)
    got = _dw(kernel, gy, x, taps)
    _check_dw(section, _run_id(case), got, gy, x, taps, stride)
    assert _same_bits(_dw(kernel, gy, x, taps), got)
    _check_dw(section, _run_id(case) + " views permuted", _dw(kernel, gy[perm].contiguous(), x[perm].contiguous(), taps), gy, x, taps, stride)


@pytest.mark.parametrize("case", LONG, ids=_run_id)
def test_weight_grad_at_the_workloads_run_length(gpu, case):
    """Two views of a whole 60 x 80 output map at C = Cout = 512 (the size used: nothing was halved): 300 tiles in 8 runs of 38, a run
    that crosses into the second view, 9600 terms, |sum| <= 115200: integer operands bit-exact against float64."""
    kernel, taps, shape = case
    _check_plan(kernel, taps, shape, LONG_PLAN, LONG_TERMS, min_run=8)
    N, C, cout, H, W = shape
    k = 3 if taps == 9 else 1
    gyi, xi = _ints(-GY_MAX, GY_MAX, _gy_shape(kernel, shape), 21 + taps, gpu), _ints(-X_MAX, X_MAX, (N, C, H, W), 22 + taps, gpu)
    got = _dw(kernel, gyi, xi, taps)
    want = G.conv_dw64(gyi, xi, k, _stride(kernel))
    assert float(want.abs().max()) > 1000 and float(want.abs().max()) <= 115200
    assert torch.equal(got.double(), want)


# ======================================================================== B. ResNet-50's own widths, each kernel alone
def _folded_case(N, cin, cout, H, W, k, seed, gpu):
    """x, the split of the folded matrix, the folded weight (Cout,Cin,k,k), shift."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=g).to(gpu)
    w = (torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5).to(gpu)
    scale = (0.5 + torch.rand(cout, generator=g)).to(gpu)
    shift = (torch.randn(cout, generator=g) * 0.1).to(gpu)
    wmat = ops.resnet.fold(w, scale)
    return x, ops.gemm_split_weight(wmat), R.unfold_matrix(wmat, cout, k), shift


def _maps(stride):
    th, tw = TILE3[stride]
    return [(5, 7), (stride * th + 1, stride * tw + 1)]       # ... and one pixel more than a tile on each axis


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout", [(256, 256), (128, 512)])
def test_conv3x3_row_blocks(gpu, stride, cin, cout):
    """Two and four row blocks, K = 2304 and 1152, both bounds."""
    from mvsdet_amd import ops
    for H, W in _maps(stride):
        x, wq, wf, shift = _folded_case(2, cin, cout, H, W, 3, 4000 + cin + H + stride, gpu)
        assert 9 * cin <= ACC_TERMS
        mag = R.mag64(x, wf, shift, None, stride, 1)
        add = shift.double().view(1, -1, 1, 1)
        three, base = R.three_term_conv64(x, wf, stride, 1) + add, R.conv64(x, wf, stride, 1) + add
        for relu in (True, False):
            got = ops.resnet.conv3x3(x, wq, shift, cout, stride=stride, relu=relu)
            assert got.shape == (2, cout, R.out_size(H, stride), R.out_size(W, stride))
            act = torch.relu if relu else (lambda t: t)
            name = f"conv3x3 s{stride} {cin}->{cout} {H}x{W} relu={relu}"
            _within("B resnet conv3x3 three-term", name, got, act(three), FR.ACC * mag)
            _within("B resnet conv3x3 float64", name, got, act(base), FR.CUT * mag)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_row_blocks_read_their_own_rows(gpu, stride):
    """The channel identity at ONE tap over 256 channels, integer x below 2^16: the output IS the shifted, strided, zero-padded x, so a
    row block that read another block's rows of the matrix, or stored to another block's channels, shows bit for bit."""
    from mvsdet_amd import ops
    C, H, W = 256, 5, 7
    x = torch.randint(1, 1 << 16, (2, C, H, W), generator=torch.Generator().manual_seed(31 + stride)).float().to(gpu)
    xp = F.pad(x, (1, 1, 1, 1))
    ho, wo = R.out_size(H, stride), R.out_size(W, stride)
    one, zero = torch.ones(C, device=gpu), torch.zeros(C, device=gpu)
    for dy in range(3):
        for dx in range(3):
            w = torch.zeros(C, C, 3, 3, device=gpu)
            w[:, :, dy, dx] = torch.eye(C, device=gpu)
            got = ops.resnet.conv3x3(x, ops.gemm_split_weight(ops.resnet.fold(w, one)), zero, C, stride=stride, relu=False)
            want = xp[:, :, dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride]
            assert torch.equal(got, want), (dy, dx)


def _grad_weights(cout, c, k, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, c, k, k, generator=g) / (k * k * c) ** 0.5).to(gpu)
    scale = (0.5 + torch.rand(cout, generator=g)).to(gpu)
    return w, scale, w * scale.view(-1, 1, 1, 1)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", [256, 512])
def test_conv3x3_input_grad_row_blocks(gpu, stride, C):
    """256 and 512 rows (two and four row blocks), K = 64: integer operands bit-exact, random operands within both bounds, with a gate."""
    from mvsdet_amd import ops
    N, K = 2, 64
    for H, W in _maps(stride):
        gshape = (N, K, G.out_size(H, stride), G.out_size(W, stride))
        gb, w = _ints(-4, 4, gshape, 41 + H + C, gpu), _ints(-3, 3, (K, C, 3, 3), 42 + H + C + stride, gpu)
        assert 4 * 3 * 9 * K < 2 ** 24
        got = ops.resnet.conv3x3_input_grad(gb, w, torch.ones(K, device=gpu), (H, W), stride)
        want = G.conv_dx64(gb, w, stride, (H, W))
        assert got.shape == (N, C, H, W) and float(want.abs().max()) > 0
        assert torch.equal(got.double(), want), (H, W)
        w, scale, wf = _grad_weights(K, C, 3, 43 + H + C + stride, gpu)
        gb, gate = _rand(gshape, 44 + H, gpu), torch.relu(_rand((N, C, H, W), 45 + H, gpu))
        mag = G.conv_dx64(gb.abs(), wf.abs(), stride, (H, W))
        three, base = G.three_term_dx64(gb, wf, stride, (H, W)), G.conv_dx64(gb, wf, stride, (H, W))
        for gated in (False, True):
            got = ops.resnet.conv3x3_input_grad(gb, w, scale, (H, W), stride, gate=gate if gated else None)
            fin = (lambda t: G.gate64(t, gate.double())) if gated else (lambda t: t)
            name = f"dx3x3 s{stride} C={C} {H}x{W} gate={gated}"
            _within("B resnet dx3x3 three-term", name, got, fin(three), FR.ACC * mag)
            _within("B resnet dx3x3 float64", name, got, fin(base), FR.CUT * mag)
            if gated:
                assert bool((got[gate <= 0] == 0).all()) and not bool(torch.signbit(got[gate <= 0]).any())


def test_conv1x1_input_grad_eight_row_blocks(gpu):
    """C = 1024 rows, K = 256, the half-resolution residual and a gate: both bounds."""
    from mvsdet_amd import ops
    N, C, K = 2, 1024, 256
    for H, W in _maps(1):
        w, scale, wf = _grad_weights(K, C, 1, 51 + H, gpu)
        g, gate = _rand((N, K, H, W), 52 + H, gpu), torch.relu(_rand((N, C, H, W), 53 + H, gpu))
        half = _rand((N, C, G.out_size(H, 2), G.out_size(W, 2)), 54 + H, gpu)
        add = G.spread64(half.double(), 2, (H, W))
        mag = G.conv_dx64(g.abs(), wf.abs(), 1, (H, W)) + add.abs()
        got = ops.resnet.conv1x1_input_grad(g, w, scale, gate=gate, residual=half, spread=2)
        assert got.shape == (N, C, H, W)
        name = f"dx1x1 C={C} K={K} {H}x{W}"
        _within("B resnet dx1x1 three-term", name, got, G.gate64(G.three_term_dx64(g, wf, 1, (H, W)) + add, gate.double()), FR.ACC * mag)
        _within("B resnet dx1x1 float64", name, got, G.gate64(G.conv_dx64(g, wf, 1, (H, W)) + add, gate.double()), FR.CUT * mag)
        assert bool((got[gate <= 0] == 0).all()) and float(got[gate > 0].abs().max()) > 0


@pytest.mark.parametrize("k", [1, 3])
def test_fpn_input_grads_at_the_c5_lateral(gpu, k):
    """C = 2048 rows (sixteen row blocks) under 256 output channels: the lateral's and the 3x3's input gradient, both bounds."""
    from mvsdet_amd import ops
    N, C, cout = 2, 2048, 256
    assert k * k * cout <= ACC_TERMS
    for H, W in _maps(1):
        gen = torch.Generator().manual_seed(61 + H + k)
        g = torch.randn(N, cout, H, W, generator=gen).to(gpu)
        w = (torch.randn(cout, C, k, k, generator=gen) / (k * k * cout) ** 0.5).to(gpu)
        got = ops.fpn.lateral_input_grad(g, w) if k == 1 else ops.fpn.conv3x3_input_grad(g, w)
        assert got.shape == (N, C, H, W)
        mag = G.conv_dx64(g.abs(), w.abs(), 1, (H, W))
        name = f"fpn dx {k}x{k} C={C} {H}x{W}"
        _within("B fpn dx three-term", name, got, G.three_term_dx64(g, w, 1, (H, W)), FR.ACC * mag)
        _within("B fpn dx float64", name, got, G.conv_dx64(g, w, 1, (H, W)), FR.CUT * mag)


# ======================================================================== the kernels of C and D, one small ragged case each
N_VIEWS, CIN, COUT, SIZE = 2, 64, 128, (9, 35)      # 3x3: 2 x 3 tiles (stride 1), 2 x 2 (stride 2); 1x1: 630 columns in ten blocks
LINEAR = ["resnet.conv1x1 s1", "resnet.conv1x1 s2", "resnet.conv3x3 s1", "resnet.conv3x3 s2", "fpn.lateral", "fpn.conv3x3",
          "fpn.conv3x3 packed", "resnet.conv1x1_input_grad", "resnet.conv3x3_input_grad s1", "resnet.conv3x3_input_grad s2"]
DW_KERNELS = [("fpn", 1), ("fpn", 9), ("s2", 1), ("s2", 9)]


def _unpack(packed, shape, gpu):
    """The packed maps back as (N,C,H,W), through the positions `ops.pack_features` gives the elements' own numbers."""
    from mvsdet_amd import ops
    numel = math.prod(shape)
    assert numel < 2 ** 24
    where = ops.pack_features(torch.arange(1, numel + 1, dtype=torch.float32, device=gpu).view(shape))
    assert where.shape == packed.shape
    live = where > 0
    assert int(live.sum()) == numel
    out = torch.empty(numel, dtype=torch.float32, device=gpu)
    out[(where[live] - 1).long()] = packed[live]
    return out.view(shape)


class Linear:
    """One forward or input-gradient kernel as a linear map of ONE operand `x`: fn(x) -> (N, rows, H', W').  `additive`: with the shift,
    bias or residual (D) or without (C).  `gate`: the input gradients' gate map or None.  k, stride, transposed: its geometry."""

    def __init__(self, name, gpu, additive, gated=False, seed=71):
        from mvsdet_amd import ops
        self.name = name
        op, _, tail = name.partition(" ")
        self.stride = 2 if tail.startswith("s2") else 1
        self.k = 3 if "3x3" in op else 1
        self.transposed = op.endswith("_input_grad")
        s, k, H, W = self.stride, self.k, SIZE[0], SIZE[1]
        g = torch.Generator().manual_seed(seed + len(name))
        self.gate = None
        if not self.transposed:
            self.x = torch.randn(N_VIEWS, CIN, H, W, generator=g).to(gpu)
            self.out_hw = (R.out_size(H, s), R.out_size(W, s))
            w = (torch.randn(COUT, CIN, k, k, generator=g) / (k * k * CIN) ** 0.5).to(gpu)
            add = (torch.randn(COUT, generator=g) * 0.1).to(gpu) if additive else torch.zeros(COUT, device=gpu)
            if op.startswith("resnet."):
                scale = (0.5 + torch.rand(COUT, generator=g)).to(gpu)
                wq = ops.gemm_split_weight(ops.resnet.fold(w, scale))
                conv = ops.resnet.conv3x3 if k == 3 else ops.resnet.conv1x1
                self.fn = lambda x: conv(x, wq, add, COUT, stride=s, relu=additive)
            elif op == "fpn.lateral":
                wq = ops.gemm_split_weight(w.view(COUT, CIN).contiguous())
                self.fn = lambda x: ops.fpn.lateral(x, wq, add)
            else:
                wq = ops.gemm_split_weight(ops.fpn.conv3x3_matrix(w))
                if tail == "packed":
                    self.fn = lambda x: _unpack(ops.fpn.conv3x3(x, wq, add, want_nchw=False, want_packed=True), (N_VIEWS, COUT, H, W), gpu)
                else:
                    self.fn = lambda x: ops.fpn.conv3x3(x, wq, add)
        else:
            # x = the output gradient (N, K = CIN, Ho, Wo); the result is (N, C = COUT, H, W)
            self.x = torch.randn(N_VIEWS, CIN, R.out_size(H, s), R.out_size(W, s), generator=g).to(gpu)
            self.out_hw = (H, W)
            w = (torch.randn(CIN, COUT, k, k, generator=g) / (k * k * COUT) ** 0.5).to(gpu)
            scale = (0.5 + torch.rand(CIN, generator=g)).to(gpu)
            if gated:
                self.gate = torch.relu(torch.randn(N_VIEWS, COUT, H, W, generator=g)).to(gpu)
            if k == 1:
                res = torch.randn(N_VIEWS, COUT, R.out_size(H, 2), R.out_size(W, 2), generator=g).to(gpu) if additive else None
                self.fn = lambda x: ops.resnet.conv1x1_input_grad(x, w, scale, gate=self.gate, residual=res, spread=2)
            else:
                self.fn = lambda x: ops.resnet.conv3x3_input_grad(x, w, scale, (H, W), s, gate=self.gate)

    def field(self, y, x):
        """The output pixels that the operation pairs the operand's pixel (y, x) with, from the shapes alone: (H', W') bool."""
        s, k, p = self.stride, self.k, self.k // 2
        m = torch.zeros(self.out_hw, dtype=torch.bool)
        for dy in range(k):
            for dx in range(k):
                if self.transposed:                           # the convolution's output pixel (y, x) reached its input (s y + dy - p, ..)
                    yo, xo = s * y + dy - p, s * x + dx - p
                else:                                         # output (yo, xo) reads the input pixel (s yo + dy - p, s xo + dx - p)
                    if (y + p - dy) % s or (x + p - dx) % s:
                        continue
                    yo, xo = (y + p - dy) // s, (x + p - dx) // s
                if 0 <= yo < self.out_hw[0] and 0 <= xo < self.out_hw[1]:
                    m[yo, xo] = True
        return m


def _dw_case(kernel, taps, gpu, seed=81):
    s = _stride(kernel)
    gy = _rand((N_VIEWS, COUT, G.out_size(SIZE[0], s), G.out_size(SIZE[1], s)), seed + taps + s, gpu)
    x = _rand((N_VIEWS, CIN) + SIZE, seed + 7 + taps + s, gpu)
    assert _plan(kernel, taps, (N_VIEWS, CIN, COUT) + SIZE)[0] >= 2 * N_VIEWS     # several tiles a view, ragged on both axes
    return gy, x


# ======================================================================== C. the range is fp32's
FP16_MAX, FP16_TINY = 65504.0, 2.0 ** -24
# The largest finite fp32 that two bf16 pieces hold exactly: hi = the largest finite bf16, (2 - 2^-7) 2^127; x rounds to it while
# x - hi < half its ulp = 2^119, and the largest bf16 below 2^119 is mid = (2 - 2^-7) 2^118.  hi + mid has 16 significant bits: 0x7f7f7f80.
TWO_PIECE_MAX = torch.tensor((2 - 2.0 ** -7) * 2.0 ** 127 + (2 - 2.0 ** -7) * 2.0 ** 118, dtype=torch.float64).float()


def _scaled(x, k):
    """x 2^k, exactly (asserted: nothing under- or overflows)."""
    y = torch.ldexp(x, torch.tensor(k, device=x.device))
    assert torch.equal(torch.ldexp(y, torch.tensor(-k, device=x.device)), x) and bool(torch.isfinite(y).all())
    return y


@pytest.mark.parametrize("name", LINEAR)
def test_power_of_two_scaling_commutes(gpu, name):
    """op(2^k x, w) == 2^k op(x, w) bit for bit at k = -40 and +40, no additive term: the cut, the products and the fp32 accumulation
    commute with an exact scaling while nothing under- or overflows.  An operand format of fp16's range cannot hold these inputs."""
    lin = Linear(name, gpu, additive=False, gated=True)
    base = lin.fn(lin.x)
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    for k in (-40, 40):
        xs = _scaled(lin.x, k)
        if k > 0:
            assert float(xs.abs().max()) > FP16_MAX
        else:
            assert float(xs.abs().max()) < FP16_TINY and float(xs.abs().max()) > 0
        assert _same_bits(lin.fn(xs), _scaled(base, k)), k


@pytest.mark.parametrize("kernel,taps", DW_KERNELS)
def test_weight_grad_scaling_cancels(gpu, kernel, taps):
    """gy 2^40 against x 2^-40: every product is the unscaled one, the result keeps its bits."""
    gy, x = _dw_case(kernel, taps, gpu)
    base = _dw(kernel, gy, x, taps)
    gs, xs = _scaled(gy, 40), _scaled(x, -40)
    assert float(gs.abs().max()) > FP16_MAX and float(xs.abs().max()) < FP16_TINY
    assert bool(torch.isfinite(base).all()) and _same_bits(_dw(kernel, gs, xs, taps), base)


IDENTITY = ["resnet.conv1x1 s1", "resnet.conv1x1 s2", "resnet.conv3x3 s1", "resnet.conv3x3 s2", "fpn.lateral", "fpn.conv3x3"]


def _identity(name, gpu):
    """The kernel with the channel identity at the centre tap and no additive term: fn(x) == x[:, :, ::s, ::s] for x two pieces hold."""
    from mvsdet_amd import ops
    op, _, tail = name.partition(" ")
    s, k, C = (2 if tail == "s2" else 1), (3 if "3x3" in op else 1), COUT
    w = torch.zeros(C, C, k, k, device=gpu)
    w[:, :, k // 2, k // 2] = torch.eye(C, device=gpu)
    zero = torch.zeros(C, device=gpu)
    if op.startswith("resnet."):
        wq = ops.gemm_split_weight(ops.resnet.fold(w, torch.ones(C, device=gpu)))
        conv = ops.resnet.conv3x3 if k == 3 else ops.resnet.conv1x1
        return s, lambda x: conv(x, wq, zero, C, stride=s, relu=False)
    if k == 1:
        wq = ops.gemm_split_weight(w.view(C, C).contiguous())
        return s, lambda x: ops.fpn.lateral(x, wq, zero)
    wq = ops.gemm_split_weight(ops.fpn.conv3x3_matrix(w))
    return s, lambda x: ops.fpn.conv3x3(x, wq, zero)


PLANT_AT = [(0, 5, 4, 16), (1, 127, 8, 34), (1, 64, 0, 0)]      # (view, channel, y, x): even pixels, which stride 2 reads as well


@pytest.mark.parametrize("name", IDENTITY)
def test_largest_two_piece_value_comes_out_as_itself(gpu, name):
    """0x7f7f7f80 = the largest finite fp32 that two bf16 pieces hold exactly (its hi piece is the largest finite bf16), both signs, in a
    map of integers below 2^16, through the identity: the output is the input, bit for bit."""
    s, fn = _identity(name, gpu)
    x = _ints(1, (1 << 16) - 1, (N_VIEWS, COUT) + SIZE, 91, gpu)
    for i, (n, c, y, xx) in enumerate(PLANT_AT):
        x[n, c, y, xx] = TWO_PIECE_MAX.to(gpu) * (-1 if i == 1 else 1)
    got = fn(x)
    assert bool(torch.isfinite(got).all())
    assert _same_bits(got, x[:, :, ::s, ::s])


SUBNORMALS = [0x00000001, 0x007fffff, 0x80000001, 0x807fffff]


@pytest.mark.parametrize("name", IDENTITY)
def test_subnormals_come_out_finite(gpu, name):
    """fp32 subnormals in an otherwise zero map through the identity: every output element is finite; each planted position holds the
    planted value as its two bf16 pieces carry it, or a zero; every other position a zero.  Which of them the hardware gives is printed,
    not asserted.

    "As the two pieces carry it" is `ops.split_bf16` on the CPU, hi + mid: bf16 has fp32's exponent range but 7 fraction bits, so its
    smallest subnormal is 2^-133 and 0x00000001 = 2^-149 cuts to zero, while 0x007fffff rounds UP to hi = 0x0080 = 2^-126, the smallest
    normal, with a remainder of -2^-149 that no piece holds.  The first form of this test asked for the planted value itself or a zero;
    MI355X gave 0x007fffff -> 0x00800000 in all six kernels (and both one-ulp values -> +0.0): the cut done as written, one subnormal ulp
    (2^-149, against CUT |x| = 2^-140.4) away.  That expectation was the wrong one, not the kernel."""
    from mvsdet_amd import ops
    s, fn = _identity(name, gpu)
    x = torch.zeros((N_VIEWS, COUT) + SIZE, device=gpu)
    spots = [(0, 5, 4, 16), (1, 127, 8, 34), (1, 64, 0, 0), (0, 31, 2, 6)]
    for (n, c, y, xx), b in zip(spots, SUBNORMALS):
        x[n, c, y, xx] = _f32(b, gpu)
    assert sorted(_bits(x)[_bits(x) != 0].tolist()) == sorted(b if b < 1 << 31 else b - (1 << 32) for b in SUBNORMALS)    # they arrive on the device as they are
    got = fn(x)
    gb = _bits(got).clone()
    assert bool(torch.isfinite(got).all())
    seen = []
    for (n, c, y, xx), b in zip(spots, SUBNORMALS):
        out = int(gb[n, c, y // s, xx // s]) & 0xffffffff
        seen.append(f"{b:#010x} -> {out:#010x}")
        gb[n, c, y // s, xx // s] = 0
    print(f"[C subnormals] {name}: " + ", ".join(seen))
    assert bool(((gb == 0) | (gb == -(1 << 31))).all())           # every position that holds no plant: +0.0 or -0.0
    for (n, c, y, xx), b in zip(spots, SUBNORMALS):
        out = int(_bits(got)[n, c, y // s, xx // s]) & 0xffffffff
        hi, mid = ops.split_bf16(_f32(b))
        cut = int(_bits((hi.float() + mid.float()).view(1)).item()) & 0xffffffff
        assert abs(float(_f32(cut)) - float(_f32(b))) <= 2.0 ** -149          # the cut itself is at most one subnormal ulp away
        assert out in (cut, 0, 0x80000000), f"{b:#010x} came out as {out:#010x} (its two pieces hold {cut:#010x})"


# ======================================================================== D. non-finite inputs stay where the operation puts them
PLANTS = [("nan", 0x7fc00000), ("+inf", 0x7f800000), ("0x7f7f8000", 0x7f7f8000)]


@pytest.mark.parametrize("name,gated", [(n, False) for n in LINEAR] + [(n, True) for n in LINEAR if "_input_grad" in n])
def test_nonfinite_reaches_exactly_the_receptive_field(gpu, name, gated):
    """One planted element, in the interior of view 0 and at the last row and column of view 1: the NaNs of the output are exactly the
    planted element's receptive field (computed from the shapes) in every output channel of its view; every other element has the clean
    run's bits.  Under a gate a dropped position of the field is +0.0.  With the shift or bias, the residual and ReLU."""
    lin = Linear(name, gpu, additive=True, gated=gated)
    clean = lin.fn(lin.x)
    assert bool(torch.isfinite(clean).all())
    h, w = lin.x.shape[2:]
    for n, c, y, xx in ((0, 37, h // 2, w // 2 - (w // 2) % 2), (1, 5, h - 1, w - 1)):
        field = torch.zeros(clean.shape, dtype=torch.bool)
        field[n, :, lin.field(y, xx)] = True
        field = field.to(gpu)
        assert int(field[n, 0].sum()) >= 1 and not bool(field[1 - n].any())
        passes = field if lin.gate is None else field & (lin.gate > 0)
        assert bool(passes.any())
        for what, b in PLANTS:
            xb = lin.x.clone()
            xb[n, c, y, xx] = _f32(b, gpu)
            got = lin.fn(xb)
            assert torch.equal(torch.isnan(got), passes), (what, n, y, xx, int(torch.isnan(got).sum()), int(passes.sum()))
            assert bool(torch.isfinite(got[~passes]).all())
            assert torch.equal(_bits(got)[~field], _bits(clean)[~field]), (what, n, y, xx)
            assert bool((_bits(got)[field & ~passes] == 0).all())         # dropped by the gate: +0.0 whatever reached it


def _paired_taps(taps, stride, operand, y, x, in_hw, out_hw):
    """The taps (dy, dx) under which the mathematical sum pairs the planted element with an element inside the other map."""
    k = 3 if taps == 9 else 1
    p = k // 2
    out = []
    for dy in range(k):
        for dx in range(k):
            if operand == "gy":                               # gy[yo, xo] meets x[s yo + dy - p, s xo + dx - p]
                ok = 0 <= stride * y + dy - p < in_hw[0] and 0 <= stride * x + dx - p < in_hw[1]
            else:                                             # x[y, x] meets gy[(y + p - dy) / s, (x + p - dx) / s]
                ny, nx = y + p - dy, x + p - dx
                ok = ny % stride == 0 and nx % stride == 0 and 0 <= ny // stride < out_hw[0] and 0 <= nx // stride < out_hw[1]
            if ok:
                out.append((dy, dx))
    return out


@pytest.mark.parametrize("kernel,taps", DW_KERNELS)
def test_nonfinite_stays_in_its_row_or_column_of_dw(gpu, kernel, taps):
    """A plant in gy[n, o] leaves every row o' != o of dW with the clean run's bits, a plant in x[n, c] every column c' != c; the taps the
    sum pairs the planted element with are NaN.  Further taps of the same row or column may be NaN as well (the ragged edge's and the
    padding's 0 * NaN): they are counted and printed, not asserted."""
    s = _stride(kernel)
    gy, x = _dw_case(kernel, taps, gpu)
    clean = _dw(kernel, gy, x, taps)
    assert bool(torch.isfinite(clean).all())
    in_hw, out_hw = tuple(x.shape[2:]), tuple(gy.shape[2:])
    for operand, t, ch in (("gy", gy, 77), ("x", x, 37)):
        h, w = t.shape[2:]
        spots = [(0, h // 2, w // 2 - (w // 2) % 2), (1, h - 1, w - 1)] + ([(0, 3, 15)] if operand == "x" else [])
        for n, y, xx in spots:
            paired = _paired_taps(taps, s, operand, y, xx, in_hw, out_hw)
            for what, b in PLANTS:
                tb = t.clone()
                tb[n, ch, y, xx] = _f32(b, gpu)
                got = _dw(kernel, tb, x, taps) if operand == "gy" else _dw(kernel, gy, tb, taps)
                own = torch.zeros(clean.shape, dtype=torch.bool, device=gpu)
                if operand == "gy":
                    own[ch] = True
                else:
                    own[:, ch] = True
                assert torch.equal(_bits(got)[~own], _bits(clean)[~own]), (operand, what, n, y, xx)
                line = got[ch] if operand == "gy" else got[:, ch]           # (C | Cout, k, k)
                must = torch.zeros(line.shape[1:], dtype=torch.bool)
                for dy, dx in paired:
                    must[dy, dx] = True
                must = must.to(gpu)
                assert bool(torch.isnan(line[:, must]).all()), (operand, what, n, y, xx, paired)
                extra = int((~torch.isfinite(line[:, ~must])).sum())
                print(f"[D dw] {kernel} {taps} taps, {what} in {operand}[{n},{ch},{y},{xx}]: {len(paired)} paired taps NaN, "
                      f"{extra} further non-finite elements of the same {'row' if operand == 'gy' else 'column'}")
