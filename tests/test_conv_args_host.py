"""What the seven convolution entry points refuse on the host, and which refusal wins where two apply.

Every call here carries at least one fault and dummy pointers: the checks return MVSDET_ERR_INVALID_ARG (1) before any HIP call, so
the tests need no GPU and launch nothing.  (A call that got past the checks would return 3 here, never 1.)

Two refusals of launch_bf16x3 / launch_s2_bf16x3 / launch_convT cannot be reached through the C entry points and so are not asserted:
"the split form needs the fp32 output" (no fp32 output means an SCL output, which already forces the unsplit form) and "statistics
are those of the raw fp32 output" (the *_stats entry points pass no affine, residual, ReLU or SCL output, and a missing fp32 output
is a NULL pointer first)."""
import ctypes
import os

import pytest

P = ctypes.c_void_p(4096)     # any 16-byte aligned address: never dereferenced
ODD8 = ctypes.c_void_p(4104)  # 8- but not 16-byte aligned
ODD4 = ctypes.c_void_p(4100)  # 4- but not 8-byte aligned


def strides(*v):
    return (ctypes.c_int64 * 4)(*v)


# a well-formed call of every entry point, as keyword -> value in the order of the C signature; every case overrides at least one
GOOD = {
    "mvsdet_conv3d_k3_bf16x3_io": dict(xs=P, x=None, x_strides=None, weight_split=P, scale=None, shift=None, residual=None, out_f32=P,
                                       out_scl=None, out_pscl=None, workspace=None, workspace_bytes=0, N=1, Cin=8, Cout=64, D=4, H=8,
                                       W=16, relu=0, stream=None),
    "mvsdet_conv3d_k3_bf16x3_stats": dict(xs=P, x=None, x_strides=None, weight_split=P, out_f32=P, stats=P, stats_bytes=1 << 30,
                                          pivot=None, N=1, Cin=8, Cout=64, D=4, H=8, W=16, stream=None),
    "mvsdet_conv3d_k3_s2_bf16x3_io": dict(x=P, x_strides=None, x_pscl=None, weight_split=P, scale=None, shift=None, out_f32=P,
                                          out_scl=None, workspace=None, workspace_bytes=0, N=1, Cin=8, Cout=64, Di=8, Hi=16, Wi=32,
                                          relu=0, stream=None),
    "mvsdet_convT3d_k3_s2_bf16x3_io": dict(xs=P, weight_split=P, scale=None, shift=None, residual=None, out_f32=P, out_scl=None, N=1,
                                           Cin=8, Cout=64, D=4, H=8, W=16, relu=0, stream=None),
    "mvsdet_conv3d_k3_fp16mx_f32in": dict(x=P, x_strides=None, weight_split_mx=P, scale=None, shift=None, out_f32=P, out_scl=None,
                                          out_pscl=None, N=1, Cin=8, Cout=64, D=4, H=8, W=16, relu=0, stream=None),
    "mvsdet_conv3d_k3_mfma_ws_f32": dict(x=P, weight_perm=P, scale=None, shift=None, residual=None, out=P, workspace=None,
                                         workspace_bytes=0, N=1, Cin=8, Cout=64, D=4, H=8, W=16, stride=1, relu=0, stream=None),
    "mvsdet_convT3d_k3_s2_mfma_f32": dict(x=P, weight_perm=P, scale=None, shift=None, residual=None, out=P, N=1, Cin=8, Cout=64, D=4,
                                          H=8, W=16, relu=0, stream=None),
}
# the operator's name that opens every message of an entry point (the stride-2 one names its input form)
NAME = {
    "mvsdet_conv3d_k3_bf16x3_io": b"conv3d_k3_bf16x3_io: ",
    "mvsdet_conv3d_k3_bf16x3_stats": b"conv3d_k3_bf16x3_stats: ",
    "mvsdet_conv3d_k3_s2_bf16x3_io": b"conv3d_k3_s2_bf16x3_f32in: ",
    "mvsdet_convT3d_k3_s2_bf16x3_io": b"convT3d_k3_s2_bf16x3: ",
    "mvsdet_conv3d_k3_fp16mx_f32in": b"conv3d_k3_fp16mx_f32in: ",
    "mvsdet_conv3d_k3_mfma_ws_f32": b"conv3d_k3_mfma_ws: ",
    "mvsdet_convT3d_k3_s2_mfma_f32": b"convT3d_k3_s2_mfma: ",
}
BF, ST, S2, CT, MX, MF, MT = list(GOOD)
NEG = strides(-1, 128, 32, 4)                      # a negative batch stride
SHORT = strides(4096, 512, 128, 15)                # rows closer together than they are long (W = 16)
WIDE = strides(1 << 40, 1 << 35, 1 << 31, 16)      # plane stride 2^31: a channel volume no int offset spans
WIDE2 = strides(1 << 40, 1 << 35, 1 << 31, 32)     # the same for the stride-2 layer's 8 x 16 x 32 input

# (entry point, overrides of GOOD, name that opens the message, words of the message)
CASES = [
    # NULL pointers
    (BF, dict(weight_split=None), None, b"NULL pointer"),
    (BF, dict(out_f32=None), None, b"NULL pointer"),
    (ST, dict(weight_split=None), None, b"NULL pointer"),
    (ST, dict(out_f32=None), None, b"NULL pointer"),
    (ST, dict(stats=None), None, b"NULL statistics buffer"),
    (S2, dict(weight_split=None), None, b"NULL pointer"),
    (S2, dict(out_f32=None), None, b"NULL pointer"),
    (CT, dict(xs=None), None, b"NULL pointer"),
    (CT, dict(out_f32=None), None, b"NULL pointer"),
    (MX, dict(x=None), None, b"NULL pointer"),
    (MX, dict(out_f32=None), None, b"NULL pointer"),
    (MF, dict(x=None), None, b"NULL pointer"),
    (MF, dict(out=None), None, b"NULL pointer"),
    (MT, dict(weight_perm=None), None, b"NULL pointer"),
    (MT, dict(out=None), None, b"NULL pointer"),
    # exactly one of the two input forms
    (BF, dict(x=P), None, b"exactly one of xs (SCL) and x (fp32)"),
    (BF, dict(xs=None), None, b"exactly one of xs (SCL) and x (fp32)"),
    (ST, dict(x=P), None, b"exactly one of xs (SCL) and x (fp32)"),
    (ST, dict(xs=None), None, b"exactly one of xs (SCL) and x (fp32)"),
    (S2, dict(x_pscl=P), b"conv3d_k3_s2_bf16x3: ", b"exactly one of x (fp32) and x_pscl"),
    (S2, dict(x=None), b"conv3d_k3_s2_bf16x3: ", b"exactly one of x (fp32) and x_pscl"),
    # scale and shift together
    (BF, dict(scale=P), None, b"scale and shift come together"),
    (BF, dict(shift=P), None, b"scale and shift come together"),
    (S2, dict(scale=P), None, b"scale and shift come together"),
    (S2, dict(x=None, x_pscl=P, shift=P), b"conv3d_k3_s2_bf16x3 (PSCL input): ", b"scale and shift come together"),
    (CT, dict(shift=P), None, b"scale and shift come together"),
    (MX, dict(scale=P), None, b"scale and shift come together"),
    (MF, dict(shift=P), None, b"scale and shift come together"),
    (MT, dict(scale=P), None, b"scale and shift come together"),
    # a positive shape
    (BF, dict(N=0), None, b"bad shape N=0 Cin=8 D=4 H=8 W=16"),
    (BF, dict(W=-1), None, b"bad shape N=1 Cin=8 D=4 H=8 W=-1"),
    (ST, dict(Cin=0), None, b"bad shape N=1 Cin=0 D=4 H=8 W=16"),
    (S2, dict(Di=0), None, b"bad shape N=1 Cin=8 D=0 H=16 W=32"),
    (CT, dict(H=0), None, b"bad shape N=1 Cin=8 D=4 H=0 W=16"),
    (MX, dict(D=0), None, b"bad shape N=1 Cin=8 D=0 H=8 W=16"),
    (MF, dict(N=-2), None, b"bad shape N=-2 Cin=8 D=4 H=8 W=16"),
    (MT, dict(W=0), None, b"bad shape N=1 Cin=8 D=4 H=8 W=0"),
    # Cout a positive multiple of 64
    (BF, dict(Cout=96), None, b"Cout=96 must be a multiple of 64"),
    (BF, dict(Cout=0), None, b"Cout=0 must be a multiple of 64"),
    (ST, dict(Cout=32), None, b"Cout=32 must be a multiple of 64"),
    (S2, dict(Cout=65), None, b"Cout=65 must be a multiple of 64"),
    (CT, dict(Cout=96), None, b"Cout=96 must be a multiple of 64"),
    (MX, dict(Cout=-64), None, b"Cout=-64 must be a multiple of 64"),
    (MF, dict(Cout=96), None, b"Cout=96 must be a multiple of 64"),
    (MT, dict(Cout=1), None, b"Cout=1 must be a multiple of 64"),
    # 16-byte alignment of weights and SCL buffers
    (BF, dict(weight_split=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (BF, dict(xs=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (BF, dict(out_scl=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (BF, dict(out_pscl=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (ST, dict(weight_split=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (S2, dict(weight_split=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (S2, dict(out_scl=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (S2, dict(x=None, x_pscl=ODD8), b"conv3d_k3_s2_bf16x3 (PSCL input): ", b"SCL buffers and weights must be 16-byte aligned"),
    (CT, dict(xs=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (CT, dict(weight_split=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (CT, dict(out_scl=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (MX, dict(weight_split_mx=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (MX, dict(out_pscl=ODD8), None, b"SCL buffers and weights must be 16-byte aligned"),
    (MF, dict(weight_perm=ODD8), None, b"weights must be 16-byte aligned"),
    (MT, dict(weight_perm=ODD8), None, b"weights must be 16-byte aligned"),
    # 8-byte alignment of out and residual: the transposed kernels write and read float2
    (CT, dict(out_f32=ODD4), None, b"out and residual must be 8-byte aligned"),
    (CT, dict(residual=ODD4), None, b"out and residual must be 8-byte aligned"),
    (MT, dict(out=ODD4), None, b"out and residual must be 8-byte aligned"),
    (MT, dict(residual=ODD4), None, b"out and residual must be 8-byte aligned"),
    # the fp32 view
    (BF, dict(xs=None, x=P, x_strides=NEG), None, b"bad strides"),
    (BF, dict(xs=None, x=P, x_strides=SHORT), None, b"bad strides"),
    (BF, dict(xs=None, x=P, x_strides=WIDE), None, b"one channel volume spans more than 2^31 elements"),
    (ST, dict(xs=None, x=P, x_strides=SHORT), None, b"bad strides"),
    (ST, dict(xs=None, x=P, x_strides=WIDE), None, b"one channel volume spans more than 2^31 elements"),
    (S2, dict(x_strides=strides(4096, 512, -1, 32)), None, b"bad strides"),
    (S2, dict(x_strides=WIDE2), None, b"one channel volume spans more than 2^31 elements"),
    (MX, dict(x_strides=NEG), None, b"bad strides"),
    (MX, dict(x_strides=SHORT), None, b"bad strides"),
    (MX, dict(x_strides=WIDE), None, b"beyond the kernel's 32-bit buffer offsets (mvsdet_conv3d_k3_fp16mx_ok"),
    # what the fp32-MFMA entry points check beside
    (MF, dict(stride=3), None, b"stride 3 not in {1,2}"),
    (MF, dict(residual=P, stride=2), None, b"a residual needs stride 1"),
]

# two faults in one call: the refusal that wins
WINS = [
    (BF, dict(Cout=96, weight_split=ODD8), None, b"Cout=96 must be a multiple of 64"),
    (BF, dict(weight_split=None, scale=P), None, b"NULL pointer"),
    (ST, dict(stats=None, x=P), None, b"exactly one of xs (SCL) and x (fp32)"),
    (ST, dict(N=0, Cout=96), None, b"bad shape N=0"),
    (S2, dict(scale=P, Di=0), None, b"scale and shift come together"),
    (S2, dict(x=None, weight_split=None), b"conv3d_k3_s2_bf16x3: ", b"exactly one of x (fp32) and x_pscl"),
    (CT, dict(weight_split=ODD8, out_f32=ODD4), None, b"SCL buffers and weights must be 16-byte aligned"),
    (CT, dict(Cout=96, residual=ODD4), None, b"Cout=96 must be a multiple of 64"),
    (MX, dict(x=None, Cout=96), None, b"NULL pointer"),
    (MX, dict(out_scl=ODD8, x_strides=SHORT), None, b"SCL buffers and weights must be 16-byte aligned"),
    (MF, dict(Cout=96, weight_perm=ODD8), None, b"weights must be 16-byte aligned"),   # the fp32-MFMA pair checks Cout last
    (MF, dict(Cout=96, stride=3), None, b"stride 3 not in {1,2}"),
    (MF, dict(residual=P, stride=2, x=None), None, b"a residual needs stride 1"),
    (MT, dict(Cout=96, out=ODD4), None, b"Cout=96 must be a multiple of 64"),
    (MT, dict(weight_perm=ODD8, Cout=96), None, b"weights must be 16-byte aligned"),
]


@pytest.fixture(scope="module")
def lib():
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _ident(case):
    fn, over, _, words = case
    return f"{fn[7:]}-{'+'.join(over)}-{words[:24].decode().strip().replace(' ', '_')}"


@pytest.mark.parametrize("case", CASES + WINS, ids=_ident)
def test_refusal(lib, case):
    fn, over, opens, words = case
    assert over and set(over) <= set(GOOD[fn]), "every case changes arguments of the well-formed call"
    args = dict(GOOD[fn], **over)
    rc = getattr(lib, fn)(*args.values())
    msg = lib.mvsdet_last_error()
    assert rc == 1, (rc, msg)
    assert msg.startswith(opens or NAME[fn]), msg
    assert words in msg, msg


def test_every_entry_point_has_every_refusal():
    """The table above covers, per entry point, each refusal the entry points share, and one overlapping pair at least."""
    shared = [b"NULL pointer", b"scale and shift", b"bad shape", b"must be a multiple of 64", b"16-byte aligned"]
    for fn in GOOD:
        words = [c[3] for c in CASES if c[0] == fn]
        for s in shared:
            if fn == ST and s == b"scale and shift":
                continue   # the statistics form takes no affine
            assert any(s in w for w in words), (fn, s)
        assert sum(1 for c in WINS if c[0] == fn and len(c[1]) >= 2) >= 1, fn
    for fn in (CT, MT):
        assert any(b"8-byte aligned" in c[3] for c in CASES if c[0] == fn), fn
    for fn in (BF, ST, S2, MX):
        assert any(b"bad strides" in c[3] for c in CASES if c[0] == fn), fn
    for fn in (BF, ST, S2):
        assert any(b"exactly one of" in c[3] for c in CASES if c[0] == fn), fn
        assert any(b"2^31 elements" in c[3] for c in CASES if c[0] == fn), fn
