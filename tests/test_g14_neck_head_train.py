"""Training of the 3-D neck and the detection head against G14 -- one training step of the reference's
`IndoorImVoxelNeck(256, 128, [1, 1, 1])` feeding `NerfDetHead(128, 6, 18, 3)` (tests/golden/make_goldens_g14.py) -- on both routes
of `autograd_route`, and the kernels behind the HIP route (csrc/neck_gemm.hip input / weight gradients, csrc/costreg_bn.hip
residual-inside-ReLU BatchNorm) against float64 at the neck's shapes and at edge shapes, inside guarded buffers."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
from lcg import lcg_fill_state, lcg_uniform  # noqa: E402

G14 = "g14_neck_head_train"


# ------------------------------------------------------------------------------------------------------------------ helpers
def _models(g, device, route="aten", arkit=False):
    from mvsdet_amd.head import NerfDetHeadConvs
    from mvsdet_amd.neck import IndoorImVoxelNeck
    neck = IndoorImVoxelNeck(256, 128, [1, 1, 1]).train()
    head = NerfDetHeadConvs(17 if arkit else 18, 3, 128, 7 if arkit else 6, arkit_head=arkit).train()
    with torch.no_grad():
        lcg_fill_state(neck, int(g["weight_seed_neck"]))
        lcg_fill_state(head, int(g["weight_seed_head"]))
        for s, v in zip(head.scales, g["head_scales"]):
            s.scale.fill_(float(v))
    neck.autograd_route = head.autograd_route = route
    return neck.to(device), head.to(device)


def _input(g, device):
    x = torch.from_numpy(lcg_uniform(256 * 40 * 40 * 16, int(g["input_seed"]))).reshape(1, 256, 40, 40, 16)
    keep = torch.from_numpy(lcg_uniform(40 * 40 * 16, int(g["mask_seed"]))).reshape(1, 1, 40, 40, 16) > float(g["mask_threshold"])
    return (x * keep).to(device)


def _loss(heads, r_seed):
    """make_goldens_g14.loss_weights: sum over levels of sum(center R_c + bbox R_r + cls R_cls)."""
    loss = 0.0
    for i, ts in enumerate(zip(*heads)):
        for k, t in enumerate(ts):
            r = torch.from_numpy(lcg_uniform(t.numel(), r_seed + 10 * i + k)).reshape(t.shape).to(t.device)
            loss = loss + (t * r).sum()
    return loss


def _step(neck, head, x, g, backward=True):
    x = x.detach().clone().requires_grad_(backward)
    levels = neck(x)
    heads = head(levels)
    if backward:
        _loss(heads, int(g["r_seed"])).backward()
    return x, levels, heads


def _relu_modules(neck):
    """The neck's hook keys by the reference's ReLU module names (`.activate` of a ConvModule, `.activation` of a ResModule, the
    nn.ReLU of an up / out block)."""
    mods = dict(neck.named_modules())
    out = {}
    for name, m in neck.named_modules():
        if isinstance(m, torch.nn.ReLU):
            out[name] = m
    for name, m in mods.items():
        if type(m).__name__ == "ResModule":
            out[name + ".activation"] = m
            out[name + ".conv0.activate"] = m.conv0
    return out


def _check_decisions(rec, neck, g):
    """Decisions recorded on `neck` (layers.RELU_MASKS "record") against the fixture: every `mask_stride`-th decision of each layer
    (a flip allowed on at most 1e-5 of the samples, for another host's summation order) and each layer's count of positive ones."""
    keys = _relu_modules(neck)
    names = [str(n) for n in g["mask_names"]]
    assert sorted(keys) == sorted(names) and set(rec) == set(keys.values())
    stride = int(g["mask_stride"])
    flips = samples = 0
    for name in names:
        m = rec[keys[name]].cpu()
        assert tuple(m.shape) == tuple(int(v) for v in g["maskshape:" + name]), name
        got = m.reshape(-1)[::stride].numpy()
        ref = np.unpackbits(g["maskbits:" + name])[: got.size].astype(bool)
        flips += int((got != ref).sum())
        samples += got.size
        pos = int(m.sum())
        assert abs(pos - int(g["maskpos:" + name])) <= max(8, 1e-6 * m.numel()), f"{name}: {pos} positive decisions, reference {int(g['maskpos:' + name])}"
    assert flips <= 1e-5 * samples, f"{flips} of {samples} sampled ReLU decisions differ from the reference's"


def _reference_decisions(g):
    """The reference's ReLU decisions, by the reference's ReLU names: recorded from the package's framework route on the CPU (the
    reference's own layers and arithmetic) and checked against the fixture's samples and counts."""
    cpu = torch.device("cpu")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    neck, head = _models(g, cpu)
    rec = {}
    with torch.no_grad():
        _, levels, heads = _with_hook(("record", rec), lambda: _step(neck, head, _input(g, cpu), g, backward=False))
    _check_decisions(rec, neck, g)
    return {name: rec[m] for name, m in _relu_modules(neck).items()}, (levels, heads)


def _decisions_for(neck, by_name, device):
    """The hook's ("apply", ...) table for `neck` from decisions kept by name."""
    return {m: by_name[name].to(device) for name, m in _relu_modules(neck).items()}


def _with_hook(hook, fn):
    from mvsdet_amd import layers
    was = layers.RELU_MASKS
    layers.RELU_MASKS = hook
    try:
        return fn()
    finally:
        layers.RELU_MASKS = was


def _check_outputs(levels, heads, g, tol):
    def close(a, ref, name):
        a = a.detach().float().cpu().numpy()
        np.testing.assert_allclose(a, ref, rtol=0, atol=tol * max(1.0, float(np.abs(ref).max())), err_msg=name)
    def sampled(t, name):   # the fixture's slice steps (channel, d, h, w) of array `name`
        c, d, h, w = (int(v) for v in g["step:" + name])
        return t[:, ::c, ::d, ::h, ::w]
    for i in range(3):
        close(sampled(levels[i], f"level{i}"), g[f"level{i}"], f"level{i}")
        for k, t in zip(("center", "reg", "cls"), (heads[0][i], heads[1][i], heads[2][i])):
            close(sampled(t, f"{k}{i}"), g[f"{k}{i}"], f"{k}{i}")


def _check_running_stats(neck, g, tol):
    n = 0
    for k, b in neck.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(b.cpu().numpy(), g["b:" + k], rtol=tol, atol=tol, err_msg=k)
            n += 1
        elif k.endswith("num_batches_tracked"):
            assert int(b) == int(g["b:" + k]), k
    assert n == 2 * 15


# The head's `scales.<l>.scale` are scalars: each gradient is ONE sum over the level's 6 x (40 >> l)^2 (16 >> l) bbox terms of both signs
# (|sum| ~ 1/400 of the sum of |terms| at level 0), so a 1e-6 relative difference of the terms -- the bf16x3 level outputs -- shows at
# ~1e-3 of the sum.  They are held at SCALAR_TOL relative instead of the per-element bar (measured on G14 with the reference's
# decisions imposed: 1.06e-3 at level 0).
SCALAR_TOL = 5e-3


def _check_grads(neck, head, x, g, elementwise_tol, norm_tol, outlier_share=0.0):
    """Every sampled gradient element-wise (None: skipped) within elementwise_tol of its tensor's scale, and in norm; the head's
    scalar factors within SCALAR_TOL (see there)."""
    items = [("grad_input", x.grad.reshape(-1)[::int(g["grad_input_stride"])].cpu().numpy(), g["grad_input"], None)]
    params = {"neck." + k: p for k, p in neck.named_parameters()}
    params.update({"head." + k: p for k, p in head.named_parameters()})
    assert sorted(params) == sorted(str(k) for k in g["param_keys"])
    for k in sorted(params):
        gr = params[k].grad.reshape(-1)
        items.append((k, gr[::int(g["s:" + k])].cpu().numpy(), g["g:" + k], (float((gr.double() ** 2).sum()), float(g["n:" + k]))))
    for name, a, ref, norms in items:
        scale = max(float(np.abs(ref).max()), 1e-12)
        if name.startswith("head.scales."):
            assert float(np.abs(a - ref).max()) <= max(norm_tol, SCALAR_TOL) * scale, f"{name}: {a} against {ref}"
            continue
        if elementwise_tol is not None:
            bad = np.abs(a - ref) > elementwise_tol * scale
            assert bad.mean() <= outlier_share, \
                f"{name}: {bad.mean():.2e} of the sampled entries off by more than {elementwise_tol:g} x scale (max {np.abs(a - ref).max() / scale:.2e})"
        rel = float(np.linalg.norm((a - ref).astype(np.float64)) / max(np.linalg.norm(ref.astype(np.float64)), 1e-30))
        assert rel <= norm_tol, f"{name}: relative error of the sample in norm {rel:.2e}"
        if norms is not None:
            assert abs(norms[0] ** 0.5 - norms[1] ** 0.5) <= norm_tol * max(norms[1] ** 0.5, 1e-30), f"{name}: norm of the whole gradient"


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_autograd_route_default_and_environment(monkeypatch):
    from mvsdet_amd.head import NerfDetHeadConvs
    from mvsdet_amd.neck import IndoorImVoxelNeck
    monkeypatch.delenv("MVSDET_DETECTOR_AUTOGRAD", raising=False)
    assert IndoorImVoxelNeck(64, 64, [1]).autograd_route == "aten"
    assert NerfDetHeadConvs(4, 1, 64, 6).autograd_route == "aten"
    monkeypatch.setenv("MVSDET_DETECTOR_AUTOGRAD", "hip")
    assert IndoorImVoxelNeck(64, 64, [1]).autograd_route == "hip"
    assert NerfDetHeadConvs(4, 1, 64, 6).autograd_route == "hip"
    monkeypatch.setenv("MVSDET_DETECTOR_AUTOGRAD", "miopen")
    with pytest.raises(ValueError, match="MVSDET_DETECTOR_AUTOGRAD"):
        IndoorImVoxelNeck(64, 64, [1])
    monkeypatch.delenv("MVSDET_DETECTOR_AUTOGRAD")
    neck = IndoorImVoxelNeck(64, 64, [1])
    neck.autograd_route = "fast"
    with pytest.raises(ValueError, match="autograd_route"):
        neck(torch.zeros(1, 64, 2, 2, 2))


def test_g14_aten_route_reproduces_the_reference_training_step():
    """The package's modules on the framework's layers (route "aten", CPU): the reference's outputs to 1e-5 and its ReLU decisions
    (recorded through layers.RELU_MASKS, against the fixture's sampled decisions and per-layer counts); then, with those decisions imposed, every gradient element-wise to 1e-4 of its scale and the
    running statistics after the step."""
    g = load_golden(G14)
    cpu = torch.device("cpu")
    decisions, (levels, heads) = _reference_decisions(g)
    _check_outputs(levels, heads, g, 1e-5)

    neck, head = _models(g, cpu)
    xg, levels, heads = _with_hook(("apply", _decisions_for(neck, decisions, cpu)), lambda: _step(neck, head, _input(g, cpu), g))
    _check_outputs(levels, heads, g, 1e-5)
    _check_grads(neck, head, xg, g, 1e-4, 1e-5)
    _check_running_stats(neck, g, 1e-5)


@pytest.fixture(scope="module")
def lib():
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_entry_points_reject_bad_arguments(lib):
    """NULL pointers, bad shapes and misalignment are rejected on the host with a message; nothing is launched."""
    one = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4098)

    def err(rc, want, text):
        assert rc == want, (rc, lib.mvsdet_last_error())
        assert text in lib.mvsdet_last_error(), lib.mvsdet_last_error()

    err(lib.mvsdet_conv3d_k1_s2_dx_bf16x3(None, one, one, 1, 128, 32, 4, 4, 4, None), 1, b"NULL")
    err(lib.mvsdet_conv3d_k1_s2_dx_bf16x3(one, one, one, 1, 96, 32, 4, 4, 4, None), 1, b"multiple of")
    err(lib.mvsdet_conv3d_k1_s2_dx_bf16x3(one, one, one, 1, 128, 32, 4, 3, 4, None), 1, b"even")
    err(lib.mvsdet_conv3d_k1_s2_dx_bf16x3(one, one, odd, 1, 128, 32, 4, 4, 4, None), 1, b"aligned")
    err(lib.mvsdet_convT3d_k2_s2_dx_bf16x3(one, None, one, 1, 128, 4, 2, 2, 2, None), 1, b"NULL")
    err(lib.mvsdet_convT3d_k2_s2_dx_bf16x3(one, one, one, 1, 128, 3, 2, 2, 2, None), 1, b"multiple of")
    err(lib.mvsdet_convT3d_k2_s2_dx_bf16x3(one, one, one, 0, 128, 4, 2, 2, 2, None), 1, b"bad shape")
    err(lib.mvsdet_neck_gemm_dw_bf16x3(one, None, one, None, 0, 1, 0, 1, 8, 8, 2, 2, 2, None), 1, b"NULL")
    err(lib.mvsdet_neck_gemm_dw_bf16x3(one, one, one, None, 0, 1, 2, 1, 8, 8, 2, 2, 2, None), 1, b"transposed")
    err(lib.mvsdet_neck_gemm_dw_bf16x3(one, one, one, None, 0, 1, 0, 1, 8, 0, 2, 2, 2, None), 1, b"bad shape")
    err(lib.mvsdet_neck_gemm_dw_bf16x3(one, one, one, None, 0, 4, 0, 1, 8, 8, 2, 2, 2, None), 1, b"partial")
    err(lib.mvsdet_neck_gemm_dw_bf16x3(one, one, one, one, 16, 4, 1, 1, 8, 8, 2, 2, 2, None), 2, b"partial buffer")
    err(lib.mvsdet_neck_gemm_dw_bf16x3(odd, one, one, None, 0, 1, 1, 1, 8, 8, 2, 2, 2, None), 1, b"aligned")
    assert lib.mvsdet_neck_gemm_dw_partial_bytes(8, 8, 1, 4) == 4 * 8 * 64 * 4
    assert lib.mvsdet_neck_gemm_dw_partial_bytes(8, 8, 0, 1) == 0
    wb = lib.mvsdet_bn3d_workspace_bytes(4)
    err(lib.mvsdet_bn3d_res_relu_train_fwd_f32(one, None, 0, None, None, None, None, None, None, one, one, one, one, wb, 1, 4, 8,
                                               0.1, 1e-5, 1, None), 1, b"NULL")
    err(lib.mvsdet_bn3d_res_relu_train_fwd_f32(one, None, 0, None, None, None, one, None, None, one, one, one, one, wb, 1, 0, 8,
                                               0.1, 1e-5, 1, None), 1, b"bad shape")
    err(lib.mvsdet_bn3d_res_relu_train_fwd_f32(one, None, 0, None, None, None, one, None, None, one, one, one, one, 8, 1, 4, 8,
                                               0.1, 1e-5, 1, None), 2, b"workspace")
    err(lib.mvsdet_bn3d_res_relu_train_fwd_f32(one, odd, 3, None, None, None, one, None, None, one, one, one, one, wb, 1, 4, 8,
                                               0.1, 1e-5, 1, None), 1, b"16-byte")
    err(lib.mvsdet_bn3d_res_relu_bwd_f32(one, None, one, None, None, one, one, one, None, None, None, one, wb, 1, 4, 8, 1, None), 1,
        b"forward's output")
    err(lib.mvsdet_bn3d_res_relu_bwd_f32(one, one, one, None, None, one, one, odd, None, None, None, one, wb, 1, 4, 8, 1, None), 1,
        b"aligned")


# ---------------------------------------------------------------------------------------------------------------------- GPU
TOL = 1e-4


@pytest.fixture
def g14():
    return load_golden(G14)


@pytest.mark.gpu
def test_g14_hip_route_with_the_reference_relu_decisions(gpu, g14):
    """The HIP route against the REFERENCE's training step with the reference's ReLU decisions imposed (layers.RELU_MASKS; recorded
    from the framework route on the CPU and checked against the fixture's sampled decisions and counts): G12c's bf16x3 bar -- outputs and running statistics 1e-4, every gradient element-wise to 1e-3 of its tensor's scale with no outlier
    and 1e-4 in norm."""
    decisions, _ = _reference_decisions(g14)
    neck, head = _models(g14, gpu, "hip")
    xg, levels, heads = _with_hook(("apply", _decisions_for(neck, decisions, gpu)), lambda: _step(neck, head, _input(g14, gpu), g14))
    _check_outputs(levels, heads, g14, TOL)
    _check_grads(neck, head, xg, g14, 1e-3, 1e-4)
    _check_running_stats(neck, g14, TOL)


@pytest.mark.gpu
def test_g14_hip_route_free_decisions(gpu, g14):
    """The HIP route with its own ReLU decisions: gradients 2e-2 in norm (G12's bar: a decision within the bf16x3 noise of zero may
    flip), outputs 1e-4."""
    neck, head = _models(g14, gpu, "hip")
    xg, levels, heads = _step(neck, head, _input(g14, gpu), g14)
    _check_outputs(levels, heads, g14, TOL)
    _check_grads(neck, head, xg, g14, None, 2e-2)


@pytest.mark.gpu
def test_hip_route_runs_no_framework_convolution_or_batchnorm(gpu, g14, monkeypatch):
    """A HIP-route training step (neck + head) with the framework's convolutions and BatchNorm made to raise."""
    def refuse(*a, **k):
        raise AssertionError("a framework convolution / BatchNorm ran on the HIP route")
    neck, head = _models(g14, gpu, "hip")
    x = _input(g14, gpu)
    for name in ("conv3d", "conv_transpose3d", "batch_norm"):
        monkeypatch.setattr(F, name, refuse)
    xg, levels, heads = _step(neck, head, x, g14)
    assert xg.grad is not None and all(p.grad is not None for p in list(neck.parameters()) + list(head.parameters()))
    with torch.no_grad():   # training mode without autograd: still our kernels, running statistics updated
        before = neck.down_layer_0[0].conv0.bn.running_mean.clone()
        neck(x)
        assert not torch.equal(before, neck.down_layer_0[0].conv0.bn.running_mean)


@pytest.mark.gpu
def test_hip_route_is_deterministic(gpu, g14):
    """Two identical steps: bit-identical outputs, gradients and running statistics (no atomics, split-K sums in a fixed order)."""
    runs = []
    for _ in range(2):
        neck, head = _models(g14, gpu, "hip")
        xg, levels, _ = _step(neck, head, _input(g14, gpu), g14)
        runs.append([xg.grad] + [l.detach() for l in levels] + [p.grad for p in neck.parameters()] + [p.grad for p in head.parameters()]
                    + [b for b in neck.buffers()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_running_statistics_match_the_aten_route_after_two_steps(gpu, g14):
    stats = {}
    for route in ("aten", "hip"):
        neck, head = _models(g14, gpu, route)
        x = _input(g14, gpu)
        for _ in range(2):
            _step(neck, head, x, g14)
        stats[route] = {k: b.clone() for k, b in neck.named_buffers()}
    for k, b in stats["aten"].items():
        torch.testing.assert_close(stats["hip"][k], b, rtol=1e-4, atol=1e-4, msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("arkit", [False, True], ids=["NerfDetHead", "ImVoxelHead_ARKit"])
def test_head_hip_route_against_aten(gpu, g14, arkit):
    """The head alone at the neck's three level shapes (Cout 25 / 25 padded to 64, Cin 128, W = 4 at level 2): outputs and every
    gradient element-wise (the head has no ReLU) against the framework's layers on the same device."""
    res = {}
    for route in ("aten", "hip"):
        _, head = _models(g14, gpu, route, arkit=arkit)
        xs = [torch.from_numpy(lcg_uniform(128 * (40 >> i) * (40 >> i) * (16 >> i), 300 + i)).reshape(1, 128, 40 >> i, 40 >> i, 16 >> i)
              .to(gpu).requires_grad_(True) for i in range(3)]
        heads = head(xs)
        _loss(heads, 310).backward()
        res[route] = ([t.detach() for ts in heads for t in ts], [x.grad for x in xs], [p.grad for p in head.parameters()])
    for a_list, b_list in zip(res["hip"], res["aten"]):
        for a, b in zip(a_list, b_list):
            scale = max(float(b.abs().max()), 1e-12)
            assert float((a - b).abs().max()) <= 1e-3 * scale


# ---- kernels a-d against float64, every output inside a guarded canvas
SENTINEL = 0x5A5A5A5A
GUARD = 1 << 14


class Guarded:
    """A float32 tensor of `shape` in the middle of a sentinel canvas."""

    def __init__(self, shape, dev, init=None):
        n = int(np.prod(shape))
        self.n = n
        self.canvas = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.t = self.canvas[GUARD:GUARD + n].view(torch.float32).view(shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.canvas[:GUARD] == SENTINEL).all()) and bool((self.canvas[GUARD + self.n:] == SENTINEL).all())


def _bound(absa, absb, fn):
    """The bf16x3 error bound: 2^-14 of the float64 sum of |products| (fn applied to |A|, |B|)."""
    return 2.0 ** -14 * fn(absa, absb) + 1e-30


def _rand(shape, seed):
    return torch.from_numpy(lcg_uniform(int(np.prod(shape)), seed)).reshape(shape)


SHORTCUT_CASES = [(1, 256, 512, (40, 40, 16)), (1, 512, 1024, (20, 20, 8)), (2, 128, 32, (6, 2, 10))]   # N, Cin, Cout, fine grid


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHORTCUT_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}@{'x'.join(map(str, c[3]))}")
def test_shortcut_gradients_against_float64(gpu, case):
    """1x1x1 stride-2: input gradient accumulated into the even positions of a given tensor (the odd ones untouched) and the weight
    gradient, within the bf16x3 bound of float64."""
    from mvsdet_amd import _lib, ops
    N, Cin, Cout, (D, H, W) = case
    lib = _lib.load()
    w = _rand((Cout, Cin), 1) / Cin ** 0.5
    gy = _rand((N, Cout, D // 2, H // 2, W // 2), 2)
    x = _rand((N, Cin, D, H, W), 3)
    base = _rand((N, Cin, D, H, W), 4)
    gx = Guarded((N, Cin, D, H, W), gpu, base)
    wq = ops.gemm_split_weight(w.t().contiguous().to(gpu))
    gy_d = gy.to(gpu)
    _lib.check(lib.mvsdet_conv3d_k1_s2_dx_bf16x3(_lib.ptr(gy_d), _lib.ptr(wq), gx.ptr(), N, Cin, Cout, D, H, W, _lib.current_stream(gpu)), "dx")
    torch.cuda.synchronize()
    assert gx.intact()
    got = gx.t.cpu().double()
    want = base.double().clone()
    want[:, :, ::2, ::2, ::2] += torch.einsum("oc,nov->ncv", w.double(), gy.double().reshape(N, Cout, -1)).reshape(N, Cin, D // 2, H // 2, W // 2)
    bound = base.double().abs().clone()
    bound[:, :, ::2, ::2, ::2] = _bound(w.double().abs(), gy.double().abs(),
                                        lambda a, b: torch.einsum("oc,nov->ncv", a, b.reshape(N, Cout, -1))).reshape(N, Cin, D // 2, H // 2, W // 2)
    odd = torch.ones_like(got, dtype=torch.bool)
    odd[:, :, ::2, ::2, ::2] = False
    assert torch.equal(got[odd], base.double()[odd])
    assert bool(((got - want).abs() <= bound + 2.0 ** -23 * want.abs()).all())

    for nsplit in (0, 1, 3):
        dw = ops.neck_gemm_dw_bf16x3(x.to(gpu), gy_d, False, nsplit).cpu().double().reshape(Cout, Cin)
        xs = x.double()[:, :, ::2, ::2, ::2].reshape(N, Cin, -1)
        want = torch.einsum("nov,ncv->oc", gy.double().reshape(N, Cout, -1), xs)
        bound = _bound(gy.double().abs(), xs.abs(), lambda a, b: torch.einsum("nov,ncv->oc", a.reshape(N, Cout, -1), b))
        assert bool(((dw - want).abs() <= bound).all()), nsplit


CONVT_CASES = [(1, 1024, 512, (10, 10, 4)), (1, 512, 256, (20, 20, 8)), (2, 128, 4, (3, 5, 7))]   # N, Cin, Cout, coarse grid


@pytest.mark.gpu
@pytest.mark.parametrize("case", CONVT_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}@{'x'.join(map(str, c[3]))}")
def test_transposed_gradients_against_float64(gpu, case):
    """ConvTranspose3d(k=2, s=2): input gradient (a guarded output) and weight gradient within the bf16x3 bound of float64."""
    from mvsdet_amd import _lib, ops
    N, Cin, Cout, (D, H, W) = case
    lib = _lib.load()
    w = _rand((Cin, Cout, 2, 2, 2), 5) / (8 * Cout) ** 0.5
    gy = _rand((N, Cout, 2 * D, 2 * H, 2 * W), 6)
    x = _rand((N, Cin, D, H, W), 7)
    gx = Guarded((N, Cin, D, H, W), gpu)
    wq = ops.gemm_split_weight(w.reshape(Cin, 8 * Cout).to(gpu))
    gy_d = gy.to(gpu)
    _lib.check(lib.mvsdet_convT3d_k2_s2_dx_bf16x3(_lib.ptr(gy_d), _lib.ptr(wq), gx.ptr(), N, Cin, Cout, D, H, W, _lib.current_stream(gpu)), "dx")
    torch.cuda.synchronize()
    assert gx.intact()
    want = F.conv3d(gy.double(), w.double(), stride=2)
    bound = 2.0 ** -14 * F.conv3d(gy.double().abs(), w.double().abs(), stride=2) + 1e-30
    assert bool(((gx.t.cpu().double() - want).abs() <= bound).all())

    for nsplit in (0, 1, 3):
        dw = ops.neck_gemm_dw_bf16x3(x.to(gpu), gy_d, True, nsplit).cpu().double()
        g8 = gy.double().reshape(N, Cout, D, 2, H, 2, W, 2).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, Cout, 8, -1)
        want = torch.einsum("ncv,nokv->cok", x.double().reshape(N, Cin, -1), g8).reshape(Cin, Cout, 2, 2, 2)
        bound = 2.0 ** -14 * torch.einsum("ncv,nokv->cok", x.double().abs().reshape(N, Cin, -1), g8.abs()).reshape(Cin, Cout, 2, 2, 2) + 1e-30
        assert bool(((dw - want).abs() <= bound).all()), nsplit


BN_CASES = [(1, 512, (20, 20, 8), False), (2, 3, (3, 5, 7), False), (2, 5, (2, 4, 4), True)]   # N, C, grid, statistics from parts


@pytest.mark.gpu
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: f"{c[0]}x{c[1]}@{'x'.join(map(str, c[2]))}{'-parts' if c[3] else ''}")
def test_residual_batchnorm_against_float64(gpu, case):
    """out = relu(bn(x) + residual) with batch statistics (from a pass over x, or from partial sums around a pivot) and its
    backward -- grad_x, grad_gamma, grad_beta, grad_residual = grad_out [out > 0] -- against float64 with the kernel's own ReLU
    decisions (a flip is only allowed within 1e-5 of zero); outputs inside guarded canvases."""
    from mvsdet_amd import _lib
    N, C, (D, H, W), use_parts = case
    lib = _lib.load()
    vol = D * H * W
    x = _rand((N, C, D, H, W), 8) * 2.0 + 0.5
    res = _rand((N, C, D, H, W), 9)
    gam = 1.0 + 0.25 * _rand((C,), 10)
    bet = 0.1 * _rand((C,), 11)
    gy = _rand((N, C, D, H, W), 12)
    dev = lambda t: t.to(gpu).contiguous()  # noqa: E731
    xd, rd, gd, bd, gyd = dev(x), dev(res), dev(gam), dev(bet), dev(gy)
    out, mean, invstd = Guarded(x.shape, gpu), Guarded((C,), gpu), Guarded((C,), gpu)
    wb = lib.mvsdet_bn3d_workspace_bytes(C)
    ws = torch.empty(wb // 8, dtype=torch.float64, device=gpu)
    parts = pivot = None
    if use_parts:   # four chunks per channel, sums of (x - pivot) and of its squares
        pivot = dev(0.3 * _rand((C,), 13))
        xc = (x.double() - pivot.cpu().double().view(1, C, 1, 1, 1)).transpose(0, 1).reshape(C, 4, -1)
        parts = dev(torch.stack((xc.sum(-1), (xc * xc).sum(-1)), -1))
    stream = _lib.current_stream(gpu)
    _lib.check(lib.mvsdet_bn3d_res_relu_train_fwd_f32(_lib.ptr(xd), _lib.ptr(parts), 4 if use_parts else 0, _lib.ptr(pivot), _lib.ptr(gd),
                                                      _lib.ptr(bd), _lib.ptr(rd), None, None, out.ptr(), mean.ptr(), invstd.ptr(),
                                                      _lib.ptr(ws), wb, N, C, vol, 0.0, 1e-5, 1, stream), "fwd")
    gx, ggam, gbet, gres = Guarded(x.shape, gpu), Guarded((C,), gpu), Guarded((C,), gpu), Guarded(x.shape, gpu)
    _lib.check(lib.mvsdet_bn3d_res_relu_bwd_f32(_lib.ptr(xd), out.ptr(), _lib.ptr(gyd), _lib.ptr(gd), _lib.ptr(bd), mean.ptr(), invstd.ptr(),
                                                gx.ptr(), ggam.ptr(), gbet.ptr(), gres.ptr(), _lib.ptr(ws), wb, N, C, vol, 1, stream), "bwd")
    torch.cuda.synchronize()
    assert all(t.intact() for t in (out, mean, invstd, gx, ggam, gbet, gres))

    xr = x.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True)
    m = xr.mean(dim=(0, 2, 3, 4), keepdim=True)
    v = ((xr - m) ** 2).mean(dim=(0, 2, 3, 4), keepdim=True)
    pre = (xr - m) / torch.sqrt(v + 1e-5) * g64.view(1, C, 1, 1, 1) + b64.view(1, C, 1, 1, 1) + r64
    ours = out.t.cpu()
    mask = ours > 0
    assert bool(((mask == (pre.detach() > 0)) | (pre.detach().abs() < 1e-5)).all())
    y = pre * mask.double()
    np.testing.assert_allclose(ours.double().numpy(), y.detach().numpy(), rtol=0, atol=2e-5 * max(1.0, float(y.detach().abs().max())))
    np.testing.assert_allclose(mean.t.cpu().double().numpy(), m.detach().reshape(-1).numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(invstd.t.cpu().double().numpy(), (1 / torch.sqrt(v + 1e-5)).detach().reshape(-1).numpy(), rtol=1e-5)
    (y * gy.double()).sum().backward()
    for name, got, want in (("grad_x", gx.t, xr.grad), ("grad_gamma", ggam.t, g64.grad), ("grad_beta", gbet.t, b64.grad),
                            ("grad_residual", gres.t, r64.grad)):
        want = want.numpy()
        np.testing.assert_allclose(got.cpu().double().numpy(), want, rtol=0, atol=2e-5 * max(1.0, float(np.abs(want).max())), err_msg=name)
