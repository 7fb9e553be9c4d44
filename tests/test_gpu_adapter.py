"""The Gaussian adapter on the GPU (csrc/adapter.hip through ops.adapter, functional.pixel_gaussians, MVSDetHotPath.render_source_ids /
nvs_loss) against the float64 restatement of tests/adapter_restated.py, against fixture G27 (the reference's own
GaussianAdapter.forward, tests/golden/make_goldens_g27.py) and, chained with the rasteriser, against both restatements chained
(tests/adapter_scene.py).

Shapes: 5 x 7 = 35 pixels (tail lanes; two views inside what would be one wave) and 3 x 43 = 129 pixels (crosses the 64-Gaussian block
and a 128-thread boundary), V in {1, 2, 3}, S in {1, 2}, every d_sh.  Bars: elementwise max(1e-4 |x| + 1.25e-6 max|x|, 4 x the float32
restatement's own largest distance from float64) -- the rule of DESIGN 4.12; G27: 4 x the stored own distance or that bar, whichever is
larger; the composition: 4 x the chain's own float32-float64 distance.  Every test prints its figures before it asserts (pytest -s);
the measured ones are in DESIGN.md 4.16.
"""
import numpy as np
import pytest
import torch

import adapter_restated as A
import adapter_scene as AS
from canvas import Guarded, guarded_f32
from conftest import load_golden

pytestmark = pytest.mark.gpu

# name -> (V, h, w, S, d_sh)
CASES = {
    "v1_5x7_s1_sh1": (1, 5, 7, 1, 1),
    "v2_5x7_s2_sh4": (2, 5, 7, 2, 4),
    "v3_5x7_s1_sh9": (3, 5, 7, 1, 9),
    "v2_3x43_s1_sh16": (2, 3, 43, 1, 16),
    "v3_3x43_s2_sh25": (3, 3, 43, 2, 25),
    "v2_5x7_s1_sh25": (2, 5, 7, 1, 25),
    "v1_3x43_s2_sh1": (1, 3, 43, 2, 1),
}
_CACHE = {}


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def reference(name, sh_rot=None):
    """Computed once per case and shared, unchanged: the case, its blocks (the float64 builder's unless given), the weights of the
    linear loss and both restatements with their gradients."""
    key = (name, sh_rot is None)
    if key not in _CACHE:
        V, h, w, S, d_sh = CASES[name]
        c = A.case(100 + list(CASES).index(name), V, h, w, S, d_sh)
        blocks = A.sh_rotation_blocks(c["extrinsics"][:, :3, :3], d_sh) if sh_rot is None else sh_rot
        G = V * h * w * S
        weights = A.loss_weights(c["seed"], dict(means=(G, 3), covariances=(G, 3, 3), harmonics=(G, 3, d_sh)))
        o64, g64 = A.restate(c, blocks, torch.float64, weights)
        o32, g32 = A.restate(c, blocks.astype(np.float32), torch.float32, weights)
        _CACHE[key] = (c, blocks, weights, o64, g64, o32, g32)
    return _CACHE[key]


def compare(tag, got, x64, x32, extra=0.0):
    """got against the float64 value under the bar (never under `extra`); prints the figures first; returns the worst err / bar."""
    x64, x32 = np.asarray(x64, np.float64), np.asarray(x32, np.float64)
    bar, own = A.bar(x64, x32)
    bar = np.maximum(bar, extra)
    err = np.abs(np.asarray(got, np.float64) - x64)
    worst = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    print(f"{tag}: max|x| {np.abs(x64).max():.4g}  kernel-f64 {err.max():.3g}  restated f32-f64 {own:.3g}  worst err/bar {worst:.3f}")
    assert np.isfinite(got).all(), tag
    assert (err <= bar).all(), (tag, worst)
    return worst


def run(c, gpu, weights=None, sh_rot=None, with_scales=False, raw=None):
    """ops.adapter on a case -> (outputs as numpy dict, [g_raw, g_depth] or None)."""
    from mvsdet_amd.ops import adapter
    L = A.degree_of(c["d_sh"])
    cams = adapter.adapter_cameras(dev(c["extrinsics"], gpu), dev(c["intrinsics"], gpu), c["h"], c["w"], L,
                                   None if sh_rot is None else dev(np.asarray(sh_rot, np.float32), gpu))
    raw = (dev(c["raw"], gpu) if raw is None else raw).detach().requires_grad_(weights is not None)
    depth = dev(c["depth"], gpu).requires_grad_(weights is not None)
    out = adapter.pixel_gaussians(raw, depth, cams, c["h"], c["w"], c["s_min"], c["s_max"], L, with_scales)
    names = A.FIELDS + (("scales", "rotations") if with_scales else ())
    grads = None
    if weights is not None:
        loss = sum((o * dev(weights[k], gpu)).sum() for k, o in zip(A.FIELDS, out))
        grads = [g.cpu().numpy() for g in torch.autograd.grad(loss, [raw, depth])]
    return {k: o.detach().cpu().numpy() for k, o in zip(names, out)}, grads


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_against_the_restatement(gpu, name):
    """The whole path with the default rotation builder (cameras kernel) against the restatement with its own float64 builder: the
    fields, scales and rotations, and the gradients of a seeded random linear loss in raw and depth."""
    c, blocks, weights, o64, g64, o32, g32 = reference(name)
    out, grads = run(c, gpu, weights, with_scales=True)
    worst = [compare(f"{name} {k}", out[k], o64[k], o32[k]) for k in A.FIELDS + ("scales", "rotations")]
    worst += [compare(f"{name} d {k}", g, a, b) for k, g, a, b in zip(("raw", "depth"), grads, g64, g32)]
    print(f"{name}: worst ratio to the bar {max(worst):.3f}")
    assert tuple(out["means"].shape) == (c["V"] * c["h"] * c["w"] * c["S"], 3)


def test_g27_with_identity_blocks(gpu):
    """The reference's own GaussianAdapter.forward (its rotate_sh replaced by the identity) against the kernel run with identity blocks."""
    g = load_golden("g27_adapter")
    for tag in [str(t) for t in g["cases"]]:
        V, h, w, S, d_sh = (int(v) for v in g[tag + ".shape"])
        c = dict(V=V, h=h, w=w, S=S, d_sh=d_sh, s_min=float(g[tag + ".scale_range"][0]), s_max=float(g[tag + ".scale_range"][1]),
                 **{k: g[f"{tag}.in_{k}"] for k in ("extrinsics", "intrinsics", "raw", "depth", "opacity")})
        L = A.degree_of(d_sh)
        identity = np.zeros((V, A.ROT_OFF[L + 1]))
        for l in range(L + 1):
            identity[:, A.ROT_OFF[l]:A.ROT_OFF[l + 1]] = np.eye(2 * l + 1).reshape(-1)
        out, _ = run(c, gpu, None, sh_rot=identity, with_scales=True)
        o64, _ = A.restate(c, identity, torch.float64)
        o32, _ = A.restate(c, identity.astype(np.float32), torch.float32)
        for name in ("means", "covariances", "harmonics", "scales", "rotations"):
            want = g[f"{tag}.{name}"].astype(np.float64)
            bar = np.maximum(A.bar(o64[name], o32[name])[0], 4.0 * float(g[f"{tag}.own_{name}"]))
            err = np.abs(out[name].astype(np.float64) - want)
            print(f"{tag} {name}: kernel-reference {err.max():.3g}  stored own {float(g[f'{tag}.own_{name}']):.3g}  worst err/bar {float((err / bar).max()):.3f}")
            assert (err <= bar).all(), (tag, name)


def random_orthogonal_blocks(seed, V, d_sh):
    rng = np.random.RandomState(seed)
    L = A.degree_of(d_sh)
    out = np.zeros((V, A.ROT_OFF[L + 1]))
    for v in range(V):
        for l in range(L + 1):
            q, _ = np.linalg.qr(rng.normal(size=(2 * l + 1, 2 * l + 1)))
            out[v, A.ROT_OFF[l]:A.ROT_OFF[l + 1]] = q.reshape(-1)
    return out.astype(np.float32).astype(np.float64)       # the values the kernel is handed


@pytest.mark.parametrize("name", ["v2_5x7_s2_sh4", "v3_3x43_s2_sh25"])
def test_supplied_rotation_blocks_are_applied_as_given(gpu, name):
    V, h, w, S, d_sh = CASES[name]
    blocks = random_orthogonal_blocks(61, V, d_sh)
    c, _, weights, o64, g64, o32, g32 = reference(name, blocks)
    out, grads = run(c, gpu, weights, sh_rot=blocks)
    compare(f"{name} harmonics", out["harmonics"], o64["harmonics"], o32["harmonics"])
    compare(f"{name} d raw", grads[0], g64[0], g32[0])
    default, _, _, d64, _, _, _ = reference(name)
    assert np.abs(d64["harmonics"] - o64["harmonics"]).max() > 1e-3      # not the default rotation


def test_default_builder_against_the_float64_builder(gpu):
    """The D_l blocks the cameras kernel builds from csrc/sh_basis.h, C_v, the origin, K^-1 and the multiplier against float64."""
    from mvsdet_amd.ops import adapter
    c, blocks, _, _, _, _, _ = reference("v3_3x43_s2_sh25")
    cams = adapter.adapter_cameras(dev(c["extrinsics"], gpu), dev(c["intrinsics"], gpu), c["h"], c["w"], 4).cpu().numpy()
    compare("blocks", cams[:, adapter.ADAPTER_ROT:adapter.ADAPTER_ROT + 165], blocks, blocks.astype(np.float32))
    E, K = c["extrinsics"].astype(np.float64), c["intrinsics"].astype(np.float64)
    assert np.array_equal(cams[:, :9], c["extrinsics"][:, :3, :3].reshape(-1, 9)) and np.array_equal(cams[:, 9:12], c["extrinsics"][:, :3, 3])
    Ki = np.linalg.inv(K).reshape(-1, 9)
    compare("K^-1", cams[:, 12:21], Ki, Ki.astype(np.float32))
    m = 0.1 * (np.linalg.inv(K[:, :2, :2]) @ np.array([1.0 / c["w"], 1.0 / c["h"]])).sum(-1)
    compare("multiplier", cams[:, 21], m, m.astype(np.float32))
    assert np.array_equal(cams[:, 189:], np.zeros((3, 3), np.float32))
    # a lower degree leaves the higher blocks zero
    low = adapter.adapter_cameras(dev(c["extrinsics"], gpu), dev(c["intrinsics"], gpu), c["h"], c["w"], 1).cpu().numpy()
    assert np.array_equal(bits(low[:, 24:34]), bits(cams[:, 24:34])) and not low[:, 34:].any()
    assert E.shape == (3, 4, 4)


def test_raw_as_a_slice_of_a_wider_guarded_buffer(gpu):
    """raw and g_raw as slices of wider rows inside sentinel canvases, every output between guards: the same bits as the contiguous
    call, the columns beside the rows and the guards untouched."""
    from mvsdet_amd.ops import adapter
    name = "v3_3x43_s2_sh25"
    c, _, weights, _, _, _, _ = reference(name)
    V, h, w, S, d_sh = CASES[name]
    R, C, G = h * w, 9 + 3 * d_sh, V * h * w * S
    plain, grads = run(c, gpu, weights)
    wide, lead = C + 7, 3
    src = Guarded(V * R * S * wide, gpu)
    src.region.fill_(0x7FC00000)                                   # NaN beside the rows: a stray read shows
    raw = src.region.view(torch.float32).view(V, R, S, wide)[..., lead:lead + C]
    raw.copy_(dev(c["raw"], gpu))
    assert not raw.is_contiguous()
    cams = adapter.adapter_cameras(dev(c["extrinsics"], gpu), dev(c["intrinsics"], gpu), h, w, 4)
    depth = dev(c["depth"], gpu)
    outs = [guarded_f32(s, gpu) for s in ((G, 3), (G, 3, 3), (G, 3, d_sh), (G, 3), (G, 4))]
    adapter.forward_into(raw, depth, cams, h, w, c["s_min"], c["s_max"], 4, *[t for _, t in outs])
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g, _ in outs) and src.guards_intact()
    for k, (_, t) in zip(A.FIELDS, outs):
        assert np.array_equal(bits(t), bits(plain[k])), k
    dst = Guarded(V * R * S * wide, gpu)
    g_raw = dst.region.view(torch.float32).view(V, R, S, wide)[..., lead:lead + C]
    gd_guard, g_depth = guarded_f32((V, R, S), gpu)
    adapter.backward_into(raw, depth, cams, *[dev(weights[k], gpu) for k in A.FIELDS], h, w, c["s_min"], c["s_max"], 4, g_raw, g_depth)
    torch.cuda.synchronize()
    assert dst.guards_intact() and gd_guard.guards_intact() and src.guards_intact()
    assert np.array_equal(bits(g_raw), bits(grads[0]))
    assert np.array_equal(bits(g_depth.sum(2)), bits(grads[1]))
    beside = dst.region.view(V, R, S, wide)
    assert not beside[..., :lead].any() and not beside[..., lead + C:].any()      # zeroed by Guarded, never written


def test_covariance_gradient_as_upper_triangle_and_as_a_full_matrix(gpu):
    """g_covariances with the lower triangle zero (what the rasteriser sends) and as a full asymmetric 3x3: both are the restatement's
    autograd for that weight."""
    name = "v2_5x7_s1_sh25"
    c, blocks, weights, _, _, _, _ = reference(name)
    for kind in ("upper", "full"):
        wts = dict(weights)
        wts["covariances"] = np.triu(weights["covariances"]) if kind == "upper" else weights["covariances"]
        assert kind == "upper" or np.abs(wts["covariances"] - wts["covariances"].transpose(0, 2, 1)).max() > 0.1
        _, g64 = A.restate(c, blocks, torch.float64, wts)
        _, g32 = A.restate(c, blocks.astype(np.float32), torch.float32, wts)
        _, grads = run(c, gpu, wts)
        compare(f"{kind} d raw", grads[0], g64[0], g32[0])
        compare(f"{kind} d depth", grads[1], g64[1], g32[1])


def test_two_runs_give_the_same_bits(gpu):
    c, _, weights, _, _, _, _ = reference("v3_3x43_s2_sh25")
    a, ga = run(c, gpu, weights, with_scales=True)
    b, gb = run(c, gpu, weights, with_scales=True)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for x, y in zip(ga, gb):
        assert np.array_equal(bits(x), bits(y))


def test_fake_kernels_and_refusals(gpu):
    from mvsdet_amd.ops import adapter
    c, _, _, _, _, _, _ = reference("v2_5x7_s2_sh4")
    V, h, w, S, d_sh = CASES["v2_5x7_s2_sh4"]
    G = V * h * w * S
    ext, K, raw, depth = (dev(c[k], gpu) for k in ("extrinsics", "intrinsics", "raw", "depth"))
    cams = adapter.adapter_cameras(ext, K, h, w, 1)
    torch.library.opcheck(torch.ops.mvsdet_amd.adapter_cameras.default, (ext, K, h, w, 1, None), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.mvsdet_amd.adapter_pixel_gaussians.default, (raw, depth, cams, h, w, 0.5, 15.0, 1, True),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.mvsdet_amd.adapter_pixel_gaussians_backward.default,
                          (raw, depth, cams, torch.ones(G, 3, device=gpu), None, torch.ones(G, 3, d_sh, device=gpu), h, w, 0.5, 15.0, 1),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError, match="sh_degree"):
        adapter.adapter_cameras(ext, K, h, w, 5)
    with pytest.raises(ValueError, match="sh_rot"):
        adapter.adapter_cameras(ext, K, h, w, 1, torch.zeros(V, 9, device=gpu))
    with pytest.raises(ValueError, match="raw"):
        adapter.pixel_gaussians(raw[..., :20], depth, cams, h, w, 0.5, 15.0, 1)
    with pytest.raises(ValueError, match="raw"):
        adapter.pixel_gaussians(raw, depth, cams, h + 1, w, 0.5, 15.0, 1)
    with pytest.raises(TypeError, match="float32"):
        adapter.pixel_gaussians(raw.double(), depth, cams, h, w, 0.5, 15.0, 1)
    with pytest.raises(RuntimeError, match="no gradient"):
        adapter.pixel_gaussians(raw, depth, cams.clone().requires_grad_(True), h, w, 0.5, 15.0, 1)
    # the C entry points refuse before any launch
    from mvsdet_amd import _lib
    lib = _lib.load()
    assert lib.mvsdet_adapter_forward_f32(None, 0, 21, None, None, None, None, None, None, None, V, h, w, S, d_sh, 0.5, 15.0, None) == 1
    one = _lib.ptr(raw)
    assert lib.mvsdet_adapter_forward_f32(one, 0, 21, one, one, one, one, one, None, None, V, h, w, S, 5, 0.5, 15.0, None) == 1
    assert b"d_sh" in lib.mvsdet_last_error()
    assert lib.mvsdet_adapter_forward_f32(one, 0, 20, one, one, one, one, one, None, None, V, h, w, S, d_sh, 0.5, 15.0, None) == 1
    assert lib.mvsdet_adapter_forward_f32(one, 0, 21, one, one, one, one, one, None, None, 65536, h, w, S, d_sh, 0.5, 15.0, None) == 1
    assert lib.mvsdet_adapter_backward_f32(one, 0, 21, one, one, None, None, None, one, 0, 21, one, V, 1 << 15, 1 << 15, 2, 25, 0.5, 15.0, None) == 1
    assert b"limits" in lib.mvsdet_last_error()
    # under autocast low-precision inputs are computed in float32
    plain = adapter.pixel_gaussians(raw.half().float(), depth, cams, h, w, 0.5, 15.0, 1)
    with torch.autocast("cuda", dtype=torch.float16):
        amp = adapter.pixel_gaussians(raw.half(), depth, cams, h, w, 0.5, 15.0, 1)
    assert all(t.dtype == torch.float32 and np.array_equal(bits(t), bits(p)) for t, p in zip(amp, plain))


def test_no_host_synchronisation(gpu):
    from mvsdet_amd import functional as F_
    c, _, weights, _, _, _, _ = reference("v2_5x7_s1_sh25")
    args = [dev(c[k], gpu) for k in ("extrinsics", "intrinsics")]
    raw, depth, opac = (dev(c[k], gpu).requires_grad_(True) for k in ("raw", "depth", "opacity"))
    wd = dev(weights["harmonics"], gpu)

    def step():
        g = F_.pixel_gaussians(*args, raw, depth, opac, (c["h"], c["w"]), 0.5, 15.0, 4)
        ((g.harmonics[0] * wd).sum() + g.means.sum() + g.covariances.sum() + g.opacities.sum()).backward()
        return g
    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        g = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert tuple(g.opacities.shape) == (1, 70) and torch.isfinite(raw.grad).all()


def test_composition_with_the_rasteriser_and_the_nvs_loss(gpu):
    """functional.pixel_gaussians -> functional.decode_splatting -> nvs_loss on 2 source views and 1 target: the loss and its gradients
    in raw, depth and opacity against both restatements chained in float64.  Bar: 4 x the chain's own float32-float64 distance."""
    from mvsdet_amd import functional as F_
    from mvsdet_amd.hotpath import MVSDetHotPath
    ref = AS.composition_reference()
    c, tgt = ref["case"], ref["tgt"]
    raw, depth, opac = (dev(c[k], gpu).requires_grad_(True) for k in ("raw", "depth", "opacity"))
    g = F_.pixel_gaussians(dev(c["extrinsics"], gpu), dev(c["intrinsics"], gpu), raw, depth, opac, (c["h"], c["w"]), c["s_min"], c["s_max"],
                           A.degree_of(c["d_sh"]))
    colour = F_.decode_splatting(g, dev(tgt["tgt_extrinsics"], gpu)[None], dev(tgt["tgt_intrinsics"], gpu)[None], dev(tgt["near"], gpu)[None],
                                 dev(tgt["far"], gpu)[None], (AS.H, AS.W), dev(tgt["bg"], gpu))
    assert tuple(colour.shape) == (1, 1, 3, AS.H, AS.W)
    mask = dev(ref["kept"][:, None].astype(np.float32), gpu)
    hot = MVSDetHotPath.__new__(MVSDetHotPath)                     # nvs_loss keeps no state
    loss = hot.nvs_loss([colour * mask], [dev(tgt["gt"], gpu) * mask])["loss_nvs"]
    grads = [t.cpu().numpy() for t in torch.autograd.grad(loss, [raw, depth, opac])]
    own = abs(ref["loss32"] - ref["loss64"])
    err = abs(float(loss.detach()) - ref["loss64"])
    print(f"loss {float(loss.detach()):.9g}  float64 {ref['loss64']:.9g}  kernel-f64 {err:.3g}  chain f32-f64 {own:.3g}  ratio {err / (4 * own) if own else float('inf'):.3f}")
    worst = []
    for k, got, g64, g32 in zip(("raw", "depth", "opacity"), grads, ref["grads64"], ref["grads32"]):
        own_k = float(np.abs(g32.astype(np.float64) - g64).max())
        err_k = float(np.abs(got.astype(np.float64) - g64).max())
        worst.append(err_k / (4 * own_k))
        print(f"d loss / d {k}: max|x| {np.abs(g64).max():.3g}  kernel-f64 {err_k:.3g}  chain f32-f64 {own_k:.3g}  ratio {worst[-1]:.3f}")
    assert err <= 4 * own
    assert max(worst) <= 1.0


def test_render_source_ids_equal_the_reference_sequence(gpu):
    """Seeded poses with distinct distances: the 3 nearest sources of every target, unique and ascending, as get_nearest_pose_ids +
    torch.unique give them on the CPU."""
    from mvsdet_amd import functional as F_
    from mvsdet_amd.hotpath import MVSDetHotPath
    rng = np.random.RandomState(10)          # a seed whose 48 distances are at least 1e-3 apart (asserted below)
    n = 12
    c2w = np.tile(np.eye(4), (n, 1, 1))
    c2w[:, :3, 3] = rng.uniform(-3, 3, (n, 3))
    tgt = np.tile(np.eye(4), (4, 1, 1))
    tgt[:, :3, 3] = rng.uniform(-3, 3, (4, 3))
    dist = np.linalg.norm(tgt[:, None, :3, 3] - c2w[None, :, :3, 3], axis=-1)
    assert np.diff(np.sort(dist, axis=1), axis=1).min() > 1e-3
    meta = dict(lidar2img=dict(extrinsic=[np.linalg.inv(m) for m in c2w], intrinsic=np.eye(4)), ori_shape=(480, 640), img_shape=(240, 320))
    hot = MVSDetHotPath.__new__(MVSDetHotPath)
    hot.stride = 4
    got = hot.render_source_ids(meta, tgt, 3)
    src = torch.tensor(np.array(meta["lidar2img"]["extrinsic"])).inverse()
    want = torch.unique(F_.get_nearest_pose_ids(torch.tensor(tgt), src, num_select=3, maskself=False).view(-1))
    assert got.dtype == torch.int64 and not got.is_cuda and torch.equal(got, want)
    assert want.tolist() == sorted(set(np.argsort(dist, axis=1)[:, :3].reshape(-1).tolist()))
    assert 3 <= len(want) <= 12


def test_novel_views_is_the_glue_of_the_nvs_branch(gpu):
    """MVSDetHotPath.novel_views on a 4-view scene of 5 x 8 feature pixels (stride 4, one shared K) against the same steps spelled
    out here from mvsdet.py:543-583, 645-662 on functional.pixel_gaussians / decode_splatting: the same bits; the gradient of the
    NVS loss reaches the feature, the layer's weight, depth_coding and the opacity."""
    from types import SimpleNamespace
    from mvsdet_amd import functional as F_
    from mvsdet_amd import synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, hw, L = 4, 8, (6, 8), 1
    meta = synthetic.make_img_meta(N, hw, seed=5)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    assert (h, w) == (5, 8)
    gen = torch.Generator().manual_seed(3)
    feature = torch.randn(N, C, *hw, generator=gen).to(gpu).requires_grad_(True)
    depth_coding = (1.0 + 2.0 * torch.rand(N, 1, h, w, generator=gen)).to(gpu).requires_grad_(True)
    opacity = torch.rand(N, *hw, generator=gen).to(gpu).requires_grad_(True)
    rgb_raw = torch.rand(1, N, h * w, 3, generator=gen).to(gpu)
    outputs = dict(geometry=SimpleNamespace(height=h, width=w), depth_coding=depth_coding, opacity=opacity)
    torch.manual_seed(4)
    to_gaussians = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(C + 1 + 3, 2 + 7 + 3 * (L + 1) ** 2)).to(gpu)
    w2c = np.array(meta["lidar2img"]["extrinsic"], np.float64)
    c2w = np.linalg.inv(w2c)
    tgt = c2w[[0, 2]].copy()
    tgt[:, :3, 3] += 0.05
    Kt = np.array([[40.0, 0, 16.0, 0], [0, 40.0, 12.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    src_id = hp.render_source_ids(meta, tgt, 3)
    assert src_id.numel() == N                 # every view is among the 3 nearest of one of the two targets here, so rgb_raw fits
    colour = hp.novel_views(outputs, feature, meta, to_gaussians, tgt, Kt, (24, 32, 3), rgb_raw, sh_degree=L)
    assert tuple(colour.shape) == (1, 2, 3, 24, 32) and bool(torch.isfinite(colour).all()) and float(colour.detach().abs().max()) > 0
    gt = torch.rand(2, 3, 24, 32, generator=gen).to(gpu)
    loss = hp.nvs_loss(colour, gt)["loss_nvs"]
    grads = torch.autograd.grad(loss, [feature, to_gaussians[1].weight, depth_coding, opacity])
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    # the same steps, spelled out
    with torch.no_grad():
        ids = src_id.to(gpu)
        rows = torch.cat([feature[ids][:, :, :h, :w].reshape(N, C, h * w).transpose(1, 2), depth_coding[ids].reshape(N, h * w, 1), rgb_raw[0]], -1)
        raw = to_gaussians(rows).reshape(N, h * w, 1, -1)
        src_w2c, K_feat = hp._feature_cameras(meta)
        K = K_feat.clone().float()
        K[0] /= w
        K[1] /= h
        K = K[None, :3, :3].repeat(N, 1, 1).to(gpu)
        scale, _ = hp.ray_depth(meta, torch.ones(N, 1, *hw, device=gpu))
        ray = (depth_coding.reshape(N, h * w, 1) / (scale + 1e-8))[ids].reshape(N, h * w)
        g = F_.pixel_gaussians(src_w2c.inverse().float()[src_id].to(gpu), K, raw, ray, opacity[ids][:, :h, :w].reshape(N, h * w),
                               (h, w), 0.5, 15.0, L)
        Ktn = torch.tensor(Kt).float()[None].repeat(2, 1, 1)
        Ktn[:, 0] /= 32
        Ktn[:, 1] /= 24
        want = F_.decode_splatting(g, torch.tensor(tgt).float()[None].to(gpu), Ktn[None, :, :3, :3].to(gpu), torch.full((1, 2), 0.2, device=gpu),
                                   torch.full((1, 2), 5.0, device=gpu), (24, 32))
    assert np.array_equal(bits(colour), bits(want))
