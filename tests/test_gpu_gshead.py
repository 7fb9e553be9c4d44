"""The Gaussian head on the GPU (csrc/gshead.hip through ops.gshead, functional.gaussian_head / process_rgb_raw and
MVSDetHotPath.novel_views(gaussian_head="hip")) against the float64 restatement of tests/gshead_restated.py and against fixture G29
(tests/golden/make_goldens_g29.py).

Shapes: the smallest at which the kernel can go wrong -- 35 pixels (under one 32-pixel wave tile + 3) and 129 (a 128-pixel block + 1),
K + 1 = 10, 35, 45 (odd: a lone last k of an MFMA pair), 261 (a ninth 32-k stage of 5), M = 12 (under one row tile), 21 (odd: rows that
are not 16-byte aligned), 42, 84 and 168 (two 96-row groups).  Bars: elementwise max(1e-4 |x| + 1.25e-6 max|x|, 4 x the float32
restatement's own largest distance from float64) -- the rule of DESIGN 4.12; G29: 4 x the stored own distance or that bar, whichever is
larger.  Every test prints its figures before it asserts (pytest -s); the measured ones are in DESIGN.md 4.19.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adapter_restated as A
import gshead_restated as G
from canvas import guarded_f32, nan_view
from conftest import load_golden

pytestmark = pytest.mark.gpu

# name -> (N, ids, C, Hf, Wf, h, w, S, d_sh, rgb, dims of depth_coding)
CASES = {
    "a": (3, [0, 2], 8, 6, 9, 5, 7, 1, 1, None, 4),
    "b": (4, [1, 2, 3], 40, 6, 9, 5, 7, 2, 4, "rows", 4),
    "c": (2, [0, 1], 256, 4, 43, 3, 43, 1, 25, "images", 4),
    "d": (6, [0, 3, 5], 33, 3, 43, 3, 43, 1, 4, None, 3),
    "e": (1, [0], 256, 6, 9, 5, 7, 2, 25, "images", 4),
}
_CACHE = {}


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def reference(name):
    """Computed once per case and shared, unchanged: the case and both restatements with their gradients."""
    if name not in _CACHE:
        c = G.case(290 + list(CASES).index(name), *CASES[name])
        o64, g64 = G.restate(c, torch.float64)
        o32, g32 = G.restate(c, torch.float32)
        _CACHE[name] = (c, o64, g64, o32, g32)
    return _CACHE[name]


def compare(tag, got, x64, x32, extra=0.0):
    """got against the float64 value under the bar; prints the figures first; returns the worst err / bar."""
    x64, x32 = np.asarray(x64, np.float64), np.asarray(x32, np.float64)
    bar, own = G.bar(x64, x32)
    bar = np.maximum(bar, extra)
    err = np.abs(np.asarray(got, np.float64) - x64)
    worst = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    print(f"{tag}: max|x| {np.abs(x64).max():.4g}  kernel-f64 {err.max():.3g}  restated f32-f64 {own:.3g}  worst err/bar {worst:.3f}")
    assert np.isfinite(got).all(), tag
    assert (err <= bar).all(), (tag, worst)
    return worst


def run(c, gpu, grads=True, chunk_pixels=0, feature=None):
    """ops.gshead.gaussian_head on a case -> (raw as numpy, dict of the four gradients of sum(raw * loss_weight) or None)."""
    from mvsdet_amd.ops import gshead
    leaves = {k: dev(c[k], gpu).requires_grad_(grads) for k in G.GRADS}
    if feature is not None:
        leaves["feature"] = feature.detach().requires_grad_(grads)
    out = gshead.gaussian_head(leaves["feature"], leaves["depth_coding"], dev(c["ids"], gpu), leaves["weight"], leaves["bias"], c["h"], c["w"],
                               c["S"], dev(c["rgb_raw"], gpu) if "rgb_raw" in c else None, dev(c["images"], gpu) if "images" in c else None,
                               chunk_pixels)
    got = None
    if grads:
        lw = dev(G.loss_weight(c["seed"], tuple(out.shape)), gpu)
        got = dict(zip(G.GRADS, [g.cpu().numpy() for g in torch.autograd.grad((out * lw).sum(), [leaves[k] for k in G.GRADS])]))
    return out.detach().cpu().numpy(), got


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_against_the_restatement(gpu, name):
    c, o64, g64, o32, g32 = reference(name)
    out, grads = run(c, gpu)
    assert out.shape == (len(c["ids"]), c["h"] * c["w"], c["S"], c["M"] // c["S"])
    worst = [compare(f"{name} raw", out, o64, o32)]
    worst += [compare(f"{name} d {k}", grads[k], g64[k], g32[k]) for k in G.GRADS]
    print(f"{name}: worst ratio to the bar {max(worst):.3f}")
    assert grads["feature"].shape == c["feature"].shape and grads["depth_coding"].shape == c["depth_coding"].shape


def test_g29(gpu):
    """The reference's process_rgb_raw and the restated lines of extract_feat, run by make_goldens_g29.py, against the kernel."""
    from mvsdet_amd import functional as F_
    g = load_golden("g29_gshead")
    N, C, Hf, Wf, h, w = (int(v) for v in g["shape"])
    for tag in [str(t) for t in g["cases"]]:
        S, d_sh, rgb, seed = (int(v) for v in g[tag + ".meta"])
        c = dict(ids=g["ids"], h=h, w=w, S=S, seed=seed, feature=g["in_feature"], depth_coding=g["in_depth_coding"], weight=g[tag + ".weight"],
                 bias=g[tag + ".bias"])
        if rgb:
            c["images"] = g["in_images"]
        o64, g64 = G.restate(c, torch.float64)
        o32, g32 = G.restate(c, torch.float32)
        leaves = {k: dev(c[k], gpu).requires_grad_(True) for k in G.GRADS}
        out = F_.gaussian_head(leaves["feature"], leaves["depth_coding"], leaves["weight"], leaves["bias"], c["ids"].tolist(), h, w, S,
                               denorm_images=dev(c["images"], gpu) if rgb else None)
        lw = dev(G.loss_weight(seed, tuple(out.shape)), gpu)
        grads = torch.autograd.grad((out * lw).sum(), [leaves[k] for k in G.GRADS])
        got = dict(raw=out.detach().cpu().numpy(), **{"g_" + k: t.cpu().numpy() for k, t in zip(G.GRADS, grads)})
        want = dict(raw=(o64, o32), **{"g_" + k: (g64[k], g32[k]) for k in G.GRADS})
        for name, val in got.items():
            ref = g[f"{tag}.{name}"].astype(np.float64)
            bar = np.maximum(G.bar(*want[name])[0], 4.0 * float(g[f"{tag}.own_{name}"]))
            err = np.abs(val.astype(np.float64) - ref)
            print(f"{tag} {name}: kernel-reference {err.max():.3g}  stored own {float(g[f'{tag}.own_{name}']):.3g}  worst err/bar {float((err / bar).max()):.3f}")
            assert (err <= bar).all(), (tag, name)
        if rgb:
            rows = F_.process_rgb_raw(dev(c["images"], gpu), 4, h, w, c["ids"].tolist())
            assert tuple(rows.shape) == (1, len(c["ids"]), h * w, 3)
            ids = torch.from_numpy(c["ids"])
            r64 = G.process_rgb_raw(torch.from_numpy(c["images"]).double(), ids, h, w).numpy()
            r32 = G.process_rgb_raw(torch.from_numpy(c["images"]), ids, h, w).numpy()
            bar = np.maximum(G.bar(r64, r32)[0], 4.0 * float(g[tag + ".own_rgb_rows"]))
            assert (np.abs(rows[0].cpu().numpy().astype(np.float64) - g[tag + ".rgb_rows"]) <= bar).all(), tag


@pytest.mark.parametrize("name", ["b", "c"])
def test_guarded_output_and_feature_inside_a_nan_canvas(gpu, name):
    """raw through forward_into between sentinels; feature as a pitched view inside a NaN canvas (a read outside the map's rows
    would show as NaN); the gradients through backward_into into guarded, zeroed buffers: the same bits as the plain call, the guards
    intact, g_feature bit-zero in the unselected views and in the cropped-away rows and columns."""
    from mvsdet_amd.ops import gshead
    c, _, _, _, _ = reference(name)
    V, R, M, K = len(c["ids"]), c["h"] * c["w"], c["M"], c["K"]
    plain, grads = run(c, gpu)
    canvas, view = nan_view(torch.from_numpy(c["feature"])[:, :, None], gpu)
    feature = view[:, :, 0]
    assert feature.stride(2) > feature.shape[3] and not feature.is_contiguous()
    # the cropped-away rows and columns are NaN too here: nothing may read them
    feature[:, :, c["h"]:] = float("nan")
    feature[:, :, :, c["w"]:] = float("nan")
    depth, ids, weight, bias = (dev(c[k], gpu) for k in ("depth_coding", "ids", "weight", "bias"))
    rgb = dict(rgb_raw=dev(c["rgb_raw"], gpu)) if "rgb_raw" in c else dict(images=dev(c["images"], gpu))
    guard, raw = guarded_f32((V, R, M), gpu)
    gshead.forward_into(feature, depth, ids, weight, bias, c["h"], c["w"], raw, **rgb)
    torch.cuda.synchronize()
    assert guard.guards_intact()
    assert np.array_equal(bits(raw), bits(plain.reshape(V, R, M)))
    lw = dev(G.loss_weight(c["seed"], plain.shape), gpu)
    gf_guard, g_feature = guarded_f32(c["feature"].shape, gpu)
    gd_guard, g_depth = guarded_f32(c["depth_coding"].shape, gpu)
    gw_guard, g_weight = guarded_f32((M, K), gpu)
    gb_guard, g_bias = guarded_f32((M,), gpu)
    need = gshead.partial_floats(V, R, M, K)
    p_guard, partial = guarded_f32((need,), gpu)
    gshead.backward_into(feature, depth, ids, weight, lw, c["h"], c["w"], g_feature, g_depth, g_weight, g_bias, partial=partial, **rgb)
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in (gf_guard, gd_guard, gw_guard, gb_guard, p_guard))
    for k, t in zip(G.GRADS, (g_feature, g_depth, g_weight, g_bias)):
        assert np.array_equal(bits(t), bits(grads[k])), k
    rest = [n for n in range(c["N"]) if n not in list(c["ids"])]
    for gf in (bits(g_feature), bits(grads["feature"])):
        assert not gf[rest].any() and not gf[:, :, c["h"]:].any() and not gf[:, :, :, c["w"]:].any()


def test_unselected_views_and_the_crop_get_a_bit_zero_gradient(gpu):
    """Case a has an unselected view (1) and a cropped-away row and two columns; case d selects 3 of 6 views and crops nothing."""
    for name in ("a", "d"):
        c, _, _, _, _ = reference(name)
        _, grads = run(c, gpu)
        gf, gd = bits(grads["feature"]), bits(grads["depth_coding"])
        rest = [n for n in range(c["N"]) if n not in list(c["ids"])]
        assert rest and not gf[rest].any() and not gd[rest].any()
        assert not gf[:, :, c["h"]:].any() and not gf[:, :, :, c["w"]:].any()
        assert gf[list(c["ids"])][:, :, :c["h"], :c["w"]].any()


@pytest.mark.parametrize("name", ["b", "c"])
def test_one_nan_reaches_exactly_its_pixel(gpu, name):
    c, _, _, _, _ = reference(name)
    clean, _ = run(c, gpu, grads=False)
    V, R, M = len(c["ids"]), c["h"] * c["w"], c["M"]
    v, k, y, x = V - 1, c["C"] - 3, c["h"] - 1, c["w"] - 2
    feature = dev(c["feature"], gpu)
    feature[int(c["ids"][v]), k, y, x] = float("nan")
    got, _ = run(c, gpu, grads=False, feature=feature)
    got, clean = got.reshape(V, R, M), clean.reshape(V, R, M)
    r = y * c["w"] + x
    assert np.isnan(got[v, r]).all()
    mask = np.ones((V, R), bool)
    mask[v, r] = False
    assert np.array_equal(bits(got[mask]), bits(clean[mask]))
    assert np.isfinite(clean).all()


def test_planted_zeros_get_no_gradient(gpu):
    for name in ("a", "b"):
        c, _, g64, _, _ = reference(name)
        _, grads = run(c, gpu)
        sel = np.zeros(c["feature"].shape, bool)
        sel[list(c["ids"]), :, :c["h"], :c["w"]] = True
        zf = c["zeros_feature"] & sel
        assert zf.sum() > 10 and np.signbit(c["feature"][zf]).any() and not np.signbit(c["feature"][zf]).all()
        assert not bits(grads["feature"])[zf].any()
        zd = c["zeros_depth"].copy()
        zd[[n for n in range(c["N"]) if n not in list(c["ids"])]] = False
        assert zd.any() and not bits(grads["depth_coding"])[zd].any()
        assert np.abs(grads["feature"][sel & ~c["zeros_feature"] & (c["feature"] > 0)]).min() > 0


def test_chunked_weight_gradient_is_deterministic(gpu):
    """Case c in chunks of 32 pixels: 258 pixels -> 9 partial sums, added in chunk order.  Two runs: the same bits; and the values
    stay under the bar."""
    from mvsdet_amd.ops import gshead
    c, _, g64, _, g32 = reference("c")
    assert gshead.partial_floats(2, 129, c["M"], c["K"], 32) == 9 * c["M"] * (c["K"] + 1)
    _, first = run(c, gpu, chunk_pixels=32)
    _, second = run(c, gpu, chunk_pixels=32)
    for k in G.GRADS:
        assert np.array_equal(bits(first[k]), bits(second[k])), k
    compare("chunks of 32: d weight", first["weight"], g64["weight"], g32["weight"])
    compare("chunks of 32: d bias", first["bias"], g64["bias"], g32["bias"])
    _, one = run(c, gpu)
    assert not np.array_equal(bits(one["weight"]), bits(first["weight"]))          # another order of the sum: the chunks were used


def test_process_rgb_raw_on_the_device(gpu):
    """functional.process_rgb_raw against F.interpolate in float64 under the bar (ATen's own float32 resize gives the `own` term)."""
    from mvsdet_amd import functional as F_
    rng = np.random.RandomState(12)
    for (Hi, Wi, h, w), ids in (((24, 36, 5, 7), [2, 0]), ((19, 27, 4, 6), [1]), ((240, 320, 59, 80), [0, 1, 2])):
        images = (rng.normal(size=(3, 3, Hi, Wi)) * np.sqrt(2.0)).astype(np.float32)
        got = F_.process_rgb_raw(dev(images, gpu), 4, h, w, ids)
        assert tuple(got.shape) == (1, len(ids), h * w, 3)
        t = torch.from_numpy(images)
        r64 = G.process_rgb_raw(t.double(), torch.tensor(ids), h, w).numpy()
        r32 = G.process_rgb_raw(t, torch.tensor(ids), h, w).numpy()
        compare(f"process_rgb_raw {Hi}x{Wi}", got[0].cpu().numpy(), r64, r32)
        mean = G.four_pixel_mean(t, torch.tensor(ids), h, w).numpy()
        assert np.array_equal(bits(got[0]), bits(mean))                              # the closed form, in the order it is written


def test_fake_kernels_refusals_and_autocast(gpu):
    from mvsdet_amd.ops import gshead
    c, _, _, _, _ = reference("b")
    f, d, ids, wt, b, rgb = (dev(c[k], gpu) for k in ("feature", "depth_coding", "ids", "weight", "bias", "rgb_raw"))
    h, w = c["h"], c["w"]
    torch.library.opcheck(torch.ops.mvsdet_amd.gshead_forward.default, (f, d, ids, wt, b, h, w, rgb, None, 0),
                          test_utils=("test_schema", "test_faketensor"))
    g = torch.ones(len(c["ids"]), h * w, c["M"], device=gpu)
    torch.library.opcheck(torch.ops.mvsdet_amd.gshead_backward.default, (f, d, ids, wt, g, h, w, rgb, None, 0, True, True),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError, match="no gradient"):
        gshead.gaussian_head(f, d, ids, wt, b, h, w, c["S"], rgb.clone().requires_grad_(True))
    with pytest.raises(TypeError, match="float32"):
        gshead.gaussian_head(f.double(), d, ids, wt, b, h, w, c["S"], rgb)
    with pytest.raises(ValueError, match="K = "):
        gshead.gaussian_head(f, d, ids, wt, b, h, w, c["S"])
    # an id outside [0, N) that only the device knows: never an address; that view's raw is NaN, the others are untouched
    bad = ids.clone()
    bad[1] = 77
    out = gshead.gaussian_head(f, d, bad, wt, b, h, w, c["S"], rgb)
    good = gshead.gaussian_head(f, d, ids, wt, b, h, w, c["S"], rgb)
    assert bool(torch.isnan(out[1]).all()) and np.array_equal(bits(out[[0, 2]]), bits(good[[0, 2]]))
    # under autocast low-precision inputs are computed in float32
    plain = gshead.gaussian_head(f.half().float(), d, ids, wt, b, h, w, c["S"], rgb)
    with torch.autocast("cuda", dtype=torch.float16):
        amp = gshead.gaussian_head(f.half(), d, ids, wt, b, h, w, c["S"], rgb)
    assert amp.dtype == torch.float32 and np.array_equal(bits(amp), bits(plain))


def test_no_host_synchronisation(gpu):
    from mvsdet_amd import functional as F_
    c, _, _, _, _ = reference("e")
    leaves = [dev(c[k], gpu).requires_grad_(True) for k in ("feature", "depth_coding", "weight", "bias")]
    ids, images = dev(c["ids"], gpu), dev(c["images"], gpu)
    lw = dev(G.loss_weight(c["seed"], (1, c["h"] * c["w"], c["S"], c["M"] // c["S"])), gpu)

    def step():
        out = F_.gaussian_head(leaves[0], leaves[1], leaves[2], leaves[3], ids, c["h"], c["w"], c["S"], denorm_images=images)
        (out * lw).sum().backward()
        return out
    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step()
        rows = F_.process_rgb_raw(images, 4, c["h"], c["w"], ids)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert tuple(out.shape) == (1, 35, 2, 84) and tuple(rows.shape) == (1, 1, 35, 3) and torch.isfinite(leaves[2].grad).all()


def test_novel_views_on_the_hip_route(gpu, monkeypatch):
    """MVSDetHotPath.novel_views(gaussian_head="hip") on the 4-view scene of test_gpu_adapter.py (5 x 8 of 6 x 8 feature pixels, rgb from
    24 x 32 images): the Gaussians handed to the rasteriser against the default route's under the bar of the two restatements
    chained (gshead_restated -> adapter_restated, float64 and float32; adapter_scene's rule: 4 x the chain's own distance, inside
    A.bar); the default route with and without the new keywords: the same bits.  The render is not compared."""
    from mvsdet_amd import functional as F_
    from mvsdet_amd import synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, hw, L = 4, 8, (6, 8), 1
    d_sh = (L + 1) ** 2
    meta = synthetic.make_img_meta(N, hw, seed=5)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    assert (h, w) == (5, 8)
    gen = torch.Generator().manual_seed(3)
    feature_h = torch.randn(N, C, *hw, generator=gen)
    depth_h = 1.0 + 2.0 * torch.rand(N, 1, h, w, generator=gen)
    opacity = torch.rand(N, *hw, generator=gen).to(gpu)
    images_h = torch.rand(N, 3, 4 * hw[0], 4 * hw[1], generator=gen)
    feature, depth_coding, images = feature_h.to(gpu), depth_h.to(gpu), images_h.to(gpu)
    outputs = dict(geometry=SimpleNamespace(height=h, width=w), depth_coding=depth_coding, opacity=opacity)
    torch.manual_seed(4)
    to_gaussians = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(C + 4, 9 + 3 * d_sh)).to(gpu)
    c2w = np.linalg.inv(np.array(meta["lidar2img"]["extrinsic"], np.float64))
    tgt = c2w[[0, 2]].copy()
    tgt[:, :3, 3] += 0.05
    Kt = np.array([[40.0, 0, 16.0, 0], [0, 40.0, 12.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    src_id = hp.render_source_ids(meta, tgt, 3)
    assert src_id.numel() == N
    args = (outputs, feature, meta, to_gaussians, tgt, Kt, (24, 32, 3))
    with torch.no_grad():
        rgb_raw = F_.process_rgb_raw(images, 4, h, w, src_id)
        plain = hp.novel_views(*args, rgb_raw, sh_degree=L)
        named = hp.novel_views(*args, rgb_raw, sh_degree=L, gaussian_head="torch", denorm_images=None)
        assert np.array_equal(bits(plain), bits(named))
        from_images = hp.novel_views(*args, sh_degree=L, denorm_images=images)
        assert np.array_equal(bits(plain), bits(from_images))                       # process_rgb_raw inside: the same rows
        handed = []
        monkeypatch.setattr(F_, "decode_splatting", lambda gaussians, *a, **k: handed.append(gaussians) or gaussians.means)
        hp.novel_views(*args, rgb_raw, sh_degree=L)
        hp.novel_views(*args, sh_degree=L, gaussian_head="hip", denorm_images=images)
        hp.novel_views(*args, rgb_raw, sh_degree=L, gaussian_head="hip")
        scale, _ = hp.ray_depth(meta, torch.ones(N, 1, *hw, device=gpu))
    default, hip, hip_rows = handed
    # both restatements chained, on the inputs the path derives
    src_w2c, K_feat = hp._feature_cameras(meta)
    Kn = K_feat.clone().float()
    Kn[0] /= w
    Kn[1] /= h
    Kn = Kn[None, :3, :3].repeat(N, 1, 1).numpy()
    ext = src_w2c.inverse().float()[src_id].numpy()
    ray = (depth_h.reshape(N, h * w, 1) / (scale.cpu() + 1e-8))[src_id].reshape(N, h * w).numpy()
    opac = opacity.cpu()[src_id][:, :h, :w].reshape(N, h * w).numpy()
    blocks = A.sh_rotation_blocks(ext[:, :3, :3], d_sh)
    chain = {}
    for dtype in (torch.float64, torch.float32):
        raw = G.gaussian_head(feature_h.to(dtype), depth_h.to(dtype), src_id, to_gaussians[1].weight.detach().cpu().to(dtype),
                              to_gaussians[1].bias.detach().cpu().to(dtype), h, w, 1, images=images_h.to(dtype))
        chain[dtype] = A.pixel_gaussians(ext, Kn, raw, ray, opac, h, w, 0.5, 15.0, d_sh, blocks if dtype == torch.float64 else blocks.astype(np.float32), dtype)
    for k in A.FIELDS:
        x64, x32 = chain[torch.float64][k].numpy(), chain[torch.float32][k].numpy()
        bar, own = A.bar(x64, x32)
        for tag, got in (("images", hip), ("rows", hip_rows)):
            a, b = getattr(got, k)[0].cpu().numpy().astype(np.float64), getattr(default, k)[0].cpu().numpy().astype(np.float64)
            print(f"{k} ({tag}): hip-default {np.abs(a - b).max():.3g}  hip-f64 {np.abs(a - x64).max():.3g}  default-f64 {np.abs(b - x64).max():.3g}  "
                  f"chain f32-f64 {own:.3g}  worst |hip-default|/bar {float((np.abs(a - b) / bar).max()):.3f}")
            assert (np.abs(a - b) <= bar).all() and (np.abs(a - x64) <= bar).all(), (k, tag)
    with pytest.raises(TypeError, match="to_gaussians"):
        hp.novel_views(outputs, feature, meta, torch.nn.Sequential(torch.nn.Linear(C + 4, 21)).to(gpu), tgt, Kt, (24, 32, 3), rgb_raw,
                       sh_degree=L, gaussian_head="hip")
    with pytest.raises(TypeError, match="to_gaussians"):
        hp.novel_views(*args, sh_degree=L, gaussian_head="hip")                   # the layer is C + 4 wide, the rows C + 1
    with pytest.raises(ValueError, match="gaussian_head"):
        hp.novel_views(*args, rgb_raw, sh_degree=L, gaussian_head="triton")
    # the gradient of the NVS loss reaches the same places on the hip route
    monkeypatch.undo()
    f2, d2 = feature.clone().requires_grad_(True), depth_coding.clone().requires_grad_(True)
    out2 = dict(outputs, depth_coding=d2)
    colour = hp.novel_views(out2, f2, meta, to_gaussians, tgt, Kt, (24, 32, 3), sh_degree=L, gaussian_head="hip", denorm_images=images)
    loss = hp.nvs_loss(colour, torch.rand(2, 3, 24, 32, generator=gen).to(gpu))["loss_nvs"]
    grads = torch.autograd.grad(loss, [f2, to_gaussians[1].weight, to_gaussians[1].bias, d2])
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
