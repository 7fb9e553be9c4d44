"""The Gaussian head without a GPU: the restatement of tests/gshead_restated.py against itself in float64, against fixture G29 (the
reference's process_rgb_raw and the restated lines of extract_feat, tests/golden/make_goldens_g29.py), the four-pixel mean the kernel
uses against F.interpolate, and the refusals of mvsdet_amd.ops.gshead / functional that need no device.
"""
import numpy as np
import pytest
import torch

import gshead_restated as G
from conftest import load_golden

# (N, ids, C, Hf, Wf, h, w, S, d_sh, rgb): (K + 1, M, pixels) = (261, 84, 387), (45, 168, 105), (10, 12, 35)
SHAPES = {
    "k261_m84": (3, [0, 1, 2], 256, 4, 43, 3, 43, 1, 25, "images"),
    "k45_m168": (4, [1, 2, 3], 40, 6, 9, 5, 7, 2, 25, "rows"),
    "k10_m12": (3, [2], 8, 6, 9, 5, 7, 1, 1, None),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_float32_restatement_against_float64(name):
    """The float32 restatement against the float64 one under the classical bound of a length-n sum of products in any order,
    n 2^-24 sum |a_i b_i| (to first order; n counts the terms, the bias and, for the image form, the four-pixel mean's roundings of x):
    so the `own` term of the bar is rounding and nothing else."""
    c = G.case(40 + list(SHAPES).index(name), *SHAPES[name])
    o64, g64 = G.restate(c, torch.float64)
    o32, g32 = G.restate(c, torch.float32)
    ids, h, w, S = torch.from_numpy(c["ids"]), c["h"], c["w"], c["S"]
    t = {k: torch.from_numpy(c[k]).double() for k in ("feature", "depth_coding", "weight", "bias", "rgb_raw", "images") if k in c}
    rgb = G.process_rgb_raw(t["images"], ids, h, w) if "images" in t else t.get("rgb_raw")
    x = torch.relu(G.rows(t["feature"], t["depth_coding"], ids, h, w, rgb)).numpy()                    # (V,R,K)
    W, lw = np.abs(c["weight"].astype(np.float64)), np.abs(G.loss_weight(c["seed"], o64.shape).astype(np.float64)).reshape(x.shape[0], x.shape[1], -1)
    K, M, P, eps = c["K"], c["M"], x.shape[0] * x.shape[1], 2.0 ** -24
    bounds = {"raw": (K + 6) * eps * (x @ W.T + np.abs(c["bias"])).reshape(o64.shape),
              "weight": (P + 6) * eps * np.einsum("vrm,vrk->mk", lw, x), "bias": P * eps * lw.sum((0, 1))}
    gx = (M + 1) * eps * (lw @ W)                                                                        # (V,R,K)
    for tag, a, b in [("raw", o64, o32), ("weight", g64["weight"], g32["weight"]), ("bias", g64["bias"], g32["bias"])]:
        err = np.abs(b.astype(np.float64) - a)
        print(f"{name} {tag}: max|x| {np.abs(a).max():.4g}  f32-f64 {err.max():.3g}  worst err/bound {float((err / np.maximum(bounds[tag], 1e-300)).max()):.3f}")
        assert (err <= bounds[tag]).all(), (name, tag)
    C = c["C"]
    err = np.abs(g32["feature"].astype(np.float64) - g64["feature"])[c["ids"], :, :h, :w].reshape(len(ids), C, -1).transpose(0, 2, 1)
    print(f"{name} feature: f32-f64 {err.max():.3g}  worst err/bound {float((err / gx[..., :C]).max()):.3f}")
    assert (err <= gx[..., :C]).all()
    err = np.abs(g32["depth_coding"].astype(np.float64) - g64["depth_coding"]).reshape(c["N"], -1)[c["ids"]]
    assert (err <= gx[..., C]).all()
    # the planted zeros: no gradient there, in either sign
    assert c["zeros_feature"].any() and not g64["feature"][c["zeros_feature"]].any()
    assert np.signbit(c["feature"][c["zeros_feature"]]).any() and not np.signbit(c["feature"][c["zeros_feature"]]).all()
    # unselected views and the cropped-away pixels: exactly zero
    N, sel = c["N"], list(c["ids"])
    rest = [n for n in range(N) if n not in sel]
    assert not g64["feature"][rest].any() and not g64["feature"][:, :, h:].any() and not g64["feature"][:, :, :, w:].any()


def test_restatement_against_g29():
    g = load_golden("g29_gshead")
    N, C, Hf, Wf, h, w = (int(v) for v in g["shape"])
    assert str(g["process_rgb_raw"]).startswith("reference")
    for tag in [str(t) for t in g["cases"]]:
        S, d_sh, rgb, seed = (int(v) for v in g[tag + ".meta"])
        c = dict(ids=g["ids"], h=h, w=w, S=S, seed=seed, feature=g["in_feature"], depth_coding=g["in_depth_coding"], weight=g[tag + ".weight"],
                 bias=g[tag + ".bias"])
        if rgb:
            c["images"] = g["in_images"]
        o64, g64 = G.restate(c, torch.float64)
        o32, g32 = G.restate(c, torch.float32)
        for name, a, b in [("raw", o64, o32)] + [("g_" + k, g64[k], g32[k]) for k in G.GRADS]:
            bar = np.maximum(G.bar(a, b)[0], 4.0 * float(g[f"{tag}.own_{name}"]))
            err = np.abs(g[f"{tag}.{name}"].astype(np.float64) - a)
            print(f"{tag} {name}: reference-f64 {err.max():.3g}  stored own {float(g[f'{tag}.own_{name}']):.3g}  worst err/bar {float((err / bar).max()):.3f}")
            assert (err <= bar).all(), (tag, name)
        if rgb:
            ids = torch.from_numpy(g["ids"])
            mean = G.four_pixel_mean(torch.from_numpy(g["in_images"]).double(), ids, h, w).numpy()
            mean32 = G.four_pixel_mean(torch.from_numpy(g["in_images"]), ids, h, w).numpy()
            bar = np.maximum(G.bar(mean, mean32)[0], 4.0 * float(g[tag + ".own_rgb_rows"]))
            assert (np.abs(g[tag + ".rgb_rows"].astype(np.float64) - mean) <= bar).all(), tag


@pytest.mark.parametrize("hw", [(240, 320), (239, 320)])
def test_four_pixel_mean_is_interpolate_to_the_bit_at_the_training_size(hw):
    rng = np.random.RandomState(7)
    images = torch.from_numpy((rng.normal(size=(3, 3) + hw) * np.sqrt(2.0)).astype(np.float32))
    ids = torch.tensor([0, 2])
    h, w = hw[0] // 4 - 1, hw[1] // 4
    want = G.process_rgb_raw(images, ids, h, w)
    got = G.four_pixel_mean(images, ids, h, w)
    assert np.array_equal(got.numpy().view(np.int32), want.contiguous().numpy().view(np.int32))


@pytest.mark.parametrize("hw", [(24, 36), (19, 27), (23, 31)])
def test_four_pixel_mean_against_interpolate_at_small_sizes(hw):
    """ATen adds in another order at small sizes: under the bar against float64, not to the bit.  19 x 27 and 23 x 31 are no multiples
    of 4: the last pixel's four lie one and three pixels inside the image."""
    rng = np.random.RandomState(8)
    images = torch.from_numpy((rng.normal(size=(2, 3) + hw) * np.sqrt(2.0)).astype(np.float32))
    ids = torch.tensor([1, 0])
    h, w = hw[0] // 4, hw[1] // 4                       # all that F.interpolate returns
    want64 = G.process_rgb_raw(images.double(), ids, h, w).numpy()
    want32 = G.process_rgb_raw(images, ids, h, w).numpy()
    got = G.four_pixel_mean(images, ids, h, w).numpy()
    bar, own = G.bar(want64, want32)
    err = np.abs(got.astype(np.float64) - want64)
    print(f"{hw}: mean-f64 {err.max():.3g}  interpolate f32-f64 {own:.3g}  worst err/bar {float((err / bar).max()):.3f}")
    assert (err <= bar).all()


def test_process_rgb_raw_refuses_other_ratios():
    from mvsdet_amd import functional as F_
    images = torch.zeros(2, 3, 24, 36)
    for ratio in (2, 8, 4.5):
        with pytest.raises(ValueError, match="ratio"):
            F_.process_rgb_raw(images, ratio, 5, 7, [0, 1])
    with pytest.raises(ValueError, match="ratio 4"):
        F_.process_rgb_raw(torch.zeros(2, 3, 18, 36), 4, 5, 7, [0, 1])          # 18 < 4 * 5 - 1 rows
    with pytest.raises(ValueError, match="outside"):
        F_.process_rgb_raw(images, 4, 5, 7, [0, 2])


def test_argument_errors_before_any_launch():
    from mvsdet_amd import functional as F_
    from mvsdet_amd.ops import gshead
    N, C, Hf, Wf, h, w, S, d_sh = 3, 8, 6, 9, 5, 7, 2, 4
    M, R = S * (9 + 3 * d_sh), h * w
    feature, depth = torch.zeros(N, C, Hf, Wf), torch.zeros(N, 1, h, w)
    w1, w4, bias = torch.zeros(M, C + 1), torch.zeros(M, C + 4), torch.zeros(M)
    rgb_raw, images = torch.zeros(2, R, 3), torch.zeros(N, 3, 24, 36)
    with pytest.raises(ValueError, match="not both"):
        F_.gaussian_head(feature, depth, w4, bias, [0, 2], h, w, S, rgb_raw=rgb_raw, denorm_images=images)
    with pytest.raises(ValueError, match="not both"):
        gshead.gaussian_head(feature, depth, [0, 2], w4, bias, h, w, S, rgb_raw, images)
    for ids in ([0, 3], [-1, 0], torch.tensor([1, 5])):
        with pytest.raises(ValueError, match="outside"):
            F_.gaussian_head(feature, depth, w1, bias, ids, h, w, S)
    with pytest.raises(ValueError, match="unique"):
        F_.gaussian_head(feature, depth, w1, bias, [1, 1], h, w, S)
    with pytest.raises(ValueError, match="K = "):
        F_.gaussian_head(feature, depth, w4, bias, [0, 2], h, w, S)              # C + 4 columns without rgb
    with pytest.raises(ValueError, match="K = "):
        F_.gaussian_head(feature, depth, w1, bias, [0, 2], h, w, S, rgb_raw=rgb_raw)
    with pytest.raises(ValueError, match="K = "):
        F_.gaussian_head(feature, depth, torch.zeros(M, C + 2), bias, [0, 2], h, w, S)
    with pytest.raises(ValueError, match="divisible"):
        F_.gaussian_head(feature, depth, w1, bias, [0, 2], h, w, 5)
    with pytest.raises(ValueError, match="depth_coding"):
        F_.gaussian_head(feature, torch.zeros(N, 1, h + 1, w), w1, bias, [0, 2], h, w, S)
    with pytest.raises(ValueError, match="inside the feature map"):
        F_.gaussian_head(feature, torch.zeros(N, 1, Hf + 1, w), w1, bias, [0, 2], Hf + 1, w, S)
    with pytest.raises(ValueError, match="rgb_raw"):
        F_.gaussian_head(feature, depth, w4, bias, [0, 2], h, w, S, rgb_raw=torch.zeros(3, R, 3))
    with pytest.raises(ValueError, match="ratio 4"):
        F_.gaussian_head(feature, depth, w4, bias, [0, 2], h, w, S, denorm_images=torch.zeros(N, 3, 18, 36))
    # with everything in order the operator then refuses the host tensors: there is no CPU path
    with pytest.raises((RuntimeError, NotImplementedError)):
        F_.gaussian_head(feature, depth, w1, bias, [0, 2], h, w, S)


def test_c_entry_points_refuse_on_the_host():
    import ctypes
    from mvsdet_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    s3, s2 = (ctypes.c_int64 * 3)(432, 54, 9), (ctypes.c_int64 * 2)(35, 7)
    assert lib.mvsdet_gshead_forward_f32(None, s3, one, s2, None, None, None, one, one, one, one, 3, 2, 8, 9, 12, 5, 7, 6, 9, 0, 0, None) == 1
    assert b"NULL" in lib.mvsdet_last_error()
    assert lib.mvsdet_gshead_forward_f32(one, s3, one, s2, None, None, None, one, one, one, one, 3, 2, 8, 12, 12, 5, 7, 6, 9, 0, 0, None) == 1
    assert b"K=12" in lib.mvsdet_last_error()
    assert lib.mvsdet_gshead_forward_f32(one, s3, one, s2, one, one, s3, one, one, one, one, 3, 2, 8, 12, 12, 5, 7, 6, 9, 24, 36, None) == 1
    assert b"not both" in lib.mvsdet_last_error()
    assert lib.mvsdet_gshead_forward_f32(one, s3, one, s2, None, one, s3, one, one, one, one, 3, 2, 8, 12, 12, 5, 7, 6, 9, 18, 36, None) == 1
    assert b"ratio 4" in lib.mvsdet_last_error()
    assert lib.mvsdet_gshead_forward_f32(one, s3, one, s2, None, None, None, one, one, one, one, 3, 2, 8, 9, 12, 7, 7, 6, 9, 0, 0, None) == 1
    neg = (ctypes.c_int64 * 3)(432, -54, 9)
    assert lib.mvsdet_gshead_forward_f32(one, neg, one, s2, None, None, None, one, one, one, one, 3, 2, 8, 9, 12, 5, 7, 6, 9, 0, 0, None) == 1
    assert b"strides" in lib.mvsdet_last_error()
    # the weight gradient: a partial buffer that is too small is a workspace error; the query rounds the chunk up to 32 pixels
    assert lib.mvsdet_gshead_partial_bytes(2, 35, 12, 9, 0) == 1 * 12 * 10 * 4
    assert lib.mvsdet_gshead_partial_bytes(2, 35, 12, 9, 20) == 3 * 12 * 10 * 4
    assert lib.mvsdet_gshead_partial_bytes(2, 35, 12, 9, -1) == 0 and lib.mvsdet_gshead_partial_bytes(0, 35, 12, 9, 0) == 0
    assert lib.mvsdet_gshead_backward_weight_f32(one, s3, one, s2, None, None, None, one, one, one, one, one, 16, 32, 3, 2, 8, 9, 12, 5, 7, 6, 9, 0,
                                                 0, None) == 2
    assert b"workspace" in lib.mvsdet_last_error()
    assert lib.mvsdet_gshead_backward_input_f32(one, s3, one, s2, one, one, one, one, s3, one, s2, 3, 2, 8, 10, 12, 5, 7, 6, 9, None) == 1
    assert b"K=10" in lib.mvsdet_last_error()
    assert lib.mvsdet_gshead_rgb_rows_f32(one, s3, one, one, 3, 2, 5, 7, 19, 26, None) == 1
