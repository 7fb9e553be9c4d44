"""The Gaussian rasteriser's restatement (tests/splat_restated.py), scenes (tests/splat_scenes.py) and fixture G26 on the CPU: what the
GPU tests of test_gpu_splat.py and test_gpu_splat_edges.py stand on.  No GPU, no kernel: the restatement against closed forms and
scipy, the scenes' conditions (the edge scenes of splat_scenes.EDGES included: every Gaussian-level decision decided by 1e-3, at most
1 % of the pixels left out, float32 and float64 restatements agreeing on every decision of the kept pixels), the fixture's contents,
and the refusals that need no device.
"""
import numpy as np
import pytest
import torch

import splat_restated as R
import splat_scenes as S
from conftest import load_golden

NAMES = ("means", "covs", "sh", "opac")
ALL = [("case", n) for n in S.CASES] + [("special", n) for n in S.SPECIAL] + [("edge", n) for n in S.EDGES]


def get(kind, name):
    return {"case": S.reference, "special": S.special_reference, "edge": S.edge_reference}[kind](name)


def test_a_single_isotropic_gaussian_against_its_closed_form():
    sigma, z, op, coeff = 0.07, 1.6, 0.8, np.array([0.9, -0.4, 0.2], np.float32)
    sc = S.special([[0.0, 0.0, z]], [S.iso(sigma)], [op], sh=coeff.reshape(1, 3, 1))
    image, info = R.render(*[torch.from_numpy(sc[k]) for k in NAMES], torch.from_numpy(sc["cams"]), torch.from_numpy(sc["bg"]), sc["H"], sc["W"])
    H, W = sc["H"], sc["W"]
    tanx, tany = float(sc["cams"][0, 32]), float(sc["cams"][0, 33])
    fx, fy = W / (2 * tanx), H / (2 * tany)
    s2, z = float(sc["covs"][0, 0, 0]), float(np.float32(z))          # the float32 inputs' own values
    a, c = fx * fx * s2 / (z * z) + 0.3, fy * fy * s2 / (z * z) + 0.3
    radius = np.ceil(3 * np.sqrt(max(a, c)))
    ys, xs = np.mgrid[:H, :W]
    alpha = float(np.float32(op)) * np.exp(-0.5 * ((xs - 20.0) ** 2 / a + (ys - 16.0) ** 2 / c))
    # the tile rectangle around pixel (20, 16) with this radius
    x0, x1 = int((20 - radius) / 16), min(int((20 + radius + 15) / 16), 3)
    y0, y1 = int((16 - radius) / 16), min(int((16 + radius + 15) / 16), 3)
    on = (alpha >= 1 / 255) & (xs // 16 >= x0) & (xs // 16 < x1) & (ys // 16 >= y0) & (ys // 16 < y1)
    colour = np.maximum(R.C0 * coeff.astype(np.float64) + 0.5, 0)
    bg = sc["bg"][0].astype(np.float64)
    want = np.where(on[None], colour[:, None, None] * alpha[None] + (1 - alpha[None]) * bg[:, None, None], bg[:, None, None])
    assert on.sum() > 40 and colour[1] > 0
    assert np.abs(image[0].numpy() - want).max() < 1e-12
    assert info["keys"] == [(x1 - x0) * (y1 - y0)]


def test_sh_basis_against_scipy():
    """Real harmonics from scipy's complex ones, l <= 4: ours = (-1)^m x the textbook real harmonic (Condon-Shortley phase removed) --
    the published code's sign convention for degrees 1..3, continued to degree 4."""
    import scipy.special as sp
    if hasattr(sp, "sph_harm_y"):
        sph_harm = lambda m, l, az, pol: sp.sph_harm_y(l, m, pol, az)  # noqa: E731
    else:
        sph_harm = sp.sph_harm
    rng = np.random.RandomState(5)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    az, pol = np.arctan2(d[:, 1], d[:, 0]), np.arccos(d[:, 2])
    ours = R.sh_basis(torch.from_numpy(d), 25).numpy()
    for n in (1, 4, 9, 16):
        assert np.array_equal(R.sh_basis(torch.from_numpy(d), n).numpy(), ours[:, :n])
    for l in range(5):
        for m in range(-l, l + 1):
            Y = sph_harm(abs(m), l, az, pol)
            real = Y.real if m == 0 else np.sqrt(2) * (-1) ** m * (Y.real if m > 0 else Y.imag)
            want = (-1) ** m * real
            assert np.abs(ours[:, l * l + l + m] - want).max() < 1e-13, (l, m)


def test_permuting_gaussians_of_distinct_depths_leaves_the_image_unchanged():
    sc, o64, _, _ = S.reference("sh4")
    perm = np.random.RandomState(9).permutation(sc["G"])
    again, _, _ = S.restate(dict(sc, **{k: sc[k][perm].copy() for k in NAMES}), torch.float64, grad=False)
    assert np.array_equal(again["image"], o64["image"])


def test_equal_depths_follow_the_index_order():
    sc, o64, _, _ = S.special_reference("equal_depths")
    depth = R.preprocess(*[torch.from_numpy(sc[k]) for k in NAMES], torch.from_numpy(sc["cams"][0]), sc["H"], sc["W"])["depth"].numpy()
    assert np.array_equal(depth[:5].view(np.int32), np.full(5, depth[0].view(np.int32)))       # bit-equal in float32
    back, _, _ = S.restate(dict(sc, **{k: sc[k][[4, 3, 2, 1, 0, 5, 6]].copy() for k in NAMES}), torch.float64, grad=False)
    assert np.abs(back["image"] - o64["image"]).max() > 1e-3          # the order among them matters ...
    # ... and is the index order: moving them apart by 1e-5 in depth, ascending with the index, gives (nearly) the same picture
    apart = sc["means"].copy()
    apart[:5, 2] += np.arange(5, dtype=np.float32) * np.float32(1e-5)
    moved, _, _ = S.restate(dict(sc, means=apart), torch.float64, grad=False)
    assert np.abs(moved["image"] - o64["image"]).max() < 1e-4


@pytest.mark.parametrize("kind,name", ALL)
def test_scene_conditions_hold(kind, name):
    sc, o64, o32, w = get(kind, name)
    margin = S.gaussian_margin(sc["means"], sc["covs"], sc["sh"], sc["opac"], sc["cams"], sc["H"], sc["W"])
    left = float((~o64["kept"]).mean())
    print(f"{name}: smallest Gaussian margin {margin.min():.3g}, pixels left out {left:.4f}, keys per Gaussian "
          f"{[k / sc['G'] for k in o64['info']['keys']]}")
    assert margin.min() >= S.MARGIN
    assert left <= S.MAX_LEFT_OUT
    assert np.array_equal(w != 0, np.broadcast_to(o64["kept"][:, None], w.shape) & (sc["g_image"] != 0))
    # float32 and float64 take the same decisions: per Gaussian everywhere, per pixel on the kept ones
    a, b = o64["info"], o32["info"]
    assert torch.equal(a["ok"], b["ok"]) and a["keys"] == b["keys"]
    keep = torch.from_numpy(o64["kept"])
    assert torch.equal(a["n_contrib"][keep], b["n_contrib"][keep]) and torch.equal(a["stopped"][keep], b["stopped"][keep])
    assert all(np.isfinite(g).all() for g in o64["grads"] + o32["grads"])


def test_g26_is_readable():
    g = load_golden("g26_splat")
    tags = [str(t) for t in g["cases"]]
    assert tags == ["single_k", "per_view_k", "plain"]
    for tag in tags:
        V = g[tag + ".extrinsics"].shape[0]
        G, d = g[tag + ".sh"].shape[1], g[tag + ".sh"].shape[3]
        assert g[tag + ".viewmatrix"].shape == (V, 4, 4) and g[tag + ".projmatrix"].shape == (V, 4, 4) and g[tag + ".tanfov"].shape == (V, 2)
        assert g[tag + ".handed_means"].shape == (V, G, 3) and g[tag + ".handed_cov6"].shape == (V, G, 6)
        assert int(g[tag + ".degree"]) == {1: 0, 4: 1, 25: 4}[d]
        for q in ("viewmatrix", "projmatrix", "tanfov", "campos"):
            assert 0 <= float(g[f"{tag}.own_{q}"]) < 1e-6
        # the restated cameras are within the reference's own distance of what it handed over
        c = R.cameras(g[tag + ".extrinsics"], g[tag + ".intrinsics"], g[tag + ".near"], g[tag + ".far"], bool(g[tag + ".scale_invariant"]), np.float64)
        assert np.abs(c[:, :16].reshape(V, 4, 4) - g[tag + ".viewmatrix"]).max() <= float(g[tag + ".own_viewmatrix"])
        assert np.abs(c[:, 16:32].reshape(V, 4, 4) - g[tag + ".projmatrix"]).max() <= float(g[tag + ".own_projmatrix"])
    k = g["single_k.intrinsics"]
    assert np.array_equal(k[0], k[1]) and not np.array_equal(g["per_view_k.intrinsics"][0], g["per_view_k.intrinsics"][1])
    assert not bool(g["plain.scale_invariant"])


def test_the_shim_and_the_operators_refuse_cpu_tensors():
    from mvsdet_amd import functional as F_
    from mvsdet_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from mvsdet_amd.ops import splat
    sc = S.SPECIAL["cap"]()
    t = {k: torch.from_numpy(sc[k]) for k in NAMES + ("cams", "bg", "extrinsics", "intrinsics", "near", "far")}
    settings = GaussianRasterizationSettings(image_height=sc["H"], image_width=sc["W"], tanfovx=0.5, tanfovy=0.5, bg=t["bg"][0], scale_modifier=1.0,
                                             viewmatrix=t["cams"][0, :16].view(4, 4), projmatrix=t["cams"][0, 16:32].view(4, 4), sh_degree=0,
                                             campos=t["cams"][0, 34:37], prefiltered=False, debug=False)
    row, col = torch.triu_indices(3, 3)
    with pytest.raises(RuntimeError, match="must live on a ROCm device"):
        GaussianRasterizer(settings)(means3D=t["means"], means2D=torch.zeros_like(t["means"]), shs=t["sh"].permute(0, 2, 1), colors_precomp=None,
                                     opacities=t["opac"][:, None], cov3D_precomp=t["covs"][:, row, col])
    with pytest.raises(NotImplementedError, match="scales / rotations"):
        GaussianRasterizer(settings)(means3D=t["means"], means2D=None, shs=t["sh"].permute(0, 2, 1), opacities=t["opac"][:, None],
                                     scales=t["means"], rotations=torch.zeros(3, 4))
    with pytest.raises((RuntimeError, NotImplementedError), match="ROCm device|CPU"):
        splat.rasterize(t["means"], t["covs"], t["sh"], t["opac"], t["cams"], t["bg"], sc["H"], sc["W"], 64, True)
    with pytest.raises((RuntimeError, NotImplementedError), match="ROCm device|CPU"):
        F_.render_cuda(t["extrinsics"], t["intrinsics"], t["near"], t["far"], (sc["H"], sc["W"]), t["bg"], t["means"][None], t["covs"][None],
                       t["sh"][None], t["opac"][None])
    assert splat.default_max_keys(100) == 800
    lib_bytes = splat.workspace_bytes(2, 256, 40, 56, 2048)
    assert lib_bytes % 256 == 0 and lib_bytes > 2 * 2048 * (8 + 8 + 4 + 4 + 4)


def test_argument_errors_return_without_launching():
    import ctypes

    from mvsdet_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    s2, s3 = (ctypes.c_int64 * 2)(3, 1), (ctypes.c_int64 * 3)(9, 3, 1)
    # means, strides, covariances, strides, harmonics, strides, opacities, stride, cams, near, far, background, image, depth, values, workspace,
    # bytes; then V, G, d_sh, use_sh, with_colour, with_depth, mode, H, W, max_keys, stream.  Colour alone: near, far, depth, values NULL
    args = (one, s2, one, s3, one, s3, one, 1, one, None, None, one, one, None, None, one, 1 << 30)
    f = lib.mvsdet_splat_forward_f32
    assert f(*args, 1, 8, 5, 1, 1, 0, 0, 16, 16, 64, None) == 1 and b"d_sh" in lib.mvsdet_last_error()
    assert f(*args, 1, 8, 4, 0, 1, 0, 0, 16, 16, 64, None) == 1 and b"precomputed" in lib.mvsdet_last_error()
    assert f(*args, 1, 8, 4, 1, 1, 0, 0, 16, 16, 0, None) == 1 and b"bad sizes" in lib.mvsdet_last_error()
    assert f(*args, 2, 1 << 30, 4, 1, 1, 0, 0, 16, 16, 64, None) == 1 and b"limits" in lib.mvsdet_last_error()
    assert f(*args[:16], 64, 1, 8, 4, 1, 1, 0, 0, 16, 16, 64, None) == 2 and b"workspace" in lib.mvsdet_last_error()
    assert f(None, *args[1:], 1, 8, 4, 1, 1, 0, 0, 16, 16, 64, None) == 1 and b"NULL" in lib.mvsdet_last_error()
    # backward: ..., background, g_image (NULL here), g_depth, values, workspace, bytes, slots, g_means, g_covariances, g_harmonics, g_opacities
    assert lib.mvsdet_splat_backward_f32(*args[:12], None, None, None, one, 1 << 30, one, one, one, one, one, 1, 8, 4, 1, 1, 0, 0, 16, 16, 64,
                                         None) == 1
    assert b"NULL" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_cameras_f32(one, 16, one, 9, 2, one, one, 1, one, 1, None) == 1 and b"intrinsics rows" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_workspace_bytes(1, 8, 16, 16, 0) == 0


# ------------------------------------------------------------------------------------------- the edge scenes' own conditions
@pytest.mark.parametrize("n", S.LIST_LENGTHS)
def test_list_scenes_have_one_tile_list_of_exactly_n_entries(n):
    """The first n non-culled Gaussians of `one_tile` in index order, one key each; some pixel walks the list to its last entry or the
    one before it, so the last LDS batch of the forward and the first of the backward are really used."""
    sc, o64, _, _ = S.edge_reference(f"list{n}")
    full = S.scene(**S.CASES["one_tile"])
    first = np.nonzero(S.visible(full)[0])[0][:n]
    info = o64["info"]
    print(f"list{n}: keys {info['keys']}, largest n_contrib {int(info['n_contrib'].max())}, stopped pixels {int(info['stopped'].sum())}")
    assert (sc["H"], sc["W"], sc["V"], sc["G"]) == (16, 16, 1, n) and np.array_equal(sc["means"], full["means"][first])
    assert bool(info["ok"].all()) and info["keys"] == [n]
    assert int(info["n_contrib"].max()) >= n - 1
    assert bool(info["stopped"].any())


def test_padding_is_culled_and_leaves_the_live_gaussians_alone():
    """What spread_out puts between the live Gaussians is culled in both views of sh4 by a decided margin; front, behind and
    interleaved put the live ones last, first, and at seeded indices with 0 and G - 1 among them."""
    sc, o64, _, _ = S.reference("sh4")
    seen = S.visible(sc)
    one = S.spread_out(S.subset(sc, [0]), 2, [1])
    assert not S.visible(one)[:, 0].any()
    assert float(S.gaussian_margin(one["means"], one["covs"], one["sh"], one["opac"], sc["cams"], sc["H"], sc["W"])[0]) >= S.MARGIN
    for G in S.PAD_SIZES:
        for where in ("front", "behind", "interleaved"):
            big, at = S.padded(sc, G, where)
            assert big["G"] == G and len(at) == sc["G"] and (np.diff(at) > 0).all()
            assert {"front": at[0] == G - sc["G"], "behind": at[-1] == sc["G"] - 1, "interleaved": at[0] == 0 and at[-1] == G - 1}[where]
            vis = S.visible(big)
            assert np.array_equal(vis[:, at], seen) and vis.sum() == seen.sum()
            assert all(np.array_equal(big[k][at], sc[k]) for k in NAMES)
    big, at = S.padded(sc, 257, "interleaved")
    again, _, _ = S.restate(big, torch.float64, grad=False)
    assert np.array_equal(again["image"], o64["image"]) and again["info"]["keys"] == o64["info"]["keys"]


def test_cut_scenes_and_the_gaussian_of_the_non_finite_variants():
    sc, o64, _, _ = S.reference("sh4")
    g = S.both_views(sc)
    one, o1, _, _ = S.edge_reference("first1")
    print("sh4: the first Gaussian that no view culls is", g, "-- keys of the scene cut to it", o1["info"]["keys"])
    assert bool(o64["info"]["ok"][:, g].all()) and bool(o1["info"]["ok"].all()) and min(o1["info"]["keys"]) >= 1
    assert one["G"] == 1 and np.array_equal(one["means"][0], sc["means"][g])
    cut, o255, _, _ = S.edge_reference("first255")
    assert cut["G"] == 255 and np.array_equal(cut["means"], sc["means"][:255])
    # without it both views of sh4 need fewer keys
    away = sc["means"].copy()
    away[g] = S.BEHIND
    gone, _, _ = S.restate(dict(sc, means=away), torch.float64, grad=False)
    assert all(a < b for a, b in zip(gone["info"]["keys"], o64["info"]["keys"])) and not bool(gone["info"]["ok"][:, g].any())


def test_small_image_and_bit_scenes_are_what_their_tests_say():
    tiles = lambda sc: -(-sc["H"] // 16) * -(-sc["W"] // 16)  # noqa: E731
    assert [v * -(-h // 16) * -(-w // 16) for v, h, w in S.BIT_SHAPES] == [2, 3, 4, 8, 16] and all(v > 1 for v, _, _ in S.BIT_SHAPES)
    for v, h, w in S.BIT_SHAPES:
        sc, o64, _, _ = S.edge_reference(f"bits{v}x{h}x{w}")
        last = o64["info"]["ok"][v - 1]
        assert sc["V"] == v and sc["G"] == 96 and v * tiles(sc) in (2, 3, 4, 8, 16) and bool(last.any())
    for h, w in S.SMALL_IMAGES:
        sc, o64, _, _ = S.edge_reference(f"small{h}x{w}")
        print(f"small{h}x{w}: keys {o64['info']['keys']}, stopped pixels {o64['info']['stopped'].sum((1, 2)).tolist()}")
        assert (sc["H"], sc["W"], sc["V"], sc["G"]) == (h, w, 2, 96) and min(o64["info"]["keys"]) >= 64
    _, o64, _, _ = S.edge_reference("small1x1")
    assert bool(o64["info"]["stopped"].all())


def test_the_front_scene_and_its_nan_variants():
    """`front`: the nearest Gaussian is small, has tile (1, 0) of 41x33 alone as its rectangle, lies at least 4 px from that tile's
    edges, and has a positive definite conic.  Restated with a NaN opacity, the image is NaN on exactly that tile; with a NaN
    coefficient in channel 1, channel 1 alone, on a proper part of the tile."""
    sc, o64, _, _ = S.edge_reference("front")
    p = R.preprocess(*[torch.from_numpy(sc[k]).double() for k in NAMES], torch.from_numpy(sc["cams"][0]), sc["H"], sc["W"])
    A, B, C = p["conic"][0].tolist()
    px, py, radius = float(p["px"][0]), float(p["py"][0]), float(p["radius"][0])
    print(f"front: pixel ({px:.4f}, {py:.4f}), radius {radius}, rectangle {p['rect'][0].tolist()}, keys {o64['info']['keys']}")
    assert bool(p["ok"].all()) and int(p["depth"].argmin()) == 0
    assert p["rect"][0].tolist() == [1, 2, 0, 1] and abs(px - 24) < 1e-3 and abs(py - 8) < 1e-3 and radius == 4
    assert A > 0 and A * C - B * B > 0
    tile = np.zeros((1, 3, sc["H"], sc["W"]), bool)
    tile[:, :, 0:16, 16:32] = True
    opac, sh = sc["opac"].copy(), sc["sh"].copy()
    opac[0], sh[0, 1, 0] = np.nan, np.nan
    a, _, _ = S.restate(dict(sc, opac=opac), torch.float64, grad=False)
    assert np.array_equal(np.isnan(a["image"]), tile)
    b, _, _ = S.restate(dict(sc, sh=sh), torch.float64, grad=False)
    nan = np.isnan(b["image"])
    assert not nan[:, [0, 2]].any() and 20 < nan[0, 1].sum() < 256 and not (nan & ~tile).any()
    assert np.array_equal(b["kept"], o64["kept"])            # no per-pixel margin depends on a colour
    assert np.array_equal(b["image"][:, [0, 2]], o64["image"][:, [0, 2]])
