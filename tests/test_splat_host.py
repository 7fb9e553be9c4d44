"""The Gaussian rasteriser's restatement (tests/splat_restated.py), scenes (tests/splat_scenes.py) and fixture G26 on the CPU: what the
GPU tests of test_gpu_splat.py stand on.  No GPU, no kernel: the restatement against closed forms and scipy, the scenes' conditions
(every Gaussian-level decision decided by 1e-3, at most 1 % of the pixels left out, float32 and float64 restatements agreeing on
every decision of the kept pixels), the fixture's contents, and the refusals that need no device.
"""
import numpy as np
import pytest
import torch

import splat_restated as R
import splat_scenes as S
from conftest import load_golden

NAMES = ("means", "covs", "sh", "opac")
ALL = [("case", n) for n in S.CASES] + [("special", n) for n in S.SPECIAL]


def get(kind, name):
    return S.reference(name) if kind == "case" else S.special_reference(name)


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
    args = (one, s2, one, s3, one, s3, one, 1, one, one, one, one, 1 << 30)
    assert lib.mvsdet_splat_forward_f32(*args, 1, 8, 5, 1, 16, 16, 64, None) == 1 and b"d_sh" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_forward_f32(*args, 1, 8, 4, 0, 16, 16, 64, None) == 1 and b"precomputed" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_forward_f32(*args, 1, 8, 4, 1, 16, 16, 0, None) == 1 and b"bad sizes" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_forward_f32(*args, 2, 1 << 30, 4, 1, 16, 16, 64, None) == 1 and b"limits" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_forward_f32(*args[:12], 64, 1, 8, 4, 1, 16, 16, 64, None) == 2 and b"workspace" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_forward_f32(None, *args[1:], 1, 8, 4, 1, 16, 16, 64, None) == 1 and b"NULL" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_backward_f32(*args[:10], None, one, 1 << 30, one, one, one, one, one, 1, 8, 4, 1, 16, 16, 64, None) == 1
    assert lib.mvsdet_splat_cameras_f32(one, 16, one, 9, 2, one, one, 1, one, 1, None) == 1 and b"intrinsics rows" in lib.mvsdet_last_error()
    assert lib.mvsdet_splat_workspace_bytes(1, 8, 16, 16, 0) == 0
