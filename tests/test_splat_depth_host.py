"""The rendered depth's restatement (tests/splat_depth_restated.py) and fixture G28 on the CPU: what test_gpu_splat_depth.py stands on.
No GPU, no kernel: the restatement against closed forms and against what the reference's own render_depth_cuda handed its rasteriser
(tests/golden/make_goldens_g28.py), the scenes' conditions in the four modes, and the refusals that need no device -- the operators',
functional.render_depth_cuda's, and the C entry points' argument errors in their depth forms.
"""
import ctypes

import numpy as np
import pytest
import torch

import splat_depth_restated as D
import splat_restated as R
import splat_scenes as S
from conftest import load_golden


def test_g28_is_readable_and_the_restated_value_is_the_reference_s():
    """fake_colour in float32 within 4 x the reference's own fp32 distance from float64 (stored per case and mode) of what the reference
    handed over, on the Gaussians that are not culled; the float64 form within that distance itself."""
    g = load_golden("g28_splat_depth")
    assert [str(t) for t in g["cases"]] == ["single_k", "plain"] and tuple(str(m) for m in g["modes"]) == D.MODES
    assert bool(g["single_k.scale_invariant"]) and not bool(g["plain.scale_invariant"])
    for tag in ("single_k", "plain"):
        V, G = g[tag + ".extrinsics"].shape[0], g[tag + ".means"].shape[0]
        vis = g[tag + ".visible"]
        assert vis.shape == (V, G) and vis.dtype == bool and 0 < vis.sum() < V * G
        args = (torch.from_numpy(g[tag + ".means"]), g[tag + ".extrinsics"], g[tag + ".near"], g[tag + ".far"])
        for mode in D.MODES:
            handed, own = g[f"{tag}.{mode}.colors_precomp"], float(g[f"{tag}.{mode}.own"])
            assert handed.shape == (V, G, 3) and handed.dtype == np.float32 and bool(g[f"{tag}.{mode}.shs_none"])
            assert np.array_equal(handed[..., 0], handed[..., 1]) and np.array_equal(handed[..., 0], handed[..., 2])
            assert 0 <= own < 1e-6
            v32 = D.fake_colour(*args, mode, torch.float32).numpy().astype(np.float64)
            v64 = D.fake_colour(*args, mode, torch.float64).numpy()
            e32, e64 = float(np.abs(v32 - handed[..., 0])[vis].max()), float(np.abs(v64 - handed[..., 0])[vis].max())
            print(f"{tag} {mode}: restated f32 - handed {e32:.3g}, f64 - handed {e64:.3g}, the reference's own {own:.3g}")
            assert e32 <= 4.0 * own and e64 <= own
        near, far = g[tag + ".near"], g[tag + ".far"]
        assert (near <= far).all()
        assert np.array_equal(g[f"{tag}.log.colors_precomp"][..., 0], np.broadcast_to(np.log(far)[:, None], (V, G)))   # the inverted clamp


def test_a_single_isotropic_gaussian_on_the_axis_gives_alpha_z_at_the_centre():
    z, op = 1.6, 0.8
    sc = S.special([[0.0, 0.0, z]], [S.iso(0.07)], [op])
    leaves = [torch.from_numpy(sc[k]) for k in D.NAMES]
    depth, value, info = D.render_depth(*leaves, sc["cams"], sc["extrinsics"], sc["near"], sc["far"], sc["H"], sc["W"], "depth")
    z32, op32 = float(np.float32(z)), float(np.float32(op))
    assert float(value[0, 0]) == z32
    assert abs(float(depth[0, 16, 20]) - op32 * z32) < 1e-12        # the optical axis hits pixel (20, 16): alpha = opacity * exp(0)
    far_off = depth[0, 0, 0]
    assert float(far_off) == 0.0                                    # background 0
    disp, _, _ = D.render_depth(*leaves, sc["cams"], sc["extrinsics"], sc["near"], sc["far"], sc["H"], sc["W"], "disparity")
    assert abs(float(disp[0, 16, 20]) - op32 / z32) < 1e-12


@pytest.mark.parametrize("name", ["sh1", "sh4"])
def test_log_mode_is_log_far_times_the_accumulated_alpha(name):
    """The reference's clamp is inverted (min with near, then max with far): every value is log(far), so the picture is
    log(far) (1 - T).  1 - T is the render of a constant colour 1 over a black background."""
    sc, o64, _, _ = D.reference("case", name, "log")
    assert (sc["near"] <= sc["far"]).all()
    assert np.array_equal(o64["values"], np.broadcast_to(np.log(sc["far"].astype(np.float64))[:, None], o64["values"].shape))
    ones = torch.ones(sc["G"], 3, 1, dtype=torch.float64)
    image, _ = R.render(torch.from_numpy(sc["means"]), torch.from_numpy(sc["covs"]), ones, torch.from_numpy(sc["opac"]),
                        torch.from_numpy(sc["cams"]), torch.zeros(sc["V"], 3), sc["H"], sc["W"], torch.float64, use_sh=False)
    want = np.log(sc["far"].astype(np.float64))[:, None, None] * image[:, 0].numpy()
    assert np.abs(o64["depth"] - want).max() < 1e-12 and want.max() > 1.0


def test_relative_disparity_is_0_at_near_and_1_at_far():
    near, far = np.array([0.5], np.float32), np.array([10.0], np.float32)
    means = torch.tensor([[0.0, 0.0, 0.5], [0.0, 0.0, 10.0], [0.3, -0.2, 2.0]], dtype=torch.float32)
    for dtype, tol in ((torch.float64, 1e-9), (torch.float32, 2e-7)):
        v = D.fake_colour(means, np.eye(4, dtype=np.float32)[None], near, far, "relative_disparity", dtype)[0]
        assert abs(float(v[0])) <= tol and float(v[1]) == 1.0 and 0.0 < float(v[2]) < 1.0
    with pytest.raises(ValueError):
        D.fake_colour(means, np.eye(4, dtype=np.float32)[None], near, far, "linear")


@pytest.mark.parametrize("name", ["sh1", "sh4"])
def test_scene_conditions_hold_in_every_mode(name):
    """Finite in every mode; the pixels left out are the colour's (no per-pixel decision depends on a colour) and stay under the
    project's 1 % cap; float32 stays close to float64."""
    _, colour64, _, _ = S.reference(name)
    for mode in D.MODES:
        sc, o64, o32, w = D.reference("case", name, mode)
        left, own = float((~o64["kept"]).mean()), float(np.abs(o32["depth"] - o64["depth"]).max())
        print(f"{name} {mode}: pixels left out {left:.4f}, largest depth {np.abs(o64['depth']).max():.3g}, float32 - float64 {own:.3g}")
        assert np.array_equal(o64["kept"], colour64["kept"]) and left <= S.MAX_LEFT_OUT
        assert np.isfinite(o64["depth"]).all() and np.isfinite(o32["depth"]).all() and own < 1e-5
        assert all(np.isfinite(g).all() for g in o64["grads"] + o32["grads"])
        assert torch.equal(o64["info"]["ok"], colour64["info"]["ok"]) and o64["info"]["keys"] == colour64["info"]["keys"]


def test_the_operators_and_the_functional_form_refuse_cpu_tensors():
    from mvsdet_amd import functional as F_
    from mvsdet_amd.ops import splat
    sc = S.SPECIAL["cap"]()
    t = {k: torch.from_numpy(sc[k]) for k in ("means", "covs", "sh", "opac", "cams", "bg", "extrinsics", "intrinsics", "near", "far")}
    H, W = sc["H"], sc["W"]
    assert splat.DEPTH_MODES == D.MODES and splat.SPLAT_SLOT == 9 and splat.SPLAT_SLOT_DEPTH == 10
    with pytest.raises((RuntimeError, NotImplementedError), match="ROCm device|CPU"):
        splat.rasterize_depth(t["means"], t["covs"], t["sh"], t["opac"], t["cams"], t["near"], t["far"], t["bg"], H, W, 64, True, "depth")
    with pytest.raises((RuntimeError, NotImplementedError), match="ROCm device|CPU"):
        splat.depth_only(t["means"], t["covs"], t["opac"], t["cams"], t["near"], t["far"], H, W, 64, "depth")
    with pytest.raises((RuntimeError, NotImplementedError), match="ROCm device|CPU"):
        F_.render_depth_cuda(t["extrinsics"], t["intrinsics"], t["near"], t["far"], (H, W), t["means"][None], t["covs"][None], t["opac"][None])
    with pytest.raises(ValueError, match="mode"):
        F_.render_depth_cuda(t["extrinsics"], t["intrinsics"], t["near"], t["far"], (H, W), t["means"][None], t["covs"][None], t["opac"][None],
                             mode="linear")


def test_argument_errors_of_the_depth_entry_points_return_without_launching():
    """Fake pointers, as in test_splat_host.py: every call must return before anything is launched or read."""
    from mvsdet_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    s2, s3 = (ctypes.c_int64 * 2)(3, 1), (ctypes.c_int64 * 3)(9, 3, 1)
    # means, strides, covariances, strides, harmonics, strides, opacities, stride, cams, near, far, background, image, depth, values, workspace, bytes
    fwd = (one, s2, one, s3, one, s3, one, 1, one, one, one, one, one, one, one, one, 1 << 30)
    sizes = lambda V=1, G=8, d_sh=4, use_sh=1, colour=1, depth=1, mode=0, H=16, W=16, keys=64: (  # noqa: E731
        V, G, d_sh, use_sh, colour, depth, mode, H, W, keys, None)
    f = lib.mvsdet_splat_forward_f32
    for mode in (-1, 4):
        assert f(*fwd, *sizes(mode=mode)) == 1 and b"mode" in lib.mvsdet_last_error()
    assert f(*fwd, *sizes(d_sh=5)) == 1 and b"d_sh" in lib.mvsdet_last_error()
    assert f(*fwd, *sizes(keys=0)) == 1 and b"bad sizes" in lib.mvsdet_last_error()
    # 9 V max_keys fits, 10 V max_keys does not
    keys = 220_000_000
    assert 9 * keys < 2 ** 31 <= 10 * keys
    assert f(*fwd, *sizes(keys=keys)) == 1 and b"10 V max_keys" in lib.mvsdet_last_error()
    for i in (0, 2, 6, 8, 9, 10, 13, 14, 15):                       # means, covariances, opacities, cams, near, far, depth, values, workspace
        assert f(*fwd[:i], None, *fwd[i + 1:], *sizes()) == 1 and b"NULL" in lib.mvsdet_last_error(), i
    for i in (4, 11, 12):                                           # harmonics, background, image: needed with colour only
        assert f(*fwd[:i], None, *fwd[i + 1:], *sizes()) == 1 and b"NULL" in lib.mvsdet_last_error(), i
    assert f(*fwd[:16], 64, *sizes()) == 2 and b"workspace" in lib.mvsdet_last_error()
    assert f(*fwd[:4], None, None, *fwd[6:11], None, None, *fwd[13:16], 64, *sizes(colour=0)) == 2      # depth alone: past the NULL check
    # backward: ..., background, g_image, g_depth, values, workspace, bytes, slots, g_means, g_covariances, g_harmonics, g_opacities
    bwd = (one, s2, one, s3, one, s3, one, 1, one, one, one, one, one, one, one, one, 1 << 30, one, one, one, one, one)
    b = lib.mvsdet_splat_backward_f32
    assert b(*bwd, *sizes(mode=7)) == 1 and b"mode" in lib.mvsdet_last_error()
    assert b(*bwd, *sizes(keys=keys)) == 1 and b"10 V max_keys" in lib.mvsdet_last_error()
    for i in (0, 9, 13, 14, 17, 18, 21):                            # means, near, g_depth, values, slots, g_means, g_opacities
        assert b(*bwd[:i], None, *bwd[i + 1:], *sizes()) == 1 and b"NULL" in lib.mvsdet_last_error(), i
    assert b(*bwd[:12], None, *bwd[13:], *sizes()) == 1 and b"NULL" in lib.mvsdet_last_error()          # g_image, with colour
    assert b(*bwd[:16], 64, *bwd[17:], *sizes()) == 2 and b"workspace" in lib.mvsdet_last_error()
    # without depth the limit is 9 V max_keys, mode is not looked at, and near, far, depth, values (g_depth) may be NULL
    plain = (*fwd[:9], None, None, *fwd[11:13], None, None, fwd[15], 64)
    assert f(*plain, *sizes(depth=0, keys=keys)) == 2 and b"workspace" in lib.mvsdet_last_error()
    assert f(*plain, *sizes(depth=0, mode=-1)) == 2 and b"workspace" in lib.mvsdet_last_error()
    assert f(*plain, *sizes(depth=0)) == 2 and b"workspace" in lib.mvsdet_last_error()
    assert b(*bwd[:9], None, None, *bwd[11:13], None, None, bwd[15], 64, *bwd[17:], *sizes(depth=0, keys=keys)) == 2
    for i in (4, 11, 12):                                           # ... but the colour's pointers may not
        assert f(*plain[:i], None, *plain[i + 1:], *sizes(depth=0)) == 1 and b"NULL" in lib.mvsdet_last_error(), i
    # neither colour nor depth: refused before anything else is looked at (the sizes are bad too)
    for fn, head in ((f, fwd), (b, bwd)):
        assert fn(*head, *sizes(colour=0, depth=0, keys=0, mode=9)) == 1 and b"neither colour nor depth" in lib.mvsdet_last_error()
