"""Photometric consistency (mvs_models/homography.py, MVSDet.warp_img / photometric_loss, mvsdet.py:701-768, 845-874) without a GPU:
the restatement of tests/photo_loss_restated.py against fixture G25 -- what the reference itself returns, and its autograd's gradient
(tests/golden/make_goldens_g25.py) --, the CPU route of the four functionals, the restatement's gradient against central differences,
and the host side of the new entry points: refusals, argument checks, fake kernels, the opt-in patch.

Bars: masks exact; everything else 4 x the reference-to-restatement distance the generator stored per case and quantity, floor 1e-6
relative (photo_loss_restated.bar); gradients relative to the largest magnitude of the reference's.  Every test prints its figures.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import photo_loss_restated as R
from conftest import load_golden


@pytest.fixture(scope="module")
def g25():
    return load_golden("g25_photo_loss")


def restated(c, dtype=np.float64):
    r = R.loss_and_depth_grad(c["img"], c["left_cam"], c["right_cam"], c["depth"], c["ref"], c["simple"], dtype)
    pc = r if not c["simple"] else R.loss_and_depth_grad(c["img"], c["left_cam"], c["right_cam"], c["depth"], c["ref"], False, dtype)
    return dict(warped=r["warped"], mask=r["mask"], L=r["L"], loss_pc=pc["loss_pc"], grad=pc["grad"], mag=r["aux"]["mag"], r=r)


def reference(c):
    r = R.loss_and_depth_grad(c["img"], c["left_cam"], c["right_cam"], c["depth"], c["ref"], c["simple"])
    return dict(warped=c["warped"], mask=c["mask"], L=c["L"], loss_pc=c["loss_pc"], grad=c["grad"], mag=r["aux"]["mag"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "fp32_order"])
@pytest.mark.parametrize("tag", R.SINGLE_CASES)
def test_restatement_matches_the_reference_on_g25(g25, tag, dtype):
    c = g25_case = R.g25_case(g25, tag)
    r = restated(g25_case, dtype)
    R.check_against(c, r["warped"], r["mask"], r["L"], r["loss_pc"], r["grad"], reference(c), f"{tag} restatement ({dtype.__name__}) vs G25")


@pytest.mark.parametrize("tag,n", R.MULTI_CASES)
def test_restatement_selects_scenes_as_the_reference(g25, tag, n):
    cs = [R.g25_case(g25, f"{tag}[{i}]") for i in range(n)]
    rs = [R.loss_and_depth_grad(c["img"], c["left_cam"], c["right_cam"], c["depth"], c["ref"]) for c in cs]
    loss, gws, wins, L = R.photometric_loss([r["warped"] for r in rs], [r["mask"] for r in rs], [c["ref"] for c in cs])
    rel = abs(float(loss) - float(g25[f"{tag}:loss_pc"])) / abs(float(g25[f"{tag}:loss_pc"]))
    print(f"{tag}: loss_pc {float(loss)!r} reference {float(g25[f'{tag}:loss_pc'])!r} relative {rel:.2e} wins {wins.tolist()}")
    assert np.array_equal(wins, g25[f"{tag}:wins"]) and np.all(wins > 0)
    assert rel <= R.bar(g25[f"{tag}:dist_loss_pc"])
    for i, (c, r) in enumerate(zip(cs, rs)):
        grad = np.sum(np.where(gws[i] != 0, gws[i] * r["aux"]["dwarped"], 0), axis=-1)
        d = float(np.abs(grad - c["grad"]).max() / np.abs(c["grad"]).max())
        print(f"{tag}[{i}]: grad {d:.2e} (bar {R.bar(c['dist_grad']):.2e})")
        assert d <= R.bar(c["dist_grad"]) and np.all(grad[c["mask"][..., 0] == 0] == 0)


def test_fixture_margins_hold(g25):
    """No mask bit, no floor and no smooth-L1 branch of G25 hangs on one ulp: the generator's conditions, measured again."""
    for tag in R.SINGLE_CASES + [f"{t}[{i}]" for t, n in R.MULTI_CASES for i in range(n)]:
        c = R.g25_case(g25, tag)
        x, y, _, _, p2 = R.project(c["left_cam"], c["right_cam"], c["depth"])
        h, w = c["depth"].shape[1:]
        border = np.minimum(np.minimum(np.abs(x), np.abs(x - (w - 1))), np.minimum(np.abs(y), np.abs(y - h))).min()
        near = (x > -1) & (x < w) & (y > -1) & (y < h + 1)
        integer = np.where(near, np.minimum(np.abs(x - np.round(x)), np.abs(y - np.round(y))), 1.0).min()
        r = R.loss_and_depth_grad(c["img"], c["left_cam"], c["right_cam"], c["depth"], c["ref"], c["simple"])
        gap = min(float(np.abs(np.abs(v) - 1).min()) for v in (r["args"][:1] if c["simple"] else r["args"]))
        print(f"{tag}: border {border:.2e} integer {integer:.2e} |p2| {np.abs(p2).min():.2e} ||d|-1| {gap:.2e}")
        assert border >= 1e-3 and integer >= 1e-4 and np.abs(p2).min() >= 1e-2 and gap >= 1e-4, tag
    b = R.g25_case(g25, "behind")
    p2 = R.project(b["left_cam"], b["right_cam"], b["depth"])[4]
    assert ((p2 < 0) & (b["mask"][..., 0] != 0)).sum() > 8 and (p2 > 0).sum() > 8          # the mask follows the formula behind the camera
    lr = R.g25_case(g25, "lastrow")
    y = R.project(lr["left_cam"], lr["right_cam"], lr["depth"])[1]
    assert ((np.floor(y) == lr["depth"].shape[1] - 1) & (lr["mask"][..., 0] != 0)).sum() >= 4   # y0 = H-1 is valid
    s = R.g25_case(g25, "small")
    a = np.concatenate([np.abs(v).ravel() for v in R.loss_and_depth_grad(s["img"], s["left_cam"], s["right_cam"], s["depth"], s["ref"])["args"]])
    assert (a > 1).sum() > 10 and (a < 1).sum() > 10                                        # both smooth-L1 branches
    assert not np.array_equal(s["left_cam"][:, 1], s["right_cam"][:, 1])                    # per-view intrinsics: K_left for both shows
    assert np.isnan(g25["ref_true:depth_pad"][:, :, 59:, :]).all() and np.isnan(g25["ref_true:depth_pad"][:, :, :, 80:]).all()


def _leaf(a):
    return torch.from_numpy(np.ascontiguousarray(a)).clone().requires_grad_(True)


@pytest.mark.parametrize("tag", [t for t in R.SINGLE_CASES if t != "warp_img"])
def test_functional_cpu_route_equals_g25(g25, tag):
    from mvsdet_amd import functional as F_
    c = R.g25_case(g25, tag)
    depth = _leaf(c["depth"][:, None])
    warped, mask = F_.inverse_warping(torch.from_numpy(c["img"]), torch.from_numpy(c["left_cam"]), torch.from_numpy(c["right_cam"]), depth)
    ref = torch.from_numpy(c["ref"])
    L = F_.compute_reconstr_loss(warped, ref, mask, simple=c["simple"])
    loss = F_.photometric_loss([warped], [mask], [ref])["loss_pc"]
    loss.backward()
    R.check_against(c, warped.detach().numpy(), mask.numpy(), L.detach().numpy(), loss.detach().numpy(), depth.grad[:, 0].numpy(),
                    reference(c), f"{tag} functional (CPU) vs G25")


def test_functional_warp_img_cpu_route_equals_g25(g25):
    from mvsdet_amd import functional as F_
    c = R.g25_case(g25, "warp_img")
    s = c["scene"]
    depth = _leaf(s["depth"][:, None])
    warped, mask, chosen = F_.warp_img(torch.from_numpy(s["imgs"]), torch.from_numpy(s["neighbor_ids"]), torch.from_numpy(s["w2c"]),
                                       torch.from_numpy(s["K"]), depth, ref_id=torch.from_numpy(s["ref_id"]))
    assert np.array_equal(chosen.numpy(), c["chosen"])
    L = F_.compute_reconstr_loss(warped, chosen, mask, simple=False)
    loss = F_.photometric_loss([warped], [mask], [chosen])["loss_pc"]
    loss.backward()
    g = depth.grad[:, 0].numpy()
    R.check_against(c, warped.detach().numpy(), mask.numpy(), L.detach().numpy(), loss.detach().numpy(), g[s["ref_id"]], reference(c),
                    "warp_img functional (CPU) vs G25")
    # the selection without ref_id: torch.randperm on the CPU, the reference's draw for this seed
    torch.manual_seed(2522)
    w2, m2, _ = F_.warp_img(torch.from_numpy(s["imgs"]), torch.from_numpy(s["neighbor_ids"]), torch.from_numpy(s["w2c"]),
                            torch.from_numpy(s["K"]), torch.from_numpy(s["depth"])[:, None])
    assert np.array_equal(w2.numpy(), warped.detach().numpy()) and np.array_equal(m2.numpy(), mask.numpy())


@pytest.mark.parametrize("tag,n", R.MULTI_CASES)
def test_functional_cpu_route_selects_scenes_as_g25(g25, tag, n):
    from mvsdet_amd import functional as F_
    cs = [R.g25_case(g25, f"{tag}[{i}]") for i in range(n)]
    leaves = [_leaf(c["depth"][:, None]) for c in cs]
    wm = [F_.inverse_warping(torch.from_numpy(c["img"]), torch.from_numpy(c["left_cam"]), torch.from_numpy(c["right_cam"]), d)
          for c, d in zip(cs, leaves)]
    loss = F_.photometric_loss([w for w, _ in wm], [m for _, m in wm], [torch.from_numpy(c["ref"]) for c in cs])["loss_pc"]
    loss.backward()
    rel = abs(float(loss) - float(g25[f"{tag}:loss_pc"])) / abs(float(g25[f"{tag}:loss_pc"]))
    print(f"{tag}: loss_pc relative {rel:.2e} (bar {R.bar(g25[f'{tag}:dist_loss_pc']):.2e})")
    assert rel <= R.bar(g25[f"{tag}:dist_loss_pc"])
    for c, d in zip(cs, leaves):
        assert float(np.abs(d.grad[:, 0].numpy() - c["grad"]).max() / np.abs(c["grad"]).max()) <= R.bar(c["dist_grad"])


def test_one_scene_is_L_times_the_mean_of_the_mask(g25):
    c = R.g25_case(g25, "tiny")
    assert abs(float(c["loss_pc"]) - float(c["L"]) * float(c["mask"].mean())) <= 1e-6 * float(c["loss_pc"])
    r = restated(c)
    assert abs(float(r["loss_pc"]) - float(r["L"]) * float(r["mask"].mean())) <= 1e-12


def test_restated_gradient_against_central_differences():
    """d loss_pc / d depth of the restatement on a 3x5 map: central differences in float64, step 1e-6 m (no floor is crossed: the
    coordinates stay 1e-3 px away from the integers)."""
    from golden.make_goldens_g25 import make_depth, make_images, make_views, packed, settle_depth
    B, h, w = 2, 3, 5
    w2c, K = make_views(2 * B, h, w, 77, per_view_k=True)
    left, right = packed(w2c, K, np.arange(B)), packed(w2c, K, np.arange(B, 2 * B))
    img, ref = make_images(B, h, w, 2, 78, amp=3.0)[1], make_images(B, h, w, 2, 79, amp=3.0)[1]
    depth = settle_depth(left, right, make_depth(B, h, w, 80), "fd")[0].astype(np.float64)
    r = R.loss_and_depth_grad(img, left, right, depth, ref)
    assert 0 < r["mask"].sum() < r["mask"].size
    x, y = r["aux"]["x"], r["aux"]["y"]
    assert min(np.abs(x - np.round(x)).min(), np.abs(y - np.round(y)).min()) >= 1e-4
    num = np.zeros_like(depth)
    eps = 1e-6
    for idx in np.ndindex(*depth.shape):
        up, dn = depth.copy(), depth.copy()
        up[idx] += eps
        dn[idx] -= eps
        num[idx] = (float(R.loss_and_depth_grad(img, left, right, up, ref)["loss_pc"]) -
                    float(R.loss_and_depth_grad(img, left, right, dn, ref)["loss_pc"])) / (2 * eps)
    err = float(np.abs(num - r["grad"]).max() / np.abs(r["grad"]).max())
    print(f"central differences: {err:.2e} of the largest gradient {np.abs(r['grad']).max():.3g}")
    assert err <= 1e-6
    assert np.all(r["grad"][r["mask"][..., 0] == 0] == 0)


def test_arguments_that_carry_no_gradient_are_refused():
    from mvsdet_amd import functional as F_
    img, cam, depth = torch.rand(2, 3, 4, 3), torch.eye(4)[:3].repeat(2, 2, 1, 1), torch.ones(2, 1, 3, 4)
    for bad in ("img", "left_cam", "right_cam"):
        args = dict(img=img, left_cam=cam, right_cam=cam)
        args[bad] = args[bad].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="no gradient"):
            F_.inverse_warping(args["img"], args["left_cam"], args["right_cam"], depth)
    with pytest.raises(RuntimeError, match="no gradient"):
        F_.compute_reconstr_loss(torch.rand(2, 3, 4, 3), torch.rand(2, 3, 4, 3, requires_grad=True), torch.ones(2, 3, 4, 1))
    with pytest.raises(RuntimeError, match="no gradient"):
        F_.warp_img(torch.rand(3, 3, 12, 16, requires_grad=True), torch.tensor([[1], [2], [0]]), torch.eye(4).repeat(3, 1, 1), torch.eye(4),
                    torch.ones(3, 1, 3, 4))
    with pytest.raises(ValueError, match="2,3,4"):
        F_.inverse_warping(img, cam[:, :1], cam, depth)
    with pytest.raises(ValueError, match="depth"):
        F_.inverse_warping(img, cam, cam, torch.ones(2, 1, 4, 4))
    with pytest.raises(ValueError, match="mask"):
        F_.compute_reconstr_loss(torch.rand(2, 3, 4, 3), torch.rand(2, 3, 4, 3), torch.ones(2, 3, 4))
    with pytest.raises(ValueError, match="0 warped"):
        F_.photometric_loss([], [], [])
    with pytest.raises(ValueError, match="one shape"):
        F_.photometric_loss([torch.rand(1, 3, 4, 3), torch.rand(1, 3, 5, 3)], [torch.ones(1, 3, 4, 1)] * 2, [torch.rand(1, 3, 4, 3)] * 2)
    with pytest.raises(ValueError, match="neighbor_ids"):
        F_.warp_img(torch.rand(3, 3, 12, 16), torch.tensor([1, 2, 0]), torch.eye(4).repeat(3, 1, 1), torch.eye(4), torch.ones(3, 1, 3, 4))


def test_operator_registrations_and_fakes():
    """torch.ops.mvsdet_amd.inverse_warp / reconstr_loss / photometric_select and their backward operators: names of ops.photo, not
    re-exported by the package; fake kernels with the documented shapes and dtypes; no CPU kernel."""
    from mvsdet_amd import ops
    from mvsdet_amd.ops import photo
    for name in ("photo_geometry", "inverse_warp", "inverse_warp_backward", "reconstr_loss", "reconstr_loss_backward", "photometric_select",
                 "photometric_select_backward"):
        assert not hasattr(ops, name)
        assert getattr(photo, name)._opoverload is getattr(torch.ops.mvsdet_amd, name).default
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)   # noqa: E731
    idx = m(10, dtype=torch.int64)
    geo = torch.ops.mvsdet_amd.photo_geometry(m(12, 4, 4), m(4, 4), m(12, 4, 4), idx, idx)
    assert geo.shape == (10, photo.PHOTO_GEO) and geo.dtype == torch.float32
    assert torch.ops.mvsdet_amd.photo_geometry(m(3, 2, 3, 4)[:, 0], m(3, 2, 3, 4)[:, 1], m(3, 2, 3, 4)[:, 0], None, None).shape == (3, 24)
    img, depth = m(12, 3, 60, 80).permute(0, 2, 3, 1)[:, :59], m(12, 1, 60, 81)[:, 0, :59, :80]
    warped, mask = torch.ops.mvsdet_amd.inverse_warp(img, depth, geo, idx, idx)
    assert warped.shape == (10, 59, 80, 3) and mask.shape == (10, 59, 80, 1) and warped.dtype == mask.dtype == torch.float32
    assert torch.ops.mvsdet_amd.inverse_warp_backward(img, depth, geo, idx, idx, warped).shape == (12, 59, 80)
    L, terms, count = torch.ops.mvsdet_amd.reconstr_loss(warped, warped, mask, False)
    assert L.shape == () and terms.shape == (3,) and count.shape == () and count.dtype == torch.int32 and L.dtype == torch.float32
    assert torch.ops.mvsdet_amd.reconstr_loss_backward(warped, warped, mask, L, False).shape == warped.shape
    loss, wins = torch.ops.mvsdet_amd.photometric_select(m(3, 47200), m(3))
    assert loss.shape == () and wins.shape == (3,) and wins.dtype == torch.int32
    assert torch.ops.mvsdet_amd.photometric_select_backward(wins, loss, 47200).shape == (3,)
    with pytest.raises((RuntimeError, NotImplementedError)):
        photo.inverse_warp(torch.ones(1, 3, 4, 2), torch.ones(1, 3, 4), torch.ones(1, 24), None, None)
    with pytest.raises((RuntimeError, NotImplementedError)):
        photo.reconstr_loss(torch.ones(1, 3, 4, 2), torch.ones(1, 3, 4, 2), torch.ones(1, 3, 4, 1), True)
    xg, yg = photo.pixel_grid(59, 80)
    assert xg.shape == (80,) and yg.shape == (59,) and xg.dtype == torch.float32
    # the restatement's fp32 grid follows torch.linspace's formula; ATen's vectorised kernel may round the last bit differently
    assert np.abs(xg.numpy() - R.pixel_grid(80, np.float32)).max() <= 2.0 ** -17 and np.abs(yg.numpy() - R.pixel_grid(59, np.float32)).max() <= 2.0 ** -18
    assert not np.array_equal(xg.numpy(), np.arange(80, dtype=np.float32))      # the linspace grid is not the integers


def test_entry_points_check_arguments_without_launching():
    from mvsdet_amd import _lib
    lib = _lib.load()
    q = lib.mvsdet_photo_loss_workspace_bytes
    assert q(10, 59, 80) == 185 * 32 and q(1, 16, 16) == 32 and q(1, 1, 257) == 64 and q(0, 4, 4) == 0
    s = lib.mvsdet_photo_select_workspace_bytes
    assert s(3, 47200) == 185 * 3 * 4 and s(0, 10) == 0 and s(2, 0) == 0
    one, st4, st3 = ctypes.c_void_p(4096), (ctypes.c_int64 * 4)(60, 20, 4, 1), (ctypes.c_int64 * 3)(12, 4, 1)
    assert lib.mvsdet_photo_geometry_f32(None, 16, one, 0, 4, one, 16, None, None, 2, 2, one, 2, None) == 1 and b"NULL" in lib.mvsdet_last_error()
    assert lib.mvsdet_photo_geometry_f32(one, 16, one, 0, 4, one, 16, None, None, 2, 2, one, 0, None) == 1 and b"bad sizes" in lib.mvsdet_last_error()
    assert lib.mvsdet_photo_geometry_f32(one, 16, one, 0, 2, one, 16, None, None, 2, 2, one, 2, None) == 1 and b"rows" in lib.mvsdet_last_error()

    def warp(img=one, B=2, h=3, w=4, C=3, n_img=2, n_depth=2, idx=None):
        return lib.mvsdet_photo_warp_f32(img, st4, idx, n_img, one, st3, idx, n_depth, one, one, one, one, one, B, h, w, C, None)

    assert warp(img=None) == 1 and b"NULL" in lib.mvsdet_last_error()
    assert warp(h=0) == 1 and b"bad shape" in lib.mvsdet_last_error()
    assert warp(B=1 << 12, h=1 << 10, w=1 << 10) == 1 and b"2^31" in lib.mvsdet_last_error()
    assert warp(n_img=5) == 1 and b"no index" in lib.mvsdet_last_error()
    assert warp(n_depth=5) == 1 and b"no index" in lib.mvsdet_last_error()
    assert lib.mvsdet_photo_warp_bwd_f32(one, st4, None, 2, one, st3, None, 2, one, one, one, None, one, 2, 3, 4, 3, None) == 1
    assert b"NULL" in lib.mvsdet_last_error()

    def loss(ws=one, ws_bytes=1 << 20, B=2, out=one):
        return lib.mvsdet_photo_loss_f32(one, one, one, st4, out, one, one, ws, ws_bytes, B, 3, 4, 3, 0, None)

    assert loss(out=None) == 1 and b"NULL" in lib.mvsdet_last_error()
    assert loss(B=0) == 1 and b"bad shape" in lib.mvsdet_last_error()
    assert loss(ws=ctypes.c_void_p(4100)) == 1 and b"aligned" in lib.mvsdet_last_error()
    assert loss(ws_bytes=31) == 2 and b"workspace" in lib.mvsdet_last_error()
    assert lib.mvsdet_photo_loss_bwd_f32(one, one, one, st4, None, one, 2, 3, 4, 3, 0, None) == 1 and b"NULL" in lib.mvsdet_last_error()
    assert lib.mvsdet_photo_select_f32(one, one, one, one, one, 1 << 20, 33, 100, None) == 1 and b"33 scenes" in lib.mvsdet_last_error()
    assert lib.mvsdet_photo_select_f32(one, one, one, one, one, 3, 2, 100, None) == 2 and b"workspace" in lib.mvsdet_last_error()
    assert lib.mvsdet_photo_select_bwd_f32(one, None, one, 2, 100, None) == 1 and b"NULL" in lib.mvsdet_last_error()


def test_patch_and_unpatch_round_trip_on_a_stand_in():
    """patch_reference_photometric: opt-in, CPU tensors go to the originals, unpatch puts them back; PATCHED_METHODS and the import hook
    do not know it."""
    from mvsdet_amd import integration
    calls = []

    class MVSDet:
        def warp_img(self, ref_imgs, neighbor_ids, ref_w2c, ref_feat_intrinsic, ref_depth):
            """the original warp"""
            calls.append("warp")
            return 1, 2, 3

        def photometric_loss(self, warped_img_list, mask_list, chose_ref_img_list):
            """the original loss"""
            calls.append(len(warped_img_list))
            return dict(loss_pc=-1.0)

    mod = types.SimpleNamespace(MVSDet=MVSDet)
    originals = {k: MVSDet.__dict__[k] for k in ("warp_img", "photometric_loss")}
    assert "warp_img" not in integration.PATCHED_METHODS and "photometric_loss" not in integration.PATCHED_METHODS
    saved = integration.patch_reference_photometric(mod)
    assert sorted(saved) == ["MVSDet.photometric_loss", "MVSDet.warp_img"]
    assert all(saved[f"MVSDet.{k}"] is v and MVSDet.__dict__[k] is not v for k, v in originals.items())
    assert MVSDet.warp_img.__doc__ == "the original warp" and MVSDet.photometric_loss.__doc__ == "the original loss"
    t = torch.ones(1, 3, 4, 4)
    assert MVSDet().warp_img(t, None, None, None, t) == (1, 2, 3)                                    # CPU: the originals
    assert MVSDet().photometric_loss([t], [t], [t]) == dict(loss_pc=-1.0) and MVSDet().photometric_loss([], [], []) == dict(loss_pc=-1.0)
    assert calls == ["warp", 1, 0]
    integration.unpatch_reference_photometric(mod, saved)
    assert all(MVSDet.__dict__[k] is v for k, v in originals.items())
