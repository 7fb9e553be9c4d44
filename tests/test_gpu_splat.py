"""The Gaussian rasteriser on the GPU (csrc/splat.hip through ops.splat, functional.render_cuda / decode_splatting,
mvsdet_amd.diff_gaussian_rasterization, integration.patch_reference_splatting) against the float64 restatement of
tests/splat_restated.py on the seeded scenes of tests/splat_scenes.py, and against fixture G26 (what the reference's own render_cuda
hands its rasteriser, tests/golden/make_goldens_g26.py).

Bars.  Values on kept pixels (splat_scenes.kept) and the gradients of sum(image * g_image * kept): elementwise
max(1e-4 |x| + 1.25e-6 max|x|, 4 x the float32 restatement's own largest distance from float64) -- the rule of DESIGN 4.12.  Culled
Gaussians and the lower triangle of the covariance gradient: exactly 0.  Strided inputs, two runs, functional against the shim: the
same bits.  G26 cameras: 4 x the reference's own fp32 distance from float64, stored in the fixture.  Every test prints its figures
before it asserts (pytest -s); the measured ones are in DESIGN.md 4.15.
"""
import sys
import types

import numpy as np
import pytest
import torch

import splat_restated as R
import splat_scenes as S
from canvas import Guarded
from conftest import load_golden
from splat_checks import NAMES, bits, check_case, compare, dev, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(S.CASES))
def test_image_and_gradients_against_the_restatement(gpu, name):
    """40x56 (3x4 tiles, half tiles last), G = 256, V = 2, d_sh 1 / 4 / 25 with scale_invariant, d_sh 9 without; and 700 Gaussians on
    one 16x16 tile (several LDS batches in both directions, pixels that stop early)."""
    from mvsdet_amd.ops import splat
    sc, o64, o32, w = S.reference(name)
    image, grads, ws = check_case(sc, o64, o32, w, gpu)
    st = splat.status(ws, sc["V"])
    print("keys", [s["needed"] for s in st], "of", st[0]["capacity"], "per Gaussian", [s["needed"] / sc["G"] for s in st])
    assert [s["needed"] for s in st] == o64["info"]["keys"] and not any(s["overflow"] for s in st)
    radii = splat.radii(ws, sc["V"], sc["G"]).cpu().numpy()
    assert np.array_equal(radii > 0, o64["info"]["ok"].numpy())
    if name == "one_tile":
        assert int(o64["info"]["n_contrib"].max()) > 256 and bool(o64["info"]["stopped"].any())


def test_culled_gaussians_get_exactly_zero_gradient(gpu):
    """Behind the camera, z just under and just over the near bound 0.2, far off-screen, an empty tile rectangle just outside the
    image: all but the one just over 0.2 are culled; their four gradients are exactly 0 and the picture is the restatement's."""
    sc, o64, o32, w = S.special_reference("culled")
    assert o64["info"]["ok"][0].tolist() == [False, False, True, False, False, True, True]
    assert float(S.gaussian_margin(sc["means"], sc["covs"], sc["sh"], sc["opac"], sc["cams"], sc["H"], sc["W"]).min()) >= S.MARGIN
    image, grads, _ = check_case(sc, o64, o32, w, gpu)
    for n, g in zip(NAMES, grads):
        for i in (0, 1, 3, 4):
            assert np.array_equal(bits(g[i]), np.zeros_like(bits(g[i]))), (n, i)
    assert np.abs(grads[0][2]).max() > 0 and np.abs(grads[3][2]) > 0


def test_opacity_zero_and_the_cap_at_a_pixel_centre(gpu):
    """Opacity 0: skipped everywhere (alpha < 1/255), every gradient exactly 0.  Opacity 1 with its centre exactly on pixel (20,16):
    opacity * exp(0) = 1 is capped at 0.99 and the gradient passes through the cap, as the restatement's straight-through does."""
    sc, o64, o32, w = S.special_reference("cap")
    p = R.preprocess(*[torch.from_numpy(sc[k]).double() for k in NAMES], torch.from_numpy(sc["cams"][0]), sc["H"], sc["W"])
    assert float(p["px"][1]) == 20.0 and float(p["py"][1]) == 16.0
    assert bool(o64["kept"][0, 16, 20])
    image, grads, _ = check_case(sc, o64, o32, w, gpu)
    for n, g in zip(NAMES, grads):
        assert np.array_equal(bits(g[0]), np.zeros_like(bits(g[0]))), n
    assert abs(float(grads[3][1])) > 0      # d / d opacity of the capped Gaussian is not cut off


def test_a_stack_of_opaque_gaussians_stops_the_pixel(gpu):
    """Six Gaussians of opacity 0.95 centred on pixel (20,16): T goes 0.05, 0.0025, 1.25e-4, and the fourth would take it under 1e-4,
    so the pixel stops there.  With a loss on that pixel alone, the fourth, fifth and sixth get exactly zero gradient."""
    sc, o64, o32, w = S.special_reference("stack")
    assert bool(o64["info"]["stopped"][0, 16, 20]) and int(o64["info"]["n_contrib"][0, 16, 20]) == 3 and bool(o64["kept"][0, 16, 20])
    image, grads, _ = check_case(sc, o64, o32, w, gpu)
    for n, g in zip(NAMES, grads):
        assert np.array_equal(bits(g[3:]), np.zeros_like(bits(g[3:]))), n
        if n in ("sh", "opac"):          # at the very centre (dx = dy = 0) the mean and the covariance have no first-order effect
            assert np.abs(g[:3]).max() > 0, n


def test_equal_depths_follow_the_index_order(gpu):
    """Five overlapping Gaussians of one depth (bit-equal p_view.z) between a nearer and a farther one: blended in index order."""
    sc, o64, o32, w = S.special_reference("equal_depths")
    check_case(sc, o64, o32, w, gpu)


def test_equal_depths_keep_the_index_order_in_a_long_sort(gpu):
    """4096 Gaussians of ONE bit-equal depth on a 32x32 image: the sort runs over the capacity, 32 768 keys, the size class of the
    training shape's sort (multi-block), not the single block of the small cases.  Their blend order must still be the index order.
    No CPU restatement (4096 sequential Gaussians would take too long): the same Gaussians at depths that RISE by one float32 step
    per index are ordered by depth alone, and those 4096 steps change the depth by at most 4.9e-4 relative -- projections within 16 px
    of the axis move by under 0.008 px and the 2-D covariances (sigma about 2 px) by 1e-3 relative, which changes an alpha by at most
    about 1.6 % and can flip a pixel's alpha / stop decision (worth under 0.004 each); 0.02 bounds that with room.  Depths that FALL
    with the index reverse the order: other Gaussians decide every pixel, and the picture moves by tenths."""
    from mvsdet_amd.ops import splat
    G, z = 4096, np.float32(2.0)
    rng = np.random.RandomState(31)
    means = np.stack([rng.uniform(-0.5, 0.5, G), rng.uniform(-0.4, 0.4, G), np.full(G, z)], -1).astype(np.float32)
    sc = S.special(means, np.broadcast_to(np.eye(3, dtype=np.float32) * 0.15 ** 2, (G, 3, 3)), rng.uniform(0.3, 0.9, G), H=32, W=32)
    step = np.spacing(z) * np.arange(G, dtype=np.float32)
    rising, falling = means.copy(), means.copy()
    rising[:, 2] += step
    falling[:, 2] += step[::-1]
    assert len(np.unique(rising[:, 2])) == G and float(step[-1] / z) < 4.9e-4
    equal, _, ws = run(sc, gpu)
    st = splat.status(ws, 1)[0]
    up, _, _ = run(dict(sc, means=rising), gpu)
    down, _, _ = run(dict(sc, means=falling), gpu)
    d_up, d_down = float(np.abs(equal - up).max()), float(np.abs(equal - down).max())
    print(f"keys {st['needed']} of {st['capacity']}; equal depths against rising {d_up:.3g}, against falling {d_down:.3g}")
    assert st["capacity"] == 8 * G and not st["overflow"] and st["needed"] > 2 * G
    assert d_up < 0.02 and d_down > 0.2


def test_strided_inputs_and_two_runs_give_the_same_bits(gpu):
    sc, o64, o32, w = S.reference("sh25")
    first = run(sc, gpu, w)
    second = run(sc, gpu, w)
    assert np.array_equal(bits(first[0]), bits(second[0]))
    for a, b in zip(first[1], second[1]):
        assert np.array_equal(bits(a), bits(b))
    G, d = sc["G"], sc["d_sh"]
    nan = float("nan")
    means = torch.full((G, 5), nan, device=gpu)[:, 1:4]
    covs = torch.full((G, 3, 4, 2), nan, device=gpu)[:, :, :3, 1]
    sh = torch.full((G, d, 3), nan, device=gpu).permute(0, 2, 1)          # the extension's (G, d_sh, 3) layout, read in place
    opac = torch.full((G, 3), nan, device=gpu)[:, 2]
    for t, k in zip((means, covs, sh, opac), NAMES):
        t.copy_(dev(sc[k], gpu))
        assert not t.is_contiguous()
    strided = run(sc, gpu, w, leaves=[means, covs, sh, opac])
    assert np.array_equal(bits(first[0]), bits(strided[0]))
    for a, b in zip(first[1], strided[1]):
        assert np.array_equal(bits(a), bits(b))


def test_no_host_synchronisation(gpu):
    from mvsdet_amd import functional as F_
    sc, o64, o32, w = S.reference("sh4")
    args = [dev(sc[k], gpu) for k in ("extrinsics", "intrinsics", "near", "far")]
    leaves = [dev(sc[k], gpu).requires_grad_(True) for k in NAMES]
    bg, wd = dev(sc["bg"], gpu), dev(w, gpu)

    def step():
        V = sc["V"]
        image = F_.render_cuda(*args, (sc["H"], sc["W"]), bg, *[t[None].expand(V, *t.shape) for t in leaves])
        (image * wd).sum().backward()
        return image
    step()                                   # warm: library load, operator registration, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        image = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(image).all()


def test_too_small_a_key_capacity_gives_nan_and_says_so(gpu):
    """max_keys below the need of view 0 (and of view 1): image and workspace in guarded canvases -- nothing is written outside, the
    images are NaN, the status words say so, the gradients are NaN; a second call with the default capacity is correct."""
    from mvsdet_amd.ops import splat
    sc, o64, o32, w = S.reference("sh4")
    need = o64["info"]["keys"]
    small = min(need) - 7
    V, G, H, W = sc["V"], sc["G"], sc["H"], sc["W"]
    nbytes = splat.workspace_bytes(V, G, H, W, small)
    ws = Guarded(nbytes // 4, gpu)
    out = Guarded(V * 3 * H * W, gpu)
    image = out.region.view(torch.float32).view(V, 3, H, W)
    leaves = [dev(sc[k], gpu) for k in NAMES]
    splat.rasterize_into(*leaves, dev(sc["cams"], gpu), dev(sc["bg"], gpu), H, W, small, True, image, ws.region)
    torch.cuda.synchronize()
    assert ws.guards_intact() and out.guards_intact()
    assert bool(torch.isnan(image).all())
    st = splat.status(ws.region, V)
    print("status", st)
    assert [s["needed"] for s in st] == need and all(s["overflow"] and s["capacity"] == small for s in st)
    # one view fits, the other does not: the first is right, the second NaN
    mid = (min(need) + max(need)) // 2 if need[0] != need[1] else None
    if mid is not None:
        img, _, wsm = run(sc, gpu, None, max_keys=mid)
        fits = [n <= mid for n in need]
        for v in range(V):
            assert bool(np.isnan(img[v]).all()) != fits[v]
    # through autograd: NaN image, NaN gradients
    img, grads, ws2 = run(sc, gpu, w, max_keys=small)
    iu = np.triu_indices(3)
    assert np.isnan(img).all() and all(np.isnan(g[:, iu[0], iu[1]] if n == "covs" else g).all() for n, g in zip(NAMES, grads))
    check_case(sc, o64, o32, w, gpu)


def test_cameras_and_render_cuda_against_g26(gpu):
    """Fixture G26: the reference's own render_cuda on the CPU, for a single shared K, per-view non-square K and scale_invariant off.
    Our camera kernel against the matrices it handed its rasteriser (bar: 4 x the reference's own fp32 distance from float64, and never
    under one rounding to float32, 2^-24 of the largest entry: the kernel rounds float64 values once), and functional.render_cuda on the fixture's inputs against the float64 restatement fed with what the
    reference handed over (its scaled means and 6-vector covariances, scale 1)."""
    from mvsdet_amd import functional as F_
    from mvsdet_amd.ops import splat
    g = load_golden("g26_splat")
    for tag in [str(t) for t in g["cases"]]:
        c = {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + ".")}
        V, G = c["extrinsics"].shape[0], c["means"].shape[1]
        H, W = (int(v) for v in c["image_shape"])
        si = bool(c["scale_invariant"])
        cams = splat.splat_cameras(*[dev(c[k], gpu) for k in ("extrinsics", "intrinsics", "near", "far")], si).cpu().numpy()
        for name, got, want in (("viewmatrix", cams[:, :16], c["viewmatrix"].reshape(V, 16)),
                                ("projmatrix", cams[:, 16:32], c["projmatrix"].reshape(V, 16)),
                                ("tanfov", cams[:, 32:34], c["tanfov"]), ("campos", cams[:, 34:37], c["campos"])):
            bar = max(4.0 * float(c["own_" + name]), 2.0 ** -24 * float(np.abs(want).max()))   # never under one rounding to float32
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"{tag} {name}: kernel-reference {err:.3g}  bar {bar:.3g}")
            assert err <= bar, (tag, name)
        assert int(c["degree"]) == int(round(c["sh"].shape[-1] ** 0.5)) - 1
        # the picture: restatement on what the reference handed its rasteriser
        handed = np.zeros((V, R.CAM), np.float32)
        handed[:, :16], handed[:, 16:32] = c["viewmatrix"].reshape(V, 16), c["projmatrix"].reshape(V, 16)
        handed[:, 32:34], handed[:, 34:37], handed[:, 37] = c["tanfov"], c["campos"], 1.0
        images = F_.render_cuda(*[dev(c[k], gpu) for k in ("extrinsics", "intrinsics", "near", "far")], (H, W), dev(c["bg"], gpu),
                                *[dev(c[k], gpu) for k in ("means", "covs", "sh", "opac")], scale_invariant=si).cpu().numpy()
        iu = np.triu_indices(3)
        for v in range(V):
            cov = np.zeros((G, 3, 3), np.float32)
            cov[:, iu[0], iu[1]] = c["handed_cov6"][v]
            cov = cov + np.triu(cov, 1).transpose(0, 2, 1)
            sc = dict(means=c["handed_means"][v], covs=cov, sh=c["sh"][v], opac=c["opac"][v], cams=handed[v:v + 1], bg=c["bg"][v:v + 1], H=H, W=W)
            o64, _, _ = S.restate(sc, torch.float64, grad=False)
            o32, _, _ = S.restate(sc, torch.float32, grad=False)
            assert (~o64["kept"]).mean() <= S.MAX_LEFT_OUT
            keep = np.broadcast_to(o64["kept"][:, None], (1, 3, H, W))
            compare(f"{tag} view {v}", images[v:v + 1], o64["image"], o32["image"], keep)


def reference_way(sc, gpu, cams, leaves):
    """cuda_splatting.py:66-138 with the shim's classes and a given camera block: scaled copies, one rasteriser per view."""
    from mvsdet_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    means, covs, sh, opac = leaves
    V = sc["V"]
    scale = cams[:, 37]
    covs = covs[None] * (scale[:, None, None, None] ** 2)
    means = means[None] * scale[:, None, None]
    shs = sh[None].expand(V, *sh.shape).permute(0, 1, 3, 2).contiguous()
    images = []
    for i in range(V):
        settings = GaussianRasterizationSettings(image_height=sc["H"], image_width=sc["W"], tanfovx=cams[i, 32], tanfovy=cams[i, 33],
                                                 bg=dev(sc["bg"], gpu)[i], scale_modifier=1.0, viewmatrix=cams[i, :16].view(4, 4),
                                                 projmatrix=cams[i, 16:32].view(4, 4), sh_degree=int(round(sc["d_sh"] ** 0.5)) - 1,
                                                 campos=cams[i, 34:37], prefiltered=False, debug=False)
        row, col = torch.triu_indices(3, 3)
        image, radii = GaussianRasterizer(settings)(means3D=means[i], means2D=torch.zeros_like(means[i], requires_grad=True), shs=shs[i],
                                                    colors_precomp=None, opacities=opac[..., None], cov3D_precomp=covs[i][:, row, col])
        assert radii.dtype == torch.int32 and tuple(radii.shape) == (sc["G"],)
        images.append(image)
    return torch.stack(images)


def test_render_cuda_gives_the_bits_of_the_shim_called_the_reference_way(gpu):
    from mvsdet_amd import functional as F_
    from mvsdet_amd.ops import splat
    sc, o64, o32, w = S.reference("sh25")
    V = sc["V"]
    cam_args = [dev(sc[k], gpu) for k in ("extrinsics", "intrinsics", "near", "far")]
    wd = dev(w, gpu)
    a = [dev(sc[k], gpu).requires_grad_(True) for k in NAMES]
    image_a = F_.render_cuda(*cam_args, (sc["H"], sc["W"]), dev(sc["bg"], gpu), *[t[None].expand(V, *t.shape) for t in a])
    (image_a * wd).sum().backward()
    b = [dev(sc[k], gpu).requires_grad_(True) for k in NAMES]
    image_b = reference_way(sc, gpu, splat.splat_cameras(*cam_args, True), b)
    (image_b * wd).sum().backward()
    assert np.array_equal(bits(image_a), bits(image_b))
    # distinct batch rows (copies) go one call per row: the same pictures
    image_c = F_.render_cuda(*cam_args, (sc["H"], sc["W"]), dev(sc["bg"], gpu), *[t.detach()[None].repeat(V, *([1] * t.dim())) for t in a])
    assert np.array_equal(bits(image_a), bits(image_c))
    # gradients: the kernel's sums over the views against autograd's over the per-view calls -- the same terms in another order
    for n, x, y in zip(NAMES, a, b):
        gx, gy = x.grad.cpu().numpy(), y.grad.cpu().numpy()
        scale_ = np.abs(gx).max()
        print(f"d {n}: one call - per view {np.abs(gx - gy).max():.3g} of {scale_:.3g}")
        assert np.abs(gx - gy).max() <= 4e-6 * scale_, n
    # ... and the restatement, through the camera kernel instead of the scene's own camera block
    keep = np.broadcast_to(o64["kept"][:, None], o64["image"].shape)
    err = np.abs(image_a.detach().cpu().numpy() - o64["image"])[keep].max()
    print("functional against the restatement", err)
    assert err < 2e-5

    class Gs:
        means, covariances, harmonics, opacities = [t.detach()[None] for t in a]
    colour = F_.decode_splatting(Gs, cam_args[0][None], cam_args[1][None], cam_args[2][None], cam_args[3][None], (sc["H"], sc["W"]),
                                 dev(sc["bg"][0], gpu))
    assert tuple(colour.shape) == (1, V, 3, sc["H"], sc["W"])
    one_bg = F_.render_cuda(*cam_args, (sc["H"], sc["W"]), dev(sc["bg"][:1], gpu).expand(V, 3), *[t.detach()[None].expand(V, *t.shape) for t in a])
    assert np.array_equal(bits(colour[0]), bits(one_bg))


def test_precomputed_colours(gpu):
    """use_sh = False: the (G,3,1) coefficients are the colours -- no basis, no + 0.5, no clamp (negative colours stay)."""
    sc, _, _, _ = S.reference("sh1")
    o64, o32, w = S.with_gradients(sc, use_sh=False)
    assert o64["image"].min() < 0
    check_case(sc, o64, o32, w, gpu, use_sh=False)


def test_refusals_and_autocast(gpu):
    from mvsdet_amd import functional as F_
    from mvsdet_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from mvsdet_amd.ops import splat
    sc, o64, _, _ = S.reference("sh4")
    leaves = [dev(sc[k], gpu) for k in NAMES]
    cams, bg = dev(sc["cams"], gpu), dev(sc["bg"], gpu)
    H, W, keys = sc["H"], sc["W"], splat.default_max_keys(sc["G"])
    with pytest.raises(ValueError, match="d_sh"):
        splat.rasterize(leaves[0], leaves[1], leaves[2][:, :, :3], leaves[3], cams, bg, H, W, keys, True)
    with pytest.raises(ValueError, match="precomputed"):
        splat.rasterize(*leaves, cams, bg, H, W, keys, False)
    with pytest.raises(TypeError, match="float32"):
        splat.rasterize(leaves[0].double(), *leaves[1:], cams, bg, H, W, keys, True)
    with pytest.raises(ValueError, match="cams"):
        splat.rasterize(*leaves, cams[:, :39], bg, H, W, keys, True)
    with pytest.raises(ValueError, match="max_keys"):
        splat.rasterize(*leaves, cams, bg, H, W, 0, True)
    with pytest.raises(RuntimeError, match="no gradient"):
        splat.rasterize(*leaves, cams.clone().requires_grad_(True), bg, H, W, keys, True)
    settings = GaussianRasterizationSettings(H, W, 0.5, 0.5, bg[0], 1.0, cams[0, :16].view(4, 4), cams[0, 16:32].view(4, 4), 1, cams[0, 34:37])
    with pytest.raises(NotImplementedError, match="scales / rotations"):
        GaussianRasterizer(settings)(means3D=leaves[0], means2D=None, opacities=leaves[3][:, None], shs=leaves[2].permute(0, 2, 1),
                                     scales=leaves[0], rotations=torch.zeros(sc["G"], 4, device=gpu))
    with pytest.raises(ValueError, match="exactly one"):
        GaussianRasterizer(settings)(means3D=leaves[0], means2D=None, opacities=leaves[3][:, None], cov3D_precomp=torch.zeros(sc["G"], 6, device=gpu))
    # under autocast low-precision inputs are computed in float32
    V = sc["V"]
    args = [dev(sc[k], gpu) for k in ("extrinsics", "intrinsics", "near", "far")]
    batch = [t[None].expand(V, *t.shape) for t in leaves]
    plain = F_.render_cuda(*args, (H, W), bg, batch[0], batch[1], batch[2].half().float(), batch[3])
    with torch.autocast("cuda", dtype=torch.float16):
        amp = F_.render_cuda(*args, (H, W), bg, batch[0], batch[1], batch[2].half(), batch[3])
    assert amp.dtype == torch.float32 and np.array_equal(bits(plain), bits(amp))
    with pytest.raises(TypeError, match="float32"):
        F_.render_cuda(*args, (H, W), bg, batch[0], batch[1], batch[2].half(), batch[3])


def test_opt_in_patch_on_a_stand_in(gpu):
    """integration.patch_reference_splatting registers the shim as `diff_gaussian_rasterization` (the real extension is not
    installed) and rebinds the two classes of a module that imported them; a stand-in for cuda_splatting.py then renders through
    the HIP rasteriser; unpatching takes both back."""
    from mvsdet_amd import diff_gaussian_rasterization as shim
    from mvsdet_amd import integration
    from mvsdet_amd.ops import splat
    assert integration.SPLATTING_EXTENSION not in sys.modules
    stand_in = types.ModuleType("cuda_splatting_stand_in")
    stand_in.GaussianRasterizer = "theirs"
    state = integration.patch_reference_splatting(stand_in)
    try:
        import diff_gaussian_rasterization as registered
        assert registered is shim and stand_in.GaussianRasterizer is shim.GaussianRasterizer
        assert stand_in.GaussianRasterizationSettings is shim.GaussianRasterizationSettings
        sc, o64, o32, w = S.reference("sh4")
        cams = dev(sc["cams"], gpu)
        image = reference_way(sc, gpu, cams, [dev(sc[k], gpu) for k in NAMES]).cpu().numpy()
        keep = np.broadcast_to(o64["kept"][:, None], image.shape)
        compare("stand-in", image, o64["image"], o32["image"], keep)
    finally:
        integration.unpatch_reference_splatting(state)
    assert integration.SPLATTING_EXTENSION not in sys.modules and stand_in.GaussianRasterizer == "theirs"
    assert not hasattr(stand_in, "GaussianRasterizationSettings")
