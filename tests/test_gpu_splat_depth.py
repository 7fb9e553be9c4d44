"""The rendered depth of the Gaussian rasteriser on the GPU (csrc/splat.hip through ops.splat.rasterize_depth / depth_only,
functional.render_depth_cuda / decode_splatting(depth_mode=), MVSDetHotPath.novel_views(depth_mode=) / nvs_scores) against the
float64 restatement of tests/splat_depth_restated.py on the seeded scenes of tests/splat_scenes.py, against the colour-only rasteriser
that the parent already had, and against fixture G28 (what the reference's own render_depth_cuda hands its rasteriser).

Bars.  Depth on kept pixels and the gradients of sum(depth * g_depth * kept): the colour's bar, splat_restated.bar -- elementwise
max(1e-4 |x| + 1.25e-6 max|x|, 4 x the float32 restatement's own largest distance from float64).  Fused against separate, the
reference's route on our own kernels, strided inputs, two runs, expanded against distinct rows: the same bits.  G28: 4 x the
reference's own fp32 distance from float64, stored in the fixture.  Culled Gaussians: exactly 0.  Every test prints its figures
before it asserts (pytest -s); the measured ones are in DESIGN.md 4.18.
"""
import numpy as np
import pytest
import torch

import splat_depth_restated as D
import splat_restated as R
import splat_scenes as S
from conftest import load_golden
from splat_checks import bits, compare, dev, run

pytestmark = pytest.mark.gpu

COLOUR = ("means", "covs", "sh", "opac")


def cam_args(sc, gpu):
    return dev(sc["cams"], gpu), dev(sc["near"], gpu), dev(sc["far"], gpu)


def run_depth(sc, gpu, mode, weights=None, max_keys=None, leaves=None):
    """ops.splat.depth_only on a scene -> depth, the three gradients (numpy), values, workspace."""
    from mvsdet_amd.ops import splat
    leaves = [dev(sc[k], gpu) for k in D.NAMES] if leaves is None else leaves
    leaves = [t.detach().requires_grad_(True) for t in leaves]
    keys = splat.default_max_keys(sc["G"]) if max_keys is None else max_keys
    depth, values, ws = splat.depth_only(*leaves, *cam_args(sc, gpu), sc["H"], sc["W"], keys, mode)
    assert not values.requires_grad and not ws.requires_grad and depth.dtype == torch.float32
    assert tuple(depth.shape) == (sc["V"], sc["H"], sc["W"]) and tuple(values.shape) == (sc["V"], sc["G"])
    grads = None
    if weights is not None:
        grads = [g.cpu().numpy() for g in torch.autograd.grad((depth * dev(weights, gpu)).sum(), leaves)]
    return depth.detach().cpu().numpy(), grads, values.cpu().numpy(), ws


def run_fused(sc, gpu, mode, w_image=None, w_depth=None, max_keys=None, leaves=None):
    """ops.splat.rasterize_depth -> image, depth, the four gradients of sum(image w_image) + sum(depth w_depth), values, workspace."""
    from mvsdet_amd.ops import splat
    leaves = [dev(sc[k], gpu) for k in COLOUR] if leaves is None else leaves
    leaves = [t.detach().requires_grad_(True) for t in leaves]
    keys = splat.default_max_keys(sc["G"]) if max_keys is None else max_keys
    cams, near, far = cam_args(sc, gpu)
    image, depth, values, ws = splat.rasterize_depth(*leaves, cams, near, far, dev(sc["bg"], gpu), sc["H"], sc["W"], keys, True, mode)
    grads = None
    if w_image is not None:
        grads = [g.cpu().numpy() for g in torch.autograd.grad((image * dev(w_image, gpu)).sum() + (depth * dev(w_depth, gpu)).sum(), leaves)]
    return image.detach().cpu().numpy(), depth.detach().cpu().numpy(), grads, values.cpu().numpy(), ws


def check_depth(sc, o64, o32, w, gpu, mode, tag=""):
    depth, grads, values, ws = run_depth(sc, gpu, mode, w)
    compare(f"{tag}{mode} depth", depth, o64["depth"], o32["depth"], o64["kept"])
    for n, g, g64, g32 in zip(D.NAMES, grads, o64["grads"], o32["grads"]):
        compare(f"{tag}{mode} d {n}", g, g64, g32)
    lower = grads[1][:, [1, 2, 2], [0, 0, 1]]
    assert np.array_equal(bits(lower), np.zeros_like(bits(lower)))
    return depth, grads, values, ws


# ------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("name", ["sh1", "sh4", "sh25"])
def test_depth_and_gradients_against_the_restatement(gpu, name, mode):
    """40x56 (3x4 tiles, half tiles last), G = 256, V = 2, in the four modes: depth, and the gradients in means, covariances and
    opacities, against render_depth in float64; the returned values against fake_colour on the Gaussians that are not culled."""
    from mvsdet_amd.ops import splat
    sc, o64, o32, w = D.reference("case", name, mode)
    depth, grads, values, ws = check_depth(sc, o64, o32, w, gpu, mode, name + " ")
    ok = o64["info"]["ok"].numpy()
    assert np.array_equal(splat.radii(ws, sc["V"], sc["G"]).cpu().numpy() > 0, ok)
    assert [s["needed"] for s in splat.status(ws, sc["V"])] == o64["info"]["keys"]
    compare(f"{name} {mode} values", values, o64["values"], o32["values"], ok)
    assert np.array_equal(bits(values[~ok]), np.zeros_like(bits(values[~ok])))


# ------------------------------------------------------------------------------------------- 2. fused equals separate
@pytest.mark.parametrize("mode", ["disparity", "log"])
def test_the_fused_call_equals_the_separate_ones(gpu, mode):
    sc, o64, o32, w = S.reference("sh25")
    wd = D.g_depth(sc)
    image, depth, _, values, _ = run_fused(sc, gpu, mode)
    alone, g_colour, _ = run(sc, gpu, sc["g_image"])
    d_alone, g_depth, v_alone, _ = run_depth(sc, gpu, mode, wd)
    assert np.array_equal(bits(image), bits(alone)) and np.array_equal(bits(depth), bits(d_alone)) and np.array_equal(bits(values), bits(v_alone))
    zero_i, zero_d = np.zeros_like(sc["g_image"]), np.zeros_like(wd)
    _, _, with_image, _, _ = run_fused(sc, gpu, mode, sc["g_image"], zero_d)
    for n, a, b in zip(COLOUR, with_image, g_colour):
        assert np.array_equal(a, b), n
    _, _, with_depth, _, _ = run_fused(sc, gpu, mode, zero_i, wd)
    for n, a, b in zip(D.NAMES, [with_depth[0], with_depth[1], with_depth[3]], g_depth):
        assert np.array_equal(a, b), n
    assert np.array_equal(with_depth[2], np.zeros_like(with_depth[2]))
    # an output that received no gradient at all: the backward of the form that has the other one alone
    from mvsdet_amd.ops import splat
    leaves = [dev(sc[k], gpu).requires_grad_(True) for k in COLOUR]
    cams, near, far = cam_args(sc, gpu)
    img, dep, _, _ = splat.rasterize_depth(*leaves, cams, near, far, dev(sc["bg"], gpu), sc["H"], sc["W"], splat.default_max_keys(sc["G"]), True, mode)
    for n, a, b in zip(COLOUR, torch.autograd.grad((img * dev(sc["g_image"], gpu)).sum(), leaves, retain_graph=True), g_colour):
        assert np.array_equal(bits(a), bits(b)), n
    only = torch.autograd.grad((dep * dev(wd, gpu)).sum(), leaves)
    for n, a, b in zip(D.NAMES, [only[0], only[1], only[3]], g_depth):
        assert np.array_equal(bits(a), bits(b)), n


# ------------------------------------------------------------------------------------------- 3. the reference's route on our own kernels
@pytest.mark.parametrize("mode", ["depth", "disparity", "relative_disparity"])
def test_equals_the_reference_s_route_through_the_colour_rasteriser(gpu, mode):
    """render_depth_cuda's own way -- the value as three equal precomputed colour channels through the colour rasteriser, one view at a
    time because the value differs per view, black background, channel 0 -- gives the bits of the new depth when fed the returned
    values; with the value built by torch operations from the means on the GPU, autograd chains it, and the means' gradient of the new
    call meets that route's under the bar."""
    from mvsdet_amd.ops import splat
    sc, o64, o32, w = D.reference("case", "sh4", mode)
    depth, grads, values, _ = run_depth(sc, gpu, mode, w)
    V, G, H, W = sc["V"], sc["G"], sc["H"], sc["W"]
    cams, keys, black = dev(sc["cams"], gpu), splat.default_max_keys(G), torch.zeros(1, 3, device=gpu)
    means, covs, opac = (dev(sc[k], gpu).requires_grad_(True) for k in D.NAMES)
    made = D.fake_colour(means, sc["extrinsics"], sc["near"], sc["far"], mode, torch.float32)
    route, chained = [], []
    for v in range(V):
        given = dev(values[v], gpu)[:, None, None].expand(G, 3, 1)
        route.append(splat.rasterize(means, covs, given, opac, cams[v:v + 1], black, H, W, keys, False)[0][0, 0])
        chained.append(splat.rasterize(means, covs, made[v][:, None, None].expand(G, 3, 1), opac, cams[v:v + 1], black, H, W, keys, False)[0][0].mean(0))
    assert np.array_equal(bits(torch.stack(route)), bits(depth))
    g_route = torch.autograd.grad((torch.stack(chained) * dev(w, gpu)).sum(), [means])[0].cpu().numpy()
    bar, own = R.bar(o64["grads"][0], o32["grads"][0])
    err = np.abs(grads[0].astype(np.float64) - g_route)
    print(f"{mode} d means: new call - the route {err.max():.3g} of {np.abs(g_route).max():.3g}, worst err/bar {(err / bar).max():.3f}")
    assert (err <= bar).all()


# ------------------------------------------------------------------------------------------- 4. G28
def test_values_against_g28(gpu):
    """What the reference's unmodified render_depth_cuda handed its rasteriser as colors_precomp, in the four modes, with and without
    scale_invariant: our per-Gaussian values within 4 x the reference's own fp32 distance from float64; culled Gaussians excluded."""
    from mvsdet_amd.ops import splat
    g = load_golden("g28_splat_depth")
    for tag in [str(t) for t in g["cases"]]:
        c = {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + ".")}
        V, G = c["extrinsics"].shape[0], c["means"].shape[0]
        H, W = (int(v) for v in c["image_shape"])
        near, far = dev(c["near"], gpu), dev(c["far"], gpu)
        cams = splat.splat_cameras(dev(c["extrinsics"], gpu), dev(c["intrinsics"], gpu), near, far, bool(c["scale_invariant"]))
        for mode in D.MODES:
            _, values, ws = splat.depth_only(*[dev(c[k], gpu) for k in D.NAMES], cams, near, far, H, W, splat.default_max_keys(G), mode)
            seen = splat.radii(ws, V, G).cpu().numpy() > 0
            assert np.array_equal(seen, c["visible"])
            want, own = c[mode + ".colors_precomp"][..., 0].astype(np.float64), float(c[mode + ".own"])
            err = float(np.abs(values.cpu().numpy().astype(np.float64) - want)[seen].max())
            print(f"{tag} {mode}: kernel - reference {err:.3g}  bar {4.0 * own:.3g}  (largest value {np.abs(want[seen]).max():.3g})")
            assert err <= 4.0 * own, (tag, mode)


# ------------------------------------------------------------------------------------------- 5. edges
@pytest.mark.parametrize("name", [f"list{n}" for n in S.LIST_LENGTHS])
def test_tile_lists_around_the_lds_batches(gpu, name):
    """One 16x16 tile with a list of 63 .. 257 entries: one under, at and one over the backward's batch of 64 and the forward's of
    256, where the depth's extra LDS word and the tenth slot are staged and reduced."""
    sc, o64, o32, w = D.reference("edge", name, "disparity")
    check_depth(sc, o64, o32, w, gpu, "disparity", name + " ")


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (16, 17)])
def test_small_images(gpu, hw):
    sc, o64, o32, w = D.reference("edge", f"small{hw[0]}x{hw[1]}", "relative_disparity")
    check_depth(sc, o64, o32, w, gpu, "relative_disparity", f"small{hw[0]}x{hw[1]} ")


@pytest.mark.parametrize("mode", ["depth", "disparity"])
def test_culled_gaussians_get_exactly_zero_gradient(gpu, mode):
    """Behind the camera (1 / z and -1 / z^2 are finite there, and would not be 0), just under the near bound, off-screen, an empty
    tile rectangle: exactly 0 in every gradient and in the returned values, in the fused form too."""
    sc, o64, o32, w = D.reference("special", "culled", mode)
    assert o64["info"]["ok"][0].tolist() == [False, False, True, False, False, True, True]
    depth, grads, values, _ = check_depth(sc, o64, o32, w, gpu, mode, "culled ")
    _, _, fused, _, _ = run_fused(sc, gpu, mode, sc["g_image"], D.g_depth(sc))
    for g in grads + fused:
        for i in (0, 1, 3, 4):
            assert np.array_equal(bits(g[i]), np.zeros_like(bits(g[i])))
    assert np.array_equal(bits(values[0, [0, 1, 3, 4]]), np.zeros(4, np.int32))
    assert np.abs(grads[0][2]).max() > 0 and np.abs(grads[2][2]) > 0


def test_the_early_stop_is_shared_by_the_depth_channel(gpu):
    """Six Gaussians of opacity 0.95 on pixel (20,16): the pixel stops after three.  With the depth's loss on that pixel alone the
    fourth, fifth and sixth get exactly zero gradient, and the depth there is the restatement's sum of three."""
    sc, o64, o32, w = D.reference("special", "stack", "depth")
    assert bool(o64["info"]["stopped"][0, 16, 20]) and int(o64["info"]["n_contrib"][0, 16, 20]) == 3 and bool(o64["kept"][0, 16, 20])
    assert np.count_nonzero(w) == 1 and w[0, 16, 20] != 0
    depth, grads, _, _ = check_depth(sc, o64, o32, w, gpu, "depth", "stack ")
    for n, g in zip(D.NAMES, grads):
        assert np.array_equal(bits(g[3:]), np.zeros_like(bits(g[3:]))), n
    assert np.abs(grads[2][:3]).min() > 0 and np.abs(grads[0][:3, 2]).min() > 0       # opacity, and z through the value itself


def test_one_key_under_the_need_gives_a_nan_depth_on_that_view_only(gpu):
    from mvsdet_amd.ops import splat
    sc, o64, _, _ = D.reference("case", "sh4", "depth")
    need = o64["info"]["keys"]
    big = int(np.argmax(need))
    small = max(need) - 1
    assert min(need) <= small and sc["V"] == 2
    whole, _, _, _ = run_depth(sc, gpu, "depth")
    depth, grads, values, ws = run_depth(sc, gpu, "depth", D.g_depth(sc), max_keys=small)
    st = splat.status(ws, 2)
    print("status", st)
    assert [s["overflow"] for s in st] == [v == big for v in range(2)] and [s["needed"] for s in st] == need
    assert np.isnan(depth[big]).all() and np.array_equal(bits(depth[1 - big]), bits(whole[1 - big]))
    iu = np.triu_indices(3)
    assert np.isnan(grads[0]).all() and np.isnan(grads[1][:, iu[0], iu[1]]).all() and np.isnan(grads[2]).all()
    image, fused, _, _, ws = run_fused(sc, gpu, "depth", max_keys=small)
    assert np.isnan(fused[big]).all() and np.isnan(image[big]).all() and np.array_equal(bits(fused[1 - big]), bits(whole[1 - big]))


# ------------------------------------------------------------------------------------------- 6. strides and repeatability
def test_strided_inputs_and_two_runs_give_the_same_bits(gpu):
    sc, _, _, _ = S.reference("sh25")
    wd = D.g_depth(sc)
    first = run_fused(sc, gpu, "relative_disparity", sc["g_image"], wd)
    second = run_fused(sc, gpu, "relative_disparity", sc["g_image"], wd)
    G, d = sc["G"], sc["d_sh"]
    nan = float("nan")
    means = torch.full((G, 5), nan, device=gpu)[:, 1:4]
    covs = torch.full((G, 3, 4, 2), nan, device=gpu)[:, :, :3, 1]
    sh = torch.full((G, d, 3), nan, device=gpu).permute(0, 2, 1)
    opac = torch.full((G, 3), nan, device=gpu)[:, 2]
    for t, k in zip((means, covs, sh, opac), COLOUR):
        t.copy_(dev(sc[k], gpu))
        assert not t.is_contiguous()
    strided = run_fused(sc, gpu, "relative_disparity", sc["g_image"], wd, leaves=[means, covs, sh, opac])
    alone = run_depth(sc, gpu, "relative_disparity", wd)
    alone_strided = run_depth(sc, gpu, "relative_disparity", wd, leaves=[means, covs, opac])
    for other in (second, strided):
        assert np.array_equal(bits(first[0]), bits(other[0])) and np.array_equal(bits(first[1]), bits(other[1]))
        assert np.array_equal(bits(first[3]), bits(other[3]))
        for a, b in zip(first[2], other[2]):
            assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(alone[0]), bits(alone_strided[0]))
    for a, b in zip(alone[1], alone_strided[1]):
        assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------- 7. no host synchronisation
def test_no_host_synchronisation(gpu):
    from mvsdet_amd import functional as F_
    sc, _, _, _ = S.reference("sh4")
    V = sc["V"]
    args = [dev(sc[k], gpu) for k in ("extrinsics", "intrinsics", "near", "far")]
    leaves = [dev(sc[k], gpu).requires_grad_(True) for k in COLOUR]
    wi, wd = dev(sc["g_image"], gpu), dev(D.g_depth(sc), gpu)

    class Gs:
        means, covariances, harmonics, opacities = [t[None] for t in leaves]

    def step():
        colour, depth = F_.decode_splatting(Gs, *[t[None] for t in args], (sc["H"], sc["W"]), depth_mode="disparity")
        alone = F_.render_depth_cuda(*args, (sc["H"], sc["W"]), *[leaves[i][None].expand(V, *leaves[i].shape) for i in (0, 1, 3)], mode="log")
        ((colour[0] * wi).sum() + (depth[0] * wd).sum() + (alone * wd).sum()).backward()
        return depth, alone
    step()                                   # warm: library load, operator registration, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        depth, alone = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(depth).all() and torch.isfinite(alone).all()


# ------------------------------------------------------------------------------------------- 8. call forms
def test_render_depth_cuda_and_decode_splatting(gpu):
    from mvsdet_amd import functional as F_
    from mvsdet_amd.ops import splat
    sc, o64, o32, _ = D.reference("case", "sh4", "disparity")
    V, H, W = sc["V"], sc["H"], sc["W"]
    args = [dev(sc[k], gpu) for k in ("extrinsics", "intrinsics", "near", "far")]
    leaves = [dev(sc[k], gpu) for k in COLOUR]
    three = [leaves[i] for i in (0, 1, 3)]
    expanded = F_.render_depth_cuda(*args, (H, W), *[t[None].expand(V, *t.shape) for t in three], mode="disparity")
    distinct = F_.render_depth_cuda(*args, (H, W), *[t[None].repeat(V, *([1] * t.dim())) for t in three], mode="disparity")
    assert tuple(expanded.shape) == (V, H, W) and np.array_equal(bits(expanded), bits(distinct))
    compare("render_depth_cuda", expanded.cpu().numpy(), o64["depth"], o32["depth"], o64["kept"])      # through the camera kernel
    with pytest.raises(ValueError, match="mode"):
        F_.render_depth_cuda(*args, (H, W), *[t[None].expand(V, *t.shape) for t in three], mode="linear")

    class Gs:
        means, covariances, harmonics, opacities = [t[None] for t in leaves]
    batch = [t[None] for t in args]
    colour = F_.decode_splatting(Gs, *batch, (H, W), dev(sc["bg"][0], gpu))
    both = F_.decode_splatting(Gs, *batch, (H, W), dev(sc["bg"][0], gpu), depth_mode="disparity")
    assert isinstance(colour, torch.Tensor) and isinstance(both, tuple) and len(both) == 2
    assert tuple(both[0].shape) == (1, V, 3, H, W) and tuple(both[1].shape) == (1, V, H, W)
    assert np.array_equal(bits(both[0]), bits(colour)) and np.array_equal(bits(both[1][0]), bits(expanded))
    with pytest.raises(ValueError, match="depth_mode"):
        F_.decode_splatting(Gs, *batch, (H, W), depth_mode="linear")
    # refusals, fakes, autocast
    cams, near, far = cam_args(sc, gpu)
    bg, keys = dev(sc["bg"], gpu), splat.default_max_keys(sc["G"])
    with pytest.raises(ValueError, match="mode"):
        splat.depth_only(*three, cams, near, far, H, W, keys, "linear")
    for bad in ("cams", "near", "far", "background"):
        extra = {"cams": cams, "near": near, "far": far, "background": bg}
        extra[bad] = extra[bad].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="no gradient"):
            splat.rasterize_depth(*leaves, extra["cams"], extra["near"], extra["far"], extra["background"], H, W, keys, True, "depth")
        if bad != "background":
            with pytest.raises(RuntimeError, match="no gradient"):
                splat.depth_only(*three, extra["cams"], extra["near"], extra["far"], H, W, keys, "depth")
    with pytest.raises(ValueError, match="near"):
        splat.depth_only(*three, cams, near[:1], far, H, W, keys, "depth")
    with pytest.raises(TypeError, match="float32"):
        splat.depth_only(three[0].double(), three[1], three[2], cams, near, far, H, W, keys, "depth")
    ops_ = torch.ops.mvsdet_amd
    _, _, values, ws = splat.rasterize_depth(*leaves, cams, near, far, bg, H, W, keys, True, "depth")
    g_image, g_dep = torch.ones(V, 3, H, W, device=gpu), torch.ones(V, H, W, device=gpu)
    for op, a in ((ops_.splat_rasterize_depth, (*leaves, cams, near, far, bg, H, W, keys, True, "depth")),
                  (ops_.splat_depth_only, (*three, cams, near, far, H, W, keys, "depth")),
                  (ops_.splat_rasterize_depth_backward, (*leaves, cams, near, far, bg, values, ws, g_image, g_dep, H, W, keys, True, "depth")),
                  (ops_.splat_depth_only_backward, (*three, cams, near, far, values, ws, g_dep, H, W, keys, "depth"))):
        torch.library.opcheck(op.default, a, test_utils=("test_schema", "test_faketensor"))
    half = [three[0][None].expand(V, -1, -1), three[1][None].expand(V, -1, -1, -1).half(), three[2][None].expand(V, -1)]
    want = F_.render_depth_cuda(*args, (H, W), half[0], half[1].float(), half[2], mode="disparity")
    with torch.autocast("cuda", dtype=torch.float16):
        amp = F_.render_depth_cuda(*args, (H, W), *half, mode="disparity")
    assert amp.dtype == torch.float32 and np.array_equal(bits(amp), bits(want))
    with pytest.raises(TypeError, match="float32"):
        F_.render_depth_cuda(*args, (H, W), *half, mode="disparity")


def test_novel_views_with_a_depth_mode_and_the_scores(gpu):
    """MVSDetHotPath.novel_views(depth_mode=) on the 4-view scene of test_gpu_adapter.py (5 x 8 feature pixels, two 24x32 targets): the
    colour keeps its bits, the depth is finite and (1,n_tgt,H,W), a backward through depth.sum() reaches to_gaussians' parameters, and
    nvs_scores with the depth pair gives save_rendered_depth's rmse."""
    from types import SimpleNamespace

    from mvsdet_amd import functional as F_
    from mvsdet_amd import synthetic
    from mvsdet_amd.evaluation import NVSEvaluator
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, hw, L = 4, 8, (6, 8), 1
    meta = synthetic.make_img_meta(N, hw, seed=5)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    gen = torch.Generator().manual_seed(3)
    feature = torch.randn(N, C, *hw, generator=gen).to(gpu).requires_grad_(True)
    depth_coding = (1.0 + 2.0 * torch.rand(N, 1, h, w, generator=gen)).to(gpu).requires_grad_(True)
    opacity = torch.rand(N, *hw, generator=gen).to(gpu).requires_grad_(True)
    rgb_raw = torch.rand(1, N, h * w, 3, generator=gen).to(gpu)
    outputs = dict(geometry=SimpleNamespace(height=h, width=w), depth_coding=depth_coding, opacity=opacity)
    torch.manual_seed(4)
    to_gaussians = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(C + 1 + 3, 2 + 7 + 3 * (L + 1) ** 2)).to(gpu)
    c2w = np.linalg.inv(np.array(meta["lidar2img"]["extrinsic"], np.float64))
    tgt = c2w[[0, 2]].copy()
    tgt[:, :3, 3] += 0.05
    Kt = np.array([[40.0, 0, 16.0, 0], [0, 40.0, 12.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    colour = hp.novel_views(outputs, feature, meta, to_gaussians, tgt, Kt, (24, 32, 3), rgb_raw, sh_degree=L)
    both = hp.novel_views(outputs, feature, meta, to_gaussians, tgt, Kt, (24, 32, 3), rgb_raw, sh_degree=L, depth_mode="depth")
    assert isinstance(both, tuple) and np.array_equal(bits(both[0]), bits(colour))
    depth = both[1]
    assert tuple(depth.shape) == (1, 2, 24, 32) and bool(torch.isfinite(depth).all()) and float(depth.detach().max()) > 0
    grads = torch.autograd.grad(depth.sum(), [to_gaussians[1].weight, to_gaussians[1].bias, depth_coding])
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    with pytest.raises(ValueError, match="depth_mode"):
        hp.novel_views(outputs, feature, meta, to_gaussians, tgt, Kt, (24, 32, 3), rgb_raw, sh_degree=L, depth_mode="linear")
    gt_rgb = torch.rand(2, 3, 24, 32, generator=gen).to(gpu)
    gt_depth = (1.0 + torch.rand(2, 24, 32, generator=gen)).to(gpu)
    want = F_.save_rendered_depth(depth.detach()[0], gt_depth)
    without = hp.nvs_scores(colour.detach(), gt_rgb)
    scores = hp.nvs_scores(colour.detach(), gt_rgb, depth_preds=depth.detach(), gt_depth=gt_depth)
    ev = NVSEvaluator(gpu)
    fed = hp.nvs_scores(colour.detach(), gt_rgb, ev, depth.detach(), gt_depth)
    print("rmse", float(scores["rmse"]), "save_rendered_depth", float(want))
    assert float(without["rmse"]) == 0.0 and float(want) > 0
    # float64 sums of the same 2 x 768 float32 terms: another association moves them by at most 1536 x 2^-53 relative
    for got in (float(scores["rmse"]), float(fed["rmse"]), ev.compute()["rmse"]):
        assert abs(got - float(want)) <= 1e-12 * float(want)
    assert float(scores["psnr"]) == float(without["psnr"]) and float(scores["ssim"]) == float(without["ssim"])
    with pytest.raises(ValueError, match="pair"):
        hp.nvs_scores(colour.detach(), gt_rgb, depth_preds=depth.detach())
