"""The Gaussian rasteriser (csrc/splat.hip) at the sizes where its own machinery changes form: tile lists at the edges of the LDS
batches (64 in the backward, 256 in the forward), the key capacity exactly at the need, the emit kernel beyond one pass of its grid,
the scan's chunks, the number of sorted key bits, images smaller than or one pixel over a tile, and non-finite inputs.  The scenes are
splat_scenes.EDGES; their conditions (margins, pixels left out, list lengths) are asserted on the CPU in test_splat_host.py.

Bars.  Against the float64 restatement: splat_restated.bar through splat_checks.check_case, as in test_gpu_splat.py.  Two runs of the
kernel against each other: the same bits.  Culled Gaussians: exactly 0.  Every test prints its figures before it asserts (pytest -s);
the measured ones are in DESIGN.md 4.15.
"""
import numpy as np
import pytest
import torch

import splat_scenes as S
from canvas import Guarded
from splat_checks import NAMES, bits, check_case, dev, run

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def zero(a):
    return not bits(a).any()


def needed(ws, V):
    from mvsdet_amd.ops import splat
    return [s["needed"] for s in splat.status(ws, V)]


def guarded_forward(sc, gpu, max_keys):
    """The forward into guarded canvases -> image (numpy), the workspace canvas; asserts that nothing was written outside either."""
    from mvsdet_amd.ops import splat
    V, G, H, W = sc["V"], sc["G"], sc["H"], sc["W"]
    ws = Guarded(splat.workspace_bytes(V, G, H, W, max_keys) // 4, gpu)
    out = Guarded(V * 3 * H * W, gpu)
    image = out.region.view(torch.float32).view(V, 3, H, W)
    splat.rasterize_into(*[dev(sc[k], gpu) for k in NAMES], dev(sc["cams"], gpu), dev(sc["bg"], gpu), H, W, max_keys, True, image, ws.region)
    torch.cuda.synchronize()
    assert ws.guards_intact() and out.guards_intact()
    return image.cpu().numpy(), ws


def check_edge(name, gpu):
    """An edge scene against the restatement: image, the four gradients, the key counts and which Gaussians are culled."""
    from mvsdet_amd.ops import splat
    sc, o64, o32, w = S.edge_reference(name)
    image, grads, ws = check_case(sc, o64, o32, w, gpu)
    st = splat.status(ws, sc["V"])
    print(name, "keys", [s["needed"] for s in st], "of", st[0]["capacity"])
    assert [s["needed"] for s in st] == o64["info"]["keys"] and not any(s["overflow"] for s in st)
    ok = o64["info"]["ok"].numpy()
    assert np.array_equal(splat.radii(ws, sc["V"], sc["G"]).cpu().numpy() > 0, ok)
    for n, g in zip(NAMES, grads):
        assert zero(g[~ok.any(0)]), n
    return sc, o64, image, grads


# ------------------------------------------------------------------------------------------- 1. list lengths
@pytest.mark.parametrize("n", S.LIST_LENGTHS)
def test_list_lengths_at_the_lds_batch_edges(gpu, n):
    """One 16x16 tile whose list has exactly n = 63, 64, 65, 255, 256, 257 entries: one under, at and one over the backward's batch
    of 64 and the forward's of 256.  Some pixel walks all of the list but at most its last entry (test_splat_host.py), so the last,
    partial or one-entry batch is used in both directions."""
    sc, o64, _, _ = check_edge(f"list{n}", gpu)
    assert sc["G"] == n and o64["info"]["keys"] == [n]


# ------------------------------------------------------------------------------------------- 2. capacity at the need
def test_key_capacity_exactly_at_the_need_and_one_under(gpu):
    """sh4 needs M and m keys in its two views.  max_keys = M: no overflow, no padding key in that view, the bits of the
    default-capacity run in image and gradients.  M - 1: that view is NaN and flagged, the other has the default run's bits.  m: as
    M - 1.  m - 1: both NaN.  M and M - 1 also with image and workspace in guarded canvases."""
    from mvsdet_amd.ops import splat
    sc, o64, _, w = S.reference("sh4")
    need = o64["info"]["keys"]
    M, m = max(need), min(need)
    assert M - 1 > m
    image0, grads0, ws0 = run(sc, gpu, w)
    assert needed(ws0, sc["V"]) == need
    iu = np.triu_indices(3)
    for K in (M, M - 1, m, m - 1):
        image, grads, ws = run(sc, gpu, w, max_keys=K)
        st = splat.status(ws, sc["V"])
        print("max_keys", K, "status", st)
        assert [s["needed"] for s in st] == need and all(s["capacity"] == K for s in st)
        for v in range(sc["V"]):
            assert st[v]["overflow"] == (need[v] > K), (K, v)
            if need[v] > K:
                assert np.isnan(image[v]).all(), (K, v)
            else:
                assert same(image[v], image0[v]), (K, v)
        if K == M:
            for n, a, b in zip(NAMES, grads, grads0):
                assert same(a, b), n
        else:
            assert all(np.isnan(g[:, iu[0], iu[1]] if n == "covs" else g).all() for n, g in zip(NAMES, grads))
        if K >= M - 1:
            guarded, _ = guarded_forward(sc, gpu, K)
            assert same(guarded, image)


# ------------------------------------------------------------------------------------------- 3. beyond the emit grid
def on_device(sc, gpu, w, max_keys):
    from mvsdet_amd.ops import splat
    leaves = [dev(sc[k], gpu).requires_grad_(True) for k in NAMES]
    image, ws = splat.rasterize(*leaves, dev(sc["cams"], gpu), dev(sc["bg"], gpu), sc["H"], sc["W"], max_keys, True)
    grads = torch.autograd.grad((image * dev(w, gpu)).sum(), leaves)
    return image.detach(), grads, ws


def test_more_gaussians_than_one_pass_of_the_emit_grid(gpu):
    """V G = 1 200 000 > 4096 x 256: the emit kernel's first loop strides.  sh4's 256 Gaussians at seeded indices of 600 000 (0 and the
    last among them), every other one behind the cameras, max_keys 4096: image, key counts, radii and the gradient rows of the 256
    have the bits of the plain run, every other row and radius is exactly 0 (checked on the device); the forward again into a
    zeroed, guarded workspace."""
    from mvsdet_amd.ops import splat
    sc, o64, _, w = S.reference("sh4")
    G, V = 600_000, sc["V"]
    big, at = S.padded(sc, G, "interleaved", seed=29)
    assert V * G > 4096 * 256 and at[0] == 0 and at[-1] == G - 1 and len(at) == sc["G"]
    image0, grads0, ws0 = on_device(sc, gpu, w, 4096)
    image, grads, ws = on_device(big, gpu, w, 4096)
    st = splat.status(ws, V)
    print("V G", V * G, "status", st)
    assert [s["needed"] for s in st] == o64["info"]["keys"] == needed(ws0, V) and not any(s["overflow"] for s in st)
    assert same(image, image0)
    idx = dev(at, gpu)
    rest = torch.ones(G, dtype=torch.bool, device=gpu)
    rest[idx] = False
    assert int(rest.sum()) == G - sc["G"]
    for n, g, g0 in zip(NAMES, grads, grads0):
        assert same(g[idx], g0), n
        assert not bool(g[rest].view(torch.int32).any()), n
    radii, radii0 = splat.radii(ws, V, G), splat.radii(ws0, V, sc["G"])
    assert same(radii[:, idx], radii0) and not bool(radii[:, rest].any())
    assert np.array_equal(radii0.cpu().numpy() > 0, o64["info"]["ok"].numpy())
    # again into a zeroed workspace: a key that is never written would read as (view 0, tile 0, depth 0), not as what the allocator left
    guarded, _ = guarded_forward(big, gpu, 4096)
    assert same(guarded, image0)


def test_more_keys_than_one_pass_of_the_emit_grid(gpu):
    """V max_keys = 1 200 000 > 4096 x 256: the emit kernel's padding loop strides.  sh4 with max_keys = 600 000: the bits of the
    default-capacity run in image and gradients; the forward again into a zeroed, guarded workspace."""
    sc, o64, _, w = S.reference("sh4")
    image0, grads0, ws0 = run(sc, gpu, w)
    image, grads, ws = run(sc, gpu, w, max_keys=600_000)
    assert sc["V"] * 600_000 > 4096 * 256 and needed(ws, sc["V"]) == o64["info"]["keys"]
    assert same(image, image0)
    for n, a, b in zip(NAMES, grads, grads0):
        assert same(a, b), n
    # again into a zeroed workspace: a padding key that is never written would read as (view 0, tile 0, depth 0) and join tile 0
    guarded, _ = guarded_forward(sc, gpu, 600_000)
    assert same(guarded, image0)


# ------------------------------------------------------------------------------------------- 4. scan chunking
@pytest.mark.parametrize("G", S.PAD_SIZES)
def test_culled_padding_around_the_scan_chunks_changes_no_bit(gpu, G):
    """sh4's 256 Gaussians among culled ones, G = 257 (the scan's chunk becomes 2 and half its threads idle), 511, 513, 1000; the
    padding in front, behind and interleaved: image, key counts and the live gradient rows have the plain run's bits, the padding's
    rows are exactly 0."""
    sc, o64, _, w = S.reference("sh4")
    image0, grads0, ws0 = run(sc, gpu, w)
    for where in ("front", "behind", "interleaved"):
        big, at = S.padded(sc, G, where)
        image, grads, ws = run(big, gpu, w)
        assert needed(ws, sc["V"]) == o64["info"]["keys"], where
        assert same(image, image0), where
        rest = np.setdiff1d(np.arange(G), at)
        for n, g, g0 in zip(NAMES, grads, grads0):
            assert same(g[at], g0) and zero(g[rest]), (where, n)
    print("G", G, "keys", o64["info"]["keys"], "the same bits with the padding in front, behind and interleaved")


@pytest.mark.parametrize("n", (1, 255))
def test_fewer_gaussians_than_scan_threads(gpu, n):
    """sh4 cut to one Gaussian (255 of the scan's threads have none) and to 255 (one has none), against the restatement."""
    check_edge(f"first{n}", gpu)


# ------------------------------------------------------------------------------------------- 5. sorted key bits
@pytest.mark.parametrize("V,H,W", S.BIT_SHAPES)
def test_one_call_over_the_views_against_one_call_per_view(gpu, V, H, W):
    """V tiles = 2, 3, 4, 8, 16: at a power of two the sorted bits must still hold V tiles itself, or the padding keys mix into the
    last tile of the last view.  One call over the V views against V calls of one view: the same image bits, and the gradient is the
    float32 sum of the per-view gradients added in view order from 0 -- the same bits.  With max_keys at the largest need (no
    padding in that view) and one above."""
    sc, o64, _, w = S.edge_reference(f"bits{V}x{H}x{W}")
    need = o64["info"]["keys"]
    tiles = -(-H // 16) * -(-W // 16)
    for K in (max(need), max(need) + 1):
        image, grads, ws = run(sc, gpu, w, max_keys=K)
        assert needed(ws, V) == need
        total = [np.zeros_like(g) for g in grads]
        for v in range(V):
            one = dict(sc, V=1, cams=sc["cams"][v:v + 1], bg=sc["bg"][v:v + 1])
            image_v, grads_v, ws_v = run(one, gpu, w[v:v + 1], max_keys=K)
            assert needed(ws_v, 1) == need[v:v + 1]
            assert same(image[v], image_v[0]), (K, v)
            total = [t + g for t, g in zip(total, grads_v)]
        print(f"V tiles {V * tiles}, max_keys {K}, needs {need}: largest gradients",
              [f"{np.abs(g).max():.3g}" for g in grads], "differ in", [int((bits(a) != bits(b)).sum()) for a, b in zip(grads, total)])
        assert np.isfinite(image).all() and all(t.dtype == np.float32 for t in total)
        for n, a, b in zip(NAMES, grads, total):
            assert same(a, b), (K, n)


# ------------------------------------------------------------------------------------------- 6. small and one-over images
@pytest.mark.parametrize("h,w", S.SMALL_IMAGES)
def test_images_under_a_tile_and_one_pixel_over(gpu, h, w):
    """1x1, 5x7 (under a tile both ways), 16x17 and 17x16 (a tile column / row of one pixel), 15x33, 32x48, against the restatement;
    the forward again into guarded canvases: the same bits, nothing written outside."""
    sc, o64, image, _ = check_edge(f"small{h}x{w}", gpu)
    guarded, _ = guarded_forward(sc, gpu, 8 * sc["G"])
    assert same(guarded, image)


# ------------------------------------------------------------------------------------------- 7. non-finite geometry
def test_non_finite_geometry_culls_that_gaussian_alone(gpu):
    """A Gaussian of sh4 that both views see gets a NaN in a mean coordinate, +-inf as the mean's z, NaN or +inf in an upper-triangle
    covariance entry: it is culled in every view -- the bits of the scene with it behind the cameras in image, key counts and every
    other Gaussian's gradients, exactly 0 in its own, radius 0.  NaN in its covariance's lower triangle: the clean scene's bits."""
    from mvsdet_amd.ops import splat
    sc, o64, _, w = S.reference("sh4")
    g = S.both_views(sc)
    V, G = sc["V"], sc["G"]
    others = np.arange(G) != g
    away = sc["means"].copy()
    away[g] = S.BEHIND
    image0, grads0, ws0 = run(dict(sc, means=away), gpu, w)
    need0 = needed(ws0, V)
    assert all(a < b for a, b in zip(need0, o64["info"]["keys"]))          # it had keys in both views
    variants = [(f"mean[{i}] NaN", "means", (g, i), NAN) for i in range(3)]
    variants += [("mean z +inf", "means", (g, 2), INF), ("mean z -inf", "means", (g, 2), -INF)]
    variants += [(f"cov{ij} {x}", "covs", (g,) + ij, x) for ij in UPPER for x in (NAN, INF)]
    for tag, key, at, value in variants:
        broken = sc[key].copy()
        broken[at] = value
        image, grads, ws = run(dict(sc, **{key: broken}), gpu, w)
        print(tag, "keys", needed(ws, V), "radii", splat.radii(ws, V, G)[:, g].tolist())
        assert needed(ws, V) == need0, tag
        assert not bool(splat.radii(ws, V, G)[:, g].any()), tag
        assert same(image, image0), tag
        for n, a, b in zip(NAMES, grads, grads0):
            assert same(a[others], b[others]) and zero(a[g]), (tag, n)
    clean = run(sc, gpu, w)
    lower = sc["covs"].copy()
    lower[g, [1, 2, 2], [0, 0, 1]] = NAN
    image, grads, ws = run(dict(sc, covs=lower), gpu, w)
    assert same(image, clean[0]) and needed(ws, V) == o64["info"]["keys"]
    for n, a, b in zip(NAMES, grads, clean[1]):
        assert same(a, b), n


# ------------------------------------------------------------------------------------------- 8. NaN opacity, NaN colour
def test_a_nan_opacity_shows_on_every_pixel_of_its_tiles(gpu):
    """The nearest Gaussian of `front` (one tile, (1, 0) of 41x33) with opacity NaN: its conic is positive definite, power <= 0 on
    every pixel, so alpha is NaN on the whole tile and every channel there is NaN, as in the restatement (min(0.99, NaN) must not
    come out 0.99: at evaluation no backward would show it).  Outside the tile: the bits of the scene with it behind the camera.  Its
    opacity gradient is not finite."""
    sc, _, _, _ = S.edge_reference("front")
    opac = sc["opac"].copy()
    opac[0] = NAN
    broken = dict(sc, opac=opac)
    r64, _, _ = S.restate(broken, torch.float64, grad=False)
    want = np.isnan(r64["image"])
    tile = np.zeros((1, 3, sc["H"], sc["W"]), bool)
    tile[:, :, 0:16, 16:32] = True
    assert np.array_equal(want, tile)
    away = sc["means"].copy()
    away[0] = S.BEHIND
    image0, _, _ = run(dict(sc, means=away), gpu)
    image, grads, _ = run(broken, gpu, sc["g_image"])
    got = np.isnan(image)
    print("NaN pixels", int(got[0, 0].sum()), int(got[0, 1].sum()), int(got[0, 2].sum()), "of the tile's 256; d opacity", grads[3])
    assert np.array_equal(got, want)
    assert same(image[~tile], image0[~tile])
    assert not np.isfinite(grads[3][0])


def test_a_nan_colour_shows_where_the_gaussian_is_blended(gpu):
    """One NaN coefficient (d_sh 1, channel 1) of `front`'s nearest Gaussian: channel 1 is NaN exactly on the restatement's pixels (its
    alpha reaches 1/255 there; pixels whose decision margin in the clean scene is under 1e-3 are left out), channels 0 and 2 have
    the clean scene's bits everywhere."""
    sc, o64, _, _ = S.edge_reference("front")
    sh = sc["sh"].copy()
    sh[0, 1, 0] = NAN
    broken = dict(sc, sh=sh)
    r64, _, _ = S.restate(broken, torch.float64, grad=False)
    want = np.isnan(r64["image"])
    keep = o64["kept"]
    image0, _, _ = run(sc, gpu)
    image, _, _ = run(broken, gpu)
    got = np.isnan(image)
    print("NaN pixels in channel 1:", int(got[0, 1].sum()), "restated", int(want[0, 1].sum()), "left out", int((~keep).sum()))
    assert not want[:, [0, 2]].any() and 0 < want[0, 1].sum() < 256
    assert np.array_equal(got[:, 1][keep], want[:, 1][keep])
    assert same(image[:, [0, 2]], image0[:, [0, 2]])
    assert same(image[:, 1][keep & ~want[:, 1]], image0[:, 1][keep & ~want[:, 1]])
