"""Photometric consistency on the GPU (csrc/photoloss.hip through ops.photo, functional.inverse_warping / compute_reconstr_loss /
photometric_loss / warp_img, MVSDetHotPath.photometric_loss) against the float64 restatement of tests/photo_loss_restated.py AND
fixture G25 (the reference itself on the CPU, tests/golden/make_goldens_g25.py).

Bars: masks and counts exact; warped inside the mask (absolute), outside it (relative to sum |w_i tap_i|), L, loss_pc (relative) and
the depth gradient (relative to the reference's largest magnitude) within 4 x the reference-to-restatement distance the generator
stored for that case and quantity, floor 1e-6 (photo_loss_restated.bar); the gradient outside the mask exactly 0.  Every test prints
its figures before it asserts (pytest -s).

Measured on one MI355X, kernel against G25 / against the restatement (largest over the cases, in units of the bar's own scale):
see DESIGN.md 4.14.
"""
import sys
import types

import numpy as np
import pytest
import torch

import photo_loss_restated as R
from conftest import GOLDEN, load_golden

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from lcg import lcg_uniform
from test_photo_loss_host import reference, restated

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def g25():
    return load_golden("g25_photo_loss")


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def run_ops(gpu, img, left_cam, right_cam, depth, ref, simple, src_idx=None, depth_idx=None, geo=None):
    """The operators under autograd -> dict of numpy results; depth (n,h,w) a device tensor (any strides), gradient at its shape."""
    from mvsdet_amd.ops import photo
    if geo is None:
        geo = photo.photo_geometry(left_cam[:, 0], left_cam[:, 1], right_cam[:, 0], None, None)
    leaf = depth.detach().requires_grad_(True)
    warped, mask = photo.inverse_warp(img, leaf, geo, src_idx, depth_idx)
    assert not mask.requires_grad
    L, terms, count = photo.reconstr_loss(warped, ref, mask, simple)
    Lpc = L if not simple else photo.reconstr_loss(warped, ref, mask, False)[0]
    loss, wins = photo.photometric_select(mask.reshape(1, -1), Lpc.reshape(1))
    (gL,) = torch.autograd.grad(L, leaf, retain_graph=True)
    (grad,) = torch.autograd.grad(loss, leaf)
    return dict(gL=gL.cpu().numpy(), warped=warped.detach().cpu().numpy(), mask=mask.cpu().numpy(), L=L.detach().cpu().numpy(), count=int(count),
                terms=terms.cpu().numpy(), loss_pc=loss.detach().cpu().numpy(), wins=wins.cpu().numpy(), grad=grad.cpu().numpy(), geo=geo)


def run_functional(gpu, c):
    from mvsdet_amd import functional as F_
    leaf = dev(c["depth"][:, None], gpu).requires_grad_(True)
    warped, mask = F_.inverse_warping(dev(c["img"], gpu), dev(c["left_cam"], gpu), dev(c["right_cam"], gpu), leaf)
    ref = dev(c["ref"], gpu)
    L = F_.compute_reconstr_loss(warped, ref, mask, simple=c["simple"])
    out = F_.photometric_loss([warped], [mask], [ref])
    assert set(out) == {"loss_pc"} and out["loss_pc"].dim() == 0 and out["loss_pc"].dtype == torch.float32
    out["loss_pc"].backward()
    return dict(warped=warped.detach().cpu().numpy(), mask=mask.cpu().numpy(), L=L.detach().cpu().numpy(),
                loss_pc=out["loss_pc"].detach().cpu().numpy(), grad=leaf.grad[:, 0].cpu().numpy())


def same_bits(a, b, keys=("warped", "mask", "L", "loss_pc", "grad")):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


@pytest.mark.parametrize("tag", [t for t in R.SINGLE_CASES if t != "warp_img"])
def test_operators_and_functional_against_the_restatement_and_g25(gpu, g25, tag):
    c = R.g25_case(g25, tag)
    got = run_ops(gpu, dev(c["img"], gpu), dev(c["left_cam"], gpu), dev(c["right_cam"], gpu), dev(c["depth"], gpu), dev(c["ref"], gpu),
                  c["simple"])
    assert got["count"] == int((c["mask"] != 0).sum()) and got["wins"].tolist() == [got["count"]]
    for other, name in ((reference(c), "G25"), (restated(c), "restatement")):
        R.check_against(c, got["warped"], got["mask"], got["L"], got["loss_pc"], got["grad"], other, f"{tag} kernel vs {name}")
    if "gL" in c:                                  # d L / d depth of this case's own `simple` (ref_true: loss_pc's gradient is that map scaled)
        r = restated(c)["r"]
        g64 = r["grad"] / (r["wins"][0] / c["mask"].size)
        for want, name in ((c["gL"], "G25"), (g64, "restatement")):
            rel = float(np.abs(got["gL"] - want).max() / np.abs(c["gL"]).max())
            print(f"{tag} kernel vs {name}: d L / d depth {rel:.2e} (bar {R.bar(c['dist_gL']):.2e})")
            assert rel <= R.bar(c["dist_gL"])
        assert np.all(got["gL"][c["mask"][..., 0] == 0] == 0)
    assert same_bits(got, run_functional(gpu, c)), "functional and operators disagree"


def test_scene_form_reads_planar_images_and_the_padded_depth_in_place(gpu, g25):
    """ref_true as warp_img hands it over: planar NCHW images, the (N,4,4) cameras and the [:59,:80] crop of a (12,1,60,81) depth whose
    padding is NaN, through ref_id and neighbor_ids[ref_id, 0] -- the same bits as the gathered, contiguous, packed form; no NaN arrives."""
    from mvsdet_amd.ops import photo
    c = R.g25_case(g25, "ref_true")
    s = c["scene"]
    planar = dev(s["imgs"].transpose(0, 3, 1, 2), gpu)                      # (N,3,59,80), as F.interpolate leaves it
    pad = dev(s["depth_pad"], gpu)
    ref_id, src_id = dev(s["ref_id"], gpu), dev(c["src_id"], gpu)
    geo = photo.photo_geometry(dev(s["w2c"], gpu), dev(s["K"], gpu), dev(s["w2c"], gpu), ref_id, src_id)
    ref = planar.permute(0, 2, 3, 1)[ref_id]
    scene = run_ops(gpu, planar.permute(0, 2, 3, 1), None, None, pad[:, 0, :59, :80], ref, False, src_idx=src_id, depth_idx=ref_id, geo=geo)
    assert scene["grad"].shape == (12, 59, 80) and np.isfinite(scene["warped"]).all() and np.isfinite(scene["grad"]).all()
    unchosen = np.setdiff1d(np.arange(12), s["ref_id"])
    assert np.all(scene["grad"][unchosen] == 0)
    packed = run_ops(gpu, dev(c["img"], gpu), dev(c["left_cam"], gpu), dev(c["right_cam"], gpu), dev(c["depth"], gpu), dev(c["ref"], gpu), False)
    assert np.array_equal(bits(geo), bits(packed["geo"]))
    scene["grad"] = scene["grad"][s["ref_id"]]
    assert same_bits(scene, packed)
    R.check_against(c, scene["warped"], scene["mask"], scene["L"], scene["loss_pc"], scene["grad"], reference(c), "ref_true scene form vs G25")
    # per-view intrinsics as a (N,4,4) stack give the geometry of the packed cameras too
    sm = R.g25_case(g25, "small")
    w2c = np.tile(np.eye(4, dtype=F32), (6, 1, 1))
    w2c[:3, :3], w2c[3:, :3] = sm["left_cam"][:, 0], sm["right_cam"][:, 0]
    K = np.tile(np.eye(4, dtype=F32), (6, 1, 1))
    K[:3, :3, :3], K[3:, :3, :3] = sm["left_cam"][:, 1, :, :3], sm["right_cam"][:, 1, :, :3]
    g_scene = photo.photo_geometry(dev(w2c, gpu), dev(K, gpu), dev(w2c, gpu), dev(np.arange(3), gpu), dev(np.arange(3, 6), gpu))
    g_packed = photo.photo_geometry(dev(sm["left_cam"], gpu)[:, 0], dev(sm["left_cam"], gpu)[:, 1], dev(sm["right_cam"], gpu)[:, 0], None, None)
    assert np.array_equal(bits(g_scene), bits(g_packed))


def test_geometry_against_float64(gpu, g25):
    from mvsdet_amd.ops import photo
    for tag in ("small", "behind", "ref_true"):
        c = R.g25_case(g25, tag)
        geo = photo.photo_geometry(dev(c["left_cam"], gpu)[:, 0], dev(c["left_cam"], gpu)[:, 1], dev(c["right_cam"], gpu)[:, 0], None, None)
        Kinv, P = R.pair_geometry(c["left_cam"], c["right_cam"])
        g = geo.cpu().numpy()
        # float64 rounded once: the fp32 neighbours of numpy's LAPACK inverse / products (which carry a few float64 roundings of their own)
        assert np.array_equal(g[:, :9].reshape(-1, 3, 3), Kinv.astype(F32)) or np.abs(g[:, :9].reshape(-1, 3, 3) - Kinv).max() <= 1e-7 * np.abs(Kinv).max()
        assert np.abs(g[:, 9:21].reshape(-1, 3, 4) - P).max() <= 6e-8 * np.abs(P).max()
        assert np.all(g[:, 21:] == 0)


def test_warp_img_on_the_device(gpu, g25):
    from mvsdet_amd import functional as F_
    c = R.g25_case(g25, "warp_img")
    s = c["scene"]
    leaf = dev(s["depth"][:, None], gpu).requires_grad_(True)
    imgs = dev(s["imgs"], gpu)
    args = (imgs, dev(s["neighbor_ids"], gpu), dev(s["w2c"], gpu), dev(s["K"], gpu))
    warped, mask, chosen = F_.warp_img(*args, leaf, ref_id=torch.from_numpy(s["ref_id"]))
    small = torch.nn.functional.interpolate(imgs, scale_factor=0.25, mode="bilinear").permute(0, 2, 3, 1)
    assert torch.equal(chosen, small[dev(s["ref_id"], gpu)])
    assert float((chosen.cpu() - torch.from_numpy(c["chosen"])).abs().max()) <= 1e-6      # the resize is ATen's own, on the device
    L = F_.compute_reconstr_loss(warped, chosen, mask, simple=False)
    loss = F_.photometric_loss([warped], [mask], [chosen])["loss_pc"]
    loss.backward()
    grad = leaf.grad[:, 0].cpu().numpy()
    # the images differ from the CPU resize by the device's rounding of the resize (<= 1e-6): compared through the stored distances
    cc = dict(c, img=small.cpu().numpy()[c["src_id"]], ref=chosen.cpu().numpy())
    for other, name in ((reference(c), "G25"), (restated(cc), "restatement")):
        R.check_against(c, warped.detach().cpu().numpy(), mask.cpu().numpy(), L.detach().cpu().numpy(), loss.detach().cpu().numpy(),
                        grad[s["ref_id"]], other, f"warp_img kernel vs {name}")
    # ref_id=None draws torch.randperm on the CPU as the reference does
    torch.manual_seed(2522)
    w2, m2, _ = F_.warp_img(*args, leaf.detach())
    assert np.array_equal(bits(w2), bits(warped)) and np.array_equal(bits(m2), bits(mask))
    # CPU-resident neighbour ids and cameras are taken to the device
    w3, _, _ = F_.warp_img(imgs, torch.from_numpy(s["neighbor_ids"]), torch.from_numpy(s["w2c"]), torch.from_numpy(s["K"]), leaf.detach(),
                           ref_id=s["ref_id"].tolist())
    assert np.array_equal(bits(w3), bits(warped))


@pytest.mark.parametrize("tag,n", R.MULTI_CASES)
def test_minimum_over_scenes(gpu, g25, tag, n):
    from mvsdet_amd import functional as F_
    cs = [R.g25_case(g25, f"{tag}[{i}]") for i in range(n)]
    leaves = [dev(c["depth"][:, None], gpu).requires_grad_(True) for c in cs]
    wm = [F_.inverse_warping(dev(c["img"], gpu), dev(c["left_cam"], gpu), dev(c["right_cam"], gpu), d) for c, d in zip(cs, leaves)]
    refs = [dev(c["ref"], gpu) for c in cs]
    loss = F_.photometric_loss([w for w, _ in wm], [m for _, m in wm], refs)["loss_pc"]
    loss.backward()
    from mvsdet_amd.ops import photo
    L = torch.stack([photo.reconstr_loss(w.detach(), r, m, False)[0] for (w, m), r in zip(wm, refs)])
    _, wins = photo.photometric_select(torch.cat([m.reshape(1, -1) for _, m in wm]), L)
    assert np.array_equal(wins.cpu().numpy(), g25[f"{tag}:wins"])
    rs = [R.loss_and_depth_grad(c["img"], c["left_cam"], c["right_cam"], c["depth"], c["ref"]) for c in cs]
    loss64 = R.photometric_loss([r["warped"] for r in rs], [r["mask"] for r in rs], [c["ref"] for c in cs])[0]
    for want, name in ((float(g25[f"{tag}:loss_pc"]), "G25"), (float(loss64), "restatement")):
        rel = abs(float(loss.detach()) - want) / abs(want)
        print(f"{tag} kernel vs {name}: loss_pc {rel:.2e} (bar {R.bar(g25[f'{tag}:dist_loss_pc']):.2e})")
        assert rel <= R.bar(g25[f"{tag}:dist_loss_pc"])
    total = cs[0]["mask"].size
    for i, (c, d, r) in enumerate(zip(cs, leaves, rs)):
        g = d.grad[:, 0].cpu().numpy()
        g64 = r["grad"] / (r["wins"][0] / total) * (int(g25[f"{tag}:wins"][i]) / total)
        for want, name in ((c["grad"], "G25"), (g64, "restatement")):
            rel = float(np.abs(g - want).max() / np.abs(c["grad"]).max())
            print(f"{tag}[{i}] kernel vs {name}: grad {rel:.2e} (bar {R.bar(c['dist_grad']):.2e})")
            assert rel <= R.bar(c["dist_grad"])
        assert np.all(g[c["mask"][..., 0] == 0] == 0)
    # equal L_i: the lower scene takes the pixels both see
    masks = torch.cat([m.reshape(1, -1) for _, m in wm][:2])
    _, tie = photo.photometric_select(masks, torch.full((2,), 0.25, device=gpu))
    m0, m1 = (cs[i]["mask"].reshape(-1) != 0 for i in range(2))
    assert tie.cpu().tolist() == [int(m0.sum()), int((m1 & ~m0).sum())]


def test_two_runs_give_the_same_bits(gpu, g25):
    c = R.g25_case(g25, "ref_true")
    args = [dev(c[k], gpu) for k in ("img", "left_cam", "right_cam", "depth", "ref")]
    a, b = run_ops(gpu, *args, False), run_ops(gpu, *args, False)
    assert same_bits(a, b) and np.array_equal(bits(a["terms"]), bits(b["terms"]))


@pytest.mark.parametrize("shape", [(1, 10, 25), (1, 16, 16), (3, 13, 21), (1, 257, 256)], ids=lambda s: "x".join(map(str, s)))
def test_block_counts(gpu, shape):
    """250 pixels (one partial block), 256 (exactly one), 819 (three and a partial one), 65792 (257 blocks: one thread of the finishing
    launch adds a run of two partials, and the threads past the last run none): the loss launches alone on LCG images under a mask with
    holes, both forms, against the float64 restatement.  Count exact; L and each term within bar(0) = 1e-6 relative, the floor this
    file's bar states: the terms are non-negative fp32 numbers of a few roundings each (differences of magnitude 1 on values below 1.5),
    added in float64 and rounded to fp32 once."""
    from mvsdet_amd.ops import photo
    B, h, w = shape
    C, n = 3, B * h * w
    warped, ref = (F32(1.5) * lcg_uniform(n * C, seed + h).reshape(B, h, w, C).astype(F32) for seed in (31, 57))
    mask = (lcg_uniform(n, 83 + w) > -0.3).astype(F32).reshape(B, h, w, 1)
    for simple in (False, True):
        want_L, want_terms, _, _ = R.compute_reconstr_loss(warped, ref, mask, simple)
        want_count = int((mask != 0).sum())
        assert 0 < want_count < n
        L, terms, count = photo.reconstr_loss(dev(warped, gpu), dev(ref, gpu), dev(mask, gpu), simple)
        L, terms = float(L), terms.cpu().numpy()
        rel = [abs(L - float(want_L)) / abs(float(want_L))] + [abs(float(t) - float(v)) / abs(float(v)) for t, v in zip(terms, want_terms) if v != 0]
        print(f"{shape} simple={simple}: count {int(count)} of {n}, L and terms from the restatement {['%.2e' % r for r in rel]} (bar {R.bar(0):.0e})")
        assert int(count) == want_count
        assert len(rel) == (2 if simple else 4) and max(rel) <= R.bar(0)
        assert all(float(t) == 0.0 for t, v in zip(terms, want_terms) if v == 0)


def test_single_masked_pixel_in_the_last_partial_block(gpu):
    """527 pixels: blocks of 256, 256 and 15, the mask on the last pixel alone.  warped 2.5 against ref 0.5: smooth_l1(2) = 1.5 in each
    of the 3 channels of that pixel (photo), of its left neighbour (d/dx, in the last block too) and of its upper neighbour (d/dy)."""
    from mvsdet_amd.ops import photo
    B, h, w, C = 1, 17, 31, 3
    mask = np.zeros((B, h, w, 1), F32)
    mask[0, h - 1, w - 1] = 1
    warped, ref = np.full((B, h, w, C), 2.5, F32), np.full((B, h, w, C), 0.5, F32)
    m = [F32(4.5 / (B * h * w * C)), F32(4.5 / (B * h * (w - 1) * C)), F32(4.5 / (B * (h - 1) * w * C))]
    for simple in (False, True):
        L, terms, count = photo.reconstr_loss(dev(warped, gpu), dev(ref, gpu), dev(mask, gpu), simple)
        want = [m[0], F32(0), F32(0)] if simple else m
        assert int(count) == 1 and np.array_equal(bits(terms), bits(np.array(want, F32)))
        assert F32(L.cpu().numpy()) == (m[0] if simple else F32(0.5) * m[0] + F32(0.5) * (m[1] + m[2]))


def test_strided_inputs_give_the_bits_of_contiguous_ones(gpu, g25):
    c = R.g25_case(g25, "small")
    img, depth, ref = dev(c["img"], gpu), dev(c["depth"], gpu), dev(c["ref"], gpu)
    left, right = dev(c["left_cam"], gpu), dev(c["right_cam"], gpu)
    want = run_ops(gpu, img, left, right, depth, ref, False)
    planar = img.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)                          # NCHW storage seen channel-last
    wide = torch.full((3, 14, 19), float("nan"), device=gpu)
    wide[:, 1:13, 2:18] = depth
    ref_wide = torch.zeros((3, 12, 16, 5), device=gpu)
    ref_wide[..., 1:4] = ref
    got = run_ops(gpu, planar, left, right, wide[:, 1:13, 2:18], ref_wide[..., 1:4], False)
    assert same_bits(want, got)
    # a depth map that two pairs read gets the sum of both contributions, in pair order; one nobody reads gets 0
    from mvsdet_amd.ops import photo
    idx = dev(np.array([1, 1, 0]), gpu)
    leaf = depth.detach().requires_grad_(True)
    w, m = photo.inverse_warp(img, leaf, want["geo"], None, idx)
    g_in = torch.ones_like(w)
    (g,) = torch.autograd.grad(w, leaf, g_in)
    parts = [photo.inverse_warp_backward(img, depth, want["geo"], None, dev(np.array(k), gpu), g_in) for k in ([1, 3, 3], [3, 1, 3], [3, 3, 0])]
    assert bool((g[2] == 0).all()) and torch.equal(g[1], parts[0][1] + parts[1][1]) and torch.equal(g[0], parts[2][0])


def test_an_index_outside_the_views_reads_nothing(gpu, g25):
    """src_idx / depth_idx live on the device, so they cannot be checked on the host without a synchronisation: the kernels check them
    and write NaN (mask 0, gradient 0) instead of reading."""
    from mvsdet_amd.ops import photo
    c = R.g25_case(g25, "tiny")
    img, depth = dev(c["img"], gpu), dev(c["depth"], gpu)
    geo = photo.photo_geometry(dev(c["left_cam"], gpu)[:, 0], dev(c["left_cam"], gpu)[:, 1], dev(c["right_cam"], gpu)[:, 0], None, None)
    w, m = photo.inverse_warp(img, depth, geo, dev(np.array([0, 2]), gpu), dev(np.array([-1, 1]), gpu))
    assert bool(torch.isnan(w[0]).all()) and bool((m[0] == 0).all()) and bool(torch.isnan(w[1]).all()) and bool((m[1] == 0).all())
    g = photo.inverse_warp_backward(img, depth, geo, dev(np.array([0, 2]), gpu), dev(np.array([0, 1]), gpu), torch.ones_like(w))
    assert bool((g[1] == 0).all()) and bool(torch.isfinite(g).all())
    bad = photo.photo_geometry(dev(c["left_cam"], gpu)[:, 0], dev(c["left_cam"], gpu)[:, 1], dev(c["right_cam"], gpu)[:, 0],
                               dev(np.array([0, 5]), gpu), dev(np.array([1, 0]), gpu))
    assert bool(torch.isfinite(bad[0]).all()) and bool(torch.isnan(bad[1]).all())


def test_no_host_synchronisation(gpu, g25):
    from mvsdet_amd import functional as F_
    c = R.g25_case(g25, "ref_true")
    s = c["scene"]
    imgs = dev(s["imgs"].transpose(0, 3, 1, 2), gpu).repeat_interleave(4, 2).repeat_interleave(4, 3)   # (12,3,236,320)
    nbr, w2c, K, pad = (dev(s[k], gpu) for k in ("neighbor_ids", "w2c", "K", "depth_pad"))
    ref_id = dev(s["ref_id"], gpu)

    def step():
        leaf = pad.detach().requires_grad_(True)
        warped, mask, chosen = F_.warp_img(imgs, nbr, w2c, K, leaf[:, :, :59, :80], ref_id=ref_id)
        loss = F_.photometric_loss([warped], [mask], [chosen])["loss_pc"]
        loss.backward()
        return loss, leaf.grad

    step()   # warm: library load, allocator, the pixel grid's upload
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, grad = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(loss)) and grad.shape == pad.shape
    assert bool((grad[:, :, 59:] == 0).all()) and bool((grad[:, :, :, 80:] == 0).all()) and bool((grad != 0).any())


def test_refusals_and_autocast_on_the_device(gpu, g25):
    from mvsdet_amd import functional as F_
    from mvsdet_amd.ops import photo
    c = R.g25_case(g25, "tiny")
    img, left, right, depth, ref = (dev(c[k], gpu) for k in ("img", "left_cam", "right_cam", "depth", "ref"))
    with pytest.raises(RuntimeError, match="no gradient"):
        F_.inverse_warping(img.clone().requires_grad_(True), left, right, depth[:, None])
    geo = photo.photo_geometry(left[:, 0], left[:, 1], right[:, 0], None, None)
    with pytest.raises(RuntimeError, match="no gradient"):
        photo.inverse_warp(img.clone().requires_grad_(True), depth.clone().requires_grad_(True), geo, None, None)
    w, m = photo.inverse_warp(img, depth, geo, None, None)
    with pytest.raises(RuntimeError, match="no gradient"):
        photo.reconstr_loss(w.clone().requires_grad_(True), ref.clone().requires_grad_(True), m, False)
    with pytest.raises(TypeError):
        photo.inverse_warp(img.half(), depth, geo, None, None)
    with pytest.raises(ValueError, match="no src_idx"):
        photo.inverse_warp(img[:1], depth, geo, None, None)
    with torch.autocast("cuda", dtype=torch.float16):
        w16, m16 = F_.inverse_warping(img.half(), left, right, depth[:, None].half())
        L16 = F_.compute_reconstr_loss(w16, ref.half(), m16, simple=False)
    w32, m32 = photo.inverse_warp(img.half().float(), depth.half().float(), geo, None, None)
    assert w16.dtype == torch.float32 and L16.dtype == torch.float32 and torch.equal(w16, w32) and torch.equal(m16, m32)


def test_hot_path_photometric_loss_reaches_the_cost_logits(gpu):
    """MVSDetHotPath.photometric_loss on a synthetic scene, one process: the loss and the gradient on depth_coding are those of feeding
    functional.warp_img / photometric_loss by hand, and cost_logits.grad is the existing stage-2 backward fed with it as g_avg."""
    from mvsdet_amd import functional as F_
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    from test_host_logic import meta_from
    g5 = load_golden("g5_backproject_scannet")
    N = g5["est_depth"].shape[0]
    meta = meta_from(g5)
    h, w = int(g5["img_shape"][0] // 4), int(g5["img_shape"][1] // 4)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12, topk=3)
    feature = torch.from_numpy(g5["feature"]).to(gpu)
    logits = synthetic.make_cost_logits(N, 12, (60, 80), seed=52, sharp=2.0).to(gpu).requires_grad_(True)
    Hi, Wi = int(meta["img_shape"][0]), int(meta["img_shape"][1])
    images = dev(((lcg_uniform(N * 3 * Hi * Wi, 2599).reshape(N, 3, Hi, Wi) + 1) * 0.5).astype(F32), gpu)
    ref_id = list(range(N))[::-1][:min(10, N)]
    out = hp.forward_scene(feature, meta, cost_logits=logits)
    keys = set(out)
    res = hp.photometric_loss(out, images, meta, ref_id=ref_id)
    assert set(res) == {"loss_pc"} and set(out) == keys
    res["loss_pc"].backward()
    # by hand
    dc = out["depth_coding"].detach().requires_grad_(True)
    assert dc.shape == (N, 1, h, w)
    w2c, K_feat = hp._feature_cameras(meta)
    wv, mv, rv = F_.warp_img(images, out["geometry"].neighbor_ids, w2c.float().to(gpu), K_feat.float().to(gpu), dc, ref_id=ref_id)
    loss = F_.photometric_loss([wv], [mv], [rv])["loss_pc"]
    loss.backward()
    assert torch.equal(loss.detach(), res["loss_pc"].detach()) and 0 < int(mv.sum()) < mv.numel()
    assert bool((dc.grad != 0).any())
    prob, off, est_depth, est_dens, est_idx, avg = hp.depth_distribution(logits.detach())
    g_avg = torch.zeros_like(avg)
    g_avg[:, :h, :w] = dc.grad[:, 0]
    z = torch.zeros_like
    g_cost, g_off = ops.depth_prob_topk_backward(prob, off, est_idx, z(prob), z(est_depth), z(est_dens), g_avg,
                                                 float(hp.near_far_range[0]), float(hp.depth_interval))
    assert bool((logits.grad != 0).any())
    assert np.array_equal(bits(logits.grad[:, 0]), bits(g_cost)) and np.array_equal(bits(logits.grad[:, 1]), bits(g_off))
    # a sequence of scenes: the minimum over two equal scenes is the scene itself
    two = hp.photometric_loss([out, out], [images, images], [meta, meta], ref_id=[ref_id, ref_id])["loss_pc"]
    assert torch.equal(two.detach(), loss.detach())


def test_opt_in_patch_on_a_stand_in(gpu, g25):
    from mvsdet_amd import functional as F_
    from mvsdet_amd import integration

    class MVSDet:
        def warp_img(self, ref_imgs, neighbor_ids, ref_w2c, ref_feat_intrinsic, ref_depth):
            return "original"

        def photometric_loss(self, warped_img_list, mask_list, chose_ref_img_list):
            return dict(loss_pc="original")

    mod = types.SimpleNamespace(MVSDet=MVSDet)
    saved = integration.patch_reference_photometric(mod)
    try:
        s = R.g25_case(g25, "warp_img")["scene"]
        args = [dev(s[k], gpu) for k in ("imgs", "neighbor_ids", "w2c", "K")] + [dev(s["depth"][:, None], gpu)]
        torch.manual_seed(2522)
        warped, mask, chosen = MVSDet().warp_img(*args)
        want = F_.warp_img(*args, ref_id=s["ref_id"].tolist())
        assert torch.equal(warped, want[0]) and torch.equal(mask, want[1]) and torch.equal(chosen, want[2])
        got = MVSDet().photometric_loss([warped], [mask], [chosen])["loss_pc"]
        assert torch.equal(got, F_.photometric_loss([warped], [mask], [chosen])["loss_pc"])
        assert MVSDet().warp_img(*[a.cpu() for a in args]) == "original"
        assert MVSDet().photometric_loss([warped.cpu()], [mask.cpu()], [chosen.cpu()]) == dict(loss_pc="original")
    finally:
        integration.unpatch_reference_photometric(mod, saved)
    assert MVSDet().warp_img(*args) == "original" and MVSDet().photometric_loss([warped], [mask], [chosen]) == dict(loss_pc="original")
