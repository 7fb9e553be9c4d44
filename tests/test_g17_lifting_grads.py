"""G17: the lifting block's backward against the reference's own autograd (tests/golden/make_goldens_g17.py).

The fixture holds d loss / d cost logits and d loss / d feature maps of the reference's `extract_feat` (mvsdet.py:336-698,
the lifting block :470-515 and the opacity of :582) under torch autograd on the CPU, for a ScanNet-shaped and an
ARKit-shaped scene, with the loss

    <R_v, volume_mean> + <R_dc, depth_coding> + <R_p, prob_volume> + <R_o, max(prob_volume, 1)[0][:, :h, :w]>.

Inputs and cotangents come from the committed LCG (seeds stored); cotangents on a discrete decision within fp32 noise of its
threshold (top-k ranking, open depth window, voxel rounding, the window's argmax, the top-1 of the opacity) are zeroed by the
generator, and the masks are stored.  So the reference gradient is well posed everywhere, and the kernels' gradients are
compared with it over the whole arrays, padded row included.

CPU: the fixture is well posed and non-trivial on every path; `-m refcheck` regenerates it bit for bit from the reference.
GPU: the scene driver, a batch of the two scenes and the function-level patched route on the HIP kernels.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import make_goldens_g17 as G  # noqa: E402

# The north-star bar is 1e-4 of each gradient's scale.  Measured on the first MI355X run: at most 3.0e-7 (d loss / d logits,
# ScanNet-shaped; features 1.8e-7), the same on the patched route; the bar is 10x that
BAR = 3e-6


def _case(g, case):
    return {k.split(":", 1)[1]: g[k] for k in g.files if k.startswith(case + ":")}


def _masked_cotangents(f, case, dev):
    meta, feat, logits, cots = G.inputs(case)
    cots["v"] = cots["v"] * torch.from_numpy(f["decided_voxels"]).view(1, *G.N_VOXELS).float()
    cots["o"] = cots["o"] * torch.from_numpy(f["opacity_decided"]).float()
    return meta, feat, logits, {k: v.to(dev) for k, v in cots.items()}


def _loss(volume, depth_coding, prob, opacity, cots, h, w):
    return ((volume * cots["v"]).sum() + (depth_coding * cots["dc"]).sum() + (prob * cots["p"]).sum()
            + (opacity[:, :h, :w] * cots["o"]).sum())


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max())
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max()) / scale, scale


def _hotpath(case):
    from mvsdet_amd.hotpath import MVSDetHotPath
    c = G.CASES[case]
    return MVSDetHotPath(list(G.N_VOXELS), list(G.VOXEL_SIZE), list(c["near_far"]), c["D"], topk=3)


def _scene_grads(hp, meta, feat, logits, cots, dev):
    f = feat.to(dev).requires_grad_(True)
    L = logits.to(dev).requires_grad_(True)
    out = hp.forward_scene(f, meta, cost_logits=L)
    h, w = out["geometry"].height, out["geometry"].width
    _loss(out["volume"], out["depth_coding"], out["prob_volume"], out["opacity"], cots, h, w).backward()
    return out, L.grad, f.grad


# --------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("case", list(G.CASES))
def test_g17_fixture_is_well_posed(oracle, case):
    g = load_golden("g17_lifting_grads")
    assert int(g["inline_restated"]) == 1
    f = _case(g, case)
    c = G.CASES[case]
    N, D, C = c["N"], c["D"], c["C"]
    Hf, Wf = G.FEAT_HW
    assert f["grad_logits"].shape == (N, 2, D, Hf, Wf) and f["grad_features"].shape == (N, C, Hf, Wf)
    assert np.isfinite(f["grad_logits"]).all() and np.isfinite(f["grad_features"]).all()
    np.testing.assert_allclose(f["prob"].sum(axis=1), 1.0, atol=1e-5)
    assert float(f["prob"].max(axis=1).mean()) > 0.2                 # a peaked distribution
    decided = f["decided_voxels"]
    assert (~decided).mean() < 0.02 and f["clear_pixels"].mean() > 0.98 and f["opacity_decided"].mean() > 0.98
    assert int((f["valid_count"][decided] > 0).sum()) > 500
    # the masks are what the decision logic gives on the stored forward outputs
    pts = oracle.get_points(f["n_voxels"], f["voxel_size"], f["origin"])
    h, w = int(f["img_shape"][0]) // 4, int(f["img_shape"][1]) // 4
    d2, c2, o2 = G.decisions(f["prob"], f["est_depth"], f["est_dens"], f["projection"], pts, float(f["voxel_size"][-1]), h, w)
    assert (d2 == decided).mean() > 0.999 and np.array_equal(c2, f["clear_pixels"]) and np.array_equal(o2, f["opacity_decided"])
    # non-trivial on every path: logits through volume, depth_coding, prob_volume and opacity; features through the volume
    scales = f["path_scale_logits"]
    assert (scales > 0.05 * scales.max()).all(), scales
    assert float(f["path_scale_features_volume"]) > 0.1
    # the padded row of the maps gets no gradient through the lifting (the crop), only through prob_volume
    assert float(np.abs(f["grad_features"][:, :, h:]).max()) == 0.0
    assert float(np.abs(f["grad_logits"][:, :, :, h:]).max()) > 0.0
    assert os.path.getsize(os.path.join(GOLDEN, "g17_lifting_grads.npz")) <= 1 << 20


@pytest.mark.refcheck
def test_g17_regenerates():
    from _ref_loader import _NERFDET
    if not os.path.isdir(_NERFDET):
        pytest.skip("reference tree not mounted")
    gold = load_golden("g17_lifting_grads")
    torch.set_num_threads(4)
    new = G.build()
    assert set(new) == set(gold.files)
    for k, v in new.items():
        if k in ("torch_version", "generator"):
            continue
        assert np.array_equal(np.asarray(v), gold[k]), k


# --------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(G.CASES))
def test_g17_scene_driver(gpu, record_property, case):
    """MVSDetHotPath.forward_scene with leaf cost logits and leaf features, then the fixture's loss backward: both gradients
    over the whole padded arrays against the reference's."""
    f = _case(load_golden("g17_lifting_grads"), case)
    meta, feat, logits, cots = _masked_cotangents(f, case, gpu)
    out, gl, gf = _scene_grads(_hotpath(case), meta, feat, logits, cots, gpu)
    h = out["geometry"].height
    np.testing.assert_array_equal(out["valid"].cpu().numpy().reshape(-1)[f["decided_voxels"]],
                                  f["valid_count"][f["decided_voxels"]])
    el, sl = _rel(gl, f["grad_logits"])
    ef, sf = _rel(gf, f["grad_features"])
    record_property(f"g17_{case}_logits_rel_err", el)
    record_property(f"g17_{case}_features_rel_err", ef)
    record_property("g17_bar", BAR)
    print(f"G17 {case}: logits {el:.3e} of {sl:.3e}, features {ef:.3e} of {sf:.3e} (bar {BAR:.0e})")
    assert el <= BAR, f"{case}: d loss / d logits {el:.3e} of scale {sl:.3e} > {BAR:.0e}"
    assert ef <= BAR, f"{case}: d loss / d features {ef:.3e} of scale {sf:.3e} > {BAR:.0e}"
    assert float(gf[:, :, h:].abs().max()) == 0.0


@pytest.mark.gpu
def test_g17_batch_of_scenes(gpu, record_property):
    """forward_scenes with the two scenes (6 and 4 views) as one batch, under the ScanNet planes: each scene's gradients are
    those of its single-scene run (the other scene's cotangents do not leak in), and the ScanNet scene's are the reference's."""
    from mvsdet_amd.hotpath import MVSDetHotPath
    g = load_golden("g17_lifting_grads")
    cases = list(G.CASES)
    hp = MVSDetHotPath(list(G.N_VOXELS), list(G.VOXEL_SIZE), list(G.CASES["scannet"]["near_far"]), 12, topk=3)
    data = {k: _masked_cotangents(_case(g, k), k, gpu) for k in cases}
    single = {k: _scene_grads(hp, *data[k], gpu)[1:] for k in cases}
    fs = [data[k][1].to(gpu).requires_grad_(True) for k in cases]
    ls = [data[k][2].to(gpu).requires_grad_(True) for k in cases]
    res = hp.forward_scenes(fs, [data[k][0] for k in cases], cost_logits=ls)
    loss = 0.0
    for i, k in enumerate(cases):
        out = res["scenes"][i]
        h, w = out["geometry"].height, out["geometry"].width
        loss = loss + _loss(res["volume"][i], out["depth_coding"], out["prob_volume"], out["opacity"], data[k][3], h, w)
    loss.backward()
    worst = 0.0
    for i, k in enumerate(cases):
        for name, got, ref in (("logits", ls[i].grad, single[k][0]), ("features", fs[i].grad, single[k][1])):
            e, s = _rel(got, ref.cpu().numpy())
            worst = max(worst, e)
            assert e <= 1e-6, f"batch scene {k}: d loss / d {name} differs from its own run by {e:.3e} of {s:.3e}"
    el, _ = _rel(ls[0].grad, _case(g, "scannet")["grad_logits"])
    ef, _ = _rel(fs[0].grad, _case(g, "scannet")["grad_features"])
    record_property("g17_batch_vs_single_rel_diff", worst)
    record_property("g17_batch_vs_single_bar", 1e-6)
    record_property("g17_batch_scannet_rel_err", max(el, ef))
    record_property("g17_bar", BAR)
    assert el <= BAR and ef <= BAR, (el, ef)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(G.CASES))
def test_g17_patched_route(gpu, record_property, case):
    """The function-level patch (test_g13_chain._patched_route: the reference's statements on the patched sample_depth_prob /
    compute_avg_depth / backproject_Weigh) under autograd with a stand-in network that hands out the leaf logits: `_sdp_bwd`
    composed with the per-view backproject_Weigh backward.  The feature maps are held fixed (the route's plane sweep is
    forward only); d loss / d logits against the reference's."""
    from test_g13_chain import _patched_route
    f = _case(load_golden("g17_lifting_grads"), case)
    meta, feat, logits, cots = _masked_cotangents(f, case, gpu)
    hp = _hotpath(case)
    L = logits.to(gpu).requires_grad_(True)
    got = _patched_route(feat.to(gpu), meta, lambda v: L, lambda x: x, lambda x: None, hp, gpu)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    opacity = torch.max(got["prob"], dim=1)[0]                       # mvsdet.py:582 as it stands
    volume = got["volume"].reshape(cots["v"].shape)
    _loss(volume, got["depth_coding"], got["prob"], opacity, cots, h, w).backward()
    e, s = _rel(L.grad, f["grad_logits"])
    record_property(f"g17_patched_{case}_logits_rel_err", e)
    record_property("g17_bar", BAR)
    assert e <= BAR, f"patched route {case}: d loss / d logits {e:.3e} of scale {s:.3e} > {BAR:.0e}"
