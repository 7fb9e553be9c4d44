"""The lifting block's backward (stage 2: depth_prob_topk / sample_depth_prob; stage 3: backproject_weigh[_mean]; the NVS
input ray_depth) at its edges, against plain references.

Stage 2 is compared with a float64 torch autograd restatement of mvsdet.py:266-317 and :470-475 (softmax, sigmoid, top-k
gather, sum) fed the kernel's own `est_idx`, so ties and near-ties of the ranking do not enter the comparison; the ranking
itself is pinned separately where it is exactly decided (equal logits, saturated logits: the lower plane wins).  Cases cover
every forward specialisation (D <= 16, D <= 64, D up to MVSDET_MAX_DEPTH = 512; the KT = 3 and MVSDET_MAX_TOPK candidate
lists), partial and multiple workgroups of pixels, the strided read of one (N, 2, D, H, W) network output, and every subset
of absent cotangents (losses over a subset of the outputs, through autograd: what `_dp_bwd` / `_sdp_bwd` then receive).

Bars.  Each gradient is held to a multiple of the fp32 rounding of the operations that produce it, relative to the
gradient's scale (max |reference|): the softmax backward sums D products per pixel (dot = sum_d gp_d p_d) on top of a
forward whose probabilities carry the D-term normaliser, so its bar grows with D; everything else is a few operations
per element.  No bar is looser than 1e-5 of scale.  Measured errors are recorded with record_property; on the first MI355X
run: cost-logit gradients at most 0.55 of their bar (5.4e-6 of scale at D = 512), offset-logit gradients 2.6e-7, the
sample_depth_prob gradients 1.9e-7, est_ray_depth's 5.7e-8.

Stage 3 is compared with the CPU oracle's backward (oracle.backproject_weigh_bwd, pinned against the reference's
autograd by test_oracle_golden.py) at J in {1, 8}, with empty voxels and with more than 64 views.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24          # fp32 unit roundoff
CEIL = 1e-5               # no bar here is looser than this, relative to the gradient's scale


def stage2_bar(D):
    """d(loss)/d(cost logits): the dot over D planes plus the D-term normaliser of the forward, a few roundings each."""
    return min(CEIL, 4.0 * (D + 8) * EPS)


OFF_BAR = 16 * EPS        # d(loss)/d(offset logits) and the sample_depth_prob gradients: a handful of roundings per element


def _rel(got, ref):
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    return err / scale if scale > 0 else err, scale


def _restated(a, b, idx, near, iv, from_logits):
    """mvsdet.py:470-475 (from_logits), :266-283, :298-317 in float64: -> prob, off, est_depth, est_dens, avg."""
    if from_logits:
        prob, off = torch.softmax(a, dim=1), torch.sigmoid(b)
    else:
        prob, off = a, b
    d = torch.arange(prob.shape[1], dtype=torch.float64, device=prob.device).view(1, -1, 1, 1)
    depth = (d * iv + near) + off * iv
    return prob, off, depth.gather(1, idx), prob.gather(1, idx), (prob * depth).sum(dim=1)


def _ref_parts(a, b, idx, near, iv, cots, from_logits):
    """Float64 gradient of <cot_i, output_i> w.r.t. (a, b), one pair per output (the loss is linear in the cotangents)."""
    a64 = a.detach().double().requires_grad_(True)
    b64 = b.detach().double().requires_grad_(True)
    outs = _restated(a64, b64, idx.long(), float(np.float32(near)), float(np.float32(iv)), from_logits)
    if not from_logits:
        outs = outs[2:]
    parts = []
    for o, c in zip(outs, cots):
        if c is None:
            parts.append((torch.zeros_like(a64), torch.zeros_like(b64)))
            continue
        ga, gb = torch.autograd.grad(o, (a64, b64), c.double(), retain_graph=True, allow_unused=True)
        parts.append((torch.zeros_like(a64) if ga is None else ga, torch.zeros_like(b64) if gb is None else gb))
    return parts


def _check(got, ref, bar, what):
    """-> error relative to the reference's scale; a reference that is exactly zero (D = 1: the softmax is constant)
    demands an exact zero."""
    e, s = _rel(got, ref)
    if s == 0.0:
        assert e == 0.0, f"{what}: {e:.3e} where the reference gradient is exactly zero"
        return 0.0
    assert e <= bar, f"{what}: max |d| {e * s:.3e} = {e:.3e} of scale {s:.3e} > bar {bar:.3e}"
    return e


def _logits(N, D, H, W, seed, dev, sharp=3.0):
    g = torch.Generator().manual_seed(seed)
    both = torch.randn((N, 2, D, H, W), generator=g)
    both[:, 0] *= sharp
    return both.to(dev)


PIXELS = [(1, 1), (16, 16), (1, 257), (59, 80)]     # one lane; one full workgroup; one more than that; the cropped map
CASES = [(D, k) for D in (1, 3, 16, 17, 64, 65, 200, 512) for k in (1, 3, 4, 8) if k <= D]


# --------------------------------------------------------------------------------------------- depth_prob_topk
@pytest.mark.parametrize("D,topk", CASES)
def test_depth_prob_topk_backward_vs_float64(gpu, record_property, D, topk):
    """All five float outputs' cotangents present, through autograd, with cost and offset read in place as the two channel
    slices of one (N, 2, D, H, W) leaf (what MVSDetHotPath.depth_distribution hands the op)."""
    from mvsdet_amd import ops
    near, iv = 0.2, 4.8 / D
    worst = {"cost": 0.0, "off": 0.0}
    for i, (H, W) in enumerate(PIXELS):
        N = 3 if H * W > 1 else 2
        both = _logits(N, D, H, W, 100 * D + 10 * topk + i, gpu).requires_grad_(True)
        prob, off, ed, en, ei, av = ops.depth_prob_topk(both[:, 0], both[:, 1], near, iv, topk)
        g = torch.Generator().manual_seed(7 + i)
        cots = [torch.randn(t.shape, generator=g).to(gpu) for t in (prob, off, ed, en, av)]
        sum((t * c).sum() for t, c in zip((prob, off, ed, en, av), cots)).backward()
        parts = _ref_parts(both[:, 0], both[:, 1], ei, near, iv, cots, True)
        ref_c, ref_o = sum(p[0] for p in parts), sum(p[1] for p in parts)
        assert float(ref_o.abs().max()) > 0 and (D == 1 or float(ref_c.abs().max()) > 0)
        ec = _check(both.grad[:, 0], ref_c, stage2_bar(D), f"{(N, D, H, W, topk)}: d/d cost logits")
        eo = _check(both.grad[:, 1], ref_o, OFF_BAR, f"{(N, D, H, W, topk)}: d/d offset logits")
        worst["cost"], worst["off"] = max(worst["cost"], ec), max(worst["off"], eo)
    record_property("dp_bwd_cost_rel_err", worst["cost"])
    record_property("dp_bwd_cost_bar", stage2_bar(D))
    record_property("dp_bwd_off_rel_err", worst["off"])
    record_property("dp_bwd_off_bar", OFF_BAR)
    print(f"depth_prob_topk bwd D={D} topk={topk}: {worst} bars {stage2_bar(D):.2e} / {OFF_BAR:.2e}")


@pytest.mark.parametrize("D,topk", [(3, 3), (17, 4), (65, 8), (512, 3)])
def test_depth_prob_topk_backward_absent_cotangents(gpu, record_property, D, topk):
    """Losses over every subset of the five float outputs (prob, off -- the direct gradient on the sigmoid output --,
    est_depth, est_dens, avg_depth), through autograd: the unused outputs' cotangents reach `_dp_bwd` absent."""
    from mvsdet_amd import ops
    near, iv = 0.5, 4.5 / D
    N, H, W = 2, 9, 31
    both = _logits(N, D, H, W, 5000 + D, gpu)
    prob, off, ed, en, ei, av = ops.depth_prob_topk(both[:, 0], both[:, 1], near, iv, topk)
    g = torch.Generator().manual_seed(11)
    cots = [torch.randn(t.shape, generator=g).to(gpu) for t in (prob, off, ed, en, av)]
    parts = _ref_parts(both[:, 0], both[:, 1], ei, near, iv, cots, True)
    worst = 0.0
    for mask in itertools.product((False, True), repeat=5):
        if not any(mask):
            continue
        # a fresh graph per subset: the unused outputs reach `_dp_bwd` as autograd hands them over
        leaf = both.clone().requires_grad_(True)
        outs = ops.depth_prob_topk(leaf[:, 0], leaf[:, 1], near, iv, topk)
        outs = (outs[0], outs[1], outs[2], outs[3], outs[5])
        loss = sum((t * c).sum() for t, c, m in zip(outs, cots, mask) if m)
        g, = torch.autograd.grad(loss, (leaf,))
        ref_c = sum(p[0] for p, m in zip(parts, mask) if m)
        ref_o = sum(p[1] for p, m in zip(parts, mask) if m)
        for name, got, ref, bar in (("cost", g[:, 0], ref_c, stage2_bar(D)), ("off", g[:, 1], ref_o, OFF_BAR)):
            worst = max(worst, _check(got, ref, bar, f"cotangents {mask}: d/d {name}") / bar)
    record_property("dp_bwd_subsets_worst_err_over_bar", worst)
    record_property("dp_bwd_subsets_bars", f"cost {stage2_bar(D):.3e}, off {OFF_BAR:.3e}")


def test_depth_prob_topk_backward_ties_go_to_the_lower_plane(gpu, record_property):
    """Planes with exactly equal logits, and saturated logits (+-80: the probabilities of all but the top plane underflow to
    exact zeros, which tie): the kernel's rule is that the lower plane wins a tie, so the top-k slots and with them the
    gradients of est_depth / est_dens go to the lowest tied planes."""
    from mvsdet_amd import ops
    N, D, H, W, topk = 2, 20, 8, 40, 4
    near, iv = 0.2, 0.24
    both = _logits(N, D, H, W, 77, gpu)
    c = both[:, 0]
    c[:, :, 0:2] = 0.25                       # rows 0-1: all planes equal
    c[:, 1::2, 2:4] = c[:, 0::2, 2:4]         # rows 2-3: plane 2i+1 repeats plane 2i -> pairs of exact ties
    c[:, :, 4:6] = torch.where(torch.arange(D, device=gpu).view(1, D, 1, 1) == 7, 80.0, -80.0)   # rows 4-5: saturated
    c[:, :, 6:8] = -80.0                      # rows 6-7: all saturated equal
    both.requires_grad_(True)
    prob, off, ed, en, ei, av = ops.depth_prob_topk(both[:, 0], both[:, 1], near, iv, topk)
    # the expected ranking: a stable ascending sort of the negated float32 probabilities (ties keep the lower plane first)
    expect = np.argsort(-prob.detach().cpu().numpy(), axis=1, kind="stable")[:, :topk]
    np.testing.assert_array_equal(ei.cpu().numpy(), expect)
    assert (ei[:, :, 0:2].cpu() == torch.arange(topk).view(1, -1, 1, 1)).all()
    assert (ei[:, 0, 4:6] == 7).all() and (ei[:, 1:, 4:6].cpu() == torch.arange(topk - 1).view(1, -1, 1, 1)).all()
    assert float(prob[:, :, 4:6].detach().sort(dim=1)[0][:, :-1].abs().max()) == 0.0   # the exact zeros that tie
    g = torch.Generator().manual_seed(3)
    cots = [torch.randn(t.shape, generator=g).to(gpu) for t in (ed, en)]
    ((ed * cots[0]).sum() + (en * cots[1]).sum()).backward()
    parts = _ref_parts(both[:, 0], both[:, 1], ei, near, iv, [None, None] + cots + [None], True)[2:4]
    ref_c, ref_o = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    ec = _check(both.grad[:, 0], ref_c, stage2_bar(D), "ties: d/d cost logits")
    eo = _check(both.grad[:, 1], ref_o, OFF_BAR, "ties: d/d offset logits")
    # the depth cotangent reaches exactly the slots' planes: nothing on a tied plane above them
    hit = torch.zeros((N, D, H, W), dtype=torch.bool, device=gpu).scatter_(1, ei.long(), True)
    assert float(both.grad[:, 1][~hit].abs().max()) == 0.0
    record_property("dp_bwd_ties_rel_err_cost", ec)
    record_property("dp_bwd_ties_bar_cost", stage2_bar(D))
    record_property("dp_bwd_ties_rel_err_off", eo)
    record_property("dp_bwd_ties_bar_off", OFF_BAR)


# --------------------------------------------------------------------------------------------- sample_depth_prob
def _prob_off(N, D, H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    prob = torch.softmax(3.0 * torch.randn((N, D, H, W), generator=g), dim=1)
    off = torch.rand((N, D, H, W), generator=g)
    return prob.to(dev), off.to(dev)


@pytest.mark.parametrize("D,topk", CASES)
def test_sample_depth_prob_backward_vs_float64(gpu, record_property, D, topk):
    """`_sdp_bwd`, the backward of the function-level patch (integration.PATCHED_METHODS["sample_depth_prob"] /
    ["compute_avg_depth"]): the gradients w.r.t. prob and off themselves, every subset of the three cotangents."""
    from mvsdet_amd import ops
    near, iv = 0.2, 4.8 / D
    worst = 0.0
    for i, (H, W) in enumerate(PIXELS):
        N = 3 if H * W > 1 else 1
        prob, off = _prob_off(N, D, H, W, 300 * D + 10 * topk + i, gpu)
        p, o = prob.clone().requires_grad_(True), off.clone().requires_grad_(True)
        ed, en, ei, av = ops.sample_depth_prob(p, o, near, iv, topk)
        g = torch.Generator().manual_seed(9 + i)
        cots = [torch.randn(t.shape, generator=g).to(gpu) for t in (ed, en, av)]
        sum((t * c).sum() for t, c in zip((ed, en, av), cots)).backward()
        parts = _ref_parts(prob, off, ei, near, iv, cots, False)
        for name, got, ref in (("prob", p.grad, sum(q[0] for q in parts)), ("off", o.grad, sum(q[1] for q in parts))):
            assert float(ref.abs().max()) > 0
            worst = max(worst, _check(got, ref, OFF_BAR, f"{(N, D, H, W, topk)}: d/d {name}"))
        for mask in itertools.product((False, True), repeat=3):
            if not any(mask):
                continue
            pl, ol = prob.clone().requires_grad_(True), off.clone().requires_grad_(True)
            outs = ops.sample_depth_prob(pl, ol, near, iv, topk)
            loss = sum((t * c).sum() for t, c, m in zip((outs[0], outs[1], outs[3]), cots, mask) if m)
            gp, go = torch.autograd.grad(loss, (pl, ol))
            for name, got, k in (("prob", gp, 0), ("off", go, 1)):
                ref = sum(q[k] for q, m in zip(parts, mask) if m)
                worst = max(worst, _check(got, ref, OFF_BAR, f"{(N, D, H, W, topk)} cotangents {mask}: d/d {name}"))
    record_property("sdp_bwd_rel_err", worst)
    record_property("sdp_bwd_bar", OFF_BAR)


# --------------------------------------------------------------------------------------------- stage 3
# against the oracle's fp32 backward: the density gradient sums C channel products per voxel and the voxels landing on one
# pixel (device atomics, in another order than the oracle's loop).  Measured 2.8e-7 of scale at most (J = 8, N = 5); the
# bar is 7x that
S3_BAR = 2e-6

def _stage3_scene(oracle, N, C, J, seed, nv, vs, origin):
    """N views; above 10, the cameras and depth distributions of 2 views come round again (with maps of their own), so that
    a voxel can be seen by more than 64 of them."""
    from mvsdet_amd import synthetic
    hw = (24, 32)
    base = N if N <= 10 else 2
    meta = synthetic.make_img_meta(base, hw, seed=seed, origin=origin)
    ext = meta["lidar2img"]["extrinsic"]
    meta["lidar2img"]["extrinsic"] = [ext[i % len(ext)] for i in range(N)]
    feat = synthetic.make_features(N, C, hw, seed=seed)
    logits = synthetic.make_cost_logits(base, 12, hw, seed=seed, sharp=2.0)[torch.arange(N) % base]
    r = oracle.depth_prob_topk(logits[:, 0], logits[:, 1], 0.2, 0.4, J)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    proj = oracle.compute_projection(meta["lidar2img"]["extrinsic"], meta["lidar2img"]["intrinsic"], meta["img_shape"],
                                     meta["ori_shape"])
    pts = oracle.get_points(nv, vs, meta["lidar2img"]["origin"])
    return feat, r, proj, pts, hw, h, w


@pytest.mark.parametrize("J", [1, 8])
@pytest.mark.parametrize("N", [5, 70])
def test_backproject_backward_j_and_view_count(gpu, oracle, record_property, J, N):
    """Both stage-3 forms at J = 1 and 8 against the oracle's backward, on a grid reaching past the views (empty voxels);
    N = 70 is more than the 64 views of one chunk of the fused forward, whose count the mean backward divides by."""
    from mvsdet_amd import functional as F_, ops
    C, nv, vs = 40, [12, 10, 6], [0.4, 0.4, 0.4]
    feat, r, proj, pts, hw, h, w = _stage3_scene(oracle, N, C, J, {1: 31, 8: 39}[J], nv, vs, (0.0, 0.0, 0.5))
    ed, en = r["est_depth"], r["est_dens"]           # padded (N, J, 24, 32): the crop is a strided view, as in the hot path
    V = int(np.prod(nv))
    gen = torch.Generator().manual_seed(5 + J)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(gpu)   # noqa: E731
    f = feat.to(gpu).requires_grad_(True)
    dn = dev(en).requires_grad_(True)
    dd = dev(ed)
    worst = 0.0
    # per-view form through the reference-named function (the (N, h*w, 1, J) layout of mvsdet.py:1372)
    if N <= 8:
        d_r = dd[:, :, :h, :w].reshape(N, J, -1).transpose(2, 1).unsqueeze(2)
        dcrop = dn[:, :, :h, :w]
        p_r = dcrop.reshape(N, J, -1).transpose(2, 1).unsqueeze(2)
        volume, valid, _, _ = F_.backproject_Weigh(f[:, :, :h, :w], dev(pts).view(3, *nv), dev(proj), d_r, vs, p_r)
        o = oracle.backproject_weigh(feat.numpy()[:, :, :h, :w], pts, proj, ed[:, :, :h, :w], en[:, :, :h, :w], vs[-1])
        np.testing.assert_array_equal(valid.cpu().numpy().reshape(N, V), o["valid"])
        R = torch.randn((N, C, V), generator=gen)
        (volume.reshape(N, C, V) * R.to(gpu)).sum().backward()
        gf, gd = oracle.backproject_weigh_bwd(feat.numpy()[:, :, :h, :w], pts, proj, ed[:, :, :h, :w], en[:, :, :h, :w],
                                              vs[-1], R.numpy())
        assert np.abs(gf).max() > 0 and (J == 1 or np.abs(gd).max() > 0)   # J = 1: prob_norm = 1, no density gradient
        for got, ref in ((f.grad[:, :, :h, :w], gf), (dn.grad[:, :, :h, :w], gd)):
            worst = max(worst, _check(got, torch.from_numpy(ref).double().to(gpu), S3_BAR, f"per-view J={J}"))
        assert float(f.grad[:, :, h:].abs().max()) == 0.0 and float(dn.grad[:, :, h:].abs().max()) == 0.0
        f.grad, dn.grad = None, None
    # fused mean form
    mean, count = ops.backproject_weigh_mean(f[:, :, :h, :w], ops.pack_features(f.detach()), dev(pts).view(3, *nv), dev(proj),
                                             dd[:, :, :h, :w], dn[:, :, :h, :w], hw[0], hw[1], vs[-1])
    m = oracle.backproject_weigh_mean(feat.numpy()[:, :, :h, :w], pts, proj, ed[:, :, :h, :w], en[:, :, :h, :w], vs[-1])
    cnt = m["valid_count"]
    np.testing.assert_array_equal(count.cpu().numpy(), cnt)
    assert (cnt == 0).sum() > 0 and (cnt > 0).sum() > 20, "the grid must hold both empty and seen voxels"
    if N > 64:   # counts gathered from both view chunks of the fused forward
        assert cnt.max() > 64
    Rm = torch.randn((C, V), generator=gen)
    (mean.view(C, V) * Rm.to(gpu)).sum().backward()
    gv = Rm.numpy() / (cnt.astype(np.float32) + np.float32(1e-8))
    gv[:, cnt == 0] = 0
    gf, gd = oracle.backproject_weigh_bwd(feat.numpy()[:, :, :h, :w], pts, proj, ed[:, :, :h, :w], en[:, :, :h, :w], vs[-1],
                                          np.broadcast_to(gv, (N,) + gv.shape).copy())
    assert np.abs(gf).max() > 0 and (J == 1 or np.abs(gd).max() > 0)
    for got, ref in ((f.grad[:, :, :h, :w], gf), (dn.grad[:, :, :h, :w], gd)):
        worst = max(worst, _check(got, torch.from_numpy(ref).double().to(gpu), S3_BAR, f"mean J={J} N={N}"))
    assert float(f.grad[:, :, h:].abs().max()) == 0.0 and float(dn.grad[:, :, h:].abs().max()) == 0.0
    record_property("bp_bwd_rel_err", worst)
    record_property("bp_bwd_bar", S3_BAR)


# --------------------------------------------------------------------------------------------- ray_depth
@pytest.mark.parametrize("tag", ["scannet", "arkit"])
def test_ray_depth_gradient_vs_float64(gpu, record_property, tag):
    """est_ray_depth = est_depth / (scale + 1e-8) (mvsdet.py:494) carries its gradient to est_depth: 1 / (scale + 1e-8) on
    the (h, w) window, 0 on the padding; the forward values are those of the no-grad path, bit for bit."""
    from conftest import load_golden
    from mvsdet_amd.hotpath import MVSDetHotPath
    g = load_golden("g9_depth_scale")
    intr = g[f"{tag}_intrinsic"]
    meta = {"lidar2img": {"extrinsic": list(g[f"{tag}_extrinsic"]), "intrinsic": (list(intr) if intr.ndim == 3 else intr),
                          "origin": np.zeros(3, np.float32)},
            "img_shape": (236, 320), "ori_shape": tuple(int(v) for v in g["ori_shape"])}   # 59 x 80 of 60 x 80 maps
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12)
    est = torch.from_numpy(g[f"{tag}_est_depth"]).to(gpu)
    with torch.no_grad():
        scale0, ray0 = hp.ray_depth(meta, est)
    leaf = est.clone().requires_grad_(True)
    scale, ray = hp.ray_depth(meta, leaf)
    assert ray.requires_grad and not scale.requires_grad
    assert torch.equal(ray.detach(), ray0) and torch.equal(scale, scale0)
    N, J, H, W = est.shape
    h, w = 59, 80
    R = torch.randn(ray.shape, generator=torch.Generator().manual_seed(2)).to(gpu)
    (ray * R).sum().backward()
    ref = torch.zeros((N, J, H, W), dtype=torch.float64, device=gpu)
    r64 = R.double().squeeze(2).transpose(2, 1)                               # (N, J, h*w)
    ref[:, :, :h, :w] = (r64 / (scale.double().view(N, 1, h * w) + 1e-8)).view(N, J, h, w)
    e = _check(leaf.grad, ref, 4 * EPS, "d est_ray_depth / d est_depth")     # one addition and one division in fp32
    record_property(f"ray_depth_grad_{tag}_rel_err", e)
    record_property(f"ray_depth_grad_{tag}_bar", 4 * EPS)
    assert float(leaf.grad[:, :, h:].abs().max()) == 0.0
