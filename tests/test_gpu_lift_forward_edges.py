"""The lifting block's FORWARD values (stage 2: depth_prob_topk / sample_depth_prob; stage 3: backproject_weigh, its mean and sum
forms; the NVS input ray_depth) at their edges, against plain references.  test_gpu_lift_grad_edges.py pins the gradients of the
same kernels but feeds its reference the kernel's own plane indices; here the ranking and the values themselves are compared.

Stage 2 -- every forward specialisation (D <= 16, D <= 64, D up to MVSDET_MAX_DEPTH = 512 x the KT = 3 and MVSDET_MAX_TOPK candidate
lists, and the two of sample_depth_prob), the dense and the strided entry, one lane / one workgroup / one more / the cropped map:
  * ranking, exact, no exclusions: est_idx is the defined ranking (lift_restated.rank: descending, NaN above every number, the
    lower plane first among equals and among NaNs -- without NaN, a stable descending argsort) of the kernel's own float32 prob;
    est_dens is prob gathered there and est_depth ((idx * iv + near) + off[idx] * iv) evaluated in float32 on the CPU from the
    kernel's own off, both bit for bit;
  * prob, off and avg_depth against the float64 restatement tests/lift_restated.py (itself pinned against fixture g4_depth_prob and
    the oracle by test_lift_forward_host.py).  Bars, from the roundings that make each value, in units of the fp32 unit roundoff
    EPS = 2^-24 and of the output's scale (1 for prob and off, `far` for avg_depth):
      prob      (D + 8) EPS: D - 1 additions of the normaliser (worst case, every partial sum <= s), the subtraction of the
                maximum (|c - m| e^-|c - m| <= 0.37), expf (within 1 ulp = 2 EPS) and the division, then rounded up; capped at the
                1e-6 the suite already holds against the oracle for D <= 128, and at 1e-5 above
      off       6 EPS: expf within 2 ulp reaches 1 / (1 + e) as at most e / (1 + e)^2 <= 1/4 of it, plus the addition and the
                division
      avg_depth (2 D + 12) EPS of far: the probabilities' (D + 8), three roundings of a depth and its offset, the product, and
                D - 1 additions whose partial sums stay below far; capped at 1e-5 of far.  From ready-made probabilities
                (sample_depth_prob) the first term is absent: (D + 4) EPS of far.
    No bar is looser than 4 (D + 8) EPS of scale, capped at 1e-5.  Measured errors and bars go to record_property.
    First measured values: MEASURED below.
  * structured ties (planes 2i / 2i+1 equal, all equal, one plane saturated at +-80) at every DREG x KT combination;
  * non-finite inputs: a pixel with one NaN or +Inf logit, or all -Inf, has NaN probabilities; NaN ranks first (the lower plane
    first), est_idx stays in [0, D) and distinct, est_depth is the depth formula there, and no output holds the candidate list's
    initial -1; the pixels around are those of the same call without the poison, bit for bit; chained through
    MVSDetHotPath.depth_distribution and lift, the volume is NaN where the oracle chain's is.

Stage 3 against the CPU oracle (bit-exact against the reference: test_oracle_golden.py), bit for bit: J in {1, 2, 8}, N across the
64-view mask chunks, C across the 64-channel-group chunks and ragged slabs, V around the 32-voxel tile of the fused kernel and the
256-voxel workgroup of the per-view one, with hand-placed voxels on the image border's half-even roundings, q2 <= 0, a NaN
projection, depths exactly on the window's edge, a pixel whose densities sum to zero and one with a NaN density.

ray_depth against a float64 restatement of mvsdet.py:1300-1313 + :494 at h < H, w < W, J in {0, 1, 8}, skewed intrinsics.

MEASURED (first MI355X run; worst case over the grid, error / bar):
  prob       8.3e-7 / 1.0e-6 at D = 65 (the 64 sequential additions of the normaliser, worst of 14 160 pixels); 0.83 of its bar
  off        8.7e-8 / 3.6e-7                                                                                0.24
  avg_depth  2.0e-7 / 1.07e-6 of far (D = 3)                                                                0.19
  sample_depth_prob avg_depth 1.5e-7 / 4.2e-7 of far (D = 3)                                                0.35
  ray_depth  est_ray_depth 1.2e-7 / 1.16e-6 of scale; depth_scale below that
"""
import ctypes

import numpy as np
import pytest
import torch

from lift_restated import depth_of_planes, rank, restated

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
CEIL = 1e-5


def prob_bar(D):
    return min((D + 8) * EPS, 1e-6 if D <= 128 else CEIL)


OFF_BAR = 6 * EPS


def avg_bar(D, from_logits=True):
    return min(((2 * D + 12) if from_logits else (D + 4)) * EPS, CEIL)


def test_bars_respect_their_limits():
    for D in (1, 3, 16, 17, 64, 65, 128, 200, 512):
        limit = min(4 * (D + 8) * EPS, CEIL)
        assert prob_bar(D) <= limit and OFF_BAR <= limit and avg_bar(D) <= limit and avg_bar(D, False) <= limit
        assert D > 128 or (prob_bar(D) <= 1e-6 and OFF_BAR <= 1e-6)


def _logits(N, D, H, W, seed, dev, sharp=3.0):
    g = torch.Generator().manual_seed(seed)
    both = torch.randn((N, 2, D, H, W), generator=g)
    both[:, 0] *= sharp
    return both.to(dev)


def _same_bits(a, b):
    """float32 tensors equal bit for bit, any NaN standing for any NaN (the payload and sign of a produced NaN are not pinned)."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool((na == nb).all()) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def _check_exact(prob, off, ed, en, ei, near, iv, what):
    """The ranking and what hangs on it, from the kernel's own float32 prob / off: exact."""
    prob, off, ed, en, ei = [t.detach().cpu() for t in (prob, off, ed, en, ei)]
    topk = ei.shape[1]
    want = rank(prob, topk)
    assert torch.equal(ei.long(), want), f"{what}: est_idx is not the defined ranking of prob"
    assert _same_bits(en, prob.gather(1, want)), f"{what}: est_dens != prob[est_idx]"
    assert _same_bits(ed, depth_of_planes(off, near, iv).gather(1, want)), f"{what}: est_depth != depth formula at est_idx"
    assert int(ei.min()) >= 0 and int(ei.max()) < prob.shape[1]
    if topk > 1:
        s = ei.sort(dim=1).values
        assert bool((s[:, 1:] != s[:, :-1]).all()), f"{what}: a plane twice in one pixel"


def _err(got, ref):
    return float((got.double() - ref).abs().max())


PIXELS = [(1, 1), (16, 16), (1, 257), (59, 80)]
CASES = [(D, k) for D in (1, 3, 16, 17, 64, 65, 200, 512) for k in (1, 3, 4, 8) if k <= D]


def _views(D, H, W):
    """3 views (1 at a single pixel); the cropped map at D >= 200 keeps to one view: the planes, not the pixels, are the case."""
    if H * W == 1:
        return 2
    return 1 if (D >= 200 and H * W > 1000) else 3


# --------------------------------------------------------------------------------------------- depth_prob_topk
@pytest.mark.parametrize("D,topk", CASES)
def test_depth_prob_topk_forward(gpu, record_property, D, topk):
    from mvsdet_amd import ops
    near, iv = 0.2, 4.8 / D
    far = near + D * iv
    worst = {"prob": 0.0, "off": 0.0, "avg": 0.0}
    for i, (H, W) in enumerate(PIXELS):
        N = _views(D, H, W)
        both = _logits(N, D, H, W, 100 * D + 10 * topk + i, gpu)
        strided = ops.depth_prob_topk(both[:, 0], both[:, 1], near, iv, topk)            # one (N, 2, D, H, W) tensor, in place
        dense = ops.depth_prob_topk(both[:, 0].contiguous(), both[:, 1].contiguous(), near, iv, topk)
        for a, b in zip(strided, dense):
            assert torch.equal(a, b), f"{(N, D, H, W, topk)}: the strided and the dense entry differ"
        prob, off, ed, en, ei, av = strided
        _check_exact(prob, off, ed, en, ei, near, iv, f"{(N, D, H, W, topk)}")
        r = restated(both[:, 0], both[:, 1], near, iv, topk)                            # float64, on the device
        e = {"prob": _err(prob, r["prob"]), "off": _err(off, r["off"]), "avg": _err(av, r["avg_depth"]) / far}
        print(f"depth_prob_topk fwd {(N, D, H, W, topk)}: {e} bars {prob_bar(D):.2e} {OFF_BAR:.2e} {avg_bar(D):.2e}")
        assert e["prob"] <= prob_bar(D), f"{(N, D, H, W, topk)}: prob off the float64 softmax by {e['prob']:.3e} > {prob_bar(D):.3e}"
        assert e["off"] <= OFF_BAR, f"{(N, D, H, W, topk)}: off {e['off']:.3e} > {OFF_BAR:.3e}"
        assert e["avg"] <= avg_bar(D), f"{(N, D, H, W, topk)}: avg_depth {e['avg']:.3e} of far > {avg_bar(D):.3e}"
        for k in worst:
            worst[k] = max(worst[k], e[k])
    for k, bar in (("prob", prob_bar(D)), ("off", OFF_BAR), ("avg", avg_bar(D))):
        record_property(f"dp_fwd_{k}_err", worst[k])
        record_property(f"dp_fwd_{k}_bar", bar)


def _prob_off(N, D, H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    prob = torch.softmax(3.0 * torch.randn((N, D, H, W), generator=g), dim=1)
    off = torch.rand((N, D, H, W), generator=g)
    return prob.to(dev), off.to(dev)


@pytest.mark.parametrize("D,topk", CASES)
def test_sample_depth_prob_forward(gpu, record_property, D, topk):
    from mvsdet_amd import ops
    near, iv = 0.2, 4.8 / D
    far = near + D * iv
    worst = 0.0
    for i, (H, W) in enumerate(PIXELS):
        N = _views(D, H, W)
        prob, off = _prob_off(N, D, H, W, 300 * D + 10 * topk + i, gpu)
        ed, en, ei, av = ops.sample_depth_prob(prob, off, near, iv, topk)
        big = torch.full((N + 1, D + 2, H, W + 3), float("nan"), device=gpu)          # the same through non-contiguous views
        pv, ov = big[:N, 1:D + 1, :, 2:W + 2], big.clone()[:N, 1:D + 1, :, 2:W + 2]
        pv.copy_(prob)
        ov.copy_(off)
        for a, b in zip((ed, en, ei, av), ops.sample_depth_prob(pv, ov, near, iv, topk)):
            assert torch.equal(a, b)
        _check_exact(prob, off, ed, en, ei, near, iv, f"sample {(N, D, H, W, topk)}")
        e = _err(av, restated(prob, off, near, iv, topk, from_logits=False)["avg_depth"]) / far
        print(f"sample_depth_prob fwd {(N, D, H, W, topk)}: avg {e:.3e} bar {avg_bar(D, False):.2e}")
        assert e <= avg_bar(D, False), f"sample {(N, D, H, W, topk)}: avg_depth {e:.3e} of far > {avg_bar(D, False):.3e}"
        worst = max(worst, e)
    record_property("sdp_fwd_avg_err", worst)
    record_property("sdp_fwd_avg_bar", avg_bar(D, False))


@pytest.mark.parametrize("D,topk", [(D, k) for D in (16, 64, 65, 512) for k in (3, 8)])
def test_structured_ties_follow_the_defined_rule(gpu, D, topk):
    """Rows 0-1: every plane equal.  Rows 2-3: plane 2i+1 repeats plane 2i.  Rows 4-5: plane 7 at +80, the rest at -80 (their
    float32 probabilities underflow to exact zeros, which tie).  Rows 6-7: all at -80.  The expectation is the restatement's
    ranking of its own float64 probabilities, and the stated picks."""
    from mvsdet_amd import ops
    N, H, W = 2, 8, 40
    near, iv = 0.2, 4.8 / D
    both = _logits(N, D, H, W, 77 + D, gpu)
    c = both[:, 0]
    c[:, :, 0:2] = 0.25
    c[:, 1::2, 2:4] = c[:, 0:D - D % 2:2, 2:4]
    if D % 2:
        c[:, D - 1, 2:4] = -30.0                 # the unpaired last plane of an odd D stays out of the top
    c[:, :, 4:6] = torch.where(torch.arange(D, device=gpu).view(1, D, 1, 1) == 7, 80.0, -80.0)
    c[:, :, 6:8] = -80.0
    for entry in ("logits", "prob"):
        if entry == "logits":
            prob, off, ed, en, ei, av = ops.depth_prob_topk(both[:, 0], both[:, 1], near, iv, topk)
        else:   # the same probabilities, ready-made, through sample_depth_prob's two specialisations
            ed, en, ei, av = ops.sample_depth_prob(prob, off, near, iv, topk)
        _check_exact(prob, off, ed, en, ei, near, iv, f"ties {entry} {(D, topk)}")
        r = restated(both[:, 0], both[:, 1], near, iv, topk)
        assert torch.equal(ei.long(), r["est_idx"]), f"ties {entry} {(D, topk)}: not the float64 restatement's ranking"
        lowest = torch.arange(topk, device=gpu).view(1, -1, 1, 1)
        assert (ei[:, :, 0:2] == lowest).all() and (ei[:, :, 6:8] == lowest).all()
        assert (ei[:, 0, 4:6] == 7).all() and (ei[:, 1:, 4:6] == lowest[:, :topk - 1]).all()
        pair = ei[:, :, 2:4]
        assert (pair[:, 1::2] == pair[:, 0:2 * (topk // 2):2] + 1).all() and (pair[:, 0::2] % 2 == 0).all()
        assert float(prob[:, :, 4:6].sort(dim=1)[0][:, :-1].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- non-finite inputs
NAN, INF = float("nan"), float("inf")


def _no_sentinel(*tensors):
    for t in tensors:
        assert not bool((t == -1).any()), "an output holds the candidate list's initial -1"


@pytest.mark.parametrize("D,topk", [(12, 3), (12, 8), (64, 3), (64, 8), (100, 3), (100, 8)])
def test_depth_prob_topk_non_finite_logits(gpu, D, topk):
    """The reference's behaviour (torch.softmax, torch.topk): a pixel with one NaN or +Inf logit, or with all -Inf, has NaN
    probabilities throughout; NaN ranks above every number and the lower plane first, so est_idx = 0 .. topk-1, est_dens NaN,
    est_depth the depth formula at those planes, avg_depth NaN.  A NaN offset logit reaches its plane's offset and depth and
    the expectation only.  Every other pixel equals the same call without the poison, bit for bit -- forward and backward."""
    from mvsdet_amd import ops
    N, H, W = 2, 4, 70
    near, iv = 0.2, 4.8 / D
    clean = _logits(N, D, H, W, 900 + D, gpu)
    clean[1, 0, :, 3, 7] = torch.linspace(0, 1, D, device=gpu)
    clean[1, 0, D - 2, 3, 7] = 9.0                               # plane D - 2 is the pick of the pixel whose offset is poisoned
    both = clean.clone()
    both[0, 0, 5, 0, 0] = NAN
    both[0, 0, 0, 0, 1] = NAN
    both[0, 0, D - 1, 0, 69] = NAN
    both[0, 0, 2, 1, 3] = INF
    both[1, 0, :, 2, 5] = -INF
    both[1, 1, D - 2, 3, 7] = NAN
    poisoned = torch.zeros((N, H, W), dtype=torch.bool, device=gpu)
    for n, y, x in ((0, 0, 0), (0, 0, 1), (0, 0, 69), (0, 1, 3), (1, 2, 5)):
        poisoned[n, y, x] = True
    off_only = torch.zeros_like(poisoned)
    off_only[1, 3, 7] = True
    ordinary = ~(poisoned | off_only)

    for strided in (True, False):
        a = both if strided else both.contiguous()
        leaf = a.clone().requires_grad_(True)
        cleaf = clean.clone().requires_grad_(True)
        args = (lambda t: (t[:, 0], t[:, 1])) if strided else (lambda t: (t[:, 0].contiguous(), t[:, 1].contiguous()))
        out = ops.depth_prob_topk(*args(leaf), near, iv, topk)
        ref = ops.depth_prob_topk(*args(cleaf), near, iv, topk)
        prob, off, ed, en, ei, av = [t.detach() for t in out]
        r = restated(both[:, 0], both[:, 1], near, iv, topk)
        # NaN exactly where the float64 softmax is: the whole pixel
        assert torch.equal(torch.isnan(prob), torch.isnan(r["prob"]))
        assert torch.equal(torch.isnan(prob), poisoned.unsqueeze(1).expand_as(prob))
        _check_exact(prob, off, ed, en, ei, near, iv, f"non-finite {(D, topk, strided)}")
        _no_sentinel(prob, off, ed, en, av)
        lowest = torch.arange(topk, device=gpu, dtype=ei.dtype).repeat(int(poisoned.sum()), 1)
        assert torch.equal(ei.permute(0, 2, 3, 1)[poisoned], lowest)
        assert torch.isnan(en.permute(0, 2, 3, 1)[poisoned]).all() and torch.isnan(av[poisoned]).all()
        assert torch.isfinite(ed.permute(0, 2, 3, 1)[poisoned]).all()
        # the NaN offset: prob untouched, the pick's depth and the expectation NaN
        assert int(ei[1, 0, 3, 7]) == D - 2 and torch.isnan(ed[1, 0, 3, 7]) and torch.isnan(av[1, 3, 7])
        assert torch.isnan(off[1, D - 2, 3, 7]) and int(torch.isnan(off).sum()) == 1
        assert torch.isfinite(ed[1, 1:, 3, 7]).all() and torch.isfinite(en[1, :, 3, 7]).all()
        assert torch.equal(prob[1, :, 3, 7], ref[0].detach()[1, :, 3, 7])
        # the ordinary pixels: the bits of the clean call
        for got, want in zip((prob, off, ed, en, ei, av), [t.detach() for t in ref]):
            sel = ordinary if got.dim() == 3 else ordinary.unsqueeze(1).expand_as(got)
            assert torch.equal(got[sel], want[sel])
            assert torch.isfinite(got[sel].float()).all()
        # backward: returns, and leaves the ordinary pixels' gradients as they are without the poison
        g = torch.Generator().manual_seed(5)
        cots = [torch.randn(t.shape, generator=g).to(gpu) for t in (out[0], out[1], out[2], out[3], out[5])]
        sum((t * c).sum() for t, c in zip((out[0], out[1], out[2], out[3], out[5]), cots)).backward()
        sum((t * c).sum() for t, c in zip((ref[0], ref[1], ref[2], ref[3], ref[5]), cots)).backward()
        torch.cuda.synchronize()
        sel = ordinary.view(N, 1, 1, H, W).expand_as(leaf.grad)
        assert torch.equal(leaf.grad[sel], cleaf.grad[sel]) and torch.isfinite(leaf.grad[sel]).all()


@pytest.mark.parametrize("D,topk", [(8, 3), (8, 8), (100, 3), (100, 8)])
def test_sample_depth_prob_nan_probabilities(gpu, D, topk):
    """Ready-made probabilities can be NaN plane by plane: two NaNs among numbers rank first, the lower plane first, then the
    numbers in descending order; an all-NaN column ranks 0 .. topk-1.  Both of sample_depth_prob's specialisations."""
    from mvsdet_amd import ops
    N, H, W = 2, 3, 50
    near, iv = 0.2, 4.8 / D
    clean_p, clean_o = _prob_off(N, D, H, W, 40 + D, gpu)
    prob, off = clean_p.clone(), clean_o.clone()
    prob[0, :6, 1, 4] = torch.tensor([0.1, NAN, 0.5, 0.2, NAN, 0.05], device=gpu)
    prob[0, 6:, 1, 4] = 0.001
    prob[1, :, 2, 49] = NAN
    prob[1, D - 1, 0, 0] = NAN                                       # one NaN, on the last plane
    poisoned = torch.zeros((N, H, W), dtype=torch.bool, device=gpu)
    poisoned[0, 1, 4] = poisoned[1, 2, 49] = poisoned[1, 0, 0] = True
    ed, en, ei, av = ops.sample_depth_prob(prob, off, near, iv, topk)
    ced, cen, cei, cav = ops.sample_depth_prob(clean_p, clean_o, near, iv, topk)
    _check_exact(prob, off, ed, en, ei, near, iv, f"sample NaN {(D, topk)}")
    _no_sentinel(ed, en, av)
    head = [1, 4, 2, 3, 0, 5, 6, 7][:topk]
    assert ei[0, :, 1, 4].tolist() == head
    assert torch.isnan(en[0, :2, 1, 4]).all() and torch.isfinite(en[0, 2:, 1, 4]).all()
    assert ei[1, :, 2, 49].tolist() == list(range(topk)) and torch.isnan(en[1, :, 2, 49]).all()
    assert int(ei[1, 0, 0, 0]) == D - 1 and torch.isnan(en[1, 0, 0, 0]) and torch.isfinite(en[1, 1:, 0, 0]).all()
    assert torch.isnan(av[poisoned]).all() and torch.isfinite(ed).all()
    for got, want in ((ed, ced), (en, cen), (ei, cei), (av, cav)):
        sel = ~poisoned if got.dim() == 3 else (~poisoned).unsqueeze(1).expand_as(got)
        assert torch.equal(got[sel], want[sel])
    # the plain-tensor backward of the function-level patch: returns, ordinary pixels untouched
    p, o = prob.clone().requires_grad_(True), off.clone().requires_grad_(True)
    cp, co = clean_p.clone().requires_grad_(True), clean_o.clone().requires_grad_(True)
    R = torch.randn(ed.shape, generator=torch.Generator().manual_seed(1)).to(gpu)
    for a, b in ((p, o), (cp, co)):
        e2, n2, _, a2 = ops.sample_depth_prob(a, b, near, iv, topk)
        ((e2 + n2) * R).sum().backward()
    sel = (~poisoned).unsqueeze(1).expand_as(p.grad)
    assert torch.equal(p.grad[sel], cp.grad[sel]) and torch.equal(o.grad[sel], co.grad[sel])


def test_nan_pixel_reaches_the_volume_as_in_the_oracle_chain(gpu, oracle):
    """A pixel with a NaN logit through MVSDetHotPath.depth_distribution and lift: its densities are NaN and its candidate depths
    those of planes 0 .. 2, so every voxel whose ray meets that pixel inside that depth window is counted valid with a NaN
    weight: the volume is NaN there, as in the oracle chain -- not a finite value weighted 1/J."""
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 4, 8, 12, (24, 32)
    hp = MVSDetHotPath([24, 24, 10], [0.2, 0.2, 0.2], [0.2, 5.0], D, topk=3)
    meta = synthetic.make_img_meta(N, hw, seed=21)
    feat = synthetic.make_features(N, C, hw, seed=21)
    logits = synthetic.make_cost_logits(N, D, hw, seed=21)
    geo = hp.prepare_scene(meta, gpu)
    h, w = geo.height, geo.width
    pts, proj = geo.points.cpu().numpy(), geo.projection.cpu().numpy()
    iv = float(hp.depth_interval)
    # the pixel of view 0 that most voxels meet at the depths of planes 0 .. 2 (+- the voxel height)
    probe = oracle.depth_prob_topk(logits[:, 0], logits[:, 1], 0.2, iv, 3)
    pv = oracle.backproject_weigh(feat.numpy()[:, :, :h, :w], pts, proj, probe["est_depth"][:, :, :h, :w],
                                  probe["est_dens"][:, :, :h, :w], 0.2, want_index=True)
    x0, y0, z0 = pv["x"][0], pv["y"][0], pv["z"][0]
    near_cam = (x0 >= 0) & (x0 < w) & (y0 >= 0) & (y0 < h) & (z0 > 0.25) & (z0 < 0.2 + 2 * iv)
    assert near_cam.sum() > 0, "no voxel of the grid close enough to camera 0"
    pix, cnt = np.unique(y0[near_cam].astype(np.int64) * w + x0[near_cam], return_counts=True)
    py, px = divmod(int(pix[cnt.argmax()]), w)
    logits[0, 0, 4, py, px] = NAN
    prob, off, ed, en, ei, av = hp.depth_distribution(logits.to(gpu))
    assert torch.isnan(en[0, :, py, px]).all() and ei[0, :, py, px].tolist() == [0, 1, 2]
    featg = feat.to(gpu)
    mean, count = hp.lift(featg, ops.pack_features(featg), geo, ed, en)
    # the oracle chain: its stage 2 poisons the same pixel in the same way ...
    r = oracle.depth_prob_topk(logits[:, 0], logits[:, 1], 0.2, iv, 3)
    np.testing.assert_array_equal(np.isnan(r["est_dens"]), torch.isnan(en).cpu().numpy())
    assert r["est_idx"][0, :, py, px].tolist() == [0, 1, 2]
    np.testing.assert_allclose(r["est_depth"][0, :, py, px], ed[0, :, py, px].cpu().numpy(), rtol=0, atol=1e-6)   # off: 1e-6
    # ... and its stage 3, fed the kernel's candidates as in smoke(), is the kernel's volume bit for bit, NaN included
    edn, enn = ed.cpu().numpy()[:, :, :h, :w], en.cpu().numpy()[:, :, :h, :w]
    o = oracle.backproject_weigh(feat.numpy()[:, :, :h, :w], pts, proj, edn, enn, 0.2, want_index=True)
    m = oracle.backproject_weigh_mean(feat.numpy()[:, :, :h, :w], pts, proj, edn, enn, 0.2)
    hit = o["valid"][0] & (o["x"][0] == px) & (o["y"][0] == py)         # inside the window, through the poisoned pixel
    assert hit.sum() > 0 and np.isnan(o["volume"][0][:, hit]).all()
    got = mean.view(C, -1).cpu().numpy()
    assert np.isnan(got[:, hit]).all(), "a voxel through the NaN pixel is valid with a finite value"
    assert np.isnan(m["volume_mean"]).any() and np.isfinite(m["volume_mean"]).any()
    np.testing.assert_array_equal(got, m["volume_mean"])
    np.testing.assert_array_equal(count.view(-1).cpu().numpy(), m["valid_count"])


# --------------------------------------------------------------------------------------------- stage 3
VZ = 0.25


def _stage3_fixture(N, C, J, V, hw, seed):
    """Identity-like projections (q = (X + a_i Z, Y + b_i Z, Z): pixel = (X / Z + a_i, Y / Z + b_i), depth Z; view i shifts the
    image by whole pixels (a_i, b_i), view i % 7 == 3 has a NaN row), candidate depths 2.0 + 0.125 j at every pixel, and voxels
    placed by hand in front of random ones.  -> dict of numpy inputs and the hand-placed kinds {name: voxel index}."""
    h, w = hw
    H, W = h + 2, w + 3
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((N, C, H, W)).astype(np.float32)
    depth = np.broadcast_to((2.0 + 0.125 * np.arange(J, dtype=np.float32)).reshape(1, J, 1, 1), (N, J, H, W)).copy()
    dens = (rng.random((N, J, H, W)).astype(np.float32) + 0.05)
    dens[:, :, 1, 1] = 0.0                       # psum == 0
    dens[:, J // 2, 2, 2] = np.nan               # one NaN density
    depth[:, :, :, w:] = np.nan                  # the padding is never read
    depth[:, :, h:, :] = np.nan
    proj = np.zeros((N, 3, 4), np.float32)
    for i in range(N):
        a, b = (0, 0) if i == 0 else (int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))
        proj[i] = [[1, 0, a, 0], [0, 1, b, 0], [0, 0, 1, 0]]
        if i % 7 == 3:
            proj[i, 1] = np.nan
    Z = 2.0
    top = 2.0 + 0.125 * (J - 1)
    kinds = {
        "inside": (3 * Z, 3 * Z, Z),
        "x=-0.5": (-0.5 * Z, 3 * Z, Z),                     # rounds to -0: inside
        "x=-1.5": (-1.5 * Z, 3 * Z, Z),                     # rounds to -2: outside
        "x=w-0.5": ((w - 0.5) * Z, 2 * Z, Z),               # rounds to even: w - 1 (inside) if w is odd, w (outside) if even
        "y=h-0.5": (2 * Z, (h - 0.5) * Z, Z),
        "x=w-1.5": ((w - 1.5) * Z, 2 * Z, Z),
        "q2==0": (1.0, 1.0, 0.0),
        "q2<0": (3 * -Z, 3 * -Z, -Z),
        "z==d0-vz": (3 * 1.75, 3 * 1.75, 1.75),             # exactly on the window's lower edge: outside (strict <)
        "z>d0-vz": (4 * np.float32(1.7500001), 3 * np.float32(1.7500001), np.float32(1.7500001)),
        "z==dJ+vz": (3 * (top + VZ), 4 * (top + VZ), top + VZ),
        "z<dJ+vz": (4 * np.float32(top + VZ - 2e-7), 4 * np.float32(top + VZ - 2e-7), np.float32(top + VZ - 2e-7)),
        "psum==0": (1 * Z, 1 * Z, Z),
        "nan density": (2 * Z, 2 * Z, Z),
        "far": (3 * 9.0, 3 * 9.0, 9.0),
    }
    hand = np.array(list(kinds.values()), np.float32)
    if V > len(hand):
        zr = rng.uniform(1.5, 3.2, V - len(hand)).astype(np.float32)
        rest = np.stack([rng.uniform(-2, w + 2, len(zr)).astype(np.float32) * zr, rng.uniform(-2, h + 2, len(zr)).astype(np.float32) * zr, zr], 1)
        hand = np.concatenate([hand, rest])
    pts = np.ascontiguousarray(hand[:V].T)
    return dict(feat=feat, depth=depth, dens=dens, proj=proj, pts=pts, h=h, w=w, H=H, W=W,
                kinds={k: i for i, k in enumerate(kinds) if i < V})


S3_CASES = [  # J, N, C, V: every J, N, C and V of the grid at least twice; the large N and C with few voxels
    (1, 1, 6, 1), (2, 1, 256, 31), (8, 1, 260, 33), (1, 64, 6, 255), (2, 64, 300, 33), (8, 65, 6, 257), (1, 65, 260, 31),
    (2, 129, 6, 33), (8, 129, 256, 31), (1, 129, 300, 1), (8, 64, 256, 1), (2, 65, 300, 255), (3, 5, 40, 257),
]


@pytest.mark.parametrize("hw", [(6, 7), (5, 8)])
@pytest.mark.parametrize("J,N,C,V", S3_CASES)
def test_backproject_forward_vs_oracle(gpu, oracle, J, N, C, V, hw):
    from mvsdet_amd import _lib, ops
    fx = _stage3_fixture(N, C, J, V, hw, seed=1000 * J + N + C + V)
    h, w, H, W = fx["h"], fx["w"], fx["H"], fx["W"]
    crop = lambda a: a[:, :, :h, :w]                                                        # noqa: E731
    o = oracle.backproject_weigh(crop(fx["feat"]), fx["pts"], fx["proj"], crop(fx["depth"]), crop(fx["dens"]), VZ, want_index=True)
    m = oracle.backproject_weigh_mean(crop(fx["feat"]), fx["pts"], fx["proj"], crop(fx["depth"]), crop(fx["dens"]), VZ)
    valid0, k = o["valid"][0], fx["kinds"]
    if V >= 31:   # the fixture holds what it is meant to hold (view 0: the unshifted image)
        assert len(k) == 15
        for name in ("inside", "x=-0.5", "x=w-1.5", "z>d0-vz", "z<dJ+vz", "psum==0", "nan density"):
            assert valid0[k[name]], name
        for name in ("x=-1.5", "q2==0", "q2<0", "z==d0-vz", "z==dJ+vz", "far"):
            assert not valid0[k[name]], name
        assert valid0[k["x=w-0.5"]] == (w % 2 == 1) and valid0[k["y=h-0.5"]] == (h % 2 == 1)   # half to even at the border
        assert o["x"][0][k["x=-0.5"]] == 0 and o["x"][0][k["x=w-0.5"]] == (w - 1 if w % 2 else w)
        assert o["y"][0][k["y=h-0.5"]] == (h - 1 if h % 2 else h)
        assert np.isnan(o["volume"][0][:, k["psum==0"]]).all() and np.isnan(o["volume"][0][:, k["nan density"]]).all()
        assert np.isfinite(o["volume"][0][:, k["inside"]]).all() and np.abs(o["volume"][0][:, k["inside"]]).max() > 0
        if N > 3:
            assert not o["valid"][3].any() and (o["y"][3] == np.iinfo(np.int32).min).all()     # the NaN projection row
        if V > 100:
            assert 0.05 < o["valid"].mean() < 0.95
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(gpu)                       # noqa: E731
    feat, depth, dens = dev(fx["feat"]), dev(fx["depth"]), dev(fx["dens"])
    pts, proj = dev(fx["pts"]), dev(fx["proj"])
    fc, dc, nc = crop(feat), crop(depth), crop(dens)
    # per view, through the C ABI with the pixel indices
    xi = torch.empty((N, V), dtype=torch.int32, device=gpu)
    yi = torch.empty((N, V), dtype=torch.int32, device=gpu)
    vol = torch.empty((N, C, V), device=gpu)
    val = torch.empty((N, V), dtype=torch.uint8, device=gpu)
    rc = _lib.load().mvsdet_backproject_weigh_f32(_lib.ptr(fc), _lib.strides4(fc), _lib.ptr(pts), _lib.ptr(proj), _lib.ptr(dc),
                                                  _lib.ptr(nc), _lib.strides4(dc), _lib.ptr(vol), _lib.ptr(val), _lib.ptr(xi),
                                                  _lib.ptr(yi), N, C, h, w, V, J, ctypes.c_float(VZ), _lib.current_stream(gpu))
    assert rc == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(val.cpu().numpy().astype(bool), o["valid"])
    np.testing.assert_array_equal(xi.cpu().numpy(), o["x"])
    np.testing.assert_array_equal(yi.cpu().numpy(), o["y"])
    np.testing.assert_array_equal(vol.cpu().numpy(), o["volume"])            # NaN in the same places (NaN == NaN here)
    vol2, val2 = ops.backproject_weigh(fc, pts, proj, dc, nc, VZ)
    assert torch.equal(val2, val.bool()) and _same_bits(vol2, vol)
    # fused mean and sum
    packed = ops.pack_features(feat)
    mean, count = ops.backproject_weigh_mean(fc, packed, pts, proj, dc, nc, H, W, VZ)
    total, count2 = ops.backproject_weigh_sum_shard(packed, pts, proj, dc, nc, N, 0, C, H, W, VZ)
    cnt = o["valid"].sum(0).astype(np.int32)
    np.testing.assert_array_equal(count.cpu().numpy(), cnt)
    np.testing.assert_array_equal(count2.cpu().numpy(), cnt)
    np.testing.assert_array_equal(cnt, m["valid_count"])
    acc = np.zeros((C, V), np.float32)
    for i in range(N):                                                        # ascending views, fp32, one rounding per addition
        acc = acc + o["volume"][i]
    np.testing.assert_array_equal(total.cpu().numpy(), acc)
    with np.errstate(invalid="ignore"):
        want = np.where(cnt > 0, acc / (cnt.astype(np.float32) + np.float32(1e-8)), np.float32(0)).astype(np.float32)
    np.testing.assert_array_equal(mean.cpu().numpy(), want)
    np.testing.assert_array_equal(mean.cpu().numpy(), m["volume_mean"])


# --------------------------------------------------------------------------------------------- ray_depth
@pytest.mark.parametrize("J", [0, 1, 8])
def test_ray_depth_forward_vs_float64(gpu, record_property, J):
    """depth_scale = 1 / |(xl, yl, 1)| with xl = (x - cx + cy sk / fy - sk y / fy) / fx, yl = (y - cy) / fy (mvsdet.py:1300-1313),
    est_ray_depth = est_depth / (depth_scale + 1e-8) (:494), in float64 from the float32 intrinsics.
    Bars: xl's numerator is four terms of size <= M = max(w, |cx|, |cy sk / fy|, |sk h / fy|), each sum rounded (<= 3 x 4 M EPS)
    and two of them carrying two roundings of their own (<= 4 M EPS): dxl <= (16 M / fx + 1) EPS, and d scale = scale^3 xl dxl
    <= 0.39 dxl, plus the square root, the sum of squares and the division (4 EPS): scale within (8 M / fx + 5) EPS.
    est_ray_depth adds that relative to the smallest scale, one addition and one division: (8 M / fx + 5) / min(scale) + 2 EPS of
    the largest |est_ray_depth|."""
    from mvsdet_amd import ops
    N, H, W, h, w = 3, 13, 21, 11, 18
    intr = torch.tensor([[20.0, 19.0, 9.3, 5.1, 0.0], [15.5, 16.5, 8.0, 6.0, 0.7], [31.0, 29.0, 2.5, 9.5, -1.3]])
    g = torch.Generator().manual_seed(J)
    est = None
    if J:
        est = torch.rand((N, J, H, W), generator=g) * 4.8 + 0.2
        est[:, :, h:] = NAN
        est[:, :, :, w:] = NAN
    scale, ray = ops.ray_depth(intr.to(gpu), None if est is None else est.to(gpu), h, w)
    i64 = intr.double()
    fx, fy, cx, cy, sk = [i64[:, k].view(N, 1, 1) for k in range(5)]
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    xl = (x - cx + cy * sk / fy - sk * y / fy) / fx
    yl = (y - cy) / fy
    ref = 1.0 / torch.sqrt(xl * xl + yl * yl + 1.0)
    M = torch.maximum(torch.maximum(torch.full_like(cx, float(w)), cx.abs()), torch.maximum((cy * sk / fy).abs(), (sk * h / fy).abs()))
    sbar = float((8 * M / fx + 5).max()) * EPS
    assert scale.shape == (N, h * w, 1)
    es = _err(scale.cpu().view(N, h, w), ref)
    record_property("ray_depth_scale_err", es)
    record_property("ray_depth_scale_bar", sbar)
    print(f"ray_depth J={J}: depth_scale err {es:.3e} bar {sbar:.3e}")
    assert es <= sbar
    if not J:
        assert ray is None
        return
    assert ray.shape == (N, h * w, 1, J)
    want = est.double()[:, :, :h, :w] / (ref.unsqueeze(1) + 1e-8)                        # (N, J, h, w)
    got = ray.cpu().squeeze(2).transpose(2, 1).reshape(N, J, h, w)
    assert torch.isfinite(got).all(), "the NaN padding of est_depth was read"
    rbar = (sbar / float(ref.min()) + 2 * EPS)
    er = _err(got, want) / float(want.abs().max())
    record_property("ray_depth_ray_err", er)
    record_property("ray_depth_ray_bar", rbar)
    print(f"ray_depth J={J}: est_ray_depth err {er:.3e} of scale, bar {rbar:.3e}")
    assert er <= rbar
