"""Depth supervision on the GPU (csrc/depthloss.hip; ops.depth.depth_loss / depth_loss_backward; functional.depth_loss_func_new,
functional.mvsnet_loss; MVSDetHotPath.depth_loss) against the restatement of tests/depth_loss_restated.py and fixture G24 (the
reference's own numbers and autograd, tests/golden/make_goldens_g24.py).

Bars.
  loss, l1        against the restatement |d| <= 2e-6 + 1e-6 |loss|: two ulps of the largest depth (8 m) per term carried through a mean,
                  plus the final fp32 rounding with margin; against G24's fp32 value rtol 1e-5, the reference's own fp32 mean over at
                  most 2^20 terms
  loss, smooth_l1 rtol 1e-6 against the restatement (no resize), 1e-5 against G24
  count           exact
  gradient, l1    bit-equal to the restatement's fl32(g / count) * sign; equal to G24's wherever G24's is non-zero, masks identical
  gradient, smooth_l1   rtol 1e-6 against both
torch.autograd.gradcheck is not used (the arithmetic is fp32); one central-difference spot check on a 3x5 map away from the kinks.
Measured on one MI355X: l1 loss equal to the restatement's and to G24's fp32 number on all four cases, smooth-L1 equal to the restatement's and
8e-8 relative from G24's, central differences within 1.2e-6 of the gradient; the whole file takes 5 s.
"""
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from depth_loss_restated import F32, L1, SMOOTH_L1, restate
from lcg import lcg_uniform
from test_depth_loss_host import L1_CASES, SMOOTH_CASES, g24_case

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def run(est, gt, mask, kind):
    """est: a device tensor (any view) -> (loss float32 scalar, count int, grad (N,h,w) array of d loss / d est)."""
    from mvsdet_amd.ops import depth
    leaf = est.detach().requires_grad_(True)
    loss, count = depth.depth_loss(leaf, gt, mask, kind)
    assert loss.shape == () and count.shape == () and loss.dtype == torch.float32 and count.dtype == torch.int32
    loss.backward()
    return F32(loss.detach().cpu().numpy()), int(count.cpu()), leaf.grad.cpu().numpy()


def holes_map(N, H, W, seed, hole=0.7):
    """Depths in [0.5, 6.5) with zeros over a third of the map (LCG: the same on every machine)."""
    u = lcg_uniform(2 * N * H * W, seed).reshape(2, N, H, W)
    return np.where(u[1] > hole - 0.37, F32(0), F32(3.5) + F32(3) * u[0]).astype(F32)


def close_to_restatement(loss, ref):
    return abs(float(loss) - float(ref)) <= 2e-6 + 1e-6 * abs(float(ref))


@pytest.mark.parametrize("tag", L1_CASES)
def test_l1_against_the_restatement_and_g24(gpu, tag):
    c = g24_case(tag)
    gt = torch.from_numpy(c["gt"]).to(gpu)
    if tag == "ref_true":
        full = c["est_full"].copy()
        full[:, 59:] = np.nan                                                 # the padding row of the 60x80 map is never read
        est = torch.from_numpy(full).to(gpu)[:, :59, :80]
        assert not est.is_contiguous()
    else:
        est = torch.from_numpy(c["est"]).to(gpu)
    loss, count, grad = run(est, gt, None, L1)
    r = restate(c["est"], c["gt"])
    print(f"{tag}: loss {float(loss)!r} restatement {float(r['loss'])!r} (distance {abs(float(loss) - float(r['loss'])):.2e}) G24 "
          f"{float(c['loss'])!r} (relative {abs(float(loss) - float(c['loss'])) / float(c['loss']):.2e}), count {count}")
    assert close_to_restatement(loss, r["loss"])
    assert abs(float(loss) - float(c["loss"])) <= 1e-5 * abs(float(c["loss"]))
    assert count == r["count"] == int(c["count"])
    assert np.array_equal(grad.view(np.int32), r["grad"].view(np.int32))
    nz = c["grad"] != 0
    assert np.array_equal(grad != 0, nz) and np.array_equal(grad[nz], c["grad"][nz])


@pytest.mark.parametrize("tag", SMOOTH_CASES)
def test_smooth_l1_against_the_restatement_and_g24(gpu, tag):
    c = g24_case(tag)
    est, gt, mask = (torch.from_numpy(c[k]).to(gpu) for k in ("est", "gt", "mask"))
    loss, count, grad = run(est, gt, mask, SMOOTH_L1)
    r = restate(c["est"], c["gt"], c["mask"], SMOOTH_L1)
    print(f"{tag}: loss {float(loss)!r} restatement {float(r['loss'])!r} G24 {float(c['loss'])!r}, count {count}")
    assert abs(float(loss) - float(r["loss"])) <= 1e-6 * abs(float(r["loss"]))
    assert abs(float(loss) - float(c["loss"])) <= 1e-5 * abs(float(c["loss"]))
    assert count == r["count"] == int(c["count"])
    np.testing.assert_allclose(grad, r["grad"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(grad, c["grad"], rtol=1e-6, atol=0)
    assert np.array_equal(grad != 0, c["grad"] != 0)


def test_exact_tie_has_gradient_zero(gpu):
    c = g24_case("same")
    est = c["est"].copy()
    assert c["gt"][0, 2, 3] > 0 and c["gt"][1, 6, 8] > 0
    est[0, 2, 3], est[1, 6, 8] = c["gt"][0, 2, 3], c["gt"][1, 6, 8]           # est == gt: |.| has no slope there, sign(0) = 0
    loss, count, grad = run(torch.from_numpy(est).to(gpu), torch.from_numpy(c["gt"]).to(gpu), None, L1)
    r = restate(est, c["gt"])
    assert grad[0, 2, 3] == 0 and grad[1, 6, 8] == 0 and count == int(c["count"])      # inside the mask, counted, no gradient
    assert np.array_equal(grad.view(np.int32), r["grad"].view(np.int32)) and close_to_restatement(loss, r["loss"])
    assert int((grad != 0).sum()) == count - 2


def test_empty_mask(gpu):
    """NaN loss (0 / 0, torch.mean of nothing), count 0, an all-zero gradient -- as the reference."""
    est = torch.ones(2, 5, 7, device=gpu)
    for gt, mask, kind in ((torch.zeros(2, 11, 13, device=gpu), None, L1),
                           (torch.full((2, 11, 13), float("nan"), device=gpu), None, L1),
                           (torch.ones(2, 5, 7, device=gpu), torch.full((2, 5, 7), 0.5, device=gpu), SMOOTH_L1)):
        loss, count, grad = run(est, gt, mask, kind)
        assert np.isnan(loss) and count == 0 and (grad == 0).all() and grad.shape == (2, 5, 7)


def test_single_masked_pixel_in_the_last_partial_block(gpu):
    N, h, w = 1, 17, 31                                                       # 527 pixels: blocks of 256, 256 and 15
    gt = np.zeros((N, h, w), F32)
    gt[0, h - 1, w - 1] = 2.5
    est = np.full((N, h, w), 1.25, F32)
    loss, count, grad = run(torch.from_numpy(est).to(gpu), torch.from_numpy(gt).to(gpu), None, L1)
    assert float(loss) == 1.25 and count == 1
    assert grad[0, h - 1, w - 1] == -1.0 and int((grad != 0).sum()) == 1
    m = np.zeros((N, h, w), F32)
    m[0, h - 1, w - 1] = 1
    loss, count, grad = run(torch.from_numpy(est).to(gpu), torch.from_numpy(gt).to(gpu), torch.from_numpy(m).to(gpu), SMOOTH_L1)
    assert float(loss) == 0.75 and count == 1 and grad[0, h - 1, w - 1] == -1.0 and int((grad != 0).sum()) == 1


@pytest.mark.parametrize("shape", [(1, 10, 25), (1, 16, 16), (3, 13, 21), (7, 97, 101)], ids=lambda s: "x".join(map(str, s)))
def test_block_counts(gpu, shape):
    """250 pixels (one partial block), 256 (exactly one), 819 (three and a partial one), 68579 (268 blocks: past 256 a thread of the
    finishing launch adds a run of two partials, and the threads past the last run none): both kinds against the restatement,
    gradient bit for bit."""
    N, h, w = shape
    gt = holes_map(N, 2 * h + 3, 3 * w - 1, seed=sum(shape))
    est = (F32(3.5) + F32(2) * lcg_uniform(N * h * w, 77 + h).reshape(N, h, w)).astype(F32)
    loss, count, grad = run(torch.from_numpy(est).to(gpu), torch.from_numpy(gt).to(gpu), None, L1)
    r = restate(est, gt)
    assert 0 < r["count"] < N * h * w and count == r["count"] and close_to_restatement(loss, r["loss"])
    assert np.array_equal(grad.view(np.int32), r["grad"].view(np.int32))
    gt2, mask = holes_map(N, h, w, seed=5 + w, hole=2.0), (holes_map(N, h, w, seed=9 + h) > 0).astype(F32)
    loss, count, grad = run(torch.from_numpy(est).to(gpu), torch.from_numpy(gt2).to(gpu), torch.from_numpy(mask).to(gpu), SMOOTH_L1)
    r = restate(est, gt2, mask, SMOOTH_L1)
    assert count == r["count"] == int(mask.sum()) and abs(float(loss) - float(r["loss"])) <= 1e-6 * abs(float(r["loss"]))
    np.testing.assert_allclose(grad, r["grad"], rtol=1e-6, atol=0)


def test_nan_and_inf_taps(gpu):
    """A NaN tap makes its pixels NaN: they leave the mask.  An inf tap makes its pixels inf: they enter it and the loss is inf.  The
    gradient stays finite (fl32(1 / count) * sign) and is the restatement's bit for bit."""
    c = g24_case("odd")
    gt = c["gt"].copy()
    gt[0, 6, 7] = np.nan
    gt[1, 11, 15] = np.inf
    gt[2, 20, 29] = np.inf
    gt[2, 20, 28] = np.nan
    loss, count, grad = run(torch.from_numpy(c["est"]).to(gpu), torch.from_numpy(gt).to(gpu), None, L1)
    r = restate(c["est"], gt)
    assert np.isnan(r["g"]).sum() >= 2 and np.isinf(r["g"]).sum() >= 1
    assert np.isinf(loss) and loss > 0 and count == r["count"]
    assert np.isfinite(grad).all() and np.array_equal(grad.view(np.int32), r["grad"].view(np.int32))
    assert (grad[np.isnan(r["g"])] == 0).all() and (grad[np.isinf(r["g"])] < 0).all()
    # only NaN: the loss stays finite and is the restatement's
    gt[np.isinf(gt)] = np.nan
    loss, count, grad = run(torch.from_numpy(c["est"]).to(gpu), torch.from_numpy(gt).to(gpu), None, L1)
    r = restate(c["est"], gt)
    assert np.isfinite(loss) and close_to_restatement(loss, r["loss"]) and count == r["count"] < int(c["count"])


def test_strided_inputs_are_read_in_place(gpu):
    """est as the crop of a padded map, gt as a window of a NaN canvas and as a transposed view: the bits of the contiguous call."""
    c = g24_case("odd")
    est_c, gt_c = torch.from_numpy(c["est"]).to(gpu), torch.from_numpy(c["gt"]).to(gpu)
    want = run(est_c, gt_c, None, L1)
    N, h, w = c["est"].shape
    Hg, Wg = c["gt"].shape[1:]
    pad = torch.full((N, h + 1, w + 3), float("nan"), device=gpu)
    pad[:, :h, :w] = est_c
    canvas = torch.full((N + 1, Hg + 2, Wg + 5), float("nan"), device=gpu)
    canvas[1:, 1:-1, 2:-3] = gt_c
    gt_t = gt_c.permute(0, 2, 1).contiguous().permute(0, 2, 1)                # same values, x stride Hg
    assert not gt_t.is_contiguous()
    for est, gt in ((pad[:, :h, :w], canvas[1:, 1:-1, 2:-3]), (est_c, gt_t)):
        got = run(est, gt, None, L1)
        assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2].view(np.int32), want[2].view(np.int32))
    s = g24_case("smooth_small")
    e, g, m = (torch.from_numpy(s[k]).to(gpu) for k in ("est", "gt", "mask"))
    want = run(e, g, m, SMOOTH_L1)
    mc = torch.full((2, 5, 9), float("nan"), device=gpu)
    mc[:, :, 1:8] = m
    got = run(e, g.permute(0, 2, 1).contiguous().permute(0, 2, 1), mc[:, :, 1:8], SMOOTH_L1)
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2].view(np.int32), want[2].view(np.int32))


def test_two_runs_give_the_same_bits(gpu):
    c = g24_case("ref_true")
    est, gt = torch.from_numpy(c["est_full"]).to(gpu)[:, :59, :80], torch.from_numpy(c["gt"]).to(gpu)
    a, b = run(est, gt, None, L1), run(est, gt, None, L1)
    assert a[0].view(np.int32) == b[0].view(np.int32) and a[1] == b[1] and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))


def test_no_host_synchronisation(gpu):
    from mvsdet_amd import functional as F_
    c, s = g24_case("ref_true"), g24_case("smooth_big")
    full, gt = torch.from_numpy(c["est_full"]).to(gpu), torch.from_numpy(c["gt"]).to(gpu)
    e, g, m = (torch.from_numpy(s[k]).to(gpu) for k in ("est", "gt", "mask"))

    def step():
        a, b = full.detach().requires_grad_(True), e.detach().requires_grad_(True)
        la = F_.depth_loss_func_new([a[:, :59, :80].unsqueeze(1)], [gt])["loss_depth"]
        lb = F_.mvsnet_loss(b, g, m)
        la.backward()
        lb.backward()
        return la, lb, a.grad, b.grad

    step()   # warm: library load, allocator
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        la, lb, ga, gb = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert abs(float(la) - float(c["loss"])) <= 1e-5 * float(c["loss"]) and abs(float(lb) - float(s["loss"])) <= 1e-5 * float(s["loss"])
    assert ga.shape == full.shape and bool((ga[:, 59:] == 0).all()) and gb.shape == e.shape


def test_finite_difference_spot_check(gpu):
    """3x5, every |d| in [0.2, 0.8] or [1.3, 1.9]: a step of 2^-6 crosses no kink, both objectives are at most quadratic along it, so
    the central difference IS the derivative up to the rounding of two fp32 losses (6e-8 * 1.5 / 2^-5 = 3e-6; bar 2e-5)."""
    from mvsdet_amd.ops import depth
    u = lcg_uniform(30, 4242).reshape(2, 1, 3, 5)
    gt = (F32(2) + u[0]).astype(F32)
    size = np.where(np.arange(15).reshape(1, 3, 5) % 2 == 0, 0.2 + 0.6 * np.abs(u[1]), 1.3 + 0.6 * np.abs(u[1]))
    est = (gt + np.where(u[1] > 0, 1, -1) * size).astype(F32)
    mask = np.ones((1, 3, 5), F32)
    mask[0, 1, 2] = 0
    gt_d, mask_d = torch.from_numpy(gt).to(gpu), torch.from_numpy(mask).to(gpu)
    eps = 2.0 ** -6
    for kind, mk in ((L1, None), (SMOOTH_L1, mask_d)):
        _, _, grad = run(torch.from_numpy(est).to(gpu), gt_d, mk, kind)
        for (y, x) in ((0, 0), (1, 2), (1, 3), (2, 4)):
            vals = []
            for sgn in (1, -1):
                e = est.copy()
                e[0, y, x] += F32(sgn * eps)
                vals.append(float(depth.depth_loss(torch.from_numpy(e).to(gpu), gt_d, mk, kind)[0].cpu()))
            fd = (vals[0] - vals[1]) / (2 * eps)
            print(f"kind {kind} pixel {(y, x)}: gradient {grad[0, y, x]!r} central difference {fd!r}")
            assert abs(fd - float(grad[0, y, x])) <= 2e-5
    assert grad[0, 1, 2] == 0                                                 # outside the smooth-L1 mask


def test_functionals_on_two_scene_lists(gpu):
    from mvsdet_amd import functional as F_
    a, b, g = g24_case("odd"), g24_case("enlarge"), load_golden("g24_depth_loss")
    ea, eb = (torch.from_numpy(c["est"]).to(gpu).requires_grad_(True) for c in (a, b))
    out = F_.depth_loss_func_new([ea.unsqueeze(1), eb.unsqueeze(1)], [torch.from_numpy(a["gt"]).to(gpu), torch.from_numpy(b["gt"])])
    loss = out["loss_depth"]
    assert set(out) == {"loss_depth"} and loss.dim() == 0 and loss.device == ea.device and loss.dtype == torch.float32
    loss.backward()
    ra, rb = restate(a["est"], a["gt"]), restate(b["est"], b["gt"])
    la, lb = run(ea, torch.from_numpy(a["gt"]).to(gpu), None, L1)[0], run(eb, torch.from_numpy(b["gt"]).to(gpu), None, L1)[0]
    assert F32(loss.detach().cpu().numpy()) == F32(la + lb)                   # the scenes' means added in list order, fp32
    assert abs(float(loss) - float(g["batch2:loss"])) <= 1e-5 * float(g["batch2:loss"])
    assert np.array_equal(ea.grad.cpu().numpy(), ra["grad"]) and np.array_equal(eb.grad.cpu().numpy(), rb["grad"])
    one = F_.depth_loss_func_new([ea.detach().unsqueeze(1)], [torch.from_numpy(a["gt"]).to(gpu)])["loss_depth"]
    assert F32(one.cpu().numpy()) == la                                       # one scene: 0. + x = x, no addition launched
    with pytest.raises(RuntimeError, match="no gradient"):
        F_.depth_loss_func_new([ea.unsqueeze(1)], [torch.from_numpy(a["gt"]).to(gpu).requires_grad_(True)])
    # mvsnet_loss: a (B,1,H,W) batch and a bool mask, as loaders hand them over
    s = g24_case("smooth_small")
    e = torch.from_numpy(s["est"]).to(gpu).requires_grad_(True)
    loss = F_.mvsnet_loss(e.unsqueeze(1), torch.from_numpy(s["gt"]).to(gpu).unsqueeze(1), torch.from_numpy(s["mask"] > 0.5).to(gpu).unsqueeze(1))
    loss.backward()
    r = restate(s["est"], s["gt"], s["mask"], SMOOTH_L1)
    assert abs(float(loss) - float(r["loss"])) <= 1e-6 * float(r["loss"])
    np.testing.assert_allclose(e.grad.cpu().numpy(), r["grad"], rtol=1e-6, atol=0)


def test_autocast_takes_the_inputs_to_fp32(gpu):
    from mvsdet_amd import functional as F_
    c = g24_case("odd")
    est16 = torch.from_numpy(c["est"]).to(gpu).half()
    gt = torch.from_numpy(c["gt"]).to(gpu)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = F_.depth_loss_func_new([est16.unsqueeze(1)], [gt])["loss_depth"]
    want = run(est16.float(), gt, None, L1)[0]
    assert loss.dtype == torch.float32 and F32(loss.cpu().numpy()) == want
    with pytest.raises(TypeError):
        F_.depth_loss_func_new([est16.unsqueeze(1)], [gt])


def test_hot_path_depth_loss_reaches_the_cost_logits(gpu):
    """MVSDetHotPath.depth_loss on a synthetic scene: the loss is the operator's on out["depth_coding"], and cost_logits.grad is the
    existing stage-2 backward (depth_prob_topk_backward) fed with this operator's gradient as g_avg, bit for bit."""
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    from mvsdet_amd.ops import depth
    from test_host_logic import meta_from
    g5 = load_golden("g5_backproject_scannet")
    N = g5["est_depth"].shape[0]
    h, w = int(g5["img_shape"][0] // 4), int(g5["img_shape"][1] // 4)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 12, topk=3)
    feature = torch.from_numpy(g5["feature"]).to(gpu)
    logits = synthetic.make_cost_logits(N, 12, (60, 80), seed=51, sharp=2.0).to(gpu).requires_grad_(True)
    gt = torch.from_numpy(holes_map(N, 47, 63, seed=24)).to(gpu)
    out = hp.forward_scene(feature, meta_from(g5), cost_logits=logits)
    keys = set(out)
    res = hp.depth_loss(out, gt)
    assert set(res) == {"loss_depth"} and set(out) == keys                    # no key added to SceneOutputs
    res["loss_depth"].backward()
    dc = out["depth_coding"].detach()
    assert dc.shape == (N, 1, h, w)
    loss, count = depth.depth_loss(dc[:, 0], gt, None, L1)
    assert torch.equal(loss, res["loss_depth"].detach()) and 0 < int(count) < N * h * w
    g = depth.depth_loss_backward(dc[:, 0], gt, None, count, torch.ones((), device=gpu), L1)
    prob, off, est_depth, est_dens, est_idx, avg = hp.depth_distribution(logits.detach())
    g_avg = torch.zeros_like(avg)
    g_avg[:, :h, :w] = g
    z = torch.zeros_like
    g_cost, g_off = ops.depth_prob_topk_backward(prob, off, est_idx, z(prob), z(est_depth), z(est_dens), g_avg,
                                                 float(hp.near_far_range[0]), float(hp.depth_interval))
    assert bool((logits.grad != 0).any())
    assert np.array_equal(bits(logits.grad[:, 0]), bits(g_cost)) and np.array_equal(bits(logits.grad[:, 1]), bits(g_off))
    # a sequence of scenes with the matching depths
    two = hp.depth_loss([out, out], [gt, gt])["loss_depth"]
    assert torch.equal(two.detach(), loss + loss)


def test_opt_in_patch_on_a_stand_in(gpu):
    from mvsdet_amd import integration

    class MVSDet:
        def depth_loss_func_new(self, est_depth, gt_depth):
            return dict(loss_depth="original")

    mod = types.SimpleNamespace(MVSDet=MVSDet)
    saved = integration.patch_reference_depth_loss(mod)
    try:
        c = g24_case("odd")
        est, gt = torch.from_numpy(c["est"]).to(gpu), torch.from_numpy(c["gt"]).to(gpu)
        got = MVSDet().depth_loss_func_new([est.unsqueeze(1)], [gt])["loss_depth"]
        assert F32(got.cpu().numpy()) == run(est, gt, None, L1)[0]
        assert MVSDet().depth_loss_func_new([est.cpu().unsqueeze(1)], [gt.cpu()]) == dict(loss_depth="original")
    finally:
        integration.unpatch_reference_depth_loss(mod, saved)
    assert MVSDet().depth_loss_func_new([est.unsqueeze(1)], [gt]) == dict(loss_depth="original")
