"""tests/lift_restated.py, the float64 reference of test_gpu_lift_forward_edges.py, pinned on the CPU: against the reference's own
outputs (fixture g4_depth_prob, at the bars test_gpu_parity.test_depth_prob_topk holds the kernel to), against the CPU oracle's
plane indices wherever the float64 probabilities are separated by more than 1e-6, and on the defined ranking rule itself
(descending, NaN above every number, the lower plane first among equals and among NaNs), which the oracle follows too."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from lift_restated import rank, restated

TOL = 1e-4          # est_depth / avg_depth bar of test_gpu_parity.test_depth_prob_topk
SEP = 1e-6          # plane indices are compared where neighbouring float64 probabilities differ by more than this


def _decided(prob64, topk):
    """(N, topk, H, W) bool: slot k's probability is more than SEP away from the ranks above and below it."""
    s = torch.sort(prob64, dim=1, descending=True, stable=True).values
    gap = s[:, :-1] - s[:, 1:]                                   # gap[k] = s[k] - s[k+1]
    big = torch.full_like(s[:, :1], float("inf"))
    below = torch.cat([gap, big], 1)[:, :topk]
    above = torch.cat([big, gap], 1)[:, :topk]
    return (below > SEP) & (above > SEP)


@pytest.mark.parametrize("tag", ["d8", "d12", "d12_arkit"])
def test_restatement_reproduces_fixture_g4(oracle, tag):
    g = load_golden("g4_depth_prob")
    near, far = [float(v) for v in g[f"near_far_{tag}"]]
    cost, offl = torch.from_numpy(g[f"cost_reg_{tag}"]), torch.from_numpy(g[f"off_logit_{tag}"])
    D = cost.shape[1]
    iv = (far - near) / D
    r = restated(cost, offl, near, iv, 3)
    np.testing.assert_allclose(r["prob"].numpy(), g[f"prob_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["off"].numpy(), g[f"off_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["est_dens"].numpy(), g[f"est_dens_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["est_depth"].numpy(), g[f"est_depth_{tag}"], rtol=0, atol=TOL)
    np.testing.assert_allclose(r["avg_depth"].numpy(), g[f"avg_depth_{tag}"], rtol=0, atol=TOL)
    # a6 + a7 alone on the reference's own prob / off
    s = restated(torch.from_numpy(g[f"prob_{tag}"]), torch.from_numpy(g[f"off_{tag}"]), near, iv, 3, from_logits=False)
    np.testing.assert_allclose(s["est_dens"].numpy(), g[f"est_dens_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(s["est_depth"].numpy(), g[f"est_depth_{tag}"], rtol=0, atol=TOL)
    np.testing.assert_allclose(s["avg_depth"].numpy(), g[f"avg_depth_{tag}"], rtol=0, atol=TOL)
    # plane indices against the oracle where the ranking is decided
    o = oracle.depth_prob_topk(cost, offl, near, iv, 3)
    dec = _decided(r["prob"], 3).numpy()
    assert dec.mean() > 0.9
    np.testing.assert_array_equal(r["est_idx"].numpy()[dec], o["est_idx"][dec])


@pytest.mark.parametrize("D,topk", [(3, 3), (17, 4), (65, 8), (200, 8), (512, 3)])
def test_restatement_ranks_like_the_oracle_where_decided(oracle, D, topk):
    g = torch.Generator().manual_seed(D)
    both = torch.randn((2, 2, D, 5, 7), generator=g)
    both[:, 0] *= 3.0
    near, iv = 0.2, 4.8 / D
    r = restated(both[:, 0], both[:, 1], near, iv, topk)
    o = oracle.depth_prob_topk(both[:, 0], both[:, 1], near, iv, topk)
    dec = _decided(r["prob"], topk).numpy()
    assert dec.mean() > 0.5
    np.testing.assert_array_equal(r["est_idx"].numpy()[dec], o["est_idx"][dec])
    np.testing.assert_allclose(o["prob"], r["prob"].numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(o["avg_depth"], r["avg_depth"].numpy(), rtol=0, atol=TOL)


def test_the_ranking_rule():
    nan, inf = float("nan"), float("inf")
    col = lambda v: torch.tensor(v, dtype=torch.float64).view(1, -1, 1, 1)   # noqa: E731
    flat = lambda t: t.view(-1).tolist()                                     # noqa: E731
    assert flat(rank(col([0.25] * 20), 4)) == [0, 1, 2, 3]                    # torch.topk: [12, 14, 13, 15] on one CPU build
    assert flat(rank(col([0.1, nan, 0.5, 0.2, nan, 0.05]), 3)) == [1, 4, 2]
    assert flat(rank(col([0.1, nan, 0.5, 0.2, nan, 0.05]), 6)) == [1, 4, 2, 3, 0, 5]
    assert flat(rank(col([nan] * 5), 3)) == [0, 1, 2]
    assert flat(rank(col([0.0, inf, nan, inf, -inf]), 5)) == [2, 1, 3, 0, 4]  # NaN above +Inf too
    assert flat(rank(col([0.0, 0.5, 0.0, 0.5, 0.0]), 4)) == [1, 3, 0, 2]
    assert flat(rank(col([0.3]), 1)) == [0]
    # float32 input ranks as float32
    assert flat(rank(col([0.1, 0.7, 0.7, 0.2]).float(), 2)) == [1, 2]


def test_non_finite_logits_poison_the_pixel_and_the_oracle_ranks_alike(oracle):
    """One NaN or +Inf logit, or all -Inf, make the whole float64 softmax of that pixel NaN (torch.softmax, the reference's
    operator); the defined ranking then is planes 0 .. topk-1, densities NaN.  The CPU oracle follows the same rule.  A NaN
    offset logit touches the depths of its plane only."""
    D, topk = 7, 3
    g = torch.Generator().manual_seed(1)
    both = torch.randn((1, 2, D, 2, 4), generator=g)
    both[0, 0, 3, 0, 0] = float("nan")
    both[0, 0, 0, 0, 1] = float("nan")
    both[0, 0, 5, 0, 2] = float("inf")
    both[0, 0, :, 0, 3] = float("-inf")
    both[0, 1, 2, 1, 0] = float("nan")
    both[0, 0, :, 1, 0] = torch.tensor([0.0, 1.0, 5.0, 2.0, 0.5, 0.1, 0.2])     # plane 2 is the pick of pixel (1, 0)
    r = restated(both[:, 0], both[:, 1], 0.2, 0.6, topk)
    o = oracle.depth_prob_topk(both[:, 0], both[:, 1], 0.2, 0.6, topk)
    poisoned = torch.zeros((2, 4), dtype=torch.bool)
    poisoned[0] = True
    assert torch.isnan(r["prob"][0][:, poisoned]).all() and torch.isfinite(r["prob"][0][:, ~poisoned]).all()
    assert np.isnan(o["prob"][0][:, poisoned.numpy()]).all() and np.isfinite(o["prob"][0][:, ~poisoned.numpy()]).all()
    np.testing.assert_array_equal(r["est_idx"].numpy(), o["est_idx"])
    for k in range(topk):
        assert (o["est_idx"][0, k][poisoned.numpy()] == k).all()
    assert np.isnan(o["est_dens"][0][:, poisoned.numpy()]).all() and np.isnan(o["avg_depth"][0][poisoned.numpy()]).all()
    assert np.isfinite(o["est_depth"][0][:, poisoned.numpy()]).all()      # the depth formula at planes 0 .. topk-1
    # the NaN offset: that plane's depth and the expectation, nothing else
    assert o["est_idx"][0, 0, 1, 0] == 2 and np.isnan(o["est_depth"][0, 0, 1, 0]) and np.isnan(o["avg_depth"][0, 1, 0])
    assert np.isfinite(o["est_depth"][0, 1:, 1, 0]).all() and np.isfinite(o["est_dens"][0, :, 1, 0]).all()
    assert torch.isnan(r["est_depth"][0, 0, 1, 0]) and torch.isnan(r["avg_depth"][0, 1, 0])
