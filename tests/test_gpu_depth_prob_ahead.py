"""depth_prob_topk under option "depthprob_ahead": 1 (the default) requests a pixel's inputs before its first store, 0 keeps the
plane-by-plane order.  The arithmetic of a pixel is the same, so all outputs of the call (prob, off, est_depth, est_dens, est_idx,
avg_depth) must carry the same bits under both, NaN included; at the pixels with finite inputs they must also agree with the
CPU oracle's stage 2 by the criterion of tests/test_gpu_parity.py::test_depth_prob_topk.

Shapes: every form of the kernel at its edges (D = 1, topk = D, 16 | 17, 64 | 65 planes, a 96-plane volume with the longer
candidate list), H*W no multiple of the block, 9 x 33 = 297 pixels = two blocks, the second with 41 live threads.  Each shape runs
on dense inputs and on the two channel slices of one (N, 2, D, H, W) tensor (view stride 2*D*H*W).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_parity.py: north_star tolerance, fp32
NEAR, FAR = 0.2, 5.0
NAMES = ("prob", "off", "est_depth", "est_dens", "est_idx", "avg_depth")

SHAPES = [
    (2, 1, 5, 7, 1),      # single plane
    (2, 3, 5, 7, 3),      # topk = D
    (2, 16, 9, 33, 3),    # edge of the 16-register form
    (2, 17, 9, 33, 3),    # first D of the 64-register form
    (2, 64, 9, 33, 3),    # the headline's form
    (2, 65, 9, 33, 3),    # first D of the streaming form
    (2, 96, 4, 80, 5),    # streaming, more chunks than one, the longer candidate list
]
CASES = [(s, lay) for s in SHAPES for lay in ("dense", "sliced")]
IDS = ["N%d_D%d_%dx%d_k%d-%s" % (*s, lay) for s, lay in CASES]


def _planted(N, D, H, W):
    """(view, pixel, kind) of the planted pixels: the first pixels of view 0, the last pixels of view 1 (the last block's tail)"""
    kinds = ("equal", "nan", "pinf", "ninf", "off_hi", "off_lo")
    HW = H * W
    return [(0, 2 * i + 1, k) for i, k in enumerate(kinds)] + [(N - 1, HW - 1 - i, k) for i, k in enumerate(kinds)]


def _inputs(shape):
    N, D, H, W, topk = shape
    g = torch.Generator().manual_seed(1000 * D + H * W + topk)
    both = torch.randn((N, 2, D, H, W), generator=g)
    both[:, 0] *= 3
    flat = both.view(N, 2, D, H * W)
    finite = torch.ones((N, H * W), dtype=torch.bool)
    for n, p, kind in _planted(N, D, H, W):
        if kind == "equal":
            flat[n, 0, :, p] = 0.5
        elif kind == "nan":
            flat[n, 0, D // 2, p] = float("nan")
        elif kind == "pinf":
            flat[n, 0, D // 3, p] = float("inf")
        elif kind == "ninf":
            flat[n, 0, :, p] = float("-inf")
        elif kind == "off_hi":
            flat[n, 1, :, p] = 100.0
        else:
            flat[n, 1, :, p] = -100.0
            flat[n, 1, ::2, p] = 100.0
        if kind in ("nan", "pinf", "ninf"):
            finite[n, p] = False
    return both, finite.view(N, H, W).numpy()


@functools.lru_cache(maxsize=None)
def _results(shape, layout):
    """the call under depthprob_ahead = 0 and = 1 and the oracle, once per case"""
    from mvsdet_amd import _lib, ops
    from oracle import oracle as O
    N, D, H, W, topk = shape
    both, finite = _inputs(shape)
    dev = torch.device("cuda:0")
    iv = (FAR - NEAR) / D
    on_dev = both.to(dev)
    if layout == "dense":
        cost, offl = on_dev[:, 0].contiguous(), on_dev[:, 1].contiguous()
    else:
        cost, offl = on_dev[:, 0], on_dev[:, 1]
        assert cost.stride(0) == 2 * D * H * W
    saved = _lib.get_option("depthprob_ahead")
    got = {}
    try:
        for ahead in (0, 1):
            _lib.set_option("depthprob_ahead", ahead)
            got[ahead] = [t.cpu().numpy() for t in ops.depth_prob_topk(cost, offl, NEAR, iv, topk)]
    finally:
        _lib.set_option("depthprob_ahead", saved)
    O.build()
    ref = O.depth_prob_topk(both[:, 0].contiguous(), both[:, 1].contiguous(), NEAR, iv, topk)
    return got, ref, finite


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("shape,layout", CASES, ids=IDS)
def test_same_bits_as_the_plane_by_plane_order(gpu, shape, layout):
    got, _, _ = _results(shape, layout)
    for name, a, b in zip(NAMES, got[0], got[1]):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=name)   # the bits: NaN positions and payloads included


@pytest.mark.parametrize("shape,layout", CASES, ids=IDS)
def test_planted_pixels(gpu, shape, layout):
    N, D, H, W, topk = shape
    got, _, _ = _results(shape, layout)
    prob, off, est_depth, est_dens, est_idx, avg = [a.reshape(a.shape[0], -1, H * W) for a in got[1][:5]] + [got[1][5].reshape(N, H * W)]
    for n, p, kind in _planted(N, D, H, W):
        if kind == "equal":       # exact ties: the lowest planes, in order
            assert est_idx[n, :, p].tolist() == list(range(topk)), (n, p)
            np.testing.assert_array_equal(prob[n, :, p], np.full(D, prob[n, 0, p]))
        elif kind in ("nan", "pinf", "ninf"):   # the normaliser is NaN: every probability is, planes 0 .. topk-1 are taken
            assert np.isnan(prob[n, :, p]).all() and np.isnan(est_dens[n, :, p]).all() and np.isnan(avg[n, p]), (n, p, kind)
            assert est_idx[n, :, p].tolist() == list(range(topk)), (n, p, kind)
            iv = np.float32((FAR - NEAR) / D)
            want = (np.arange(topk, dtype=np.float32) * iv + np.float32(NEAR)) + off[n, :topk, p] * iv
            np.testing.assert_array_equal(est_depth[n, :, p], want)
        elif kind == "off_hi":
            np.testing.assert_array_equal(off[n, :, p], np.ones(D, np.float32))
        else:
            np.testing.assert_array_equal(off[n, ::2, p], np.ones((D + 1) // 2, np.float32))
            assert (off[n, 1::2, p] < 1e-30).all() and (off[n, 1::2, p] >= 0).all()


@pytest.mark.parametrize("shape,layout", CASES, ids=IDS)
def test_against_the_oracle_where_the_inputs_are_finite(gpu, shape, layout):
    N, D, H, W, topk = shape
    got, r, finite = _results(shape, layout)
    prob, off, est_depth, est_dens, est_idx, avg = got[1]
    vol = np.broadcast_to(finite[:, None], prob.shape)
    cand = np.broadcast_to(finite[:, None], est_idx.shape)
    np.testing.assert_array_equal(est_idx[cand], r["est_idx"][cand])  # plane indices bit-exact
    np.testing.assert_allclose(prob[vol], r["prob"][vol], rtol=0, atol=1e-6)
    np.testing.assert_allclose(off[vol], r["off"][vol], rtol=0, atol=1e-6)
    np.testing.assert_allclose(est_dens[cand], r["est_dens"][cand], rtol=0, atol=1e-6)
    np.testing.assert_allclose(est_depth[cand], r["est_depth"][cand], rtol=0, atol=TOL)
    np.testing.assert_allclose(avg[finite], r["avg_depth"][finite], rtol=0, atol=TOL)


def test_option_is_a_library_option(gpu):
    from mvsdet_amd import _lib
    saved = _lib.get_option("depthprob_ahead")
    try:
        _lib.set_option("depthprob_ahead", 0)
        assert _lib.get_option("depthprob_ahead") == 0
    finally:
        _lib.set_option("depthprob_ahead", saved)
    assert saved == 1   # the default
