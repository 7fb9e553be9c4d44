"""The pooled run policy of the sweep geometry (csrc/sweep_kernel.h, ops.plane_sweep_table_pooled): with two neighbours and 32x4
tiles a footprint box may take the other neighbour's idle LDS slot.  Hand-made projections (scale, shift, a small roll) and
hand-made plane depths (not monotonic: a neighbour leaves the view and comes back) control the footprints; every fixture asserts
on the table it received that it holds the case it is meant to cover.  Every output is compared bit for bit with the pooled entry
point under "sweep_pool" 0, with the sweep on an unpooled table, and with the oracle (mode 1).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CAP, PAD = 312, 8                    # texels of one slot of the 32x4 tiles (80 KiB of LDS, two neighbours), slack per slot
POOL = 2 * (CAP + PAD) - PAD
MAGIC, MAGIC_POOLED = 0x4d565347, 0x4d565350
LIVE, STAGED, REFILL, INSIDE = 1, 2, 4, 8


def _eye(N, K):
    return np.tile(np.eye(4, dtype=np.float32), (N, K, 1, 1))


def _ring(N, K):
    return np.array([[(n + 1 + j) % N for j in range(K)] for n in range(N)], dtype=np.int64)


# With P = identity the sample position of pixel (x, y) on the plane of depth d is (x + P[0,3] / d, y + P[1,3] / d): a shift
# that grows on the near planes; P[:2,:2] scales / rolls the footprint.  NEAR planes sit between two groups of FAR planes, so a
# neighbour whose shift throws it out of view on the near planes is staged before and after them with the same box.
_DEPTH12 = np.array([3.0, 3.3, 0.25, 0.3, 0.36, 0.45, 0.6, 3.6, 4.0, 0.5, 0.8, 4.4], np.float32)


def _fixture(name):
    """-> N, K, C, D, H, W, proj (N,K,4,4), depth (N,D), nbr (N,K)"""
    if name in ("wide_8x64", "wide_12x64", "wide_c40", "wide_12x80"):
        H, W = {"wide_8x64": (8, 64), "wide_12x64": (12, 64), "wide_c40": (12, 64), "wide_12x80": (12, 80)}[name]
        C = {"wide_8x64": 32, "wide_12x64": 64, "wide_c40": 40, "wide_12x80": 32}[name]
        N, K = 4, 2
        proj = _eye(N, K)
        # view 0: neighbour 0 slides fast over the near planes, neighbour 1 is in view on the far planes only
        proj[0, 0, 0, 3], proj[0, 0, 1, 3] = 6.0, 0.75
        proj[0, 1, 0, 3] = 1.1 * W
        # view 1: the mirror
        proj[1, 1, 0, 3], proj[1, 1, 1, 3] = 6.0, 0.75
        proj[1, 0, 0, 3] = 1.1 * W
        # view 2: one footprint of 313 .. 632 texels (scale 1.45, a small roll) beside a neighbour that is never in view;
        # view 3: the same beside a footprint of more than 632 texels (scale 3.2)
        c, s = np.cos(0.03), np.sin(0.03)
        proj[2, 0, :2, :2] = np.array([[c, -s], [s, c]], np.float32) * 1.45
        proj[2, 1, 0, 3] = 1e5
        proj[3, 0, :2, :2] = np.array([[c, -s], [s, c]], np.float32) * 1.45
        proj[3, 0, 0, 3] = 1.5
        proj[3, 1, :2, :2] *= 3.2
        depth = np.tile(_DEPTH12[None], (N, 1))
        depth[3] = np.sort(_DEPTH12)
        return N, K, C, 12, H, W, proj, depth, _ring(N, K)
    if name == "sizes":
        # With P[:, 3] = 0 the position of pixel (x, y) is (sx * x + ox, sy * y + oy) on every plane: one box per (view, tile),
        # loaded once, its size set by the scale and by where the image border clips it.  The five views give boxes of 88, 136,
        # 544 (multiples of 8), 105, 441 (one above), 119, 295, 399 (one below) and of 632 texels = 79 x 8, the whole pool.
        # Neighbour 1 is never in view, so every box up to the pool is staged.
        params = ((2.28, 2.09, -4.2, 1.4), (1.82, 2.12, 1.2, -3.0), (2.37, 1.6, -12.2, -0.5), (1.73, 2.06, 4.3, -0.9),
                  (2.43, 1.6, 2.3, 2.2))
        N, K, C, D, H, W = len(params), 2, 32, 8, 12, 80
        proj = _eye(N, K)
        depth = np.tile(np.linspace(1.0, 2.5, D, dtype=np.float32)[None], (N, 1))
        for n, (sx, sy, ox, oy) in enumerate(params):
            proj[n, 0, 0, 0], proj[n, 0, 1, 1], proj[n, 0, 0, 2], proj[n, 0, 1, 2] = sx, sy, ox, oy
            proj[n, 1, 0, 2] = 1e5
        return N, K, C, D, H, W, proj, depth, _ring(N, K)
    raise KeyError(name)


def _k_fixture(K):
    N, C, D, H, W = 4, 32, 8, 8, 64
    proj = _eye(N, K)
    rng = np.random.default_rng(K)
    proj[:, :, 0, 3] = rng.uniform(-8, 8, (N, K))
    proj[:, :, 1, 3] = rng.uniform(-1, 1, (N, K))
    proj[:, :, 0, 0] = rng.uniform(0.9, 1.6, (N, K))
    depth = np.tile(np.linspace(0.3, 3.0, D, dtype=np.float32)[None], (N, 1))
    return N, K, C, D, H, W, proj, depth, _ring(N, K)


def _parts(table, N, K, D, H, W):
    """header, boxes (N*tiles, D, K, 4), flags (N*tiles, D) of a geometry table of 32x4 tiles"""
    words = table.view(torch.int32).cpu().numpy().astype(np.int64)
    tiles = ((W + 31) // 32) * ((H + 3) // 4)
    nb = N * tiles * D * K * 4
    return words[:4], words[4:4 + nb].reshape(N * tiles, D, K, 4), words[4 + nb:4 + nb + N * tiles * D].reshape(N * tiles, D) & 0xffff


def _ntex(b):
    return np.maximum(b[..., 1] - b[..., 0] + 1, 0) * np.maximum(b[..., 3] - b[..., 2] + 1, 0)


def check_invariant(boxes, flags, cap=CAP):
    """For every block, every first plane d_begin and every plane from there on: follow what the slab kernel holds resident
    (a staged plane loads its box if it carries kFlagRefill or nothing was loaded yet; a box of more than `cap` texels goes to
    the pool's base, any other to its neighbour's slot; a load writes [base, base + texels + 8) and so destroys whatever of the
    other neighbour it overlaps) and assert that every staged plane READS an intact resident box that is its own box, inside the
    pool.  Hence no two boxes that are both read overlap, load_box's extra piece included."""
    B, D, K, _ = boxes.shape
    slot = cap + PAD
    for b in range(B):
        for d0 in range(D):
            res = [None] * K          # (box, lo, hi, intact)
            for d in range(d0, D):
                for j in range(K):
                    nib = (flags[b, d] >> (4 * j)) & 0xf
                    if not nib & STAGED:
                        continue
                    assert nib & LIVE
                    box = tuple(boxes[b, d, j])
                    if (nib & REFILL) or res[j] is None:
                        n = int(_ntex(boxes[b, d, j]))
                        assert 0 < n <= (POOL if K == 2 else cap)
                        lo = 0 if n > cap else j * slot
                        hi = lo + n + PAD
                        assert hi <= K * slot, "a box leaves the pool"
                        for o in range(K):
                            if o != j and res[o] is not None and res[o][1] < hi and lo < res[o][2]:
                                res[o] = res[o][:3] + (False,)
                        res[j] = (box, lo, hi, True)
                    assert res[j][3], f"block {b}, first plane {d0}: plane {d} reads neighbour {j}'s box after it was overwritten"
                    assert res[j][0] == box, f"block {b}, first plane {d0}: plane {d} of neighbour {j} expects another box than the resident one"


def _nib(flags, j):
    return (flags >> (4 * j)) & 0xf


def has_wide_then_forced_refill(bp, fp, bu, fu, j):
    """a block where neighbour j runs a wide box while neighbour 1-j has no footprint, after which 1-j is staged again with a
    refill that the unpooled table does not carry for the same box"""
    o = 1 - j
    for b in range(bp.shape[0]):
        wide = ((_nib(fp[b], j) & STAGED) != 0) & (_ntex(bp[b, :, j]) > CAP)
        if not wide.any():
            continue
        assert (_ntex(bp[b, wide][:, o]) == 0).all()
        first = int(np.nonzero(wide)[0][0])
        for d in range(first + 1, bp.shape[1]):
            if _nib(fp[b, d], o) & STAGED:
                if (_nib(fp[b, d], o) & REFILL) and not (_nib(fu[b, d], o) & REFILL) and (bp[b, d, o] == bu[b, d, o]).all():
                    return True
                break
    return False


def _tables(gpu, fx):
    from mvsdet_amd import ops
    N, K, C, D, H, W, proj, depth, nbr = fx
    pr, dp = torch.from_numpy(proj).to(gpu), torch.from_numpy(depth).to(gpu)
    pitch = ops.sweep_row_pitch(W)
    if pitch != W:
        tu = ops.plane_sweep_table_pitched(pr, dp, H, W, pitch)
        tp = ops.plane_sweep_table_pooled(pr, dp, H, W, pitch)
    else:
        tu = ops.plane_sweep_table(pr, dp, H, W)
        tp = ops.plane_sweep_table_pooled(pr, dp, H, W)
    return tu, tp, pitch


def _sweep(packed, nbr, table, C, D, H, W, pitch):
    from mvsdet_amd import ops
    if pitch != W:
        return ops.plane_sweep_variance_tabled_pitched(packed, nbr, table, C, D, H, W, pitch)
    return ops.plane_sweep_variance_tabled(packed, nbr, table, C, D, H, W)


_CACHE = {}


def _case(gpu, oracle, name):
    """tables, packed features, the unpooled result and the oracle's, computed once per fixture"""
    if name not in _CACHE:
        from mvsdet_amd import ops
        fx = _fixture(name) if not name.startswith("k") else _k_fixture(int(name[1:]))
        N, K, C, D, H, W, proj, depth, nbr = fx
        feat = torch.from_numpy(np.random.default_rng(7).standard_normal((N, C, H, W)).astype(np.float32))
        tu, tp, pitch = _tables(gpu, fx)
        packed = ops.pack_features(feat.to(gpu))
        nb = torch.from_numpy(nbr).to(gpu)
        ref = oracle.plane_sweep_variance(feat, nbr, torch.from_numpy(proj), torch.from_numpy(depth), mode=1)
        base = _sweep(packed, nb, tu, C, D, H, W, pitch)
        assert np.array_equal(base.cpu().numpy(), ref)
        _CACHE[name] = dict(fx=fx, tu=tu, tp=tp, pitch=pitch, packed=packed, nb=nb, ref=ref, feat=feat,
                            pu=_parts(tu, N, K, D, H, W), pp=_parts(tp, N, K, D, H, W))
    return _CACHE[name]


def _assert_same(c, table):
    N, K, C, D, H, W = c["fx"][:6]
    got = _sweep(c["packed"], c["nb"], table, C, D, H, W, c["pitch"]).cpu().numpy()
    assert np.array_equal(got, c["ref"], equal_nan=True)


@pytest.mark.parametrize("name", ["wide_8x64", "wide_12x64", "wide_12x80"])
def test_wide_runs_and_their_evictions(gpu, oracle, name):
    """Cases 1, 2, 3 and 8: neighbour 0 wide while neighbour 1 is out of view and the forced refill of neighbour 1 afterwards; the
    mirror; a footprint of 313..632 texels that the slot policy gathers and the pool stages, one of more than 632 texels that
    stays gathered; the invariant on every plane.  Results equal the unpooled sweep's and the oracle's bit for bit."""
    c = _case(gpu, oracle, name)
    N, K, C, D, H, W = c["fx"][:6]
    (hu, bu, fu), (hp, bp, fp) = c["pu"], c["pp"]
    assert hu[0] == MAGIC and hp[0] == MAGIC_POOLED and (hu[1:] == hp[1:]).all() and (hp[1] >> 8) == CAP and (hp[1] & 0xff) == 32
    assert has_wide_then_forced_refill(bp, fp, bu, fu, 0), "no wide run of neighbour 0 followed by a forced refill of neighbour 1"
    assert has_wide_then_forced_refill(bp, fp, bu, fu, 1), "no wide run of neighbour 1 followed by a forced refill of neighbour 0"
    own = _ntex(bu)                                         # gathered footprints keep their own box in the unpooled table
    gathered_u = ((fu[..., None] >> (4 * np.arange(K))) & 3) == LIVE
    staged_p = ((fp[..., None] >> (4 * np.arange(K))) & STAGED) != 0
    assert (gathered_u & staged_p & (own > CAP) & (own <= POOL)).any(), "no footprint of 313..632 texels newly staged"
    gathered_p = ((fp[..., None] >> (4 * np.arange(K))) & 3) == LIVE
    if H * W > POOL:   # an 8 x 64 map has no room for such a footprint
        assert (gathered_p & (_ntex(bp) > POOL)).any(), "no footprint of more than 632 texels left gathered"
    # never fewer staged footprints, kFlagInside only on staged planes, live bits unchanged
    staged_u = ((fu[..., None] >> (4 * np.arange(K))) & STAGED) != 0
    assert (staged_p | ~staged_u).all()
    assert (((fp[..., None] >> (4 * np.arange(K))) & INSIDE != 0) <= staged_p).all()
    assert ((fp & 0x11) == (fu & 0x11)).all()
    check_invariant(bp, fp)
    check_invariant(bu, fu)
    _assert_same(c, c["tp"])


def test_box_sizes_around_multiples_of_eight(gpu, oracle):
    """Case 4: wide and narrow boxes just below, at and just above a multiple of 8 texels (the DMA piece that may reach past the
    box), and the largest box the fixture's map admits inside the pool."""
    c = _case(gpu, oracle, "sizes")
    hp, bp, fp = c["pp"]
    loaded = ((fp & STAGED) != 0) & ((fp & REFILL) != 0)
    n = _ntex(bp[:, :, 0])[loaded]
    for part in (n[n <= CAP], n[n > CAP]):           # boxes in their own slot, boxes at the pool's base
        assert {7, 0, 1} <= set((part % 8).tolist()), sorted(set(part.tolist()))
    assert n.max() == POOL, n.max()                  # the largest admissible box: 79 x 8 texels
    check_invariant(bp, fp)
    _assert_same(c, c["tp"])


@pytest.mark.parametrize("dsplit", [2, 3])
def test_blocks_that_start_inside_a_wide_run(gpu, oracle, dsplit):
    """Case 5: "sweep_dsplit" 2 and 3 cut the 12 planes at 6 and at 4, 8: blocks start inside a wide run and inside the evicted
    neighbour's gap (asserted on the flags)."""
    from mvsdet_amd import _lib
    c = _case(gpu, oracle, "wide_12x64")
    hp, bp, fp = c["pp"]
    D = c["fx"][3]
    per = (D + dsplit - 1) // dsplit
    starts = list(range(per, D, per))
    wide = ((((fp[..., None] >> (4 * np.arange(2))) & STAGED) != 0) & (_ntex(bp) > CAP))          # (B, D, K)
    hit = False
    for s in starts:
        for j in (0, 1):
            hit |= bool((wide[:, s, j] & wide[:, s - 1, j] & (bp[:, s, j] == bp[:, s - 1, j]).all(-1)).any())
    assert hit, "no block starts inside a wide run"
    saved = _lib.get_option("sweep_dsplit")
    try:
        _lib.set_option("sweep_dsplit", dsplit)
        _assert_same(c, c["tp"])
        _assert_same(c, c["tu"])
    finally:
        _lib.set_option("sweep_dsplit", saved)


@pytest.mark.parametrize("inside", [0, 1])
def test_general_store_form_and_lean_decode(gpu, oracle, inside):
    """Case 6: C = 40 (the non-FAST form of the slab kernel) under "sweep_inside" 0 and 1; the 12x80 pitched route under both."""
    from mvsdet_amd import _lib
    saved = _lib.get_option("sweep_inside")
    try:
        _lib.set_option("sweep_inside", inside)
        for name in ("wide_c40", "wide_12x80"):
            c = _case(gpu, oracle, name)
            assert (_ntex(c["pp"][1]) > CAP).any()
            _assert_same(c, c["tp"])
    finally:
        _lib.set_option("sweep_inside", saved)


@pytest.mark.parametrize("name", ["wide_8x64", "wide_12x64"])
def test_fp16_storage(gpu, oracle, name):
    """Case 6: the fp16-output instantiation on a pooled table: the oracle's fp32 values rounded to nearest-even, and what the
    unpooled table and the fused fp16 call give."""
    from mvsdet_amd import ops
    c = _case(gpu, oracle, name)
    N, K, C, D, H, W, proj, depth, nbr = c["fx"]
    got = ops.plane_sweep_variance_tabled_f16(c["packed"], c["nb"], c["tp"], C, D, H, W)
    base = ops.plane_sweep_variance_tabled_f16(c["packed"], c["nb"], c["tu"], C, D, H, W)
    fused = ops.plane_sweep_variance_shard(c["packed"], c["nb"], torch.from_numpy(proj).to(gpu), torch.from_numpy(depth).to(gpu),
                                           N, 0, C, H, W, half_out=True)
    assert got.dtype == torch.float16
    assert torch.equal(got.view(torch.int16), base.view(torch.int16)) and torch.equal(got.view(torch.int16), fused.view(torch.int16))
    with np.errstate(over="ignore"):
        want = c["ref"].astype(np.float16)
    assert np.array_equal(got.cpu().numpy().view(np.int16), want.view(np.int16))


@pytest.mark.parametrize("K", [1, 3])
def test_other_neighbour_counts_keep_their_slots(gpu, oracle, K):
    """Case 7: K = 1 and K = 3 give the unpooled table under the pooled mark, and equal results."""
    c = _case(gpu, oracle, f"k{K}")
    (hu, bu, fu), (hp, bp, fp) = c["pu"], c["pp"]
    assert hu[0] == MAGIC and hp[0] == MAGIC_POOLED and (hu[1:] == hp[1:]).all()
    assert (bu == bp).all() and (fu == fp).all()
    check_invariant(bp, fp, cap=int(hp[1] >> 8))
    _assert_same(c, c["tp"])


def test_backward_refuses_a_pooled_table(gpu, oracle):
    """Case 9: the backward kernel does not know the pooled form: all-NaN gradient, as for any mismatched geometry; the
    unpooled table of the same cameras still gives the gradient."""
    from mvsdet_amd import ops
    c = _case(gpu, oracle, "wide_8x64")
    N, K, C, D, H, W = c["fx"][:6]
    R = torch.randn((N, C, D, H, W), device=gpu, generator=torch.Generator(device=gpu).manual_seed(2))
    bad = ops.plane_sweep_variance_backward_packed(c["packed"], c["nb"], c["tp"], R)
    good = ops.plane_sweep_variance_backward_packed(c["packed"], c["nb"], c["tu"], R)
    torch.cuda.synchronize()
    assert torch.isnan(bad).all()
    ref = oracle.plane_sweep_variance_bwd(c["feat"], c["fx"][8], torch.from_numpy(c["fx"][6]), torch.from_numpy(c["fx"][7]), R.cpu())
    np.testing.assert_allclose(good.cpu().numpy(), ref, rtol=1e-4, atol=2e-5 * max(float(np.abs(ref).max()), 1.0))


def test_option_off_gives_the_unpooled_table(gpu, oracle):
    """Case 10: under "sweep_pool" 0 the pooled entry point writes what plane_sweep_table[_pitched] writes, mark included."""
    from mvsdet_amd import _lib
    saved = _lib.get_option("sweep_pool")
    try:
        _lib.set_option("sweep_pool", 0)
        for name in ("wide_12x64", "wide_12x80"):
            c = _case(gpu, oracle, name)
            _, tz, _ = _tables(gpu, c["fx"])
            N, K, C, D, H, W = c["fx"][:6]
            for a, b in zip(_parts(tz, N, K, D, H, W), c["pu"]):
                assert (a == b).all()
            _assert_same(c, tz)
    finally:
        _lib.set_option("sweep_pool", saved)
    assert _lib.get_option("sweep_pool") == saved
