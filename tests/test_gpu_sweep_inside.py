"""The plane sweep's lean decode (kFlagInside, option "sweep_inside"): planes whose bilinear taps all lie inside the source
image skip the range tests and clamps of the general decode.  It is a schedule: every comparison here is torch.equal against
the same call under sweep_inside = 0 and against the device-rounding CPU oracle the parity tests use -- a plane flagged
although one of its taps lies outside the image would fetch a texel where the general form weighs a zero, and miss both.
Every case asserts through ops.sweep_inside_count that it reaches the lean form AND the general one.

Projections are written down directly: rotation = identity, translation (tx, ty, 0) gives the pixel position
(x + tx / d, y + ty / d) on the plane of depth d, so the shift shrinks from plane to plane and a footprint walks across the
image border inside one sweep."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, K, D = 3, 2, 8
# The sample position scales by size / (size - 1) (module.py normalises by size - 1, grid_sample by size), so a tile that spans
# the whole width or height of the source image never has all its taps inside: a map serves the tile shape that cuts it 2 x 2.
MAP_OF_TW = {16: (16, 32), 32: (8, 64)}
DEPTH = np.linspace(0.5, 4.0, D).astype(np.float32)


@contextlib.contextmanager
def _options(**kw):
    from mvsdet_amd import _lib
    saved = {k: _lib.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


def _shift(tx, ty):
    P = np.eye(4, dtype=np.float32)
    P[0, 3], P[1, 3] = tx, ty
    return P


def _scene(n=N, k=K, shifts=None):
    """proj (n,k,4,4), depth (n,D), neighbour ids: mild translations, another one per (view, neighbour)"""
    proj = np.zeros((n, k, 4, 4), np.float32)
    for i in range(n):
        for j in range(k):
            tx, ty = shifts[i][j] if shifts else (1.5 + 0.75 * i - 2.5 * j, 0.9 + 0.5 * j - 0.3 * i)
            proj[i, j] = _shift(tx, ty)
    nbr = np.array([[(i + 1 + j) % n for j in range(k)] for i in range(n)], np.int64)
    depth = np.tile(DEPTH, (n, 1))
    return proj, depth, nbr


def _feat(n, C, H, W, seed=3):
    return torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(seed))


def _all_taps_inside(P, d, xa, ya, tw, th, H, W):
    """Independent of the geometry kernel's corner formula: the positions of ALL pixels of the tile in float64 (homography,
    division by Z, normalisation by size - 1, grid_sample's by size) -- does the tile lie inside the map, and do the taps
    floor(i), floor(i) + 1 of every pixel lie inside the source image?"""
    if xa + tw > W or ya + th > H:
        return False
    x, y = np.meshgrid(np.arange(xa, xa + tw, dtype=np.float64), np.arange(ya, ya + th, dtype=np.float64))
    P = np.asarray(P, np.float64)
    X, Y, Z = ((P[r, 0] * x + P[r, 1] * y + P[r, 2]) * float(d) + P[r, 3] for r in range(3))
    with np.errstate(all="ignore"):
        ix = (X / Z) / ((W - 1) * 0.5) * (W * 0.5) - 0.5
        iy = (Y / Z) / ((H - 1) * 0.5) * (H * 0.5) - 0.5
        if not (np.isfinite(ix).all() and np.isfinite(iy).all()):
            return False
        return bool(np.floor(ix).min() >= 0 and np.floor(ix).max() + 1 <= W - 1
                    and np.floor(iy).min() >= 0 and np.floor(iy).max() + 1 <= H - 1)


def _flagged_are_inside(flags, proj, depth, tw, H, W):
    """every (view, tile, plane, neighbour) that carries kFlagInside has all its taps inside, by _all_taps_inside"""
    th, tiles_x = 128 // tw, (W + tw - 1) // tw
    n_flagged = 0
    for n, tile, d in zip(*np.nonzero(flags.numpy() & 0x8888)):
        for j in range(proj.shape[1]):
            if (int(flags[n, tile, d]) >> (4 * j)) & 8:
                n_flagged += 1
                assert _all_taps_inside(proj[n, j], depth[n, d], (tile % tiles_x) * tw, (tile // tiles_x) * th, tw, th, H, W), \
                    (n, tile, d, j)
    return n_flagged


def _both_forms(gpu, oracle, feat, nbr, proj, depth, expect_lean=True, **opts):
    """the sweep under sweep_inside 1 and 0 and the oracle: all the same bits; returns (live, lean, flags) of the table"""
    from mvsdet_amd import ops
    n, C, H, W = feat.shape
    k = nbr.shape[1]
    f, nb, pr, de = feat.to(gpu), torch.tensor(nbr).to(gpu), torch.tensor(proj).to(gpu), torch.tensor(depth).to(gpu)
    with _options(**opts):
        with _options(sweep_inside=1):
            lean_out = ops.plane_sweep_variance(f, nb, pr, de)
            table = ops.plane_sweep_table(pr, de, H, W)
        with _options(sweep_inside=0):
            plain_out = ops.plane_sweep_variance(f, nb, pr, de)
        live, lean = ops.sweep_inside_count(table, n, k, depth.shape[1], H, W)
        flags = ops.sweep_flags(table, n, k, depth.shape[1], H, W).cpu()
    print(f"{opts} C={C} {H}x{W} K={k}: live {live} lean {lean}")
    # NaN payloads are not compared: equal_nan on the values, and the NaNs sit where they sat
    assert torch.equal(torch.isnan(lean_out), torch.isnan(plain_out))
    assert torch.equal(torch.nan_to_num(lean_out, nan=0.0), torch.nan_to_num(plain_out, nan=0.0)), opts
    ref = oracle.plane_sweep_variance(feat, nbr, torch.tensor(proj), torch.tensor(depth), mode=1)
    np.testing.assert_array_equal(lean_out.cpu().numpy(), ref)
    if expect_lean:
        assert 0 < lean < live, (live, lean)   # the case reaches the lean form and the general one
    tw = int(table.view(torch.int32)[1].item()) & 0xff   # the tile width the table was built with (its header)
    flagged = _flagged_are_inside(flags, proj, depth, tw, H, W)
    assert (flagged > 0) == (int((flags & 0x8888).sum()) > 0)
    return live, lean, flags


@pytest.mark.parametrize("tw", [16, 32])
@pytest.mark.parametrize("hw", [(8, 64), (16, 32)])
@pytest.mark.parametrize("C", [32, 40])
def test_lean_form_is_bit_identical(gpu, oracle, tw, hw, C):
    """interior tiles take the lean form, border tiles whose footprints leave the image the general one"""
    proj, depth, nbr = _scene()
    live, lean, _ = _both_forms(gpu, oracle, _feat(N, C, *hw), nbr, proj, depth, expect_lean=hw == MAP_OF_TW[tw], sweep_tw=tw)
    if hw != MAP_OF_TW[tw]:
        assert lean == 0 and live > 0   # every tile spans the map's width or height: all planes take the general form


def _scaled(a, tx, ty):
    P = _shift(tx, ty)
    P[0, 0] = P[1, 1] = a
    return P


@pytest.mark.parametrize("cap", [0, 40])
def test_lean_form_under_small_boxes(gpu, oracle, cap):
    """sweep_boxcap 0: every footprint is gathered, nothing is staged, nothing may be flagged.  40: the footprint of a whole
    16x8 tile (18 x 10 texels) does not fit, so the neighbours here look at the source image shrunk to a quarter -- footprints of
    about 6 x 4 texels, which fit; their shift changes by several texels between the near planes, so the unions of 40 texels
    break into short runs there (refills past the first plane) and into long ones further out.  View 0: both neighbours
    shrunk and inside (lean); view 1: neighbour 1 unshrunk, 180 texels, gathered (general form beside a flagged neighbour);
    view 2: neighbour 0 pushed over the left and top border on its near planes (staged, live, not inside)."""
    _, depth, nbr = _scene()
    proj = np.stack([np.stack([_scaled(0.25, 3.0, 2.0), _scaled(0.25, 2.0, 1.5)]),
                     np.stack([_scaled(0.25, 2.5, 1.0), _shift(1.5, 0.9)]),
                     np.stack([_scaled(0.25, -1.5, -1.0), _scaled(0.25, 1.0, 2.5)])]).astype(np.float32)
    live, lean, flags = _both_forms(gpu, oracle, _feat(N, 32, 16, 32), nbr, proj, depth, expect_lean=False, sweep_tw=16, sweep_boxcap=cap)
    nib = torch.stack([(flags >> (4 * j)) & 0xf for j in range(K)])     # (K, N, tiles, D)
    staged, gathered = ((nib & 3) == 3), ((nib & 3) == 1)
    if cap == 0:
        assert lean == 0 and live > 0 and not staged.any() and gathered.any()
    else:
        assert 0 < lean < live, (live, lean)
        assert staged.any() and gathered.any()              # staged and gathered footprints side by side
        assert ((nib[..., 1:] & 4) != 0).any()              # a refill past the first plane: more than one run per tile
        assert (staged & ((nib & 8) == 0)).any()            # staged, live and not inside


def test_lean_form_fp16_storage(gpu):
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    C = 32
    for tw in (16, 32):
        H, W = MAP_OF_TW[tw]
        packed = ops.pack_features(_feat(N, C, H, W).to(gpu))
        args = (packed, torch.tensor(nbr).to(gpu), torch.tensor(proj).to(gpu), torch.tensor(depth).to(gpu), N, 0, C, H, W)
        with _options(sweep_tw=tw):
            with _options(sweep_inside=1):
                a = ops.plane_sweep_variance_shard(*args, half_out=True)
                full = ops.plane_sweep_variance_shard(*args)
                live, lean = ops.sweep_inside_count(ops.plane_sweep_table(args[2], args[3], H, W), N, K, D, H, W)
            with _options(sweep_inside=0):
                b = ops.plane_sweep_variance_shard(*args, half_out=True)
        assert 0 < lean < live
        assert torch.equal(a, b) and torch.equal(a, full.half())


def test_lean_form_three_neighbours(gpu, oracle):
    """K = 3: the second pass has one neighbour, decoded by both quads"""
    proj, depth, nbr = _scene(n=4, k=3)
    for tw in (16, 32):
        _both_forms(gpu, oracle, _feat(4, 32, *MAP_OF_TW[tw]), nbr, proj, depth, sweep_tw=tw)


def _tile_flags(flags, view, tile, j):
    return (flags[view, tile] >> (4 * j)) & 0xf


@pytest.mark.parametrize("tw,hw", [(32, (8, 64)), (16, (16, 32))])
def test_flag_follows_the_image_border(gpu, oracle, tw, hw):
    """A footprint walked across each image border in steps of 3/8 px (never on a whole texel: positions scale by
    size / (size - 1); test_positions_on_whole_texels has those): a plane is flagged exactly as long as
    floor(min - 1e-3) >= 0 and floor(max + 1e-3) + 1 <= size - 1 hold for the corner positions in the arithmetic of sample_at,
    a flagged plane has all the taps of all its 128 pixels inside by the independent _all_taps_inside, and every step gives
    the oracle's bits."""
    H, W = hw
    feat = _feat(N, 32, H, W)
    d1 = np.ones((N, 1), np.float32)                      # one plane of depth 1: the shift in pixels is the translation
    nbr = np.array([[1, 2], [2, 0], [0, 1]], np.int64)
    th = 128 // tw
    seen = set()
    for axis in (0, 1):
        for edge in ("low", "high"):
            for step in range(-12, 13, 3):
                s = step / 8.0
                # interior shift 1.25 px in the other axis; along `axis` the tile row / column at the border is pushed outwards
                t = [1.25, 1.25]
                t[axis] = (0.5 - s) if edge == "low" else (-0.5 + s)
                proj = np.stack([np.stack([_shift(t[0], t[1]), _shift(1.25, 1.25)])] * N)
                f, nb, pr, de = feat.to(gpu), torch.tensor(nbr).to(gpu), torch.tensor(proj).to(gpu), torch.tensor(d1).to(gpu)
                from mvsdet_amd import ops
                with _options(sweep_tw=tw):
                    with _options(sweep_inside=1):
                        out = ops.plane_sweep_variance(f, nb, pr, de)
                        flags = ops.sweep_flags(ops.plane_sweep_table(pr, de, H, W), N, K, 1, H, W).cpu()
                    with _options(sweep_inside=0):
                        assert torch.equal(ops.plane_sweep_variance(f, nb, pr, de), out)
                np.testing.assert_array_equal(out.cpu().numpy(), oracle.plane_sweep_variance(feat, nbr, torch.tensor(proj), torch.tensor(d1), mode=1))
                # the expectation, per tile, from the corner positions in fp32 (the arithmetic of sample_at)
                tiles_x = W // tw
                for tile in range(tiles_x * (H // th)):
                    xa, ya = (tile % tiles_x) * tw, (tile // tiles_x) * th
                    pos = []
                    for size, lo, tt in ((W, xa, t[0]), (H, ya, t[1])):
                        span = tw if size == W else th
                        c = np.array([lo, lo + span - 1], np.float32) * np.float32(1.0) + np.float32(tt)
                        g = c / np.float32((size - 1) * 0.5) - np.float32(1.0)
                        i = ((g + np.float32(1.0)).astype(np.float64) * (size * 0.5) - 0.5).astype(np.float32)   # fmaf
                        pos.append((np.floor(i.min() - np.float32(1e-3)) >= 0) and (np.floor(i.max() + np.float32(1e-3)) + 1 <= size - 1))
                    want = bool(pos[0] and pos[1])
                    got = bool((_tile_flags(flags, 0, tile, 0) & 8).item())
                    assert got == want, (axis, edge, s, tile, got, want)
                    assert not got or _all_taps_inside(proj[0, 0], 1.0, xa, ya, tw, th, H, W), (axis, edge, s, tile)
                    assert bool(_tile_flags(flags, 0, tile, 0) & 2) or not got   # inside only beside staged
                    seen.add(got)
    assert seen == {True, False}


def _texel_map(size, scale, offset):
    """(a, b) of a projection row a * c + b whose pixel c samples position scale * c + offset EXACTLY: the position of a
    projected p is p * size / (size - 1) - 0.5, so a = scale * (size - 1) / size and b = (offset + 0.5) * (size - 1) / size;
    with size a power of two and dyadic scale / offset every step of sample_at is exact in fp32."""
    return scale * (size - 1) / size, (offset + 0.5) * (size - 1) / size


@pytest.mark.parametrize("tw,hw", [(32, (8, 64)), (16, (16, 32))])
def test_positions_on_whole_texels(gpu, oracle, tw, hw):
    """Neighbour 0 samples position c + m along one axis, m = -2 .. 2 whole texels, and 0.5 * c + 1.25 (interior for every
    tile) along the other: both fractions of that axis are 0 and the taps are c + m, c + m + 1.  By the condition the issue
    sets (floor(min - 1e-3) >= 0, floor(max + 1e-3) + 1 <= size - 1) a tile that starts at `lo` and spans `span` pixels is
    flagged exactly when lo + m - 1 >= 0 and lo + span + m <= size - 1: the largest position size - 2 exactly (largest tap
    size - 1) is flagged, size - 1 exactly (tap `size`, weight 0, outside) is not; the smallest position 1 exactly is flagged,
    0 exactly falls to the margin and is not.  Neighbour 1 is interior everywhere, so the pass is lean exactly where
    neighbour 0 is flagged.  Same bits as the general form and the oracle at every m."""
    H, W = hw
    th = 128 // tw
    feat = _feat(N, 32, H, W)
    d1 = np.ones((N, 1), np.float32)
    nbr = np.array([[1, 2], [2, 0], [0, 1]], np.int64)
    inner = np.eye(4, dtype=np.float32)
    (inner[0, 0], inner[0, 3]), (inner[1, 1], inner[1, 3]) = _texel_map(W, 0.5, 1.25), _texel_map(H, 0.5, 1.25)
    tiles_x = W // tw
    hit = set()
    for axis, size, span in ((0, W, tw), (1, H, th)):
        for m in (-2, -1, 0, 1, 2):
            P = inner.copy()
            P[axis, axis], P[axis, 3] = _texel_map(size, 1.0, float(m))
            proj = np.stack([np.stack([P, inner])] * N)
            live, lean, flags = _both_forms(gpu, oracle, feat, nbr, proj, d1, expect_lean=False, sweep_tw=tw)
            for tile in range(tiles_x * (H // th)):
                lo = ((tile % tiles_x) * tw, (tile // tiles_x) * th)[axis]
                want = lo + m - 1 >= 0 and lo + span + m <= size - 1
                got = bool(_tile_flags(flags, 0, tile, 0)[0] & 8)
                assert got == want, (axis, m, tile, got, want)
                assert bool(_tile_flags(flags, 0, tile, 1)[0] & 8)          # neighbour 1: interior, always flagged
                if lo + span - 1 + m == size - 2:
                    hit.add("max = size - 2, flagged")
                if lo + span - 1 + m == size - 1:
                    hit.add("max = size - 1, not flagged")
                if lo + m == 1:
                    hit.add("min = 1, flagged")
                if lo + m == 0:
                    hit.add("min = 0, not flagged")
            assert lean == N * sum(1 for t in range(tiles_x * (H // th))
                                   if bool(_tile_flags(flags, 0, t, 0)[0] & 8)), (axis, m, live, lean)
    assert len(hit) == 4, hit


def test_partial_tile_column_is_never_flagged(gpu, oracle):
    """W = 40 under 32x4 tiles: the second tile column has 8 of its 32 pixel columns"""
    proj, depth, nbr = _scene()
    _, _, flags = _both_forms(gpu, oracle, _feat(N, 32, 8, 40), nbr, proj, depth, sweep_tw=32)
    tiles_x = 2
    part = flags[:, 1::tiles_x]
    assert int((part & 0x8888).sum()) == 0 and int((part & 0x1111).sum()) > 0
    assert int((flags[:, 0::tiles_x] & 0x8888).sum()) > 0


@pytest.mark.parametrize("tw", [16, 32])
def test_out_of_view_nan_and_sign_change_beside_flagged(gpu, oracle, tw):
    """view 0: neighbour 1 far out of view beside a flagged neighbour 0 (the pass is lean, quad 1 decodes a position nobody
    fetches); view 1: a NaN in neighbour 1's projection; view 2: neighbour 1's Z changes sign inside the first tile.  Neither
    is ever flagged, their planes take the general form, and the NaNs of the output sit where the oracle has them."""
    proj, depth, nbr = _scene()
    proj[0, 1] = _shift(4000.0, 0.0)
    proj[1, 1, 0, 0] = np.nan
    proj[2, 1, 2, 0], proj[2, 1, 2, 2] = 1.0, -5.5      # Z = (x - 5.5) * d
    live, lean, flags = _both_forms(gpu, oracle, _feat(N, 32, *MAP_OF_TW[tw]), nbr, proj, depth, sweep_tw=tw)
    assert int((flags[0] & 0x10).sum()) == 0 and int((flags[0] & 0x08).sum()) > 0     # out of view beside flagged
    assert int((flags[1] & 0x80).sum()) == 0 and int((flags[1] & 0x10).sum()) > 0     # NaN: live (taps run), never inside
    first_col = flags[2, 0::2]   # two tile columns
    assert int((first_col & 0x80).sum()) == 0


@pytest.mark.parametrize("tw", [16, 32])
def test_tables_mix_across_the_option(gpu, tw):
    """a table built under one value of sweep_inside and consumed under the other: the same bits"""
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    (H, W), C = MAP_OF_TW[tw], 32
    packed = ops.pack_features(_feat(N, C, H, W).to(gpu))
    nb, pr, de = torch.tensor(nbr).to(gpu), torch.tensor(proj).to(gpu), torch.tensor(depth).to(gpu)
    with _options(sweep_tw=tw):   # the tile shape that cuts this map 2 x 2, for the table and for its consumer
        with _options(sweep_inside=0):
            ref = ops.plane_sweep_variance_packed(packed, nb, pr, de, C, H, W)
        for build, consume in ((0, 1), (1, 0), (1, 1)):
            with _options(sweep_inside=build):
                table = ops.plane_sweep_table(pr, de, H, W)
            with _options(sweep_inside=consume):
                assert torch.equal(ops.plane_sweep_variance_tabled(packed, nb, table, C, D, H, W), ref), (build, consume)
            live, lean = ops.sweep_inside_count(table, N, K, D, H, W)
            assert 0 < lean < live, (live, lean)
