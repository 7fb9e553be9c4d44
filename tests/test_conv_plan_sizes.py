"""The size queries of the bf16x3 convolutions return what tests/golden/conv_plan_sizes.json recorded (default options, no GPU).

The fixture was written (tests/golden/make_goldens_conv_plan.py) before the launchers' host code moved into csrc/conv_host.h; the
queries are the only CPU-visible trace of the tile choice and the split count, which a launcher and its query now take from one
function."""
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_sizes.json")


@pytest.fixture(scope="module")
def lib():
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _padded(fn, N, C, D, H, W):
    e = [ctypes.c_int(0) for _ in range(3)]
    nbytes = fn(N, C, D, H, W, *[ctypes.byref(v) for v in e])
    return [nbytes] + [v.value for v in e]


def test_queries_return_the_recorded_sizes(lib, golden):
    for r in golden["shapes"]:
        D, H, W = r["dhw"]
        for N, C, *want in r["scl"]:
            assert _padded(lib.mvsdet_scl_bytes, N, C, D, H, W) == want, ("scl", N, C, D, H, W)
        for N, C, *want in r["pscl"]:
            assert _padded(lib.mvsdet_pscl_bytes, N, C, D, H, W) == want, ("pscl", N, C, D, H, W)
        for N, Ci, Co, want in r["workspace"]:
            assert lib.mvsdet_conv3d_k3_bf16x3_workspace_bytes(N, Ci, Co, D, H, W) == want, ("workspace", N, Ci, Co, D, H, W)
        for N, f32, want in r["stats_parts"]:
            assert lib.mvsdet_conv3d_k3_bf16x3_stats_parts(N, D, H, W, f32) == want, ("stats_parts", N, D, H, W, f32)
        for N, Ci, Co, want in r["s2_workspace"]:
            assert lib.mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes(N, Ci, Co, D, H, W) == want, ("s2_workspace", N, Ci, Co, D, H, W)
        for N, want in r["convT_stats_parts"]:
            assert lib.mvsdet_convT3d_k3_s2_bf16x3_stats_parts(N, D, H, W) == want, ("convT_stats_parts", N, D, H, W)


def test_fixture_covers_the_layers_and_the_tie(golden):
    """The cost network's layers, the neck's levels and the edge suite's shapes are in the fixture; so are shapes that the two tiles
    of the transposed layer pad alike (the 4 x 8 x 16 tile wins: no statistics form, 0 parts) and their neighbours one voxel on."""
    by_shape = {tuple(r["dhw"]): r for r in golden["shapes"]}
    for s in [(12, 60, 80), (6, 30, 40), (3, 15, 20), (64, 60, 80), (32, 30, 40), (16, 15, 20), (16, 40, 40), (8, 20, 20), (4, 10, 10),
              (4, 12, 16), (5, 13, 17), (7, 17, 9), (8, 8, 8), (2, 15, 17), (8, 16, 32), (9, 17, 33), (7, 23, 15), (3, 5, 9)]:
        assert s in by_shape, s
    assert len(golden["ties"]) >= 4 and len(golden["past_tie_3x16x8"]) >= 4 and len(golden["past_tie_4x8x16"]) >= 4

    def pads(D, H, W):   # voxels of the 4 x 8 x 16 and of the 3 x 16 x 8 tiling
        up = lambda v, m: (v + m - 1) // m * m
        return up(D, 4) * up(H, 8) * up(W, 16), up(D, 3) * up(H, 16) * up(W, 8)

    for s in golden["ties"]:
        p416, p38 = pads(*s)
        assert p416 == p38, s
        assert all(parts == 0 for _, parts in by_shape[tuple(s)]["convT_stats_parts"]), s
    for s in golden["past_tie_3x16x8"]:
        p416, p38 = pads(*s)
        D, H, W = s
        assert p38 < p416, s
        assert by_shape[tuple(s)]["convT_stats_parts"] == [[N, N * -(-W // 8) * -(-H // 16) * -(-D // 3)] for N in (1, 3)], s
    for s in golden["past_tie_4x8x16"]:
        p416, p38 = pads(*s)
        assert p38 > p416, s
        assert all(parts == 0 for _, parts in by_shape[tuple(s)]["convT_stats_parts"]), s
    # a neighbour differs from a tie by one voxel in one dimension
    for s in golden["past_tie_3x16x8"] + golden["past_tie_4x8x16"]:
        assert any(sum(abs(a - b) for a, b in zip(s, t)) == 1 for t in golden["ties"]), s
