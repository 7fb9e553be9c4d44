"""The blocking of the per-pixel form of the sweep (csrc/pixel_form.h: pixel_blocking), seen through the host-only query
mvsdet_pixel_form_blocking and option "pixel_dsplit".  No GPU: nothing here launches.

  1. the query against a Python restatement of the rule and against the figures written out in tests/pixel_blocking_cases.py --
     every shape the two GPU test files of the form run (one hypothesis per block each: the gap), the fixture scenes G22 / G23, the
     workload, and the shapes of tests/test_gpu_pixel_blocking.py;
  2. the restatement and the query agree over a sweep of small shapes, under "pixel_dsplit" and "sweep_xcd" too;
  3. "pixel_dsplit": round trip, its meaning, the forward's cap of 4;
  4. refusals: bad shapes and group widths come back as errors with a message."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import pixel_blocking_cases as PB


@pytest.fixture(scope="module")
def lib():
    import os
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.load()
    return _lib


@pytest.fixture
def options(lib):
    saved = {k: lib.get_option(k) for k in ("pixel_dsplit", "sweep_xcd", "sweep_dsplit")}
    try:
        yield lib
    finally:
        for k, v in saved.items():
            lib.set_option(k, v)


def _query(lib, shape, G):
    N, K, C, D, H, W = shape
    f, b = lib.pixel_form_blocking(N, C, G, D, H, W, False), lib.pixel_form_blocking(N, C, G, D, H, W, True)
    return f, b


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("row", PB.TABLE, ids=[f"{r[0]}-G{r[2]}" for r in PB.TABLE])
def test_table_of_shapes(options, row):
    lib = options
    name, shape, G, (units, parts, fwd, bwd) = row
    N, K, C, D, H, W = shape
    assert lib.get_option("pixel_dsplit") == 0 and lib.get_option("sweep_xcd") == 1
    f, b = _query(lib, shape, G)
    assert f == (units, parts, fwd), (name, G, f)
    assert b == (-(-C // 32), 1, bwd), (name, G, b)              # the backward deals slabs, never XCD parts
    assert f == PB.restated(N, C, G, D, H, W, False) and b == PB.restated(N, C, G, D, H, W, True)


def test_what_the_table_documents():
    """Every shape the suite ran before tests/test_gpu_pixel_blocking.py, the fixture scenes included, walks ONE hypothesis per
    block; the workload walks 4 forward and all 12 backward; Q3 / Q4 / Q5 walk several under the default rule."""
    assert all(r[3][2:] == (1, 1) for r in PB.EXISTING + PB.FIXTURES)
    assert all(r[3] == (8, 1, 4, 12) for r in PB.WORKLOAD)
    assert PB.expected("Q4", 0) == (2, 4, 2, 2) and PB.expected("Q5", 0) == (3, 1, 3, 3) and PB.expected("Q3", 0) == (8, 1, 3, 3)
    assert [PB.expected(f"U-{C}", 0)[:2] for C in PB.UNIT_WIDTHS] == [(4, 2), (5, 1), (8, 1), (9, 1)]
    assert [PB.expected("U-256", G)[0] for G in PB.UNIT_GROUPS] == [1, 2, 4, 8, 8]


def test_table_holds_the_shapes_of_the_gpu_tests_and_fixtures():
    """The rows are the shapes those files use: read from the test modules and from the fixture files."""
    import test_gpu_groupcorr as TG
    import test_gpu_sweep_pixel as TS
    rows = {(r[0], r[2]): r[1] for r in PB.EXISTING}
    assert {(n, 0): s for n, s in TS.SHAPES.items()} == {k: v for k, v in rows.items() if k[1] == 0}
    assert {(n, G): TG.SHAPES[n] for n, G in TG.CASES} == {k: v for k, v in rows.items() if k[1] > 0}
    fix = {(r[0], r[2]): r[1] for r in PB.FIXTURES}
    for tag in ("n3_d8", "n6_d12_arkit"):
        g2 = load_golden("g2_variance_" + tag)
        N, C, H, W = g2["feature"].shape
        K = g2["neighbor_ids"].shape[1]
        D = load_golden(f"g22_sweep_pixel_{tag}_rough")["depth"].shape[1]
        assert fix[("G22 " + tag, 0)] == (N, K, C, D, H, W)
    for tag, kind, G in TG.G23:
        g2, g = load_golden("g2_variance_" + tag), load_golden(f"g23_groupcorr_{tag}_{kind}_g{G}")
        N, C, H, W = g2["feature"].shape
        D = g2["depth_values"].shape[1] - int(g["first_plane"]) if kind == "plane" else load_golden(f"g22_sweep_pixel_{tag}_rough")["depth"].shape[1]
        name = "G23 n6_d12_arkit" if tag == "n6_d12_arkit" else f"G23 {tag} {kind}"
        assert fix[(name, G)] == (N, g2["neighbor_ids"].shape[1], C, D, H, W), (tag, kind, G)


# ---------------------------------------------------------------------------------------------------------------- 2
def test_query_and_restatement_agree_over_a_sweep(options):
    lib = options
    rng = np.random.default_rng(7)
    n = 0
    for dsplit, xcd in ((0, 1), (0, 0), (1, 1), (2, 1), (3, 0), (5, 1), (1000, 1)):
        lib.set_option("pixel_dsplit", dsplit)
        lib.set_option("sweep_xcd", xcd)
        for _ in range(120):
            N, D = int(rng.integers(1, 50)), int(rng.integers(1, 40))
            H, W = int(rng.integers(2, 130)), int(rng.integers(2, 130))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                C, G = int(rng.integers(1, 300)), 0
            elif kind == 1:
                cg = int(rng.choice([4, 8, 16]))
                G = int(rng.integers(1, 40))
                C = cg * G
            else:
                cg = 32 * int(rng.integers(1, 5))
                G = int(rng.integers(1, 12))
                C = cg * G
            for bwd in (False, True):
                assert lib.pixel_form_blocking(N, C, G, D, H, W, bwd) == PB.restated(N, C, G, D, H, W, bwd, dsplit, xcd), (N, C, G, D, H, W, bwd, dsplit, xcd)
                n += 1
    assert n == 7 * 120 * 2


# ---------------------------------------------------------------------------------------------------------------- 3
def test_pixel_dsplit_round_trip_and_meaning(options):
    lib = options
    for v in (1, 2, 7, 0):
        lib.set_option("pixel_dsplit", v)
        assert lib.get_option("pixel_dsplit") == v
    shape = (3, 40, 0, 5, 9, 21)
    lib.set_option("pixel_dsplit", 1)                       # one block per (view, tile, unit) walks all five: forward 4 + 1
    assert lib.pixel_form_blocking(*shape, False)[2] == 4 and lib.pixel_form_blocking(*shape, True)[2] == 5
    lib.set_option("pixel_dsplit", 2)                       # 3 + 2
    assert lib.pixel_form_blocking(*shape, False)[2] == 3 and lib.pixel_form_blocking(*shape, True)[2] == 3
    lib.set_option("pixel_dsplit", 5)
    assert lib.pixel_form_blocking(*shape, False)[2] == 1 and lib.pixel_form_blocking(*shape, True)[2] == 1
    lib.set_option("pixel_dsplit", 99)                      # min(n, D)
    assert lib.pixel_form_blocking(*shape, False)[2] == 1 and lib.pixel_form_blocking(*shape, True)[2] == 1
    # the workload under a forced single split: the forward's cap stays, the backward walks all 12
    lib.set_option("pixel_dsplit", 1)
    assert lib.pixel_form_blocking(40, 256, 0, 12, 60, 80, False) == (8, 1, 4)
    assert lib.pixel_form_blocking(40, 256, 8, 12, 60, 80, True) == (8, 1, 12)
    # units and XCD parts do not depend on it; "sweep_xcd" 0 takes the parts away, and with them the rounded-up grid
    lib.set_option("pixel_dsplit", 0)
    assert lib.pixel_form_blocking(3, 40, 0, 5, 9, 21, False)[:2] == (2, 4)
    lib.set_option("sweep_xcd", 0)
    assert lib.pixel_form_blocking(3, 40, 0, 5, 9, 21, False)[:2] == (2, 1)


def test_the_plane_forms_split_option_is_its_own(options):
    lib = options
    before = lib.pixel_form_blocking(40, 256, 0, 12, 60, 80, False), lib.pixel_form_blocking(40, 256, 0, 12, 60, 80, True)
    lib.set_option("sweep_dsplit", 3)
    assert lib.get_option("pixel_dsplit") == 0
    assert (lib.pixel_form_blocking(40, 256, 0, 12, 60, 80, False), lib.pixel_form_blocking(40, 256, 0, 12, 60, 80, True)) == before
    lib.set_option("sweep_dsplit", 0)
    lib.set_option("pixel_dsplit", 3)
    assert lib.get_option("sweep_dsplit") == 0


# ---------------------------------------------------------------------------------------------------------------- 4
def test_refusals(lib):
    L = lib.load()
    u, p, d = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    out = (ctypes.byref(u), ctypes.byref(p), ctypes.byref(d))
    for args, word in (((0, 32, 0, 4, 8, 8), b"bad shape"), ((2, 0, 0, 4, 8, 8), b"bad shape"), ((2, 32, 0, 0, 8, 8), b"bad shape"),
                       ((2, 32, 0, 4, 1, 8), b"bad shape"), ((2, 32, 0, 4, 8, 1), b"bad shape"), ((2, 32, 0, 513, 8, 8), b"D >"),
                       ((2, 32, 0, 4, 70000, 8), b"65534"), ((2, 32, 0, 4, 8, 70000), b"65534"),
                       ((2, 32, 0, 4, 5000, 5000), b"2^31"), ((60000, 32, 0, 4, 4000, 4000), b"grid too large"),
                       ((2, 32, -1, 4, 8, 8), b"negative"),
                       ((2, 48, 4, 4, 8, 8), b"4, 8, 16"), ((2, 48, 1, 4, 8, 8), b"4, 8, 16"), ((2, 32, 5, 4, 8, 8), b"4, 8, 16"),
                       ((2, 8, 8, 4, 8, 8), b"4, 8, 16"), ((2, 24, 1, 4, 8, 8), b"4, 8, 16")):
        for bwd in (0, 1):
            assert L.mvsdet_pixel_form_blocking(*args, bwd, *out) == 1, args
            assert word in L.mvsdet_last_error(), (args, L.mvsdet_last_error())
    assert (u.value, p.value, d.value) == (-7, -7, -7)          # a refusal writes nothing
    assert L.mvsdet_pixel_form_blocking(2, 32, 0, 4, 8, 8, 0, None, ctypes.byref(p), ctypes.byref(d)) == 1
    assert b"NULL" in L.mvsdet_last_error()
    with pytest.raises(ValueError, match="4, 8, 16"):
        lib.pixel_form_blocking(2, 48, 4, 4, 8, 8)
    with pytest.raises((ValueError, RuntimeError), match="unknown option"):
        lib.set_option("pixel_dsplit_", 1)
    assert lib.pixel_form_blocking(2, 32, 0, 4, 8, 8) == (1, 8, 1)
