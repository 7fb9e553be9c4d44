"""How the per-pixel form of the sweep (csrc/pixel_form.h: pixel_blocking) cuts a problem into blocks, restated in Python, and the
table of shapes that tests/test_pixel_blocking_host.py (no GPU) and tests/test_gpu_pixel_blocking.py assert through the query
mvsdet_pixel_form_blocking -- TEST INFRASTRUCTURE ONLY.

A row: (name, (N, K, C, D, H, W), G, (units, xcd_parts, hypotheses per block forward, ... backward)); G = 0 is the variance / the
compatibility warp, G > 0 the group correlation with G groups.  The figures are written out, not computed: a change of the rule (the
2048-block threshold, the forward's cap of 4, the dealing of units to XCDs) must show here.

  EXISTING  every shape tests/test_gpu_sweep_pixel.py and tests/test_gpu_groupcorr.py run: one hypothesis per block throughout --
            the gap tests/test_gpu_pixel_blocking.py closes;
  FIXTURES  the scenes of fixtures G22 / G23 (tests/golden): n3_d8 (48 x 64) and n6_d12_arkit (16 x 20);
  WORKLOAD  the project's own shape: 4 per block forward, all 12 backward;
  NEW       shapes at which the default rule itself walks several hypotheses per block (Q3, Q4, Q5), and the tiny maps of the
            unit-dealing tests (U-*)."""

MAX_FORWARD = 4      # a forward block walks at most this many hypotheses
FILL_BLOCKS = 2048   # the split doubles until the grid has this many blocks


def restated(N, C, G, D, H, W, backward, pixel_dsplit=0, sweep_xcd=1):
    """(units, xcd_parts, d_per_block) as pixel_form.h computes them."""
    slabs, tiles = -(-C // 32), -(-(H * W) // 128)
    n_bt = N * tiles
    if backward:
        units, parts, grid = slabs, 1, n_bt * slabs
    else:
        units = G if G > 0 and (C // G) % 32 == 0 else slabs
        parts, grid = 1, n_bt * units
        if units < 8 and 8 % units == 0 and sweep_xcd:
            parts = 8 // units
            grid = 8 * -(-n_bt // parts)
    if pixel_dsplit > 0:
        dsplit = pixel_dsplit
    else:
        dsplit = 1
        while grid * dsplit < FILL_BLOCKS and dsplit < D:
            dsplit *= 2
    dsplit = min(dsplit, D)
    dpb = -(-D // dsplit)
    if not backward:
        dpb = min(dpb, MAX_FORWARD)
    return units, parts, dpb


EXISTING = [
    # tests/test_gpu_sweep_pixel.py
    ("S-odd", (3, 2, 40, 5, 9, 21), 0, (2, 4, 1, 1)),
    ("S-fast", (2, 1, 32, 1, 8, 32), 0, (1, 8, 1, 1)),
    ("S-80", (4, 2, 64, 12, 16, 80), 0, (2, 4, 1, 1)),
    ("S-k3", (4, 3, 16, 2, 6, 10), 0, (1, 8, 1, 1)),
    ("S-k4", (5, 4, 8, 3, 6, 10), 0, (1, 8, 1, 1)),
    # tests/test_gpu_groupcorr.py
    ("A", (3, 2, 40, 5, 9, 21), 10, (2, 4, 1, 1)),
    ("A", (3, 2, 40, 5, 9, 21), 5, (2, 4, 1, 1)),
    ("B", (2, 1, 48, 2, 8, 32), 3, (2, 4, 1, 1)),
    ("C", (3, 2, 96, 3, 9, 21), 1, (1, 8, 1, 1)),
    ("C", (3, 2, 96, 3, 9, 21), 3, (3, 1, 1, 1)),
    ("D", (4, 3, 64, 2, 6, 10), 1, (1, 8, 1, 1)),
    ("E", (4, 2, 64, 12, 16, 80), 8, (2, 4, 1, 1)),
    ("F", (5, 4, 32, 2, 6, 10), 8, (1, 8, 1, 1)),
    ("F", (5, 4, 32, 2, 6, 10), 4, (1, 8, 1, 1)),
    ("F", (5, 4, 32, 2, 6, 10), 2, (1, 8, 1, 1)),
    ("F", (5, 4, 32, 2, 6, 10), 1, (1, 8, 1, 1)),
]

WORKLOAD = [
    ("workload", (40, 2, 256, 12, 60, 80), 0, (8, 1, 4, 12)),
    ("workload", (40, 2, 256, 12, 60, 80), 8, (8, 1, 4, 12)),
]

Q3, Q4, Q5 = (4, 2, 256, 3, 64, 128), (5, 2, 40, 11, 45, 91), (6, 3, 72, 9, 45, 91)
A7 = (3, 2, 40, 7, 9, 21)
Q_NBR = {"Q3": [[1, 2], [0, 0], [3, 1], [3, 0]], "Q4": [[0, 1], [2, 2], [1, 0], [4, 2], [3, 0]],
         "Q5": [[1, 2, 3], [0, 0, 2], [2, 3, 1], [5, 4, 0], [4, 4, 1], [0, 5, 3]]}
UNIT_WIDTHS = (128, 160, 256, 288)          # the variance's 4, 5, 8 and 9 units
UNIT_GROUPS = (1, 2, 4, 8, 64)              # at C = 256: 1, 2, 4, 8 and 8 units


def unit_shape(C):
    return (2, 2, C, 3, 9, 21)


NEW = [
    ("Q4", Q4, 0, (2, 4, 2, 2)),
    ("Q4", Q4, 10, (2, 4, 2, 2)),
    ("Q4", Q4, 5, (2, 4, 2, 2)),
    ("Q5", Q5, 0, (3, 1, 3, 3)),
    ("Q5", Q5, 9, (3, 1, 3, 3)),
    ("Q3", Q3, 0, (8, 1, 3, 3)),
    ("Q3", Q3, 8, (8, 1, 3, 3)),
    ("Q3", Q3, 64, (8, 1, 3, 3)),
    # one group over all 8 slabs is ONE unit: 8 XCD parts, a grid of 256 blocks, and the default rule splits the forward into one
    # hypothesis per block; tests/test_gpu_pixel_blocking.py runs this forward under "pixel_dsplit" 1 as well
    ("Q3", Q3, 1, (1, 8, 1, 3)),
    # shape A of tests/test_gpu_groupcorr.py with D raised to 7: 4 + 3 and 3 + 3 + 1 under "pixel_dsplit" 1 and 2 (the default: 1)
    ("A7", A7, 10, (2, 4, 1, 1)),
    ("A7", A7, 5, (2, 4, 1, 1)),
    ("U-128", unit_shape(128), 0, (4, 2, 1, 1)),
    ("U-160", unit_shape(160), 0, (5, 1, 1, 1)),
    ("U-256", unit_shape(256), 0, (8, 1, 1, 1)),
    ("U-288", unit_shape(288), 0, (9, 1, 1, 1)),
    ("U-256", unit_shape(256), 1, (1, 8, 1, 1)),
    ("U-256", unit_shape(256), 2, (2, 4, 1, 1)),
    ("U-256", unit_shape(256), 4, (4, 2, 1, 1)),
    ("U-256", unit_shape(256), 8, (8, 1, 1, 1)),
    ("U-256", unit_shape(256), 64, (8, 1, 1, 1)),
]

# fixtures G22 (per-pixel variance: the rough and the smooth depth maps of a scene have one shape) and G23 (group correlation; the
# plane cases of n3_d8 drop the scene's first plane: D = 7).  tests/test_pixel_blocking_host.py checks the shapes against the files.
# Not one of them walks more than one hypothesis per block.
_N3, _N6 = (3, 2, 32, 8, 48, 64), (6, 2, 8, 12, 16, 20)
FIXTURES = [("G22 n3_d8", _N3, 0, (1, 8, 1, 1)), ("G22 n6_d12_arkit", _N6, 0, (1, 8, 1, 1))]
FIXTURES += [("G23 n3_d8 pixel", _N3, G, (1, 8, 1, 1)) for G in (1, 2, 4, 8)]
FIXTURES += [("G23 n3_d8 plane", (3, 2, 32, 7, 48, 64), G, (1, 8, 1, 1)) for G in (1, 2, 4, 8)]
FIXTURES += [("G23 n6_d12_arkit", _N6, G, (1, 8, 1, 1)) for G in (1, 2)]

TABLE = EXISTING + WORKLOAD + NEW + FIXTURES


def expected(name, G):
    """(units, xcd_parts, forward per block, backward per block) of the row (name, G)."""
    rows = [r for r in TABLE if r[0] == name and r[2] == G]
    assert len(rows) == 1, (name, G)
    return rows[0][3]
