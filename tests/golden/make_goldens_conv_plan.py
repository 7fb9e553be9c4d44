#!/usr/bin/env python3
"""Generate tests/golden/conv_plan_sizes.json: what the library's size queries of the bf16x3 convolutions return, default options.

The queries are the only trace the host-side plans leave without a GPU -- padded extents of the SCL and PSCL forms, the number of
input-channel splits (as workspace bytes), the stride-1 tile (as statistics parts) and the choice between the 4 x 8 x 16 and the
3 x 16 x 8 tile of the transposed layer (statistics parts, 0 where the 4 x 8 x 16 tile is taken).  Recorded from the library as
it stood BEFORE the launchers' host code was folded into csrc/conv_host.h; tests/test_conv_plan_sizes.py holds the library to them.

    python tests/golden/make_goldens_conv_plan.py        (needs the built library, no GPU)
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (D, H, W)
COST_NET = [(12, 60, 80), (6, 30, 40), (3, 15, 20), (64, 60, 80), (32, 30, 40), (16, 15, 20), (24, 120, 160), (128, 120, 160)]
NECK = [(16, 40, 40), (8, 20, 20), (4, 10, 10), (40, 40, 16), (20, 20, 8), (10, 10, 4)]
# tests/test_gpu_conv_edges.py: S1, the fp16 + MX cases, the stride-2 and the transposed cases
EDGES = [(1, 1, 1), (4, 12, 16), (5, 13, 17), (3, 11, 15), (4, 8, 16), (6, 16, 8), (7, 17, 9), (3, 16, 8), (8, 8, 8), (9, 9, 9), (7, 7, 7),
         (2, 15, 17), (3, 7, 15), (5, 9, 17), (2, 11, 33), (2, 2, 2), (8, 16, 32), (9, 17, 33), (7, 23, 15), (1, 3, 5), (2, 4, 8),
         (3, 5, 9)]
# the 4 x 8 x 16 and the 3 x 16 x 8 tile pad these alike (the tie goes to 4 x 8 x 16) ...
TIES = [(12, 16, 16), (24, 32, 16), (12, 16, 32), (12, 48, 16), (11, 16, 16), (12, 15, 16)]
# ... and one voxel further the 3 x 16 x 8 tile pads less (D or W grown) or more (H grown)
PAST_TIE_38 = [(13, 16, 16), (25, 32, 16), (12, 16, 33), (13, 48, 16)]
PAST_TIE_416 = [(12, 17, 16), (24, 33, 16), (12, 17, 32), (12, 49, 16)]
SHAPES = COST_NET + NECK + EDGES + TIES + PAST_TIE_38 + PAST_TIE_416

BATCHES = [1, 3]
CHANNELS = [(1, 8, 64), (1, 20, 64), (1, 32, 64), (3, 64, 128), (1, 256, 128)]   # (N, Cin, Cout)


def padded(fn, N, C, D, H, W):
    e = [ctypes.c_int(0) for _ in range(3)]
    nbytes = fn(N, C, D, H, W, *[ctypes.byref(v) for v in e])
    return [nbytes] + [v.value for v in e]


def record(lib, D, H, W):
    """What every query says of the volume (D, H, W): the stride-2 query takes it as its INPUT, the transposed one as its coarse input."""
    return {
        "dhw": [D, H, W],
        "scl": [[N, C] + padded(lib.mvsdet_scl_bytes, N, C, D, H, W) for N in BATCHES for C in (8, 20)],
        "pscl": [[N, C] + padded(lib.mvsdet_pscl_bytes, N, C, D, H, W) for N in BATCHES for C in (8, 20)],
        "workspace": [[N, Ci, Co, lib.mvsdet_conv3d_k3_bf16x3_workspace_bytes(N, Ci, Co, D, H, W)] for N, Ci, Co in CHANNELS],
        "stats_parts": [[N, f32, lib.mvsdet_conv3d_k3_bf16x3_stats_parts(N, D, H, W, f32)] for N in BATCHES for f32 in (0, 1)],
        "s2_workspace": [[N, Ci, Co, lib.mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes(N, Ci, Co, D, H, W)] for N, Ci, Co in CHANNELS],
        "convT_stats_parts": [[N, lib.mvsdet_convT3d_k3_s2_bf16x3_stats_parts(N, D, H, W)] for N in BATCHES],
    }


def main():
    from mvsdet_amd import _lib
    lib = _lib.load()
    out = {"ties": [list(s) for s in TIES], "past_tie_3x16x8": [list(s) for s in PAST_TIE_38],
           "past_tie_4x8x16": [list(s) for s in PAST_TIE_416], "shapes": [record(lib, *s) for s in SHAPES]}
    path = os.path.join(HERE, "conv_plan_sizes.json")
    with open(path, "w") as fh:
        fh.write("{\n")
        for k in ("ties", "past_tie_3x16x8", "past_tie_4x8x16"):
            fh.write(f' "{k}": {json.dumps(out[k])},\n')
        fh.write(' "shapes": [\n' + ",\n".join("  " + json.dumps(r) for r in out["shapes"]) + "\n ]\n}\n")
    print(path, os.path.getsize(path), "bytes,", len(SHAPES), "shapes")


if __name__ == "__main__":
    main()
