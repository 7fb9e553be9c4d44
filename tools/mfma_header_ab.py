"""Do two builds of the library give the same bits, at the same speed, in every operator that cuts fp32 into bf16 pieces or multiplies
on the bf16 matrix cores through csrc/mfma.h?  One fresh child process per library and run (MVSDET_HIP_LIB selects the library:
mvsdet_amd/_lib.py), one after the other, each under its own time limit; the driving process never touches the GPU.

    python tools/mfma_header_ab.py --before build_ab/libparent.so [--after mvsdet_amd/libmvsdet_hip.so] [--out FILE]
    python tools/mfma_header_ab.py --before build_ab/libparent.so --time [--runs 5] [--out FILE]      (appends to FILE)

Bits (the default): the --before library runs twice and the --after one once.  One line per operator and shape: a SHA-256 (first 32 hex
digits) of the bytes of all its outputs.  None of these operators uses an atomic, so the three digests must be equal: exit status 1 if
one differs.  Inputs are the seeded builders of tests/ at the small shapes those tests use, and `bf16x3_edge_vector`
(tests/test_gpu_bf16.py: ties of both roundings, the carry into the exponent, overflow, subnormals, infinities, a NaN).

--time: `--runs` processes per library, the libraries alternating (before, after, before, ...): the kernels that differ alone at the
scene's shapes (this file's --time-child) and the project's timing scripts.  Every "<number> ms" a script prints is one row: the
--before runs' median and spread (max - min), the --after runs' median; a row passes if the --after median is not above the --before
median plus that spread -- the smallest change the measurement can see."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_S1 = [(1, 16, 64, 4, 8, 16), (2, 24, 64, 5, 13, 21), (1, 5, 64, 1, 1, 1), (1, 24, 64, 6, 30, 40), (1, 16, 64, 3, 15, 20)]
CONV_MX = [(1, 1, 64, 1, 1, 1), (3, 5, 64, 4, 8, 16), (1, 20, 128, 3, 7, 15), (2, 64, 64, 12, 24, 32)]         # test_gpu_conv_edges; a 12-wave tile
CONV_S2 = [(1, 5, 64, 1, 1, 1), (1, 3, 64, 2, 2, 2), (1, 5, 64, 2, 2, 2), (3, 20, 64, 8, 16, 32)]        # test_gpu_bf16, test_gpu_conv_edges
CONV_T = [(1, 5, 64, 1, 1, 1), (1, 16, 64, 4, 8, 16), (1, 8, 64, 1, 1, 1), (3, 64, 64, 2, 4, 8), (1, 24, 128, 3, 15, 20)]   # the last: 3x16x8 tiles
DW_S1 = [(2, 5, 3, 1, 1, 4, 2), (3, 8, 8, 2, 3, 12, 1), (1, 40, 70, 2, 5, 20, 3)]                           # the last: a ragged tile in W
DW_S2 = [(2, 5, 3, 2, 2, 8, 2), (3, 8, 130, 2, 4, 16, 1), (1, 40, 70, 2, 6, 24, 3)]
HEAD_DW = [(1, 16, 1, 1, 4), (2, 32, 3, 7, 20), (1, 64, 4, 9, 16), (1, 64, 2, 3, 36)]                       # MT = 1, 2, 4; W = 20, 36: ragged
NECK_FWD = [(1, 32, 128, 2, 2, 2), (3, 64, 256, 4, 6, 10), (1, 96, 128, 6, 2, 14)]                          # test_gpu_conv_edges
NECK_SHORTCUT = [(1, 256, 512, (40, 40, 16)), (1, 512, 1024, (20, 20, 8)), (2, 128, 32, (6, 2, 10))]       # test_g14_neck_head_train
NECK_CONVT = [(1, 1024, 512, (10, 10, 4)), (1, 512, 256, (20, 20, 8)), (2, 128, 4, (3, 5, 7))]
TIMING = [("conv_bf16_timing.py", []), ("dw_bf16_timing.py", []), ("head_bwd_timing.py", []), ("neck_bf16_timing.py", []),
          ("fpn_timing.py", ["--views", "40", "--out", os.devnull])]


def _setup():
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
    from lcg import lcg_uniform
    dev = torch.device("cuda:0")

    def rand(shape, seed):
        return torch.from_numpy(lcg_uniform(int(np.prod(shape)), seed)).reshape(shape).to(dev)
    return torch, dev, rand


def child(out_path: str) -> None:
    torch, dev, rand = _setup()
    from mvsdet_amd import _lib, ops
    from test_gpu_bf16 import bf16x3_edge_vector
    from test_gpu_fpn import _case as fpn_case
    digests = {}

    def digest(name, *tensors):
        h = hashlib.sha256()
        for t in tensors:
            t = t.data if hasattr(t, "padded") else t      # an SclTensor / PsclTensor: the whole buffer, borders included
            h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
        assert name not in digests, name
        digests[name] = h.hexdigest()[:32]

    edge = torch.from_numpy(bf16x3_edge_vector())
    # ---- the cut as stored: scl_pack, gemm_split_weight, split_conv_weight
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 13, 5, 7, 19, generator=g) * 3.0
    x[0, 0, 0, 0, 0] = 0.0
    x[1, 12, 4, 6, 18] = -1e-30
    digest("scl_pack (2, 13, 5, 7, 19)", ops.scl_pack(x.to(dev)))
    digest("scl_pack edge vector (1, 8, 1, 2, 4)", ops.scl_pack(edge.view(1, 1, 2, 4, 8).permute(0, 4, 1, 2, 3).contiguous().to(dev)))
    digest("gemm_split_weight edge vector (128, 32)", ops.gemm_split_weight(edge.repeat(64).view(128, 32).to(dev)))
    digest("gemm_split_weight (256, 512)", ops.gemm_split_weight(rand((256, 512), 11)))
    for order in (0, 1, 2):
        for cin in (5, 24):
            shape = (cin, 64, 3, 3, 3) if order == 2 else (64, cin, 3, 3, 3)
            digest(f"split_conv_weight order={order} (64, {cin})", ops.split_conv_weight(rand(shape, 20 + order + cin), order))

    # ---- the cost network's forward convolutions: test_gpu_bf16's builders
    for N, Cin, Cout, D, H, W in CONV_S1:
        g = torch.Generator().manual_seed(N * 1000 + Cin)
        x = (torch.randn(N, Cin, D, H, W, generator=g).abs() * 2.0).to(dev)
        wq = ops.split_conv_weight((torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5).to(dev))
        scale, shift = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
        res = torch.randn(N, Cout, D, H, W, generator=g).to(dev)
        for tag, inp in (("scl", ops.scl_pack(x)), ("f32", x)):
            digest(f"conv3d_k3_bf16x3 from {tag} {(N, Cin, Cout, D, H, W)}",
                   *ops.conv3d_k3_bf16x3(inp, wq, scale, shift, True, res, outputs=("f32", "scl", "pscl")))
            digest(f"conv3d_k3_bf16x3_stats from {tag} {(N, Cin, Cout, D, H, W)}", *ops.conv3d_k3_bf16x3_stats(inp, wq, shift))
    for N, Cin, Cout, D, H, W in CONV_MX:      # the fp16 + MX kernels store their SCL / PSCL outputs through the same cut
        g = torch.Generator().manual_seed(1000 * Cin + 10 * D + W)
        x = (torch.randn((N, Cin, D, H, W), generator=g).abs() * 2.0).to(dev)
        wq = ops.split_conv_weight_mx((torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5).to(dev))
        scale, shift = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
        for form in (0, 8, 12):                # the wave-specialised kernel and the two plain ones
            _lib.set_option("conv_mx_th", form)
            digest(f"conv3d_k3_fp16mx form {form} {(N, Cin, Cout, D, H, W)}",
                   *ops.conv3d_k3_fp16mx(x, wq, scale, shift, True, outputs=("f32", "scl", "pscl")))
        _lib.set_option("conv_mx_th", 0)
    for N, Cin, Cout, D, H, W in CONV_S2:
        g = torch.Generator().manual_seed(N * 1000 + Cin + W)
        x = (torch.randn(N, Cin, D, H, W, generator=g).abs() * 2.0).to(dev)
        wq = ops.split_conv_weight((torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5).to(dev), 1)
        scale, shift = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
        for tag, inp in (("f32", x), ("pscl", ops.pscl_from_tensor(x))):
            digest(f"conv3d_k3_s2_bf16x3 from {tag} {(N, Cin, Cout, D, H, W)}",
                   *ops.conv3d_k3_s2_bf16x3(inp, wq, scale, shift, True, outputs=("f32", "scl")))
    for N, Cin, Cout, D, H, W in CONV_T:
        g = torch.Generator().manual_seed(N * 1000 + Cin + W)
        x = (torch.randn(N, Cin, D, H, W, generator=g).abs() * 2.0).to(dev)
        wq = ops.split_conv_weight((torch.randn(Cin, Cout, 3, 3, 3, generator=g) / (27 * Cin / 8) ** 0.5).to(dev), 2)
        scale, shift = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
        res = torch.randn(N, Cout, 2 * D, 2 * H, 2 * W, generator=g).to(dev)
        digest(f"convT3d_k3_s2_bf16x3 {(N, Cin, Cout, D, H, W)}", *ops.convT3d_k3_s2_bf16x3(x, wq, scale, shift, res, True, outputs=("f32", "scl")))
        stats = ops.convT3d_k3_s2_bf16x3_stats(x, wq, shift)
        if stats is not None:
            digest(f"convT3d_k3_s2_bf16x3_stats {(N, Cin, Cout, D, H, W)}", *stats)

    # ---- weight gradients
    for stride, cases in ((1, DW_S1), (2, DW_S2)):
        for N, Cin, Cout, D, H, W, nsplit in cases:
            g = torch.Generator().manual_seed(N * 100 + Cin)
            x = torch.randn(N, Cin, D, H, W, generator=g).to(dev)
            gy = torch.randn(N, Cout, D // stride, H // stride, W // stride, generator=g).to(dev)
            digest(f"conv3d_k3_dw bf16x3 stride={stride} {(N, Cin, Cout, D, H, W)} nsplit={nsplit}", ops.conv3d_k3_dw(x, gy, nsplit, stride, True))
    for N, Cin, D, H, W in HEAD_DW:
        g = torch.Generator().manual_seed(8000 + Cin + W)
        x, gy = torch.randn((N, Cin, D, H, W), generator=g).to(dev), torch.randn((N, 2, D, H, W), generator=g).to(dev)
        w = (torch.randn((2, Cin, 3, 3, 3), generator=g) / (27 * Cin) ** 0.5).to(dev)
        digest(f"conv3d_k3_cout2_backward bf16x3 {(N, Cin, D, H, W)}", *ops.conv3d_k3_cout2_backward(x, w, gy, 32, True))

    # ---- the neck's GEMM-shaped layers, MODE 0 - 3 and their weight gradients
    for N, Cin, Cout, D, H, W in NECK_FWD:
        g = torch.Generator().manual_seed(9500 + Cin + W)
        x = torch.randn((N, Cin, D, H, W), generator=g).to(dev)
        w1, b1 = (torch.randn((Cout, Cin), generator=g) / Cin ** 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
        wt, bt = (torch.randn((Cin, Cout, 2, 2, 2), generator=g) / Cin ** 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
        digest(f"conv3d_k1_s2_bf16x3 {(N, Cin, Cout, D, H, W)}", ops.conv3d_k1_s2_bf16x3(x, ops.gemm_split_weight(w1), b1, Cout))
        wqt = ops.gemm_split_weight(wt.permute(1, 2, 3, 4, 0).reshape(8 * Cout, Cin).contiguous())
        digest(f"convT3d_k2_s2_bf16x3 {(N, Cin, Cout, D, H, W)}", ops.convT3d_k2_s2_bf16x3(x, wqt, bt, Cout, True))
    for N, Cin, Cout, (D, H, W) in NECK_SHORTCUT:
        w, gy = rand((Cout, Cin), 1) / Cin ** 0.5, rand((N, Cout, D // 2, H // 2, W // 2), 2)
        x, gx = rand((N, Cin, D, H, W), 3), rand((N, Cin, D, H, W), 4)
        ops.conv3d_k1_s2_dx_bf16x3(gy, ops.gemm_split_weight(w.t().contiguous()), gx)
        digest(f"conv3d_k1_s2_dx_bf16x3 {(N, Cin, Cout, D, H, W)}", gx)
        for nsplit in (0, 1, 3):
            digest(f"neck_gemm_dw_bf16x3 shortcut {(N, Cin, Cout, D, H, W)} nsplit={nsplit}", ops.neck_gemm_dw_bf16x3(x, gy, False, nsplit))
    for N, Cin, Cout, (D, H, W) in NECK_CONVT:
        w, gy = rand((Cin, Cout, 2, 2, 2), 5) / (8 * Cout) ** 0.5, rand((N, Cout, 2 * D, 2 * H, 2 * W), 6)
        x = rand((N, Cin, D, H, W), 7)
        digest(f"convT3d_k2_s2_dx_bf16x3 {(N, Cin, Cout, D, H, W)}", ops.convT3d_k2_s2_dx_bf16x3(gy, ops.gemm_split_weight(w.reshape(Cin, 8 * Cout)), Cin))
        for nsplit in (0, 1, 3):
            digest(f"neck_gemm_dw_bf16x3 transposed {(N, Cin, Cout, D, H, W)} nsplit={nsplit}", ops.neck_gemm_dw_bf16x3(x, gy, True, nsplit))

    # ---- FPN level 0: test_gpu_fpn's builder
    for N, Cin, H, W in ((1, 32, 3, 3), (2, 256, 5, 7)):
        x, w, b = fpn_case(N, Cin, 256, H, W, 1, 100 + Cin, dev)
        digest(f"fpn.lateral {(N, Cin, H, W)}", ops.fpn.lateral(x, ops.gemm_split_weight(w.view(256, Cin)), b))
    for (N, Cin, H, W), (Ht, Wt) in (((2, 32, 7, 5), (4, 3)), ((2, 512, 15, 20), (8, 10))):
        x, w, b = fpn_case(N, Cin, 256, H, W, 1, 21, dev)
        top = torch.randn(N, 256, Ht, Wt, generator=torch.Generator().manual_seed(22)).to(dev)
        digest(f"fpn.lateral with top {(N, Cin, H, W)} <- {(Ht, Wt)}", ops.fpn.lateral(x, ops.gemm_split_weight(w.view(256, Cin)), b, top))
    for N, H, W in ((1, 1, 1), (1, 3, 3), (2, 5, 7)):
        x, w, b = fpn_case(N, 256, 256, H, W, 3, 300 + H * W + 256, dev)
        digest(f"fpn.conv3x3 fp32 and packed {(N, 256, H, W)}",
               *ops.fpn.conv3x3(x, ops.gemm_split_weight(ops.fpn.conv3x3_matrix(w)), b, want_nchw=True, want_packed=True))
    torch.cuda.synchronize()
    with open(out_path, "w") as fh:
        json.dump(digests, fh)


def time_child() -> None:
    """Every kernel that isa_compare shows as different, each alone between two events at the scene's shapes: the five built on
    gemm_bf16x3_block, then those whose cut changed formulation."""
    torch, dev, _ = _setup()
    from mvsdet_amd import ops
    torch.manual_seed(3)
    rand = lambda shape, seed: torch.randn(shape, device=dev)   # noqa: E731  (the values do not matter to the time)

    def timed(name, fn, reps=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"{name}: {e0.elapsed_time(e1) / reps:.4f} ms", flush=True)

    N, Cin, Cout, (D, H, W) = NECK_SHORTCUT[0]
    x, gy, gx = rand((N, Cin, D, H, W), 3), rand((N, Cout, D // 2, H // 2, W // 2), 2), rand((N, Cin, D, H, W), 4)
    w, b = rand((Cout, Cin), 1) / Cin ** 0.5, rand((Cout,), 8)
    wq, wqt = ops.gemm_split_weight(w), ops.gemm_split_weight(w.t().contiguous())
    timed("neck_gemm_bf16x3_kernel<0> 256 -> 512 @ 40x40x16", lambda: ops.conv3d_k1_s2_bf16x3(x, wq, b, Cout))
    timed("neck_gemm_bf16x3_kernel<2> 256 -> 512 @ 40x40x16", lambda: ops.conv3d_k1_s2_dx_bf16x3(gy, wqt, gx))
    N, Cin, Cout, (D, H, W) = NECK_CONVT[1]
    x, gy = rand((N, Cin, D, H, W), 7), rand((N, Cout, 2 * D, 2 * H, 2 * W), 6)
    w, b = rand((Cin, Cout, 2, 2, 2), 5) / (8 * Cout) ** 0.5, rand((Cout,), 9)
    wq = ops.gemm_split_weight(w.permute(1, 2, 3, 4, 0).reshape(8 * Cout, Cin).contiguous())
    wqx = ops.gemm_split_weight(w.reshape(Cin, 8 * Cout))
    timed("neck_gemm_bf16x3_kernel<1> 512 -> 256 @ 20x20x8", lambda: ops.convT3d_k2_s2_bf16x3(x, wq, b, Cout, True))
    timed("neck_gemm_bf16x3_kernel<3> 512 -> 256 @ 20x20x8", lambda: ops.convT3d_k2_s2_dx_bf16x3(gy, wqx, Cin))
    for Cin, H, W, top in ((2048, 8, 10, None), (256, 60, 80, (30, 40))):
        x, w, b = rand((40, Cin, H, W), 12), rand((256, Cin), 13) / Cin ** 0.5, rand((256,), 14)
        t = None if top is None else rand((40, 256) + top, 15)
        wq = ops.gemm_split_weight(w)
        timed(f"fpn_lateral_kernel 40 x {Cin} @ {H}x{W}{' + top' if top else ''}", lambda: ops.fpn.lateral(x, wq, b, t))
    del x, gy, gx, t

    # the kernels whose cut changed formulation, each alone: the neck's stride-1 and stride-2 layers at its three levels (mvsdet_amd/neck.py:
    # the 256-channel layers of the first level from a packed input), conv0 of the cost network on the three fp16 + MX forms, and the
    # head's backward at the channel counts of MT = 1, 2 and 4
    from mvsdet_amd import _lib
    for Cin, Cout, (D, H, W) in ((256, 256, (40, 40, 16)), (256, 128, (40, 40, 16)), (512, 512, (20, 20, 8)), (512, 128, (20, 20, 8)),
                                 (1024, 1024, (10, 10, 4)), (1024, 128, (10, 10, 4))):
        x, res = rand((1, Cin, D, H, W), 20).relu(), rand((1, Cout, D, H, W), 21)
        wq, sc = ops.split_conv_weight(rand((Cout, Cin, 3, 3, 3), 22) / (27 * Cin) ** 0.5), rand((Cout,), 23)
        timed(f"k3_bf16x3 f32 {Cin}-{Cout} @ {D}x{H}x{W}", lambda: ops.conv3d_k3_bf16x3(x, wq, sc, sc, True, res), 50)
        if Cout == 256:
            xs = ops.scl_pack(x)
            timed(f"k3_bf16x3 scl {Cin}-{Cout} @ {D}x{H}x{W}", lambda: ops.conv3d_k3_bf16x3(xs, wq, sc, sc, True, res), 50)
    for Cin, Cout, (D, H, W) in ((256, 512, (40, 40, 16)), (512, 1024, (20, 20, 8))):
        x = rand((1, Cin, D, H, W), 24).relu()
        wq, sc = ops.split_conv_weight(rand((Cout, Cin, 3, 3, 3), 25) / (27 * Cin) ** 0.5, 1), rand((Cout,), 26)
        timed(f"k3_s2_bf16x3 {Cin}-{Cout} @ {D}x{H}x{W}", lambda: ops.conv3d_k3_s2_bf16x3(x, wq, sc, sc, True), 50)
    for Cin in (16, 32, 64):
        x, gy = rand((40, Cin, 12, 60, 80), 27), rand((40, 2, 12, 60, 80), 28)
        w = rand((2, Cin, 3, 3, 3), 29) / 40
        timed(f"cout2_backward bf16x3 Cin {Cin} @ 40x12x60x80", lambda: ops.conv3d_k3_cout2_backward(x, w, gy, 32, True), 10)
    del gy
    x = torch.rand(40, 256, 12, 60, 80, device=dev)
    wmx, sc = ops.split_conv_weight_mx(rand((64, 256, 3, 3, 3), 30) * 0.02), torch.ones(64, device=dev)
    for form in (0, 8, 12):
        _lib.set_option("conv_mx_th", form)
        timed(f"k3_fp16mx form {form} conv0 @ 40x12x60x80", lambda: ops.conv3d_k3_fp16mx(x, wmx, sc, sc, True), 10)
    _lib.set_option("conv_mx_th", 0)


def time_rows(before: str, after: str, runs: int, only):
    """{row: ([before ms], [after ms])}, the rows in the order the scripts print them"""
    rows = {}
    jobs = [("mfma_header_ab.py", [sys.executable, os.path.abspath(__file__), "--time-child"])]
    jobs += [(s, [sys.executable, os.path.join(ROOT, "tools", s), *args]) for s, args in TIMING]
    for script, cmd in jobs:
        if only and script not in only:
            continue
        for r in range(runs):
            for side, lib in enumerate((before, after)):
                env = {**os.environ, "MVSDET_HIP_LIB": os.path.abspath(lib), "PYTHONPATH": ROOT}
                done = subprocess.run(cmd, timeout=300, env=env, capture_output=True, text=True, cwd=ROOT)
                if done.returncode:      # nothing more is started on the GPU after a failure
                    sys.exit(f"{script} under {lib}: exit status {done.returncode}\n{done.stdout}\n{done.stderr}")
                out = done.stdout
                seen = {}
                for line in out.splitlines():
                    for m in re.finditer(r"([0-9.]+) ms\b", line):
                        # a row's name: the line up to its colon and the words in front of the value, without the numbers among them
                        what = " ".join("#" if re.fullmatch(r"\(?[0-9.]+\)?", w) else w for w in line[:m.start()].replace(":", " ").split()[-4:])
                        key = f"{script} | {line.split(':')[0].strip()[:48]} | {what}"
                        seen[key] = seen.get(key, 0) + 1
                        if seen[key] > 1:
                            key += f" #{seen[key]}"
                        rows.setdefault(key, ([], []))[side].append(float(m.group(1)))
            print(f"# {script}: round {r + 1} of {runs} done", file=sys.stderr, flush=True)
    return rows


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--before", help="library to compare against")
    ap.add_argument("--after", default=os.path.join(ROOT, "mvsdet_amd", "libmvsdet_hip.so"))
    ap.add_argument("--out", default=None, help="also write the table to this file (--time: append it)")
    ap.add_argument("--time", action="store_true", help="the timing comparison instead of the digests")
    ap.add_argument("--runs", type=int, default=5, help="--time: processes per library and script")
    ap.add_argument("--only", default="", help="--time: comma-separated script names to run instead of all of them")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--time-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    if a.time_child:
        time_child()
        return 0
    bad = 0
    if a.time:
        rows = ["# script | line | value: before median, before spread (max - min), after median, after - before | verdict (tools/mfma_header_ab.py --time,"
                f" {a.runs} alternating runs per library)"]
        for key, (b, n) in time_rows(a.before, a.after, a.runs, [s for s in a.only.split(",") if s]).items():
            if len(b) != a.runs or len(n) != a.runs:      # a value that not every run printed under the same name
                rows.append(f"{key} | {len(b)} and {len(n)} values of {a.runs} | not compared")
                continue
            mb, mn, spread = statistics.median(b), statistics.median(n), max(b) - min(b)
            ok = mn <= mb + spread
            bad += not ok
            rows.append(f"{key} | {mb:.4f} | {spread:.4f} | {mn:.4f} | {100 * (mn - mb) / mb:+.2f} % | {'pass' if ok else 'SLOWER'}")
        rows.append(f"# {len(rows) - 1} timed values, {bad} slower than the --before median plus its spread")
    else:
        runs = []
        with tempfile.TemporaryDirectory() as tmp:
            for lib in (a.before, a.before, a.after):
                path = os.path.join(tmp, "run.json")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, timeout=300,
                               env={**os.environ, "MVSDET_HIP_LIB": os.path.abspath(lib)})
                with open(path) as fh:
                    runs.append(json.load(fh))
        before, again, after = runs
        rows = ["# operator and shape | digest of before, before's second run and after: one if the three are equal | verdict (tools/mfma_header_ab.py)"]
        for name in before:
            d = [r[name] for r in (before, again, after)]
            same = d[0] == d[1] == d[2]
            bad += not same
            rows.append(f"{name} | {d[0]} | same" if same else f"{name} | {d[0]} | {d[1]} | {d[2]} | DIFFERENT")
        rows.append(f"# {len(before)} digests, {bad} different")
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a" if a.time else "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
