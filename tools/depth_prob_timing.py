"""depth_prob_topk at the reference-true shape (40 views, 12 planes, 60x80), at the headline 64-plane shape and at the ARKit
96-plane shape (GPU box): the 16-register, the 64-register and the streaming form of the kernel.  Prints the minimum, the median
and the maximum of 7 rounds of 50 calls; for an A/B run, point MVSDET_HIP_LIB at the other build of the library, or set
MVSDET_DEPTHPROB_AHEAD=0 for the plane-by-plane order (docs/KERNEL_NOTES.md 4.2), and run again on the same box."""
import os
import statistics
import sys

import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvsdet_amd import ops  # noqa: E402
dev = torch.device("cuda:0")
for N, D, H, W in ((40, 12, 60, 80), (40, 64, 120, 160), (50, 96, 60, 80)):
    lg = torch.randn(N, 2, D, H, W, device=dev)
    lg[:, 0] *= 3
    def run(): return ops.depth_prob_topk(lg[:, 0], lg[:, 1], 0.2, 4.8 / D, 3)
    for _ in range(10): run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50): run()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 50)
    print(f"depth_prob_topk {N}x{D}x{H}x{W}: min {min(ms):.4f} / median {statistics.median(ms):.4f} / max {max(ms):.4f} ms")
