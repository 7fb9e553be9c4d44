#!/usr/bin/env python3
"""Generate tests/golden/g14_neck_head_train.npz by RUNNING THE REFERENCE (build container only: needs the reference tree).

G14: one TRAINING step of the 3-D neck and the detection head together -- mmdet3d/models/necks/imvoxel_neck.py:70-231
`IndoorImVoxelNeck(256, 128, [1, 1, 1])` in train mode (BatchNorm on batch statistics) feeding nerfdet_head.py:90-118
`NerfDetHead(128, 6, 18, 3)`, both executed where they lie as for G10 / G11 (_ref_loader), under autograd:

    loss = sum over levels of sum(center * R_c + bbox * R_r + cls * R_cls),   R from the LCG

on the G10 input (LCG (1,256,40,40,16), sparsity mask).  Stored: the head outputs and the neck levels (sampled), the input's gradient
(sampled), every parameter's gradient (sampled by stride, with its float64 squared norm and max |.|, as G12c), the running statistics
after the step, and the neck's ReLU DECISIONS (the mask `relu output > 0` of each nn.ReLU module): every MASK_STRIDE-th decision
bit-packed and each layer's count of positive ones.  All 37 M decisions would be 4.6 MB of incompressible bits; the package's
framework route reproduces them (tests/test_g14_neck_head_train.py checks it against the samples and the counts), so a test that
imposes the reference's decisions on the HIP route records them from that route instead of reading them from here.  Every sampled
array `k` has its slice steps in `step:k` (channel, d, h, w).

    python tests/golden/make_goldens_g14.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens  # noqa: E402
from make_goldens import STAND_IN, save  # noqa: E402
from _ref_loader import load_reference_head, load_reference_neck  # noqa: E402
from lcg import lcg_fill_state, lcg_uniform  # noqa: E402

WEIGHT_SEED_NECK, WEIGHT_SEED_HEAD, R_SEED = 14, 15, 140
GRAD_SAMPLES = 2048        # samples per parameter gradient
GRAD_INPUT_STRIDE = 389    # of the input's gradient
MASK_STRIDE = 61           # of the ReLU decisions (prime: no alignment with the 40 x 40 x 16 grid or the channel count)
# slice steps (channel, d, h, w) of the stored outputs: neck levels and head maps per level
LEVEL_STEPS = ((8, 4, 4, 2), (8, 2, 2, 2), (4, 1, 1, 1))
HEAD_STEPS = ((1, 4, 4, 2), (1, 2, 2, 2), (1, 1, 1, 1))
HEAD_SCALES = (0.5, 0.75, 1.0)


def g14_input():
    """The G10 input: LCG values on the shipped grid, empty columns from a second LCG stream."""
    x = torch.from_numpy(lcg_uniform(256 * 40 * 40 * 16, 100)).reshape(1, 256, 40, 40, 16)
    keep = torch.from_numpy(lcg_uniform(40 * 40 * 16, 101)).reshape(1, 1, 40, 40, 16) > 0.6
    return x * keep


def loss_weights(centers, regs, clss):
    """R_c, R_r, R_cls of each level (LCG streams R_SEED + 10 level + 0 / 1 / 2)."""
    out = []
    for i, ts in enumerate(zip(centers, regs, clss)):
        out.append([torch.from_numpy(lcg_uniform(t.numel(), R_SEED + 10 * i + k)).reshape(t.shape) for k, t in enumerate(ts)])
    return out


def sample_grad(g: torch.Tensor):
    """G12c's sampling: every `stride`-th element, stride coprime to 2 and 3, about GRAD_SAMPLES samples."""
    g = g.reshape(-1)
    stride = max(1, g.numel() // GRAD_SAMPLES)
    while stride > 1 and (stride % 2 == 0 or stride % 3 == 0):
        stride += 1
    return g[::stride].clone(), stride


def main():
    torch.set_num_threads(4)
    torch.manual_seed(0)
    neck = load_reference_neck()(256, 128, [1, 1, 1]).train()
    head = load_reference_head("NerfDetHead")(128, 6, 18, 3).train()
    with torch.no_grad():
        lcg_fill_state(neck, WEIGHT_SEED_NECK)
        lcg_fill_state(head, WEIGHT_SEED_HEAD)
        for s, v in zip(head.scales, HEAD_SCALES):
            s.scale.fill_(v)
    masks = {}
    for name, m in neck.named_modules():
        if isinstance(m, torch.nn.ReLU):   # the output of an in-place ReLU: its positive side is the decision
            m.register_forward_hook(lambda mod, inp, out, name=name: masks.__setitem__(name, (out.detach() > 0).clone()))
    x = g14_input().requires_grad_(True)
    levels = neck(x)
    centers, regs, clss = head(levels)
    loss = 0.0
    for ts, rs in zip(zip(centers, regs, clss), loss_weights(centers, regs, clss)):
        for t, r in zip(ts, rs):
            loss = loss + (t * r).sum()
    loss.backward()

    out = dict(grad_input=x.grad.reshape(-1)[::GRAD_INPUT_STRIDE].clone(), grad_input_stride=np.int64(GRAD_INPUT_STRIDE),
               loss=np.float64(loss.item()))

    def sample(name, t, steps):
        c, d, h, w = steps
        out[name] = t.detach()[:, ::c, ::d, ::h, ::w].clone()
        out["step:" + name] = np.array(steps)
    for i in range(3):
        for k, t in (("center", centers[i]), ("reg", regs[i]), ("cls", clss[i])):
            sample(f"{k}{i}", t, HEAD_STEPS[i])
        sample(f"level{i}", levels[i], LEVEL_STEPS[i])
    out["level_scales"] = np.array([float(o.detach().abs().max()) for o in levels])
    keys = []
    for prefix, net in (("neck.", neck), ("head.", head)):
        for k, p in sorted(net.named_parameters()):
            g, stride = sample_grad(p.grad)
            key = prefix + k
            keys.append(key)
            out["g:" + key] = g
            out["n:" + key] = np.float64((p.grad.double() ** 2).sum())
            out["s:" + key] = np.int64(stride)
            out["m:" + key] = np.float32(p.grad.abs().max())
    for k, b in neck.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
            out["b:" + k] = b.clone()
    for name, m in masks.items():
        out["maskbits:" + name] = np.packbits(m.numpy().reshape(-1)[::MASK_STRIDE])
        out["maskpos:" + name] = np.int64(m.sum())
        out["maskshape:" + name] = np.array(m.shape)
    make_goldens.META["generator"] = np.array("tests/golden/make_goldens_g14.py")
    save("g14_neck_head_train", weight_seed_neck=WEIGHT_SEED_NECK, weight_seed_head=WEIGHT_SEED_HEAD, input_seed=100, mask_seed=101,
         mask_threshold=np.float32(0.6), r_seed=R_SEED, head_scales=np.array(HEAD_SCALES, dtype=np.float32),
         param_keys=np.array(keys), mask_names=np.array(sorted(masks)), mask_stride=np.int64(MASK_STRIDE), stand_in=STAND_IN, **out)
    print("g14 loss", loss.item(), "levels", [float(o.detach().abs().max()) for o in levels], "positive share per ReLU",
          {k: round(float(m.float().mean()), 3) for k, m in masks.items()})


if __name__ == "__main__":
    main()
