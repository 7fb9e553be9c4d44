"""Do two builds of the library give the same bits in every operator that sums through csrc/block_reduce.h?  One fresh child process
per library (MVSDET_HIP_LIB selects it: mvsdet_amd/_lib.py), one after the other, each under its own time limit; the parent process
never touches the GPU.  The --before library runs twice and the --after one once.

    python tools/block_reduce_ab.py --before build_ab/libparent.so [--after mvsdet_amd/libmvsdet_hip.so] [--out FILE]

One line per operator and shape: a SHA-256 (first 32 hex digits) of the bytes of all its outputs from the three runs.  None of these
operators uses an atomic, so the three digests must be equal: exit status 1 if one differs.  Inputs are the seeded builders of
tests/ (the LCG, the restatements' scenes, the goldens); the shapes are the small ones where a block sum can go wrong:
  depth_loss      both kinds, forward and backward, at tests/test_gpu_depth_loss.py::test_block_counts' shapes (a partial block, exactly
                  one, three and a bit, 268 blocks: the finishing run is 2)
  photo_loss      simple 0 / 1 at (1,10,25), (1,16,16), (3,13,21), (1,257,256) with C = 3, and photo_select of 1 and 3 scenes there
  depth_diag      tests/test_gpu_depth_diag.py's first two scenes
  nvs_score       one tile, a ragged last tile (both without depth), and a scene with a depth pair
  head            head_targets + the three losses and their gradients, axis-aligned (G18) and rotated (G19) boxes, every case
  bn3d            the three training forwards (statistics from x; from a convolution's partial sums; the residual inside the ReLU) and
                  the backward, at vol % 4 == 0 and != 0
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_SHAPES = [(1, 10, 25), (1, 16, 16), (3, 13, 21), (7, 97, 101)]
PHOTO_SHAPES = [(1, 10, 25), (1, 16, 16), (3, 13, 21), (1, 257, 256)]
NVS_SHAPES = [(2, 22, 38, False), (2, 23, 39, False), (2, 23, 70, True)]   # the tile holds 32 x 16 window centres
BN_SHAPES = [(2, 5, (4, 6, 10)), (3, 4, (3, 5, 7))]


def child(out_path: str) -> None:
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
    from conftest import load_golden
    from lcg import lcg_uniform
    from mvsdet_amd import ops
    from mvsdet_amd.ops import costnet, depth, photo
    dev = torch.device("cuda:0")
    F32 = np.float32
    digests = {}

    def to(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def digest(name, *tensors):
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
        digests[name] = h.hexdigest()[:32]

    # ---- depth loss: test_block_counts' inputs
    from test_gpu_depth_loss import holes_map
    for shape in DEPTH_SHAPES:
        N, h, w = shape
        est = to((F32(3.5) + F32(2) * lcg_uniform(N * h * w, 77 + h).reshape(N, h, w)).astype(F32))
        gt2, mask = holes_map(N, h, w, seed=5 + w, hole=2.0), (holes_map(N, h, w, seed=9 + h) > 0).astype(F32)
        for kind, gt, m in ((0, to(holes_map(N, 2 * h + 3, 3 * w - 1, seed=sum(shape))), None), (1, to(gt2), to(mask))):
            leaf = est.clone().requires_grad_(True)
            loss, count = depth.depth_loss(leaf, gt, m, kind)
            loss.backward()
            digest(f"depth_loss kind={kind} {shape}", loss, count, leaf.grad)

    # ---- photometric loss and selection
    for shape in PHOTO_SHAPES:
        B, h, w = shape
        n = B * h * w
        warped, ref = (to(F32(1.5) * lcg_uniform(n * 3, seed + h).reshape(B, h, w, 3).astype(F32)) for seed in (31, 57))
        masks = [to((lcg_uniform(n, 83 + w + 7 * i) > -0.3).astype(F32).reshape(B, h, w, 1)) for i in range(3)]
        L = []
        for simple in (False, True):
            leaf = warped.clone().requires_grad_(True)
            loss, terms, count = photo.reconstr_loss(leaf, ref, masks[0], simple)
            loss.backward()
            digest(f"photo_loss simple={int(simple)} {shape}", loss, terms, count, leaf.grad)
            L.append(loss.detach())
        L.append(0.5 * (L[0] + L[1]))
        for k in (1, 3):
            loss, wins = photo.photometric_select(torch.cat([m.reshape(1, -1) for m in masks[:k]]), torch.stack(L[:k]))
            digest(f"photo_select n={k} {shape}", loss, wins)

    # ---- depth diagnostics
    import test_gpu_depth_diag as DD
    from oracle import oracle as O
    O.build()
    for N, V, J, gt_hw, hw, behind, empty, transposed in DD.SHAPES[:2]:
        case = DD.make_case(N, V, J, gt_hw, hw, seed=100 + N + V + J, behind=behind, empty=empty)
        DD.reference_of(case, O)   # plants the ground truth
        digest(f"depth_diagnostics N={N} V={V} J={J} {gt_hw}->{hw}", *ops.depth_diagnostics(*DD.device_inputs(case, dev, transposed), DD.VZ))

    # ---- view-synthesis scores
    import nvs_score_restated as NR
    for n, H, W, with_depth in NVS_SHAPES:
        sc = NR.scene(n, H, W, depth=with_depth)
        st = ops.nvsmetric.nvs_state(dev)
        per_view, scene = ops.nvsmetric.nvs_score(st, *(None if sc[k] is None else to(sc[k]) for k in ("pred", "gt", "pred_depth", "gt_depth")))
        digest(f"nvs_score {(n, H, W)} depth={int(with_depth)}", per_view, scene, st)

    # ---- head targets and losses, both box kinds
    import test_gpu_head_loss as HL
    import test_gpu_head_loss_arkit as HA
    for mod, gold_name, restated in ((HL, "g18_head_loss", HL.R), (HA, "g19_head_loss_arkit", HA.A)):
        gold = load_golden(gold_name)
        for name in mod.CASES:
            c, r, k, v, origins, gts = mod._case(gold, name, dev)
            t = mod._targets(dev, [tuple(x.shape[2:]) for x in c], origins, gts)
            digest(f"head_targets {gold_name[:3]} {name}", t.labels, t.box_index, t.center_targets, t.bbox_targets)
            maps = [m.requires_grad_(True) for m in c + r + k]
            losses = mod._head().loss_by_feat(c, r, k, v, gts, restated.metas_for(origins))
            (losses["center_loss"] + losses["bbox_loss"] + losses["cls_loss"]).backward()
            digest(f"head_loss {gold_name[:3]} {name}", *(losses[n] for n in mod.NAMES), *(m.grad for m in maps))

    # ---- training BatchNorm3d
    for N, C, grid in BN_SHAPES:
        vol = grid[0] * grid[1] * grid[2]
        u = lcg_uniform(3 * N * C * vol + 3 * C, 40 + vol).astype(F32)
        x, res, g = (to((u[i * N * C * vol:(i + 1) * N * C * vol]).reshape(N, C, *grid)) for i in range(3))
        x = x + torch.arange(C, device=dev, dtype=torch.float32).view(1, C, 1, 1, 1)
        weight, bias, pivot = (to(u[3 * N * C * vol + i * C:3 * N * C * vol + (i + 1) * C] + F32(1 - i)) for i in range(3))
        # what a convolution's epilogue leaves: float64 sums of (x - pivot) and of its square over 300 pieces of every channel
        flat = (x.double() - pivot.double().view(1, C, 1, 1, 1)).permute(1, 0, 2, 3, 4).reshape(C, -1)
        pieces = torch.tensor_split(flat, 300, dim=1)
        parts = torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], 1) for p in pieces], 1).contiguous()
        tag = f"N={N} C={C} vol={vol}"
        out, mean, invstd = costnet.bn3d_relu_train(x, weight, bias, 1e-5, True, res)
        digest(f"bn3d_relu_train_fwd_res {tag}", out, mean, invstd)
        digest(f"bn3d_relu_bwd {tag}", *costnet.bn3d_relu_backward(x, g, weight, bias, mean, invstd, True))
        digest(f"bn3d_relu_train_fwd_parts {tag}", *costnet.bn3d_relu_train(x, weight, bias, 1e-5, True, None, parts, pivot))
        digest(f"bn3d_res_relu_train_fwd {tag}", *costnet.bn3d_res_relu_train(x, weight, bias, res, 1e-5, True))
        digest(f"bn3d_res_relu_train_fwd parts {tag}", *costnet.bn3d_res_relu_train(x, weight, bias, res, 1e-5, True, parts, pivot))
    torch.cuda.synchronize()
    with open(out_path, "w") as fh:
        json.dump(digests, fh)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--before", help="library to compare against")
    ap.add_argument("--after", default=os.path.join(ROOT, "mvsdet_amd", "libmvsdet_hip.so"))
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for lib in (a.before, a.before, a.after):
            path = os.path.join(tmp, "run.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, timeout=300,
                           env={**os.environ, "MVSDET_HIP_LIB": os.path.abspath(lib)})
            with open(path) as fh:
                runs.append(json.load(fh))
    before, again, after = runs
    rows = ["# operator and shape | before | before, second run | after | verdict (tools/block_reduce_ab.py)"]
    bad = 0
    for name in before:
        d = [r[name] for r in (before, again, after)]
        same = d[0] == d[1] == d[2]
        bad += not same
        rows.append(f"{name} | {d[0]} | {d[1]} | {d[2]} | {'same' if same else 'DIFFERENT'}")
    rows.append(f"# {len(before)} digests, {bad} different")
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
