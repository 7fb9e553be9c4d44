"""The bits of the Gaussian rasteriser's operators, the three render functions of `functional` and the three camera operators: one
SHA-256 (first 32 hex digits) per case over the bytes of all outputs and all gradients.  Only the Python API is used, so the same file,
copied into another checkout's tools/, prints that checkout's digests; two trees compute the same when the two outputs are equal line
for line.  None of these operators uses an atomic.

    python tools/splat_digest.py [--out FILE]

Scenes are the seeded builders of tests/splat_scenes.py: the default scene (G 256, V 2, 40x56, 25 harmonics), a tile list one over the
backward's LDS batch (list65), a 17x16 image, V * tiles = 3 (bits3x16x16), precomputed colours (d_sh 1, use_sh False) and the default
scene through strided views of wider buffers.
"""
import argparse
import hashlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import photo_loss_restated as PR  # noqa: E402
import splat_scenes as S  # noqa: E402
from mvsdet_amd import functional as F_  # noqa: E402
from mvsdet_amd.ops import adapter, photo, splat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
args = ap.parse_args()
dev = torch.device("cuda:0")
NAMES = ("means", "covs", "sh", "opac")
lines = []


def to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def digest(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    lines.append(f"{name} | {h.hexdigest()[:32]}")
    print(lines[-1], flush=True)


def under_autograd(name, fn, leaves, n_out):
    """fn(*leaves) -> outputs, the first n_out of them differentiable; digest of the outputs and of d sum_i <out_i, w_i> / d leaves.
    The workspace (uint8) is left out: its padding and the sort's scratch are whatever the allocation held."""
    leaves = [t.detach().requires_grad_(True) for t in leaves]
    out = fn(*leaves)
    out = tuple(o for o in (out if isinstance(out, tuple) else (out,)) if o.dtype != torch.uint8)
    gen = torch.Generator().manual_seed(7)
    sum((o * torch.randn(o.shape, generator=gen).to(dev)).sum() for o in out[:n_out]).backward()
    digest(name, *out, *[t.grad for t in leaves])


def strided(t):
    """The same values as a view with no unit stride: every second element along every axis of a buffer twice the size."""
    wide = torch.zeros([2 * n for n in t.shape], dtype=t.dtype, device=t.device)
    view = wide[tuple(slice(None, None, 2) for _ in t.shape)]
    view.copy_(t)
    return view


def rasteriser(tag, sc, use_sh=True, wrap=lambda t: t):
    means, covs, sh, opac = (wrap(to(sc[k])) for k in NAMES)
    near, far, bg = to(sc["near"]), to(sc["far"]), to(sc["bg"])
    cams = splat.splat_cameras(to(sc["extrinsics"]), to(sc["intrinsics"]), near, far, bool(sc["scale_invariant"]))
    H, W, keys = sc["H"], sc["W"], splat.default_max_keys(sc["G"])
    under_autograd(f"rasterize {tag}", lambda m, c, s, o: splat.rasterize(m, c, s, o, cams, bg, H, W, keys, use_sh), (means, covs, sh, opac), 1)
    for mode in splat.DEPTH_MODES:
        under_autograd(f"rasterize_depth {mode} {tag}",
                       lambda m, c, s, o: splat.rasterize_depth(m, c, s, o, cams, near, far, bg, H, W, keys, use_sh, mode),
                       (means, covs, sh, opac), 2)
        under_autograd(f"depth_only {mode} {tag}", lambda m, c, o: splat.depth_only(m, c, o, cams, near, far, H, W, keys, mode),
                       (means, covs, opac), 1)


first = S.scene(seed=1)
rasteriser("scene1", first)
rasteriser("list65", S.EDGES["list65"]())
rasteriser("small17x16", S.small_image(17, 16))
rasteriser("bits3x16x16", S.bit_scene(3, 16, 16))
rasteriser("precomputed", S.scene(seed=2, G=96, d_sh=1), use_sh=False)
rasteriser("scene1 strided", first, wrap=strided)

# ---- functional: expanded rows (one call over the views) and B = 2 distinct rows (one call per row)
second = S.scene(seed=3)
E, K, near, far, bg = (to(first[k]) for k in ("extrinsics", "intrinsics", "near", "far", "bg"))
hw, V = (first["H"], first["W"]), first["V"]
one = [to(first[k]) for k in NAMES]
ROWS = {"expanded": lambda t, k: t[None].expand(V, *t.shape), "distinct": lambda t, k: torch.stack([t, to(second[k])])}
for tag, rows in ROWS.items():
    under_autograd(f"render_cuda {tag}", lambda *ts: F_.render_cuda(E, K, near, far, hw, bg, *[rows(t, k) for t, k in zip(ts, NAMES)]), one, 1)
    for mode in ("depth", "relative_disparity"):
        under_autograd(f"render_depth_cuda {mode} {tag}",
                       lambda m, c, o: F_.render_depth_cuda(E, K, near, far, hw, rows(m, "means"), rows(c, "covs"), rows(o, "opac"), mode=mode),
                       (one[0], one[1], one[3]), 1)
for tag, sets in (("b1", [first]), ("b2", [first, second])):
    stack = lambda k: torch.stack([to(sc[k]) for sc in sets])  # noqa: E731
    cameras = [stack(k) for k in ("extrinsics", "intrinsics", "near", "far")]
    for mode in (None, "depth", "disparity"):
        under_autograd(f"decode_splatting depth_mode={mode} {tag}",
                       lambda m, c, s, o: F_.decode_splatting(types.SimpleNamespace(means=m, covariances=c, harmonics=s, opacities=o), *cameras,
                                                              hw, bg[0], depth_mode=mode),
                       [stack(k) for k in NAMES], 1 if mode is None else 2)

# ---- cameras
cam3 = S.scene(seed=5, G=8, V=3)
E3, K3, n3, f3 = (to(cam3[k]) for k in ("extrinsics", "intrinsics", "near", "far"))
for si in (False, True):
    digest(f"splat_cameras scale_invariant={si} V=3", splat.splat_cameras(E3, K3, n3, f3, si))
for L in range(5):
    digest(f"adapter_cameras sh_degree={L} V=3", adapter.adapter_cameras(E3, K3, 5, 7, L))
g25 = np.load(os.path.join(ROOT, "tests", "golden", "g25_photo_loss.npz"))
c = PR.g25_case(g25, PR.SINGLE_CASES[0])
left, right = to(c["left_cam"]), to(c["right_cam"])
digest(f"photo_geometry g25 {PR.SINGLE_CASES[0]}", photo.photo_geometry(left[:, 0], left[:, 1], right[:, 0], None, None))
torch.cuda.synchronize()
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
