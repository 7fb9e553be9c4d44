#!/usr/bin/env python3
"""Generate tests/golden/g28_splat_depth.npz by RUNNING THE REFERENCE's render_depth_cuda on the CPU (build container only: needs the
reference tree).

G28: what gs_src/model/decoder/cuda_splatting.py::render_depth_cuda, unmodified, hands the rasteriser it imports -- through its own
render_cuda -- in the four modes.  The module is loaded as make_goldens_g26.py loads it (its loader and its recording stand-in for
`diff_gaussian_rasterization` are used as they are).

Cases: G26's `single_k` (3 views, scale_invariant) and `plain` (2 views, scale_invariant=False), the same seeded scenes.
Stored per case: the inputs and the float64 restatement's cull mask; per case and mode: `colors_precomp` per view (V,G,3) as handed
over (the three channels are equal), whether `shs` was None, and `own`: the largest distance of the reference's fp32 value from a
float64 evaluation of the same formulas (tests/splat_depth_restated.py::fake_colour) over the Gaussians that are not culled --
printed here; the tests' bars are 4 x these.  Data only.

    python tests/golden/make_goldens_g28.py [reference root]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_goldens_g26 as G26  # noqa: E402
import splat_depth_restated as D  # noqa: E402
import splat_scenes as S  # noqa: E402
from _ref_loader import REF_ROOT  # noqa: E402

CASES = ("single_k", "plain")


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else REF_ROOT
    ref = G26.load_reference(root)
    out = {"cases": np.array(list(CASES)), "modes": np.array(list(D.MODES))}
    for tag in CASES:
        sc = S.scene(**G26.CASES[tag])
        V, G, H, W = sc["V"], sc["G"], sc["H"], sc["W"]
        si = sc["scale_invariant"]
        rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[None], (V,) + a.shape))  # noqa: E731
        inputs = dict(extrinsics=sc["extrinsics"], intrinsics=sc["intrinsics"], near=sc["near"], far=sc["far"], means=sc["means"],
                      covs=sc["covs"], opac=sc["opac"])
        for k, v in inputs.items():
            out[f"{tag}.{k}"] = v
        out[f"{tag}.image_shape"] = np.array([H, W], np.int32)
        out[f"{tag}.scale_invariant"] = np.bool_(si)
        visible = S.visible(sc)
        out[f"{tag}.visible"] = visible
        t = {k: torch.from_numpy(v) for k, v in inputs.items()}
        for mode in D.MODES:
            del G26.CALLS[:]
            depth = ref.render_depth_cuda(t["extrinsics"], t["intrinsics"], t["near"], t["far"], (H, W), torch.from_numpy(rep(sc["means"])),
                                          torch.from_numpy(rep(sc["covs"])), torch.from_numpy(rep(sc["opac"])), scale_invariant=si, mode=mode)
            assert tuple(depth.shape) == (V, H, W) and len(G26.CALLS) == V
            handed = np.stack([c["colors_precomp"].numpy() for _, c in G26.CALLS])
            assert handed.shape == (V, G, 3) and handed.dtype == np.float32
            assert np.array_equal(handed[..., 0], handed[..., 1]) and np.array_equal(handed[..., 0], handed[..., 2])
            shs_none = all(c["shs"] is None for _, c in G26.CALLS)
            want = D.fake_colour(torch.from_numpy(sc["means"]), sc["extrinsics"], sc["near"], sc["far"], mode, torch.float64).numpy()
            own = float(np.abs(handed[..., 0].astype(np.float64) - want)[visible].max())
            print(f"{tag} {mode}: reference fp32 - float64 {own:.3g} (largest value {np.abs(want[visible]).max():.3g}), shs is None: {shs_none}")
            out[f"{tag}.{mode}.colors_precomp"] = handed
            out[f"{tag}.{mode}.shs_none"] = np.bool_(shs_none)
            out[f"{tag}.{mode}.own"] = np.float64(own)
    path = os.path.join(HERE, "g28_splat_depth.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
