#!/usr/bin/env python3
"""Generate tests/golden/g27_adapter.npz by RUNNING THE REFERENCE's GaussianAdapter.forward on the CPU (build container only: needs the
reference tree).

G27: what gs_src/model/encoder/common/gaussian_adapter.py::GaussianAdapter.forward, unmodified, returns for the call extract_feat
makes (mvsdet.py:586-596).  The module is loaded from the reference tree under its own package name with empty parent packages, a
stand-in for `jaxtyping` (annotations only) and a RECORDING stand-in for `gs_src.misc.sh_rotation`, written here: its rotate_sh returns
its input and keeps the rotations it was given (the real one needs e3nn, which is not installed; so the fixture pins everything BUT the
rotation of the harmonics -- the stored harmonics are the masked coefficients, i.e. identity blocks).  geometry/projection.py and
encoder/common/gaussians.py are the reference's own files.

RESTATED here (flagged in the metadata as `restated_offset_lines`): the three offset lines mvsdet.py:576-578, which are inline in
extract_feat, around the reference's own sample_image_grid; and the rearranges of :587-594 / :615-632.  The adapter broadcasts the
harmonics to the shape of the opacities (:78), so for S = 2 the opacities go in repeated over the surfaces.

Cases (tests/adapter_restated.py::case; h x w = 5 x 7):
  shared_k    3 views that share one K, S = 1, d_sh 25
  per_view_k  2 views with their own K, S = 2, d_sh 25
  sh1         2 views, S = 1, d_sh 1
Stored per case: the inputs, every field of the returned Gaussians flattened to (v, r, s) order, the rotations rotate_sh was handed,
and `own_<field>`: the largest distance of the reference's fp32 field from the float64 restatement (tests/adapter_restated.py) --
printed here; the tests' bars on the kernel are 4 x these or the project's bar, whichever is larger.

    python tests/golden/make_goldens_g27.py [reference root]
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import adapter_restated as A  # noqa: E402
from _ref_loader import REF_ROOT  # noqa: E402

CASES = {
    "shared_k": dict(seed=271, V=3, h=5, w=7, S=1, d_sh=25, shared_k=True),
    "per_view_k": dict(seed=272, V=2, h=5, w=7, S=2, d_sh=25),
    "sh1": dict(seed=273, V=2, h=5, w=7, S=1, d_sh=1),
}
HANDED = []


class _Annotation:
    def __getitem__(self, item):      # Float[Tensor, "batch 3"] -> Tensor
        return item[0] if isinstance(item, tuple) else item


def rotate_sh(sh_coefficients, rotations):
    HANDED.append(rotations.detach().clone())
    return sh_coefficients


def load_reference(root):
    def package(name):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod

    def source(name, *path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, *path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    jax = types.ModuleType("jaxtyping")
    for n in ("Float", "Bool", "Int64"):
        setattr(jax, n, _Annotation())
    sys.modules["jaxtyping"] = jax
    for name in ("gs_src", "gs_src.geometry", "gs_src.misc", "gs_src.model", "gs_src.model.encoder", "gs_src.model.encoder.common"):
        package(name)
    rot = types.ModuleType("gs_src.misc.sh_rotation")
    rot.rotate_sh = rotate_sh
    sys.modules["gs_src.misc.sh_rotation"] = rot
    proj = source("gs_src.geometry.projection", "gs_src", "geometry", "projection.py")
    source("gs_src.model.encoder.common.gaussians", "gs_src", "model", "encoder", "common", "gaussians.py")
    return proj, source("gs_src.model.encoder.common.gaussian_adapter", "gs_src", "model", "encoder", "common", "gaussian_adapter.py")


def main():
    from einops import rearrange
    root = sys.argv[1] if len(sys.argv) > 1 else REF_ROOT
    proj, ref = load_reference(root)
    out = {"cases": np.array(list(CASES)), "restated_offset_lines": np.array("mvsdet.py:576-578 and the rearranges of :587-594, :615-632")}
    for tag, kw in CASES.items():
        c = A.case(**kw)
        V, h, w, S, d_sh = c["V"], c["h"], c["w"], c["S"], c["d_sh"]
        adapter = ref.GaussianAdapter(ref.GaussianAdapterCfg(gaussian_scale_min=c["s_min"], gaussian_scale_max=c["s_max"],
                                                             sh_degree=A.degree_of(d_sh)))
        t = {k: torch.from_numpy(c[k]) for k in ("extrinsics", "intrinsics", "raw", "depth", "opacity")}
        gaussians = t["raw"][None]                                                   # (1, V, R, S, 2 + d_in)
        # --- restated: mvsdet.py:539-540, 576-578
        xy_ray, _ = proj.sample_image_grid((h, w))
        xy_ray = rearrange(xy_ray, "h w xy -> (h w) () xy")
        offset_xy = gaussians[..., :2].sigmoid()
        pixel_size = 1 / torch.tensor((w, h), dtype=torch.float32)
        xy_ray = xy_ray + (offset_xy - 0.5) * pixel_size
        # --- the reference's call, :586-596
        del HANDED[:]
        g = adapter.forward(rearrange(t["extrinsics"][None], "b v i j -> b v () () () i j"),
                            rearrange(t["intrinsics"][None], "b v i j -> b v () () () i j"),
                            rearrange(xy_ray, "b v r srf xy -> b v r srf () xy"),
                            t["depth"][None, :, :, None, None], t["opacity"][None, :, :, None, None].expand(1, V, h * w, S, 1),
                            rearrange(gaussians[..., 2:], "b v r srf c -> b v r srf () c"), (h, w))
        assert len(HANDED) == 1
        G = V * h * w * S
        rec = dict(means=g.means.reshape(G, 3), covariances=g.covariances.reshape(G, 3, 3), harmonics=g.harmonics.reshape(G, 3, d_sh),
                   opacities=g.opacities.expand(1, V, h * w, S, 1).reshape(G), scales=g.scales.reshape(G, 3),
                   rotations=g.rotations.reshape(G, 4))
        rec = {k: v.detach().numpy().astype(np.float32) for k, v in rec.items()}
        handed = HANDED[0].numpy()
        assert handed.shape[-2:] == (3, 3) and np.array_equal(handed.reshape(V, 3, 3), c["extrinsics"][:, :3, :3])
        identity = np.zeros((V, A.ROT_OFF[A.degree_of(d_sh) + 1]))
        for l in range(A.degree_of(d_sh) + 1):
            identity[:, A.ROT_OFF[l]:A.ROT_OFF[l + 1]] = np.eye(2 * l + 1).reshape(-1)
        o64, _ = A.restate(c, identity, torch.float64)
        for name, got in rec.items():
            own = float(np.abs(got.astype(np.float64) - o64[name]).max())
            print(f"{tag}: {name} reference fp32 - float64 restatement {own:.3g} (largest entry {np.abs(o64[name]).max():.3g})")
            out[f"{tag}.own_{name}"] = np.float64(own)
            out[f"{tag}.{name}"] = got
        for k in ("extrinsics", "intrinsics", "raw", "depth", "opacity"):
            out[f"{tag}.in_{k}"] = c[k]
        out[f"{tag}.handed_rotations"] = handed.reshape(V, 3, 3).astype(np.float32)
        out[f"{tag}.shape"] = np.array([V, h, w, S, d_sh], np.int32)
        out[f"{tag}.scale_range"] = np.array([c["s_min"], c["s_max"]], np.float32)
    path = os.path.join(HERE, "g27_adapter.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
