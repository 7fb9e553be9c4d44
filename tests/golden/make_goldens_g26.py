#!/usr/bin/env python3
"""Generate tests/golden/g26_splat.npz by RUNNING THE REFERENCE's render_cuda on the CPU (build container only: needs the reference tree).

G26: what gs_src/model/decoder/cuda_splatting.py::render_cuda, unmodified, hands the rasteriser it imports.  The module is loaded
from the reference tree under its own package name with empty parent packages, a stand-in for `jaxtyping` (annotations only) and a
RECORDING stand-in for `diff_gaussian_rasterization`, written here: its settings class keeps the fields, its rasteriser keeps the
call's tensors and returns zeros.  geometry/projection.py (get_fov) and encoder/epipolar/conversions.py are the reference's own files.

Cases (scenes of tests/splat_scenes.py: every Gaussian-level decision decided; G = 64, image 24x32):
  single_k   3 views that share one normalised K (ScanNet-like), d_sh 4, scale_invariant
  per_view_k 2 views with their own non-square K, d_sh 25, scale_invariant
  plain      2 views, d_sh 1, scale_invariant=False
Stored per case: the inputs, and per view viewmatrix, projmatrix, (tanfovx, tanfovy), campos, degree, the scaled means and the
6-vector covariances as handed over; `own_*`: the largest distance of the reference's fp32 matrices from a float64 evaluation of the
same formulas (tests/splat_restated.py::cameras) -- printed here; the tests' bars on our camera kernel are 4 x these.

    python tests/golden/make_goldens_g26.py [reference root]
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

import splat_restated as R  # noqa: E402
import splat_scenes as S  # noqa: E402
from _ref_loader import REF_ROOT  # noqa: E402

CASES = {
    "single_k": dict(seed=261, G=64, V=3, H=24, W=32, d_sh=4, shared_k=True),
    "per_view_k": dict(seed=262, G=64, V=2, H=24, W=32, d_sh=25),
    "plain": dict(seed=263, G=64, V=2, H=24, W=32, d_sh=1, scale_invariant=False),
}
CALLS = []


class _Annotation:
    def __getitem__(self, item):      # Float[Tensor, "batch 3"] -> Tensor
        return item[0] if isinstance(item, tuple) else item


class GaussianRasterizationSettings:
    def __init__(self, **fields):
        self.__dict__.update(fields)


class GaussianRasterizer:
    def __init__(self, settings):
        self.settings = settings

    def __call__(self, **tensors):
        CALLS.append((self.settings, {k: (None if v is None else v.detach().clone()) for k, v in tensors.items()}))
        return (torch.zeros(3, self.settings.image_height, self.settings.image_width), torch.zeros(tensors["means3D"].shape[0], dtype=torch.int32))


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
    ext = types.ModuleType("diff_gaussian_rasterization")
    ext.GaussianRasterizationSettings, ext.GaussianRasterizer = GaussianRasterizationSettings, GaussianRasterizer
    sys.modules["diff_gaussian_rasterization"] = ext
    for name in ("gs_src", "gs_src.geometry", "gs_src.model", "gs_src.model.decoder", "gs_src.model.encoder", "gs_src.model.encoder.epipolar"):
        package(name)
    source("gs_src.geometry.projection", "gs_src", "geometry", "projection.py")
    source("gs_src.model.encoder.epipolar.conversions", "gs_src", "model", "encoder", "epipolar", "conversions.py")
    return source("gs_src.model.decoder.cuda_splatting", "gs_src", "model", "decoder", "cuda_splatting.py")


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else REF_ROOT
    ref = load_reference(root)
    out = {"cases": np.array(list(CASES))}
    for tag, kw in CASES.items():
        sc = S.scene(**kw)
        V, G, H, W = sc["V"], sc["G"], sc["H"], sc["W"]
        si = sc["scale_invariant"]
        rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[None], (V,) + a.shape))  # noqa: E731
        inputs = dict(extrinsics=sc["extrinsics"], intrinsics=sc["intrinsics"], near=sc["near"], far=sc["far"], bg=sc["bg"],
                      means=rep(sc["means"]), covs=rep(sc["covs"]), sh=rep(sc["sh"]), opac=rep(sc["opac"]))
        t = {k: torch.from_numpy(v) for k, v in inputs.items()}
        del CALLS[:]
        images = ref.render_cuda(t["extrinsics"], t["intrinsics"], t["near"], t["far"], (H, W), t["bg"], t["means"], t["covs"], t["sh"],
                                 t["opac"], scale_invariant=si)
        assert tuple(images.shape) == (V, 3, H, W) and len(CALLS) == V
        rec = dict(viewmatrix=np.stack([s.viewmatrix.numpy() for s, _ in CALLS]), projmatrix=np.stack([s.projmatrix.numpy() for s, _ in CALLS]),
                   tanfov=np.array([[s.tanfovx, s.tanfovy] for s, _ in CALLS], np.float32), campos=np.stack([s.campos.numpy() for s, _ in CALLS]),
                   handed_means=np.stack([c["means3D"].numpy() for _, c in CALLS]),
                   handed_cov6=np.stack([c["cov3D_precomp"].numpy() for _, c in CALLS]))
        degree = {s.sh_degree for s, _ in CALLS}
        assert len(degree) == 1 and all(c["shs"].shape == (G, sc["d_sh"], 3) and c["colors_precomp"] is None for _, c in CALLS)
        c64 = R.cameras(sc["extrinsics"], sc["intrinsics"], sc["near"], sc["far"], si, dtype=np.float64)
        exact = dict(viewmatrix=c64[:, :16].reshape(V, 4, 4), projmatrix=c64[:, 16:32].reshape(V, 4, 4), tanfov=c64[:, 32:34], campos=c64[:, 34:37])
        for name, want in exact.items():
            own = float(np.abs(rec[name].astype(np.float64) - want).max())
            print(f"{tag}: {name} reference fp32 - float64 {own:.3g} (largest entry {np.abs(want).max():.3g})")
            out[f"{tag}.own_{name}"] = np.float64(own)
        # the scaled means and covariances are single fp32 multiplications: our in-kernel products must be these bits
        s = c64[:, 37].astype(np.float32)
        assert np.array_equal(rec["handed_means"], inputs["means"] * s[:, None, None])
        iu = np.triu_indices(3)
        assert np.array_equal(rec["handed_cov6"], (inputs["covs"] * (s[:, None, None, None] ** 2))[:, :, iu[0], iu[1]])
        for k, v in dict(inputs, **rec).items():
            out[f"{tag}.{k}"] = v
        out[f"{tag}.degree"] = np.int32(degree.pop())
        out[f"{tag}.image_shape"] = np.array([H, W], np.int32)
        out[f"{tag}.scale_invariant"] = np.bool_(si)
    path = os.path.join(HERE, "g26_splat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
