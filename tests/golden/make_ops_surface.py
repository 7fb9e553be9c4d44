"""The public surface of mvsdet_amd.ops as data: run on a checkout of the commit whose surface is to be kept,

    python tests/golden/make_ops_surface.py [path/to/ops_surface.json]

and commit the file; tests/test_ops_surface.py recomputes `surface()` from the package under test and compares.  Needs the
built library (the sweep's table-sizing fakes call its host-only size function) but no GPU.
"""
import inspect
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the sweep family at N=3, K=2, C=32, D=4, H=8, W=48, w_pitch=64, n_src=3, ref_first=0
N, K, C, D, H, W, PITCH = 3, 2, 32, 4, 8, 48, 64


def _describe(name, obj):
    """(kind, description) of a public name, or None for what is not the package's own (imported modules, typing names)."""
    import torch
    if isinstance(obj, torch.library.CustomOpDef):
        return "op", str(obj._opoverload._schema)
    if isinstance(obj, type) and issubclass(obj, tuple) and hasattr(obj, "_fields"):
        return "namedtuple", list(obj._fields)
    own = str(getattr(obj, "__module__", "")).startswith("mvsdet_amd.ops")
    if isinstance(obj, type):
        return ("class", str(inspect.signature(obj))) if own else None
    if inspect.isfunction(obj):
        return ("function", str(inspect.signature(obj))) if own else None
    if isinstance(obj, tuple) and obj and all(isinstance(o, torch.library.CustomOpDef) for o in obj):
        return "ops", [o._qualname for o in obj]
    if isinstance(obj, (bool, int, float, str, tuple, list, dict)):
        return "constant", repr(obj)
    return None


def _sweep_fakes(ops):
    """name -> [[shape, dtype], ...] of every output of the sweep family's fake kernels."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode

    out = {}

    def put(name, res):
        res = res if isinstance(res, (tuple, list)) else (res,)
        out[name] = [[list(t.shape), str(t.dtype)] for t in res]

    with FakeTensorMode():
        def f(*shape, dtype=torch.float32):
            return torch.empty(shape, dtype=dtype, device="cuda")

        feat, nbr, proj, depth = f(N, C, H, W), f(N, K, dtype=torch.int64), f(N, K, 4, 4), f(N, D)
        src, proj1, depth_px, grad = f(N, C, H, W), f(N, 4, 4), f(N, D, H, W), f(N, C, D, H, W)
        put("pack_features", ops.pack_features(feat))
        put("pack_features[f16]", ops.pack_features(f(N, C, H, W, dtype=torch.float16)))
        packed = ops.pack_features(feat)
        put("homo_warp", ops.homo_warp(src, proj1, depth))
        put("plane_sweep_variance", ops.plane_sweep_variance(feat, nbr, proj, depth))
        put("plane_sweep_variance_packed", ops.plane_sweep_variance_packed(packed, nbr, proj, depth, C, H, W))
        for half in (False, True):
            put(f"plane_sweep_variance_shard[half_out={half}]",
                ops.plane_sweep_variance_shard(packed, nbr, proj, depth, N, 0, C, H, W, half))
        put("plane_sweep_variance_keep", ops.plane_sweep_variance_keep(feat, nbr, proj, depth))
        put("plane_sweep_variance_backward", ops.plane_sweep_variance_backward(feat, nbr, proj, depth, grad))
        table = ops.plane_sweep_table(proj, depth, H, W)
        put("plane_sweep_table", table)
        put("plane_sweep_table_pooled", ops.plane_sweep_table_pooled(proj, depth, H, W))
        put("plane_sweep_table_pooled[w_pitch]", ops.plane_sweep_table_pooled(proj, depth, H, W, PITCH))
        put("plane_sweep_variance_backward_packed", ops.plane_sweep_variance_backward_packed(packed, nbr, table, grad))
        put("plane_sweep_variance_tabled", ops.plane_sweep_variance_tabled(packed, nbr, table, C, D, H, W))
        put("homo_warp_pixel", ops.homo_warp_pixel(src, proj1, depth_px))
        put("homo_warp_pixel_backward", ops.homo_warp_pixel_backward(proj1, depth_px, grad))
        put("plane_sweep_variance_pixel", ops.plane_sweep_variance_pixel(feat, nbr, proj, depth_px))
        put("plane_sweep_variance_pixel_packed", ops.plane_sweep_variance_pixel_packed(packed, nbr, proj, depth_px, C))
        put("plane_sweep_variance_pixel_backward", ops.plane_sweep_variance_pixel_backward(feat, nbr, proj, depth_px, grad))
    return out


def surface():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from mvsdet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    from mvsdet_amd import ops
    names, autocast = {}, {}
    for name, obj in sorted(vars(ops).items()):
        if name.startswith("_") or isinstance(obj, types.ModuleType):
            continue
        d = _describe(name, obj)
        if d is None:
            continue
        if d[0] == "ops":
            autocast[name] = d[1]
        else:
            names[name] = {"kind": d[0], "is": d[1]}
    return {"names": names, "autocast": autocast, "sweep_fakes": _sweep_fakes(ops)}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ops_surface.json")
    with open(path, "w") as fh:
        json.dump(surface(), fh, indent=1, sort_keys=True)
        fh.write("\n")
