"""What every stage's bindings share: the library stub (`_lib`), the operator namespace and the input checks."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib  # noqa: F401  (the stage modules import it from here)

_NS = "mvsdet_amd"


def req(t: Tensor, name: str, dtype=torch.float32, dim=None):
    if not t.is_cuda:
        raise RuntimeError(f"mvsdet_amd: `{name}` must live on a ROCm device (got {t.device}); "
                           "this package has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"mvsdet_amd: `{name}` must be {dtype} (got {t.dtype})")
    if dim is not None and t.dim() != dim:
        raise ValueError(f"mvsdet_amd: `{name}` must be {dim}-D (got shape {tuple(t.shape)})")


def camera_inputs(name: str, extrinsics: Tensor, intrinsics: Tensor):
    """What the one-thread-per-view camera kernels take: extrinsics (V,4,4) as rows of 4 adjacent floats, intrinsics (V,3,3) with unit
    stride inside a row (a copy where the caller's view is laid out otherwise) -> (extrinsics, intrinsics, V, the three element
    strides of the C entries: extrinsics view, intrinsics view, intrinsics row).  `ops.photo.photo_geometry` does not come through
    here: its cameras have 3 or 4 rows and its intrinsics may be one matrix for all views."""
    req(extrinsics, "extrinsics", dim=3)
    req(intrinsics, "intrinsics", dim=3)
    V = extrinsics.shape[0]
    if tuple(extrinsics.shape[1:]) != (4, 4) or tuple(intrinsics.shape) != (V, 3, 3) or V < 1:
        raise ValueError(f"{name}: extrinsics {tuple(extrinsics.shape)} and intrinsics {tuple(intrinsics.shape)} must be (V,4,4) and "
                         "(V,3,3)")
    if extrinsics.stride(2) != 1 or extrinsics.stride(1) != 4:
        extrinsics = extrinsics.contiguous()
    if intrinsics.stride(2) != 1:
        intrinsics = intrinsics.contiguous()
    return extrinsics, intrinsics, V, (extrinsics.stride(0), intrinsics.stride(0), intrinsics.stride(1))


def stream(t: Tensor):
    return _lib.current_stream(t.device)


def to_device(t: Tensor, dev) -> Tensor:
    """A host tensor through pinned memory (no host synchronisation); a device tensor as it is."""
    return t.to(dev) if t.is_cuda else t.pin_memory().to(dev, non_blocking=True)
