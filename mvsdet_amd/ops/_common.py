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


def stream(t: Tensor):
    return _lib.current_stream(t.device)


def to_device(t: Tensor, dev) -> Tensor:
    """A host tensor through pinned memory (no host synchronisation); a device tensor as it is."""
    return t.to(dev) if t.is_cuda else t.pin_memory().to(dev, non_blocking=True)
