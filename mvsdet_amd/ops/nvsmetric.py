"""The reference's view-synthesis scores (save_rendered_img_Image / save_rendered_depth of nerf_utils/save_rendered_img.py, averaged as
NVSMetric) on csrc/nvsmetric.hip: nvs_score scores one scene's target views (two launches: tiles, finish) on the current stream
without a host synchronisation and adds the scene to an accumulator state; everything after the load is float64.  CPU tensors take
the same expressions in torch float64 (`F.avg_pool2d(t.double(), 7, 1)` is exactly the windows that lie inside the image), so what
stands above the kernel can be exercised without a device.  mvsdet_amd.evaluation builds NVSMetric's dict from the state."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from ._common import _lib, stream
from .._lib import strides3, strides4

NVS_STATE_DOUBLES = 4    # MVSDET_NVS_STATE_DOUBLES: sums of the scenes' psnr, ssim, rmse; scenes
NVS_WINDOW = 7           # skimage's default win_size
NVS_TILE_W, NVS_TILE_H = 32, 16   # window centres of one block's tile (kTW, kTH of csrc/nvsmetric.hip); the tests build their shapes on it


def nvs_state(device) -> Tensor:
    """A cleared accumulator state on `device` (a ROCm device or the CPU): (4) float64."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.empty(NVS_STATE_DOUBLES, dtype=torch.float64, device=dev)
    nvs_reset(st)
    return st


def _check_state(st: Tensor, what: str) -> None:
    if st.dtype != torch.float64 or tuple(st.shape) != (NVS_STATE_DOUBLES,) or not st.is_contiguous():
        raise ValueError(f"{what}: the state is a contiguous ({NVS_STATE_DOUBLES},) float64 tensor (got {tuple(st.shape)} {st.dtype})")


def nvs_reset(st: Tensor) -> None:
    _check_state(st, "nvs_reset")
    if not st.is_cuda:
        st.zero_()
        return
    with torch.cuda.device(st.device):
        _lib.check(_lib.load().mvsdet_nvs_reset(_lib.ptr(st), stream(st)), "nvs_reset")


def workspace_bytes(n_tgt: int, H: int, W: int, with_depth: bool = True) -> int:
    """Bytes of nvs_score's workspace (mvsdet_nvs_workspace_bytes); 0 for sizes it does not take."""
    return int(_lib.load().mvsdet_nvs_workspace_bytes(int(n_tgt), int(H), int(W), int(bool(with_depth))))


def _fp32(name: str, *tensors):
    from ..functional import amp_fp32
    out = amp_fp32(*tensors)
    out = out if isinstance(out, tuple) else (out,)
    for t in out:
        if not isinstance(t, Tensor) or not t.is_floating_point():
            raise TypeError(f"{name}: floating-point tensors needed (got {getattr(t, 'dtype', type(t).__name__)})")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: float32 needed (got {t.dtype}; float16 / bfloat16 are cast under torch.autocast only)")
    return out


def _check_pair(name: str, a: Tensor, b: Tensor, dim: int, what: str) -> None:
    if a.dim() != dim or tuple(a.shape) != tuple(b.shape) or (dim == 4 and a.shape[1] != 3):
        raise ValueError(f"{name}: {what} {tuple(a.shape)} against {tuple(b.shape)}: two equal "
                         f"{'(n_tgt,3,H,W)' if dim == 4 else '(n_tgt,H,W)'} shapes needed")
    if a.device != b.device:
        raise RuntimeError(f"{name}: {what} on {a.device} and {b.device}")
    n, H, W = int(a.shape[0]), int(a.shape[-2]), int(a.shape[-1])
    if n < 1:
        raise ValueError(f"{name}: no target view in {tuple(a.shape)}")
    if H < NVS_WINDOW or W < NVS_WINDOW:
        raise ValueError(f"{name}: {H}x{W} views; the {NVS_WINDOW}x{NVS_WINDOW} window needs sides of {NVS_WINDOW} "
                         "(skimage: win_size exceeds image extent)")
    if n * 3 * H * W >= 1 << 31:
        raise ValueError(f"{name}: {n} views of {H}x{W}: n_tgt * 3 * H * W must stay below 2^31")


def _score_host(pred: Optional[Tensor], gt: Optional[Tensor], pred_depth: Optional[Tensor], gt_depth: Optional[Tensor]):
    """The kernel's expressions in torch float64 on the inputs' device (the CPU route)."""
    ref = pred if pred is not None else pred_depth
    n = int(ref.shape[0])
    per_view = torch.zeros((n, 2), dtype=torch.float64, device=ref.device)
    scene = torch.zeros(3, dtype=torch.float64, device=ref.device)
    if pred is not None:
        x, y = pred.double(), gt.double()
        mse = ((x - y) ** 2).reshape(n, -1).mean(dim=1)
        per_view[:, 0] = -10.0 * torch.log(mse) / math.log(10.0)
        u = lambda t: F.avg_pool2d(t, NVS_WINDOW, 1)   # noqa: E731
        ux, uy, uxx, uyy, uxy = u(x), u(y), u(x * x), u(y * y), u(x * y)
        cov_norm, C1, C2 = 49.0 / 48.0, (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        per_view[:, 1] = S.mean(dim=(2, 3)).mean(dim=1)
        scene[0], scene[1] = per_view[:, 0].sum() / n, per_view[:, 1].sum() / n
    if pred_depth is not None:
        scene[2] = ((pred_depth.double() - gt_depth.double()) ** 2).reshape(n, -1).mean(dim=1).sum() / n
    return per_view, scene


def nvs_score(st: Optional[Tensor], pred: Optional[Tensor], gt: Optional[Tensor], pred_depth: Optional[Tensor] = None,
              gt_depth: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """One scene: pred, gt (n_tgt,3,H,W) in [0,1] with any strides (a permuted (n_tgt,H,W,3) view and a window of a wider buffer are
    read in place), pred_depth, gt_depth (n_tgt,H,W) or None -> (per_view (n_tgt,2) float64 = psnr and ssim of every view, scene (3)
    float64 = their means and the depth error: the mean over views of mean((pred_depth - gt_depth)^2), 0 without a depth pair).  With
    a state the scene is added to it.  pred = gt = None scores a depth pair alone (per_view and the first two of scene stay 0; no
    state).  No host synchronisation."""
    if (pred is None) != (gt is None) or (pred_depth is None) != (gt_depth is None) or (pred is None and pred_depth is None):
        raise ValueError("nvs_score: an image pair, a depth pair or both are needed")
    if pred is not None:
        pred, gt = _fp32("nvs_score", pred, gt)
        _check_pair("nvs_score", pred, gt, 4, "render")
    elif st is not None:
        raise ValueError("nvs_score: a depth pair alone is not a scene of the state")
    if pred_depth is not None:
        pred_depth, gt_depth = _fp32("nvs_score", pred_depth, gt_depth)
        _check_pair("nvs_score", pred_depth, gt_depth, 3, "depth")
        if pred is not None and (pred_depth.device != pred.device or tuple(pred_depth.shape) != (pred.shape[0], *pred.shape[2:])):
            raise ValueError(f"nvs_score: depth {tuple(pred_depth.shape)} on {pred_depth.device} beside renders {tuple(pred.shape)} on "
                             f"{pred.device}")
    ref = pred if pred is not None else pred_depth
    if st is not None:
        _check_state(st, "nvs_score")
        if st.device != ref.device:
            raise RuntimeError(f"nvs_score: inputs on {ref.device}, the state on {st.device}")
    detached = [None if t is None else t.detach() for t in (pred, gt, pred_depth, gt_depth)]
    if not ref.is_cuda:
        per_view, scene = _score_host(*detached)
        if st is not None:
            st[:3] += scene
            st[3] += 1.0
        return per_view, scene
    pred, gt, pred_depth, gt_depth = detached
    n, H, W = int(ref.shape[0]), int(ref.shape[-2]), int(ref.shape[-1])
    dev = ref.device
    per_view = torch.zeros((n, 2), dtype=torch.float64, device=dev) if pred is None else torch.empty((n, 2), dtype=torch.float64, device=dev)
    scene = torch.empty(3, dtype=torch.float64, device=dev)
    ws = torch.empty(workspace_bytes(n, H, W, pred_depth is not None) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mvsdet_nvs_score_f32(
            _lib.ptr(st), _lib.ptr(pred), None if pred is None else strides4(pred), _lib.ptr(gt), None if gt is None else strides4(gt),
            _lib.ptr(pred_depth), None if pred_depth is None else strides3(pred_depth), _lib.ptr(gt_depth),
            None if gt_depth is None else strides3(gt_depth), n, H, W, _lib.ptr(per_view), _lib.ptr(scene), _lib.ptr(ws), ws.numel() * 8,
            stream(ref)), "nvs_score")
    return per_view, scene


def nvs_result(st: Tensor) -> Tensor:
    """(3) float64 on the state's device: NVSMetric's psnr, ssim, rmse = the means over the scenes fed (NaN before the first).  No
    host synchronisation."""
    _check_state(st, "nvs_result")
    return st[:3] / st[3]
