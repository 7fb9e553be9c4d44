"""Host-side mirror of the reference's Python interface for the hot path.

Same names, argument order, shapes and return arity as projects/NeRF-Det/nerfdet/ of Pixie8888/MVSDet
(mvs_models/module.py and mvsdet.py; file:line cited per function), so the reference's call sites -- and
tests written against them -- read the same.  Heavy tensors go to the HIP operators of the ops package.

Geometry stays on the host.  The camera matrices of a scene are a few hundred floats that arrive as numpy
arrays in img_meta (mvsdet.py:419-420).  The sampling positions are sensitive to the rounding of the 4x4
inverse at the 1e-4 px level (DESIGN.md "tolerance budget"), so `relative_projection` evaluates
`src_proj @ inverse(ref_proj)` with the very ATen-CPU ops the reference uses (module.py:116) and ships the
result to the device; nothing per-pixel ever runs on the CPU.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import ops


# ------------------------------------------------------------------------------------------- geometry (host)
# Set by integration.patch_reference: homo_warping then returns a deferred volume (lazywarp.LazyVolume) instead of
# launching the warp kernel.  Off for direct callers of this module.
LAZY_WARP = False
LAZY_ANY_DEVICE = False   # tests only: defer on CPU tensors too (the fused launches are stubbed there)


# (neighbour projection tensor, reference projection tensor) -> proj_rel on the CPU, filled by `collect_proj_for_scene`:
# the patched MVSDet.collect_proj evaluates the k products of a scene ONCE, from one device-to-host copy of the cameras;
# `homo_warping` then finds its matrix by the identity of the two tensors it is handed (the entries keep them alive, so
# an id is never reused while it is in the table).
_SCENE_PROJ: dict = {}


def amp_fp32(*tensors):
    """`--amp` (tools/train.py:24-28; mmengine's AmpOptimWrapper = torch.autocast around the forward pass): while autocast is on,
    low-precision floating tensors become float32 -- the hot path computes in float32, as torch's own autocast rule for
    `grid_sampler` / `softmax` has the reference do at these very calls.  Outside autocast nothing is touched: a float16 tensor
    handed to the float32 operators then raises their TypeError (the fp16-storage sweep is a separate, explicit entry)."""
    if not torch.is_autocast_enabled("cuda"):
        return tensors if len(tensors) != 1 else tensors[0]
    out = tuple(t.float() if isinstance(t, Tensor) and t.is_floating_point() and t.dtype != torch.float32 else t for t in tensors)
    return out if len(out) != 1 else out[0]


def relative_projection(src_proj: Tensor, ref_proj: Tensor) -> Tensor:
    """module.py:116  proj = src_proj @ inverse(ref_proj), fp32, evaluated with ATen-CPU; result on CPU."""
    hit = _SCENE_PROJ.get((id(src_proj), id(ref_proj)))
    if hit is not None and hit[0] is src_proj and hit[1] is ref_proj:
        return hit[2]
    return torch.matmul(src_proj.detach().float().cpu(), torch.inverse(ref_proj.detach().float().cpu()))


def collect_proj_for_scene(w2c: Tensor, intr: Tensor, neighbor_ids: Tensor):
    """MVSDet.collect_proj (mvsdet.py:249-264) for the patched reference: same return values on the callers' device, and
    -- from ONE host copy of `w2c` / `intr` -- the k matrices `nei_proj @ inverse(ref_proj)` (module.py:116) that the k
    `homo_warping` calls of the scene will ask for, so those cost no further synchronisation and no repeated inverse."""
    dev = w2c.device
    w2c_h, intr_h, ids_h = w2c.detach().float().cpu(), intr.detach().float().cpu(), neighbor_ids.detach().cpu()
    proj_h, nei_h = collect_proj(w2c_h, intr_h, ids_h)
    inv_ref = torch.inverse(proj_h)
    proj = proj_h.to(dev, non_blocking=True) if dev.type != "cpu" else proj_h
    nei = tuple((n.to(dev, non_blocking=True) if dev.type != "cpu" else n) for n in nei_h)
    _SCENE_PROJ.clear()                      # one scene at a time: the reference's loop is sequential
    for n_dev, n_host in zip(nei, nei_h):
        _SCENE_PROJ[(id(n_dev), id(proj))] = (n_dev, proj, torch.matmul(n_host, inv_ref))
    return proj, nei


def knn(x: Tensor, ref: Tensor, k: int, maskself: bool = False) -> Tensor:
    """mvsdet.py:43-64.  x (B,3,Ns), ref (B,3,Nr) -> indices (B,Ns,k) of the k nearest `ref` columns
    (largest negative squared distance first)."""
    cross = -2 * torch.matmul(x.transpose(2, 1), ref)
    x_sq = torch.sum(x ** 2, dim=1, keepdim=True)
    r_sq = torch.sum(ref ** 2, dim=1, keepdim=True)
    neg_dist = -r_sq - cross - x_sq.transpose(2, 1)
    if maskself:
        if x.shape != ref.shape:
            raise AssertionError("maskself needs x and ref of the same shape")
        diag = torch.arange(x_sq.shape[2])
        neg_dist[:, diag, diag] = -100000
    return neg_dist.topk(k=k, dim=-1)[1]


def get_nearest_pose_ids(tar_pose: Tensor, ref_poses: Tensor, num_select: int, maskself: bool = False,
                         angular_dist_method: str = "dist", scene_center=(0, 0, 0)) -> Tensor:
    """mvsdet.py:67-104 ('dist' method, the only one the detector uses).  c2w poses (N,4,4) -> (N,k) int64."""
    if angular_dist_method != "dist":
        raise NotImplementedError("only angular_dist_method='dist' is on the MVSDet path (mvsdet.py:434)")
    num_select = min(num_select, len(ref_poses) - 1)
    tar = tar_pose[:, :3, 3].unsqueeze(0).transpose(2, 1)
    ref = ref_poses[:, :3, 3].unsqueeze(0).transpose(2, 1)
    ids = knn(tar, ref, k=num_select, maskself=maskself)[0]
    if LAZY_WARP:
        from . import lazywarp
        lazywarp.note_neighbor_ids(ids)
    return ids


def collect_proj(w2c: Tensor, intr: Tensor, neighbor_ids: Tensor):
    """MVSDet.collect_proj, mvsdet.py:249-264 -> (proj (N,4,4), tuple of k (N,4,4) neighbour projections)."""
    if intr.dim() == 2:
        intr = intr.unsqueeze(0).repeat(w2c.shape[0], 1, 1)
    proj = torch.matmul(intr, w2c)
    n, k = neighbor_ids.shape
    nei = proj[neighbor_ids.reshape(-1)].view(n, k, 4, 4)
    return proj, torch.unbind(nei, dim=1)


def get_points(n_voxels: Tensor, voxel_size: Tensor, origin: Tensor) -> Tensor:
    """mvsdet.py:1316-1327 -> voxel corner coordinates (3,X,Y,Z)."""
    with torch.no_grad():
        grid = torch.stack(torch.meshgrid([torch.arange(int(n_voxels[0])), torch.arange(int(n_voxels[1])),
                                           torch.arange(int(n_voxels[2]))], indexing="ij"))
        new_origin = origin - n_voxels / 2. * voxel_size
        return grid * voxel_size.view(3, 1, 1, 1) + new_origin.view(3, 1, 1, 1)


def compute_projection(img_meta: dict, stride: int, angles=None) -> Tensor:
    """MVSDet._compute_projection, mvsdet.py:1124-1156 (angles=None) -> (N,3,4) voxel->feature-pixel matrices."""
    if angles is not None:
        raise NotImplementedError("predicted-angle extrinsics (SUNRGBDTotal) are outside the MVSDet configs")
    ratio = img_meta["ori_shape"][0] / (img_meta["img_shape"][0] / stride)
    extr = torch.tensor(np.array(img_meta["lidar2img"]["extrinsic"]))
    intr = torch.tensor(np.array(img_meta["lidar2img"]["intrinsic"]))
    if intr.dim() == 2:  # ScanNet: one K per scene
        K = intr[:3, :3].clone()
        K[:2] /= ratio
        return torch.stack([K @ e[:3] for e in extr])
    K = intr[:, :3, :3].clone()  # ARKitScenes: one K per view
    K[:, :2] /= ratio
    return torch.stack([K[i] @ extr[i][:3] for i in range(len(extr))])


# ------------------------------------------------------------------------------------------- a3
def homo_warping(src_fea: Tensor, src_proj: Tensor, ref_proj: Tensor, depth_values: Tensor) -> Tensor:
    """mvs_models/module.py:105-146.  src_fea (B,C,H,W), src_proj/ref_proj (B,4,4), depth_values (B,D) -- one plane per
    hypothesis -- or (B,D,H,W) -- every reference pixel its own D hypotheses (module.py:130-133) -> warped (B,C,D,H,W)."""
    if depth_values.dim() not in (2, 4):
        raise ValueError(f"homo_warping: depth_values must be (B,D) or (B,D,H,W) (got shape {tuple(depth_values.shape)})")
    pixel = depth_values.dim() == 4
    if pixel and (src_fea.dim() != 4 or depth_values.shape[0] != src_fea.shape[0]
                  or tuple(depth_values.shape[2:]) != tuple(src_fea.shape[2:])):
        raise ValueError(f"homo_warping: per-pixel depth_values {tuple(depth_values.shape)} do not match src_fea "
                         f"{tuple(src_fea.shape)}: expected (B,D,H,W)")
    src_fea, depth_values = amp_fp32(src_fea, depth_values)
    proj = relative_projection(src_proj, ref_proj).to(src_fea.device)
    depth_values = depth_values.to(src_fea.device)
    if pixel:
        depth_values = depth_values.contiguous()
    if LAZY_WARP and (src_fea.is_cuda or LAZY_ANY_DEVICE) and src_fea.dtype == torch.float32:
        # inside the patched reference: defer, so that its variance loop collapses into the fused kernel (lazywarp.py)
        from . import lazywarp
        return lazywarp.lazy_homo_warp(src_fea, proj, depth_values)
    return ops.homo_warp_pixel(src_fea, proj, depth_values) if pixel else ops.homo_warp(src_fea, proj, depth_values)


def groupwise_correlation(feature: Tensor, neighbor_ids: Tensor, ref_proj: Tensor, nei_projs: Sequence[Tensor], depth_values: Tensor,
                          num_groups: int, reduce: str = "none") -> Tensor:
    """The group-wise correlation cost of mvs_models/lss_fpn.py:499-506 on this project's cameras: feature (N,C,H,W),
    neighbor_ids (N,K), ref_proj (N,4,4), nei_projs K x (N,4,4) (what `collect_proj` returns), depth_values (N,D) or (N,D,H,W)
    -> (N,K,G,D,H,W): per neighbour j and group g the mean over the group's C/G channels of feature x homo_warping(neighbour j).
    reduce="mean": the mean over the K neighbours, (N,G,D,H,W) -- what a group-wise-correlation network feeds its regulariser.
    One fused launch; differentiable in `feature`."""
    if reduce not in ("none", "mean"):
        raise ValueError(f"groupwise_correlation: reduce must be 'none' or 'mean' (got {reduce!r})")
    if depth_values.dim() not in (2, 4):
        raise ValueError(f"groupwise_correlation: depth_values must be (N,D) or (N,D,H,W) (got shape {tuple(depth_values.shape)})")
    if feature.dim() != 4 or depth_values.shape[0] != feature.shape[0] or (
            depth_values.dim() == 4 and tuple(depth_values.shape[2:]) != tuple(feature.shape[2:])):
        raise ValueError(f"groupwise_correlation: depth_values {tuple(depth_values.shape)} do not match feature {tuple(feature.shape)}")
    nei_projs = tuple(nei_projs)
    if neighbor_ids.dim() != 2 or len(nei_projs) != neighbor_ids.shape[1] or len(nei_projs) < 1:
        raise ValueError(f"groupwise_correlation: {len(nei_projs)} neighbour projections for neighbor_ids {tuple(neighbor_ids.shape)}")
    ops.sweep._check_groups("groupwise_correlation", feature.shape[1], int(num_groups))
    feature, depth_values = amp_fp32(feature, depth_values)
    dev = feature.device
    proj = torch.stack([relative_projection(p, ref_proj) for p in nei_projs], dim=1).to(dev)     # module.py:116 per neighbour
    corr = ops.sweep.plane_sweep_groupcorr(feature, neighbor_ids.to(dev), proj, depth_values.to(dev).contiguous(), int(num_groups))
    return corr.mean(dim=1) if reduce == "mean" else corr


# ------------------------------------------------------------------------------------------- a9
def depth_diagnostics(points: Tensor, projection: Tensor, est_depth: Tensor, est_dens: Tensor, depth_mean: Tensor,
                      gt_depth: Tensor, vz: float):
    """The gt_depth branch of backproject_Weigh (mvsdet.py:1435-1484) -> (gap_all, rmse, per_view (N,4), gt_resized (N,h,w)):
    0-dim fp32 tensors on the features' device and the per-view table {gap_i, orig_gap, new_gap, n_reduce}, one operator call,
    no host synchronisation.  gap_all is NaN where the reference raises (no view keeps a voxel: it divides by len([]))."""
    depth_mean, gt_depth = amp_fp32(depth_mean, gt_depth)
    dev = est_depth.device
    if gt_depth.device != dev:
        gt_depth = gt_depth.to(dev, non_blocking=True)
    if depth_mean.device != dev:
        depth_mean = depth_mean.to(dev, non_blocking=True)
    scalars, per_view, _, gt_resized = ops.depth_diagnostics(points, projection, est_depth, est_dens, depth_mean, gt_depth, vz)
    return scalars[0], scalars[1], per_view, gt_resized


def backproject_Weigh(features: Tensor, points: Tensor, projection: Tensor, depth: Tensor, voxel_size: Sequence[float],
                      prob: Tensor, gt_depth=None, save_dir=None, img_meta=None, depth_mean=None):
    """mvsdet.py:1372-1492.  features (N,C,h,w); points (3,X,Y,Z); projection (N,3,4);
    depth, prob (N, h*w, 1, J) -> (volume (N,C,X,Y,Z), valid (N,1,X,Y,Z) bool, gap_all, rmse).
    With gt_depth (N,Hg,Wg) and depth_mean (N,h,w) the last two are the reference's "weight_gap" and "src_rmse" as 0-dim tensors
    on the features' device (ops.depth_diagnostics); volume and valid do not depend on gt_depth.  Without it they are the
    reference's placeholders torch.tensor(1.)."""
    if gt_depth is not None:
        if save_dir is not None:
            raise NotImplementedError("backproject_Weigh: save_dir needs the reference's depth-image dumper (save_src_depth, "
                                      "mvsdet.py:1448-1453), which is outside the hot path; pass save_dir=None")
        if depth_mean is None:
            raise ValueError("backproject_Weigh: gt_depth needs depth_mean, the (N,h,w) depth expectation (mvsdet.py:1443)")
    features, points, projection, depth, prob = amp_fp32(features, points, projection, depth, prob)
    n, c, h, w = features.shape
    nx, ny, nz = points.shape[-3:]
    j = depth.shape[-1] * depth.shape[-2]
    # (N, h*w, 1, J) is a view of (N,J,h,w): hand the kernel that view, no copy (mvsdet.py:1393-1395)
    est_depth = depth.reshape(n, h, w, j).permute(0, 3, 1, 2)
    est_dens = prob.reshape(n, h, w, j).permute(0, 3, 1, 2)
    vz = float(voxel_size[-1])
    lazy = LAZY_WARP and (features.is_cuda or LAZY_ANY_DEVICE) and features.dtype == torch.float32
    if gt_depth is not None:
        # launched now on both routes: two scalars, nothing to defer (the lifting below stays deferred on the lazy route)
        if lazy:
            from . import lazywarp
            lazywarp.stats["diagnostics"] += 1
        gap_all, rmse = depth_diagnostics(points, projection, est_depth, est_dens, depth_mean, gt_depth, vz)[:2]
    else:
        gap_all, rmse = torch.tensor(1.), torch.tensor(1.)
    if lazy:
        # inside the patched reference: `volume.sum(dim=0)` / `valid.sum(dim=0)` (mvsdet.py:509-511) then cost one launch
        # of the fused lifting kernel instead of a (N,C,X,Y,Z) volume and a reduction over it (lazywarp.py)
        from . import lazywarp
        volume, valid = lazywarp.lazy_backproject(features, points, projection, est_depth, est_dens, vz)
        return volume, valid, gap_all, rmse
    volume, valid = ops.backproject_weigh(features, points, projection, est_depth, est_dens, vz)
    volume = volume.view(n, c, nx, ny, nz)
    valid = valid.view(n, 1, nx, ny, nz)
    return volume, valid, gap_all, rmse


# ------------------------------------------------------------------------------------------- depth supervision
def _refuse_gt_grad(name: str, *tensors):
    for t in tensors:
        if isinstance(t, Tensor) and t.requires_grad:
            raise RuntimeError(f"{name}: the ground truth and the mask carry no gradient (the reference gives them none); detach them")


def _scene_depth_loss(est: Tensor, gt: Tensor) -> Tensor:
    """One scene of depth_loss_func_new (mvsdet.py:902-913): est (N,h,w), gt (N,Hg,Wg) -> 0-dim loss."""
    if est.is_cuda:
        est, gt = amp_fp32(est, gt)
        if gt.device != est.device:
            gt = gt.to(est.device, non_blocking=True)
        return ops.depth.depth_loss(est, gt, None, ops.depth.DEPTH_LOSS_L1)[0]
    import torch.nn.functional as F
    height, width = est.shape[1], est.shape[2]
    cur_gt = F.interpolate(gt.unsqueeze(1), size=(height, width), mode="bilinear").squeeze(1)
    tmp_mask = cur_gt > 0
    return torch.mean(torch.abs(est[tmp_mask] - cur_gt[tmp_mask]))


def depth_loss_func_new(est_depth: Sequence[Tensor], gt_depth: Sequence[Tensor]) -> dict:
    """MVSDet.depth_loss_func_new (mvsdet.py:893-915) without `self`: lists over the batch of est (N,1,h,w) and gt (N,Hg,Wg) ->
    dict(loss_depth=sum over the scenes, in list order from 0., of the mean of |est - resized gt| where resized gt > 0).
    Device tensors: one `ops.depth.depth_loss` per scene (two launches, no host synchronisation, no boolean-mask gather; est --
    a crop of the padded depth expectation -- and gt are read in place); the first scene's mean is the sum so far (0. + x = x),
    every further scene costs one 0-dim addition.  CPU tensors: the reference's own ops in its order.  Differentiable in est.
    An unmodified reference never reaches this function with data: extract_feat leaves `est_depth_crop` empty (mvsdet.py:400,698),
    so its loss_depth is the 0. of an empty loop; `MVSDetHotPath.depth_loss` hands over what it meant to, depth_coding."""
    if len(est_depth) != len(gt_depth):
        raise ValueError(f"depth_loss_func_new: {len(est_depth)} estimates for {len(gt_depth)} ground-truth maps")
    loss = 0.
    for i, (est, gt) in enumerate(zip(est_depth, gt_depth)):
        _refuse_gt_grad("depth_loss_func_new", gt)
        if est.dim() != 4 or est.shape[1] != 1 or gt.dim() != 3 or gt.shape[0] != est.shape[0]:
            raise ValueError(f"depth_loss_func_new: scene {i}: est {tuple(est.shape)} must be (N,1,h,w) and gt {tuple(gt.shape)} (N,Hg,Wg)")
        term = _scene_depth_loss(est.squeeze(1), gt)
        loss = term if (i == 0 and term.is_cuda) else loss + term
    return dict(loss_depth=loss)


def mvsnet_loss(depth_est: Tensor, depth_gt: Tensor, mask: Tensor) -> Tensor:
    """mvs_models/mvsnet.py:292-294: the mean over mask > 0.5 of smooth_l1(depth_est - depth_gt) (beta 1), three tensors of one
    shape (B,H,W).  Device tensors: one `ops.depth.depth_loss` (two launches, no host synchronisation), all three read in place; a
    mask that is not float32 (bool, as some loaders hand it over) is converted first.  CPU tensors: the reference's ops.
    Differentiable in depth_est."""
    _refuse_gt_grad("mvsnet_loss", depth_gt, mask)
    if not (depth_est.shape == depth_gt.shape == mask.shape):
        raise ValueError(f"mvsnet_loss: shapes differ: {tuple(depth_est.shape)} / {tuple(depth_gt.shape)} / {tuple(mask.shape)}")
    if not depth_est.is_cuda:
        import torch.nn.functional as F
        m = mask > 0.5
        return F.smooth_l1_loss(depth_est[m], depth_gt[m], reduction="mean")
    if depth_est.dim() < 2:
        raise ValueError(f"mvsnet_loss: depth maps must be at least 2-D (got shape {tuple(depth_est.shape)})")
    depth_est, depth_gt, mask = amp_fp32(depth_est, depth_gt, mask)
    dev = depth_est.device
    depth_gt, mask = (t if t.device == dev else t.to(dev, non_blocking=True) for t in (depth_gt, mask))
    if mask.dtype != torch.float32:
        mask = mask.float()
    if depth_est.dim() != 3:
        H, W = depth_est.shape[-2:]
        depth_est, depth_gt, mask = (t.reshape(-1, H, W) for t in (depth_est, depth_gt, mask))
    return ops.depth.depth_loss(depth_est, depth_gt, mask, ops.depth.DEPTH_LOSS_SMOOTH_L1)[0]


# ------------------------------------------------------------------------------------------- photometric consistency
def _refuse_photo_grad(name: str, **tensors):
    for what, t in tensors.items():
        if isinstance(t, Tensor) and t.requires_grad:
            raise RuntimeError(f"{name}: `{what}` carries no gradient here (the depth, through the sample position, and the warped "
                               "image do); detach it")


def _check_packed_cams(name: str, img: Tensor, left_cam: Tensor, right_cam: Tensor, depth: Tensor):
    if img.dim() != 4:
        raise ValueError(f"{name}: img must be (B,h,w,C), got {tuple(img.shape)}")
    B, h, w, _ = img.shape
    for what, cam in (("left_cam", left_cam), ("right_cam", right_cam)):
        if tuple(cam.shape) != (B, 2, 3, 4):
            raise ValueError(f"{name}: {what} must be ({B},2,3,4): [R|t] and K of every view, got {tuple(cam.shape)}")
    if depth.numel() != B * h * w or depth.dim() not in (3, 4) or tuple(depth.shape[-2:]) != (h, w):
        raise ValueError(f"{name}: depth must be ({B},1,{h},{w}), got {tuple(depth.shape)}")
    return B, h, w


def _inverse_warping_host(img: Tensor, left_cam: Tensor, right_cam: Tensor, depth: Tensor) -> Tuple[Tensor, Tensor]:
    """The reference's operation sequence (homography.py:6-201) on whatever device the tensors live on."""
    B, h, w, C = img.shape
    K_left = left_cam[:, 1, :3, :3]
    R_rel = torch.matmul(right_cam[:, 0, :3, :3], left_cam[:, 0, :3, :3].permute(0, 2, 1))
    t_rel = right_cam[:, 0, :3, 3:4] - torch.matmul(R_rel, left_cam[:, 0, :3, 3:4])
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], device=img.device).reshape(1, 1, 4).repeat(B, 1, 1)
    transform = torch.cat([torch.cat([R_rel, t_rel], dim=2).float(), bottom], dim=1)
    xg, yg = (v.to(img.device) for v in ops.photo.pixel_grid(h, w))
    grid = torch.stack([xg.repeat(h), yg.repeat_interleave(w), torch.ones(h * w, device=img.device)], dim=0)
    cam = torch.matmul(torch.inverse(K_left).float(), grid.unsqueeze(0).repeat(B, 1, 1)) * depth.reshape(B, 1, h * w).float()
    cam_hom = torch.cat([cam, torch.ones((B, 1, h * w), device=img.device)], dim=1)
    k_hom = torch.cat([torch.cat([K_left.float(), torch.zeros((B, 3, 1), device=img.device)], dim=2), bottom], dim=1)
    p = torch.matmul(torch.matmul(k_hom, transform), cam_hom)
    z = p[:, 2:3] + 1e-10
    x = (p[:, 0:1] / z).reshape(-1) / (w - 1) * 2.0 - 1.0
    y = (p[:, 1:2] / z).reshape(-1) / (h - 1) * 2.0 - 1.0
    x = (x + 1.0) * (w - 1.0) / 2.0
    y = (y + 1.0) * (h - 1.0) / 2.0
    x0 = torch.floor(x).int()
    y0 = torch.floor(y).int()
    x1, y1 = x0 + 1, y0 + 1
    mask = ((x0 >= 0) & (x1 <= w - 1) & (y0 >= 0) & (y0 <= h - 1)).float()
    x0, x1, y0, y1 = x0.clamp(0, w - 1), x1.clamp(0, w - 1), y0.clamp(0, h - 1), y1.clamp(0, h - 1)
    base = (torch.arange(B, device=img.device) * (h * w)).repeat_interleave(h * w)
    flat = img.reshape(-1, C).float()
    row0, row1 = base + y0.long() * w, base + y1.long() * w
    ax, ay = x1.float() - x, y1.float() - y
    wa, wb, wc, wd = ax * ay, ax * (1.0 - ay), (1.0 - ax) * ay, (1.0 - ax) * (1.0 - ay)
    out = (wa.unsqueeze(1) * flat[row0 + x0.long()] + wb.unsqueeze(1) * flat[row1 + x0.long()]
           + wc.unsqueeze(1) * flat[row0 + x1.long()] + wd.unsqueeze(1) * flat[row1 + x1.long()])
    return out.reshape(B, h, w, C), mask.reshape(B, h, w, 1)


def inverse_warping(img: Tensor, left_cam: Tensor, right_cam: Tensor, depth: Tensor) -> Tuple[Tensor, Tensor]:
    """mvs_models/homography.py:6-63: img (B,h,w,C) of the right views, left_cam / right_cam (B,2,3,4) ([:,0] the world-to-camera
    [R|t], [:,1,:3,:3] K), depth (B,1,h,w) of the left views -> warped (B,h,w,C), mask (B,h,w,1) float 0/1.  The reference's quirks
    are kept: the LEFT intrinsics project into the right view, the pixel grid is the fp32 linspace, the mask's last test is on y0 and
    the weights use the clamped x1, y1 (outside the mask warped is an extrapolation).  Device tensors: `ops.photo.photo_geometry` +
    `ops.photo.inverse_warp` (two launches, no torch.inverse, no host synchronisation; img and depth read in place).  CPU tensors: the
    reference's own operation sequence.  Differentiable in depth (through the sample position)."""
    B, h, w = _check_packed_cams("inverse_warping", img, left_cam, right_cam, depth)
    _refuse_photo_grad("inverse_warping", img=img, left_cam=left_cam, right_cam=right_cam)
    if not img.is_cuda:
        return _inverse_warping_host(img, left_cam, right_cam, depth)
    img, left_cam, right_cam, depth = amp_fp32(img, left_cam, right_cam, depth)
    dev = img.device
    left_cam, right_cam, depth = (t if t.device == dev else t.to(dev, non_blocking=True) for t in (left_cam, right_cam, depth))
    geo = ops.photo.photo_geometry(left_cam[:, 0], left_cam[:, 1], right_cam[:, 0], None, None)
    return ops.photo.inverse_warp(img, depth[:, 0] if depth.dim() == 4 else depth, geo, None, None)


def _reconstr_loss_host(warped: Tensor, ref: Tensor, mask: Tensor, simple: bool) -> Tensor:
    """The reference's operation sequence (homography.py:204-225) on whatever device the tensors live on."""
    import torch.nn.functional as F
    wm, rm = warped * mask, ref * mask
    photo = F.smooth_l1_loss(wm, rm, reduction="mean")
    if simple:
        return photo
    grad = (F.smooth_l1_loss(wm[:, :, 1:] - wm[:, :, :-1], rm[:, :, 1:] - rm[:, :, :-1], reduction="mean")
            + F.smooth_l1_loss(wm[:, 1:] - wm[:, :-1], rm[:, 1:] - rm[:, :-1], reduction="mean"))
    return (1 - 0.5) * photo + 0.5 * grad


def _photometric_loss_host(warped_list, mask_list, ref_list) -> dict:
    """The reference's operation sequence (mvsdet.py:845-874) on whatever device the tensors live on."""
    vols = [_reconstr_loss_host(w, r, m, False) + 1e4 * (1 - m) for w, m, r in zip(warped_list, mask_list, ref_list)]
    vol = torch.stack(vols).permute(1, 2, 3, 4, 0)
    top = torch.neg(torch.topk(torch.neg(vol), k=1, sorted=False)[0])
    top = top * (top < 1e4 * torch.ones_like(top)).float()
    return dict(loss_pc=torch.mean(torch.sum(top, dim=-1)))


def compute_reconstr_loss(warped: Tensor, ref: Tensor, mask: Tensor, simple: bool = True) -> Tensor:
    """mvs_models/homography.py:204-225 -> 0-dim L.  wm = warped * mask, rm = ref * mask; simple: smooth_l1(wm, rm) (beta 1, mean);
    else 0.5 of it + 0.5 (smooth_l1 of the forward differences along w + along h, each its own mean): a masked pixel next to a valid
    one contributes its step.  Device tensors: `ops.photo.reconstr_loss` (two launches, float64 sums in a fixed order).  CPU tensors:
    the reference's ops.  Differentiable in warped."""
    if not (warped.dim() == 4 and ref.shape == warped.shape and tuple(mask.shape) == tuple(warped.shape[:3]) + (1,)):
        raise ValueError(f"compute_reconstr_loss: warped {tuple(warped.shape)} and ref {tuple(ref.shape)} must be one (B,h,w,C) and mask "
                         f"{tuple(mask.shape)} (B,h,w,1)")
    _refuse_photo_grad("compute_reconstr_loss", ref=ref)
    if not warped.is_cuda:
        return _reconstr_loss_host(warped, ref, mask, simple)
    warped, ref, mask = amp_fp32(warped, ref, mask)
    return ops.photo.reconstr_loss(warped, ref, mask.detach(), bool(simple))[0]


def photometric_loss(warped_list: Sequence[Tensor], mask_list: Sequence[Tensor], ref_list: Sequence[Tensor]) -> dict:
    """MVSDet.photometric_loss (mvsdet.py:845-874) without `self`: one entry per scene, all of one shape -> dict(loss_pc=...).
    L_i = compute_reconstr_loss(..., simple=False); per pixel the smallest L_i + 1e4 (1 - mask_i) over the scenes, dropped where it is
    not < 1e4; the mean over (B,h,w).  For one scene that is L * mean(mask).  Device tensors: `ops.photo.reconstr_loss` per scene and
    one `ops.photo.photometric_select` (integer win counts, ties to the lower scene; d loss_pc / d L_i = the share of pixels scene i
    wins).  CPU tensors: the reference's ops."""
    n = len(warped_list)
    if n == 0 or len(mask_list) != n or len(ref_list) != n:
        raise ValueError(f"photometric_loss: {n} warped images, {len(mask_list)} masks and {len(ref_list)} reference images")
    if any(w.shape != warped_list[0].shape for w in warped_list) or any(m.shape != mask_list[0].shape for m in mask_list):
        raise ValueError("photometric_loss: the scenes must share one shape (the reference stacks them)")
    if not warped_list[0].is_cuda:
        for r in ref_list:
            _refuse_photo_grad("photometric_loss", ref=r)
        return _photometric_loss_host(warped_list, mask_list, ref_list)
    L = [compute_reconstr_loss(w, r, m, simple=False) for w, m, r in zip(warped_list, mask_list, ref_list)]
    masks = [amp_fp32(m).detach().reshape(1, -1) for m in mask_list]
    loss, _ = ops.photo.photometric_select(masks[0] if n == 1 else torch.cat(masks, dim=0), L[0].reshape(1) if n == 1 else torch.stack(L))
    return dict(loss_pc=loss)


def _warp_img_host(small: Tensor, neighbor_ids: Tensor, ref_w2c: Tensor, ref_feat_intrinsic: Tensor, ref_depth: Tensor, ref_id: Tensor):
    """The reference's gathers (mvsdet.py:723-742) behind the resize, on whatever device the tensors live on: small (N,h,w,C)."""
    N = small.shape[0]
    full_cam = torch.stack([ref_w2c.float(), ref_feat_intrinsic.float().expand(N, -1, -1)], dim=1)[:, :, :3, :]
    src_id = neighbor_ids.long()[ref_id, 0]
    warped, mask = _inverse_warping_host(small[src_id], full_cam[ref_id], full_cam[src_id], ref_depth[ref_id])
    return warped, mask, small[ref_id]


def warp_img(ref_imgs: Tensor, neighbor_ids: Tensor, ref_w2c: Tensor, ref_feat_intrinsic: Tensor, ref_depth: Tensor, ref_id=None):
    """MVSDet.warp_img (mvsdet.py:701-768) without `self`: ref_imgs (N,3,Hi,Wi) in [0,1], neighbor_ids (N,k), ref_w2c (N,4,4),
    ref_feat_intrinsic (4,4) (or (N,4,4): per-view), ref_depth (N,1,h,w) -> (warped (B,h,w,3), mask (B,h,w,1), chose_ref_imgs
    (B,h,w,3)), B = min(10, N): the images are resized by 0.25 (one F.interpolate) and cropped to (h,w); `ref_id` (B) picks the views
    (None: torch.randperm(N)[:B] drawn on the CPU, as the reference); each is compared with its FIRST neighbour warped into it by its
    own depth.  Device tensors: the operators read the resized planar images, the cameras and ref_depth (any strides: the crop of
    the padded depth expectation) in place through ref_id and neighbor_ids[ref_id, 0]; CPU tensors: the reference's own sequence."""
    import torch.nn.functional as F
    if ref_imgs.dim() != 4 or ref_depth.dim() != 4 or ref_depth.shape[1] != 1 or ref_depth.shape[0] != ref_imgs.shape[0]:
        raise ValueError(f"warp_img: ref_imgs {tuple(ref_imgs.shape)} must be (N,C,Hi,Wi) and ref_depth {tuple(ref_depth.shape)} (N,1,h,w)")
    N = ref_imgs.shape[0]
    if neighbor_ids.dim() != 2 or neighbor_ids.shape[0] != N or neighbor_ids.shape[1] < 1:
        raise ValueError(f"warp_img: neighbor_ids must be ({N},k>=1), got {tuple(neighbor_ids.shape)}")
    if tuple(ref_w2c.shape) != (N, 4, 4) or tuple(ref_feat_intrinsic.shape) not in ((4, 4), (N, 4, 4)):
        raise ValueError(f"warp_img: ref_w2c must be ({N},4,4) and ref_feat_intrinsic (4,4) or ({N},4,4), got {tuple(ref_w2c.shape)} / "
                         f"{tuple(ref_feat_intrinsic.shape)}")
    _refuse_photo_grad("warp_img", ref_imgs=ref_imgs, ref_w2c=ref_w2c, ref_feat_intrinsic=ref_feat_intrinsic)
    h, w = ref_depth.shape[2], ref_depth.shape[3]
    dev = ref_imgs.device
    ref_imgs, ref_w2c, ref_feat_intrinsic, ref_depth = amp_fp32(ref_imgs, ref_w2c, ref_feat_intrinsic, ref_depth)
    small = F.interpolate(ref_imgs, scale_factor=0.25, mode="bilinear")[:, :, :h, :w]
    if tuple(small.shape[2:]) != (h, w):
        raise ValueError(f"warp_img: a quarter of the {tuple(ref_imgs.shape[2:])} images is smaller than the depth map {(h, w)}")
    small = small.permute(0, 2, 3, 1)                                   # (N,h,w,C): a view of the planar resize
    if ref_id is None:
        ref_id = torch.randperm(N)[:min(10, N)]
    ref_id = torch.as_tensor(ref_id, dtype=torch.int64)
    if not ref_imgs.is_cuda:
        return _warp_img_host(small, neighbor_ids, ref_w2c, ref_feat_intrinsic, ref_depth, ref_id)
    from .ops._common import to_device
    ref_id = to_device(ref_id, dev)
    nbr = neighbor_ids.to(dev, non_blocking=True).long()
    src_id = nbr[ref_id, 0]
    ref_w2c, ref_feat_intrinsic, ref_depth = (t if t.device == dev else t.to(dev, non_blocking=True)
                                              for t in (ref_w2c, ref_feat_intrinsic, ref_depth))
    geo = ops.photo.photo_geometry(ref_w2c.float(), ref_feat_intrinsic.float(), ref_w2c.float(), ref_id, src_id)
    warped, mask = ops.photo.inverse_warp(small, ref_depth[:, 0], geo, src_id, ref_id)
    return warped, mask, small[ref_id]


# ------------------------------------------------------------------------------------------- Gaussian splatting (the NVS branch)
def render_cuda(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, image_shape: Tuple[int, int], background_color: Tensor,
                gaussian_means: Tensor, gaussian_covariances: Tensor, gaussian_sh_coefficients: Tensor, gaussian_opacities: Tensor,
                scale_invariant: bool = True, use_sh: bool = True, scene=None, *, max_keys=None) -> Tensor:
    """gs_src/model/decoder/cuda_splatting.py:49-138: extrinsics (B,4,4) camera-to-world, intrinsics (B,3,3) normalised, near / far
    (B), background_color (B,3), gaussian_means (B,G,3), gaussian_covariances (B,G,3,3), gaussian_sh_coefficients (B,G,3,d_sh),
    gaussian_opacities (B,G) -> images (B,3,h,w).  The camera matrices come from one launch (`ops.splat.splat_cameras`: no
    torch.inverse, no .item()); the scale_invariant multiplications happen inside the rasteriser, so no scaled copies are made.
    Batch rows that are expanded views of one Gaussian set (stride 0, what DecoderSplattingCUDA hands over before it copies them) or
    B == 1 go out as one call over B views; distinct rows one call per row.  max_keys: (Gaussian, tile) pairs a view may have
    (default 8 G); a view that needs more comes out NaN.  There is no CPU path.  `scene` is accepted and unused, as in the reference."""
    if not (use_sh or gaussian_sh_coefficients.shape[-1] == 1):
        raise ValueError("render_cuda: without use_sh the coefficients are the colours, (B,G,3,1)")
    return _render_views("render_cuda", extrinsics, intrinsics, near, far, image_shape, gaussian_means, gaussian_covariances,
                         gaussian_opacities, gaussian_sh_coefficients, background_color, scale_invariant, use_sh, max_keys)


def _render_views(name: str, extrinsics, intrinsics, near, far, image_shape, means, covs, opacs, shs=None, background=None,
                  scale_invariant=True, use_sh=True, max_keys=None, depth_mode=None):
    """What render_cuda, render_depth_cuda and decode_splatting share: amp_fp32, the shape refusal, the key capacity, one
    `splat_cameras` launch for the B views and the one-call rule.  shs and background given, depth_mode None: `rasterize` -> colour;
    shs None: `depth_only` -> depth; both given: `rasterize_depth` -> (colour, depth)."""
    extrinsics, intrinsics, near, far, background, means, covs, shs, opacs = amp_fp32(extrinsics, intrinsics, near, far, background, means,
                                                                                      covs, shs, opacs)
    colour = shs is not None
    if means.dim() != 3 or covs.dim() != 4 or (colour and shs.dim() != 4) or opacs.dim() != 2:
        got, form = (f", coefficients {tuple(shs.shape)}", ", (B,G,3,d_sh)") if colour else ("", "")
        raise ValueError(f"{name}: means {tuple(means.shape)}, covariances {tuple(covs.shape)}{got} and opacities {tuple(opacs.shape)} "
                         f"must be (B,G,3), (B,G,3,3){form} and (B,G)")
    b, G = means.shape[:2]
    h, w = (int(v) for v in image_shape)
    if extrinsics.shape[0] != b or (colour and background.shape[0] != b):
        got = f" and {background.shape[0]} backgrounds" if colour else ""
        raise ValueError(f"{name}: {extrinsics.shape[0]} cameras{got} for {b} batch rows")
    keys = ops.splat.default_max_keys(G) if max_keys is None else int(max_keys)
    cams = ops.splat.splat_cameras(extrinsics, intrinsics, near, far, bool(scale_invariant))

    def views(i, cams, near, far, background):   # Gaussian set i under these cameras -> the outputs asked for, as a tuple
        if not colour:
            return ops.splat.depth_only(means[i], covs[i], opacs[i], cams, near, far, h, w, keys, depth_mode)[:1]
        if depth_mode is None:
            return ops.splat.rasterize(means[i], covs[i], shs[i], opacs[i], cams, background, h, w, keys, bool(use_sh))[:1]
        return ops.splat.rasterize_depth(means[i], covs[i], shs[i], opacs[i], cams, near, far, background, h, w, keys, bool(use_sh),
                                         depth_mode)[:2]

    per_view = (cams, near, far, background)
    # render_cuda's rule: B == 1, or every Gaussian tensor an expanded view of one set (stride 0) -> one call over the B views
    if b == 1 or all(t.stride(0) == 0 for t in (means, covs, opacs, shs) if t is not None):
        out = views(0, *per_view)
    else:
        rows = [views(i, *[t if t is None else t[i:i + 1] for t in per_view]) for i in range(b)]
        out = tuple(torch.cat(parts) for parts in zip(*rows))
    return out[0] if len(out) == 1 else out


def render_depth_cuda(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, image_shape: Tuple[int, int],
                      gaussian_means: Tensor, gaussian_covariances: Tensor, gaussian_opacities: Tensor, scale_invariant: bool = True,
                      mode: str = "depth", *, max_keys=None) -> Tensor:
    """gs_src/model/decoder/cuda_splatting.py:237-280: extrinsics (B,4,4), intrinsics (B,3,3), near / far (B), gaussian_means (B,G,3),
    gaussian_covariances (B,G,3,3), gaussian_opacities (B,G) -> depth (B,h,w).  Every Gaussian's camera-space z, mapped by `mode`
    ("depth", "disparity", "relative_disparity", "log" -- the last with the reference's inverted clamp, log(far) whenever near <= far),
    blended over a background of 0.  The reference renders that value as three equal colour channels in a second full rasterisation and
    returns their mean, (x + x + x) / 3; here it is blended once by `ops.splat.depth_only` and returned as x: the two can differ in
    the last bit.  Batch rows go out as in `render_cuda`: expanded rows or B == 1 as one call, distinct rows one call each."""
    if mode not in ops.splat.DEPTH_MODES:
        raise ValueError(f"render_depth_cuda: mode {mode!r} must be one of {ops.splat.DEPTH_MODES}")
    return _render_views("render_depth_cuda", extrinsics, intrinsics, near, far, image_shape, gaussian_means, gaussian_covariances,
                         gaussian_opacities, scale_invariant=scale_invariant, max_keys=max_keys, depth_mode=mode)


def decode_splatting(gaussians, extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, image_shape: Tuple[int, int],
                     background_color=None, *, max_keys=None, depth_mode=None):
    """The colour output of DecoderSplattingCUDA.forward (gs_src/model/decoder/decoder_splatting_cuda.py:37-62): gaussians with
    `.means` (b,G,3), `.covariances` (b,G,3,3), `.harmonics` (b,G,3,d_sh) and `.opacities` (b,G); extrinsics (b,v,4,4), intrinsics
    (b,v,3,3), near / far (b,v) -> colour (b,v,3,h,w).  One rasteriser call per batch element over its v views: the Gaussians are not
    repeated per view.  background_color (3), default black (the decoder's registered buffer comes from the dataset config).
    depth_mode: one of render_depth_cuda's modes -> (colour, depth (b,v,h,w)), both from ONE fused call per batch element
    (`ops.splat.rasterize_depth`) where the reference rasterises a second time; the colour keeps the bits it has without it."""
    b, v = extrinsics.shape[:2]
    dev = extrinsics.device
    bg = torch.zeros(3, dtype=torch.float32, device=dev) if background_color is None else background_color.to(dev)
    if depth_mode is not None and depth_mode not in ops.splat.DEPTH_MODES:
        raise ValueError(f"decode_splatting: depth_mode {depth_mode!r} must be None or one of {ops.splat.DEPTH_MODES}")
    rows = []
    for i in range(b):
        sets = (gaussians.means[i], gaussians.covariances[i], gaussians.opacities[i], gaussians.harmonics[i])
        if depth_mode is not None:   # cast before the rows are expanded, so that they stay views of one set and go out as one call
            sets = amp_fp32(*sets)
        rows.append(_render_views("decode_splatting", extrinsics[i], intrinsics[i], near[i], far[i], image_shape,
                                  *[t.expand(v, *t.shape) for t in sets], bg.expand(v, 3), max_keys=max_keys, depth_mode=depth_mode))
    return torch.stack(rows) if depth_mode is None else tuple(torch.stack(t) for t in zip(*rows))


class PixelGaussians:
    """What `pixel_gaussians` returns and `decode_splatting` takes: `.means` (1,G,3), `.covariances` (1,G,3,3), `.harmonics`
    (1,G,3,d_sh), `.opacities` (1,G); `.scales` (1,G,3) and `.rotations` (1,G,4) when asked for, else None."""
    __slots__ = ("means", "covariances", "harmonics", "opacities", "scales", "rotations")

    def __init__(self, means, covariances, harmonics, opacities, scales=None, rotations=None):
        self.means, self.covariances, self.harmonics, self.opacities = means, covariances, harmonics, opacities
        self.scales, self.rotations = scales, rotations


def pixel_gaussians(extrinsics: Tensor, intrinsics: Tensor, raw: Tensor, depths: Tensor, opacities: Tensor, image_shape: Tuple[int, int],
                    gaussian_scale_min: float, gaussian_scale_max: float, sh_degree: int, *, sh_rotation=None,
                    with_scales: bool = False) -> PixelGaussians:
    """mvsdet.py:576-632 in one call: the offset of every pixel's ray, GaussianAdapter.forward
    (gs_src/model/encoder/common/gaussian_adapter.py:50-98) and the flattening to (v, r, s) order.  extrinsics (V,4,4) camera-to-world
    and intrinsics (V,3,3) normalised, of the chosen source views; raw (V,R,S,2 + 7 + 3 d_sh), the rearranged output of `to_gaussians`
    (it may be a slice of a wider buffer: read in place); depths (V,R) along the ray; opacities (V,R), passed through and repeated
    over S; image_shape (h, w) of the feature map, R = h w.  Two launches (cameras, Gaussians), no torch.inverse, no host read.
    sh_rotation None: the harmonics are rotated into the world frame for the basis the rasteriser evaluates; a (V,
    sum_l (2l+1)^2) tensor: those blocks instead (INTEGRATION.md shows how to pass e3nn's).  Gradients reach raw, depths, opacities."""
    h, w = (int(v) for v in image_shape)
    extrinsics, intrinsics, raw, depths, opacities, sh_rotation = amp_fp32(extrinsics, intrinsics, raw, depths, opacities, sh_rotation)
    if raw.dim() != 4 or depths.dim() != 2 or opacities.dim() != 2 or tuple(opacities.shape) != tuple(depths.shape):
        raise ValueError(f"pixel_gaussians: raw {tuple(raw.shape)}, depths {tuple(depths.shape)} and opacities {tuple(opacities.shape)} "
                         "must be (V,R,S,2 + 7 + 3 d_sh), (V,R) and (V,R)")
    V, R, S, _ = raw.shape
    cams = ops.adapter.adapter_cameras(extrinsics.detach(), intrinsics.detach(), h, w, int(sh_degree),
                                       None if sh_rotation is None else sh_rotation.detach())
    out = ops.adapter.pixel_gaussians(raw, depths, cams, h, w, gaussian_scale_min, gaussian_scale_max, int(sh_degree), with_scales)
    opac = opacities[:, :, None].expand(V, R, S).reshape(1, V * R * S)
    return PixelGaussians(*[t[None] for t in out[:3]], opac, *[t[None] for t in out[3:]])


def process_rgb_raw(orig_rgb: Tensor, ratio, height: int, width: int, src_id) -> Tensor:
    """MVSDet.process_rgb_raw (mvsdet.py:319-333): orig_rgb (n_img,3,Hi,Wi) denormalised images, src_id the chosen views ->
    (1, n_src, height width, 3): F.interpolate(scale_factor=1/ratio, mode='bilinear') of the chosen images, cropped to height x width,
    as rows.  One launch (`ops.gshead.process_rgb_raw_rows`: the mean of the four pixels around 4 d + 1.5); only ratio 4, which is
    what the reference asserts.  No gradient to the images."""
    if ratio != 4:
        raise ValueError(f"process_rgb_raw: ratio = {ratio}; only 4 is supported (the reference asserts it)")
    orig_rgb = amp_fp32(orig_rgb)
    return ops.gshead.process_rgb_raw_rows(orig_rgb, src_id, int(height), int(width))[None]


def gaussian_head(feature: Tensor, depth_coding: Tensor, weight: Tensor, bias: Tensor, src_id, height: int, width: int,
                  num_surfaces: int, rgb_raw=None, denorm_images=None) -> Tensor:
    """mvsdet.py:561-575 in one call: the rows of the chosen views (feature cropped to height x width, depth_coding, and with
    use_rgb_gaussian the rgb) through `to_gaussians` = nn.Sequential(ReLU, Linear(weight, bias)) -> raw (n_src, height width,
    num_surfaces, 2 + 7 + 3 d_sh), what `pixel_gaussians` takes.  The rgb comes as rgb_raw (n_src,R,3) / (1,n_src,R,3) from
    `process_rgb_raw`, or as denorm_images (n_img,3,Hi,Wi), which the kernel reduces itself -- never both.  src_id: a sequence or
    host tensor (checked) or an int64 device tensor.  Gradients reach feature, depth_coding, weight and bias."""
    if rgb_raw is not None and denorm_images is not None:
        raise ValueError("gaussian_head: rgb comes as rows (rgb_raw) or as images (denorm_images), not both")
    feature, depth_coding, weight, bias, rgb_raw, denorm_images = amp_fp32(feature, depth_coding, weight, bias, rgb_raw, denorm_images)
    return ops.gshead.gaussian_head(feature, depth_coding, src_id, weight, bias, int(height), int(width), int(num_surfaces), rgb_raw,
                                    denorm_images)


def nvs_loss_func(rgb_pred: Sequence[Tensor], gt_rgb: Sequence[Tensor]) -> dict:
    """MVSDet.nvs_loss_func (mvsdet.py:878-890) without use_nerf_mask: sum over the scenes of mean((rgb - gt)^2), rgb = the scene's
    colour (1,n_tgt,3,H,W) with its leading 1 taken off (or already (n_tgt,3,H,W)), gt (n_tgt,3,H,W) -> dict(loss_nvs=...).  The
    reference's assertion that gt lies in [0,1] is a host read and is left to the caller."""
    if len(rgb_pred) != len(gt_rgb) or not rgb_pred:
        raise ValueError(f"nvs_loss_func: {len(rgb_pred)} renders for {len(gt_rgb)} ground truths")
    loss = 0
    for rgb, gt in zip(rgb_pred, gt_rgb):
        rgb = rgb[0] if rgb.dim() == 5 else rgb
        if rgb.shape != gt.shape:
            raise ValueError(f"nvs_loss_func: render {tuple(rgb.shape)} against ground truth {tuple(gt.shape)}")
        loss = loss + torch.mean((rgb - gt) ** 2)
    return dict(loss_nvs=loss)


# ------------------------------------------------------------------------------------------- scores of the rendered views (test loop)
def _no_mask(name: str, mask) -> None:
    if mask is not None:
        raise NotImplementedError(f"{name}: the masked form (cv2.boundingRect; save_rendered_img.py:23-24, 32-35) is never reached by the "
                                  "reference's calls and is not provided")


def _no_save_dir(name: str, save_dir) -> None:
    if save_dir is not None:
        raise NotImplementedError(f"{name}: writing pictures under save_dir is not provided; score with save_dir=None")


def _one_view(name: str, pred: Tensor, target: Tensor):
    if pred.dim() != 3 or pred.shape != target.shape or pred.shape[-1] != 3:
        raise ValueError(f"{name}: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be two equal (H,W,3) views")
    return pred.permute(2, 0, 1)[None], target.permute(2, 0, 1)[None]


def compute_psnr(pred: Tensor, target: Tensor, mask=None) -> Tensor:
    """nerf_utils/save_rendered_img.py:17-26 for one (H,W,3) view in [0,1]: -10 log(mean((pred - target)^2)) / log(10), +inf for equal
    images, as a 0-dim float64 tensor on the inputs' device (the reference returns a host array: `.cpu().numpy()`).  The view is
    read in place through its strides; the sums are float64 (ops.nvsmetric.nvs_score).  No host synchronisation."""
    _no_mask("compute_psnr", mask)
    return ops.nvsmetric.nvs_score(None, *_one_view("compute_psnr", pred, target))[0][0, 0]


def compute_ssim(pred: Tensor, target: Tensor, mask=None) -> Tensor:
    """nerf_utils/save_rendered_img.py:29-44 for one (H,W,3) view: skimage's structural_similarity(channel_axis=-1, data_range=1)
    -- 7x7 box windows inside the image, sample covariance, K1 = 0.01, K2 = 0.03 -- evaluated in float64 on the device, as a 0-dim
    float64 tensor (the reference copies both images to the host).  A side below 7 raises ValueError, as skimage does."""
    _no_mask("compute_ssim", mask)
    return ops.nvsmetric.nvs_score(None, *_one_view("compute_ssim", pred, target))[0][0, 1]


def save_rendered_img_Image(pred: Tensor, gt: Tensor, img_meta=None, save_dir=None):
    """nerf_utils/save_rendered_img.py:178-212 without the picture writing: pred, gt (n_tgt,3,H,W) in [0,1] -> (psnr, ssim, 0), the
    means over the target views, the first two as 0-dim float64 device tensors.  One scoring call for all views, no host
    synchronisation.  img_meta is accepted and unused (the reference takes the scene's name from it for the pictures)."""
    _no_save_dir("save_rendered_img_Image", save_dir)
    scene = ops.nvsmetric.nvs_score(None, pred, gt)[1]
    return scene[0], scene[1], 0


def save_rendered_depth(pred: Tensor, gt: Tensor, img_meta=None, save_dir=None) -> Tensor:
    """nerf_utils/save_rendered_img.py:215-235 without the picture writing and without its print of the extrema (a host read): pred,
    gt (n_tgt,H,W) -> the mean over the views of mean((pred - gt)^2) as a 0-dim float64 device tensor.  The reference calls it rmse;
    it is a mean squared error with no root, and stays that.  The views go through the scoring kernel's tiles: sides of 7 needed."""
    _no_save_dir("save_rendered_depth", save_dir)
    return ops.nvsmetric.nvs_score(None, None, None, pred, gt)[1][2]
