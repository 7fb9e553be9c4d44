"""Drop-in wiring for the reference code base (Pixie8888/MVSDet, projects/NeRF-Det/nerfdet/mvsdet.py).

`patch_reference(mvsdet_module)` rebinds, inside the reference's own module, the functions of the hot path to the
HIP-backed mirrors of this package -- same names, same signatures, same return arity -- so that
`MVSDet.extract_feat` (mvsdet.py:336-698) runs them without any change to the reference source or to
projects/NeRF-Det/configs/mvsdet_res50_2x_low_res.py:

    homo_warping           (imported at mvsdet.py:31 from mvs_models/module.py:105)
    backproject_Weigh      (mvsdet.py:1372)      -- with gt_depth (extract_feat(depth=[...]), the configs' `use_depth`) it also
                                                  returns "weight_gap" and "src_rmse" as device scalars (ops.depth_diagnostics)
    get_nearest_pose_ids   (mvsdet.py:67)      -- same ATen ops, kept for completeness
    get_points             (mvsdet.py:1316)
    MVSDet.sample_depth_prob / MVSDet.compute_avg_depth / MVSDet.collect_proj  (mvsdet.py:266, 298, 249)
    CostRegNet_3DGS        (imported at mvsdet.py:32, instantiated at :228) -> mvsdet_amd.costreg.CostRegNet3DGS

With mmengine the patch is applied by adding this module to the config's `custom_imports` AFTER the reference
module; `apply_on_import()` then finds the already imported reference module in sys.modules.

Function-level patching keeps the reference's Python loop structure (k calls of homo_warping, separate softmax,
per-view volume followed by a sum over views).  The fused path -- one plane-sweep launch for all neighbours, fused
soft-max/top-k, fused per-voxel mean -- is `mvsdet_amd.hotpath.MVSDetHotPath.forward_scene`, which replaces
mvsdet.py:404-515 as a block (INTEGRATION.md shows the 12-line edit).
"""
from __future__ import annotations

import sys

import torch

from . import functional as F_


def _sample_depth_prob(self, prob_volume, off_pred, topk=3):
    from . import ops
    prob_volume, off_pred = F_.amp_fp32(prob_volume, off_pred)
    est_depth, est_dens, _, _ = ops.sample_depth_prob(prob_volume, off_pred, float(self.near_far_range[0]),
                                                      float(self.depth_interval), int(topk))
    return est_depth, est_dens


def _compute_avg_depth(self, prob_volume, off_pred):
    from . import ops
    prob_volume, off_pred = F_.amp_fp32(prob_volume, off_pred)
    k = min(3, prob_volume.shape[1])
    return ops.sample_depth_prob(prob_volume, off_pred, float(self.near_far_range[0]), float(self.depth_interval), k)[3]


def _collect_proj(self, w2c, intr, neighbor_ids):
    return F_.collect_proj_for_scene(w2c, intr, neighbor_ids)


PATCHED_FUNCTIONS = {
    "homo_warping": F_.homo_warping,
    "backproject_Weigh": F_.backproject_Weigh,
    "get_nearest_pose_ids": F_.get_nearest_pose_ids,
    "knn": F_.knn,
    "get_points": F_.get_points,
}
def _cost_network():
    from .costreg import CostRegNet3DGS
    return CostRegNet3DGS


# names the reference module looks up when it builds the model (mvsdet.py:32,228: `self.cost_regularization =
# CostRegNet_3DGS()`): the replacement has the same parameter names, so checkpoints load, and routes every layer to
# the HIP kernels in eval mode without autograd: by default bf16x3 with fp16 + MX at conv0 (6.4-6.6 ms instead of 59 ms
# per scene: README); "fp32", the fp32-MFMA kernels (28 ms here), stays a route one can choose (costreg.py)
PATCHED_CLASSES = {
    "CostRegNet_3DGS": _cost_network,
}
PATCHED_METHODS = {
    "sample_depth_prob": _sample_depth_prob,
    "compute_avg_depth": _compute_avg_depth,
    "collect_proj": _collect_proj,
}


def patch_reference(mvsdet_module, lazy_variance: bool = True) -> dict:
    """Rebind the hot-path functions of an imported reference `mvsdet` module; returns {name: original}.
    `lazy_variance`: `homo_warping` returns deferred volumes so that the reference's own variance loop
    (mvsdet.py:453-467) collapses into ONE fused plane-sweep launch (lazywarp.py); anything unexpected falls back to
    the eager kernels."""
    originals = {}
    F_.LAZY_WARP = bool(lazy_variance)
    for name, fn in PATCHED_FUNCTIONS.items():
        if hasattr(mvsdet_module, name):
            originals[name] = getattr(mvsdet_module, name)
            setattr(mvsdet_module, name, fn)
    for name, factory in PATCHED_CLASSES.items():
        if hasattr(mvsdet_module, name):
            originals[name] = getattr(mvsdet_module, name)
            setattr(mvsdet_module, name, factory())
    cls = getattr(mvsdet_module, "MVSDet", None)
    if cls is not None:
        for name, fn in PATCHED_METHODS.items():
            if hasattr(cls, name):
                originals["MVSDet." + name] = getattr(cls, name)
                setattr(cls, name, fn)
    return originals


def unpatch_reference(mvsdet_module, originals: dict) -> None:
    F_.LAZY_WARP = False
    for name, fn in originals.items():
        if name.startswith("MVSDet."):
            setattr(mvsdet_module.MVSDet, name.split(".", 1)[1], fn)
        else:
            setattr(mvsdet_module, name, fn)


def apply_on_import() -> bool:
    """Patch every already-imported module that looks like the reference's mvsdet.py (defines MVSDet,
    homo_warping and backproject_Weigh).  Returns True if something was patched."""
    done = False
    for mod in list(sys.modules.values()):
        if mod is None or not hasattr(mod, "__dict__"):
            continue
        d = mod.__dict__
        if "MVSDet" in d and "backproject_Weigh" in d and "homo_warping" in d and d["backproject_Weigh"] is not F_.backproject_Weigh:
            patch_reference(mod)
            done = True
    return done


def patch_reference_head(head_module) -> dict:
    """Opt-in (the import hook does not apply it): rebind `NerfDetHead.aligned_3d_nms` of an imported reference `nerfdet_head`
    module so that its unmodified `predict` runs the NMS on the HIP kernel (ops.aligned_3d_nms) for CUDA tensors and on the
    original static method for CPU tensors.  Returns {name: original} for `unpatch_reference_head`."""
    from . import ops
    cls = head_module.NerfDetHead
    original = cls.__dict__["aligned_3d_nms"]
    fallback = original.__func__ if isinstance(original, staticmethod) else original

    def aligned_3d_nms(boxes, scores, classes, thresh):
        if boxes.is_cuda:
            return ops.aligned_3d_nms(boxes, scores, classes, thresh)
        return fallback(boxes, scores, classes, thresh)

    aligned_3d_nms.__doc__ = fallback.__doc__
    cls.aligned_3d_nms = staticmethod(aligned_3d_nms)
    return {"NerfDetHead.aligned_3d_nms": original}


def unpatch_reference_head(head_module, originals: dict) -> None:
    for name, fn in originals.items():
        setattr(head_module.NerfDetHead, name.split(".", 1)[1], fn)


def patch_reference_depth_loss(mvsdet_module) -> dict:
    """Opt-in (the import hook does not apply it): rebind `MVSDet.depth_loss_func_new` (mvsdet.py:893-915) of an imported reference
    `mvsdet` module so that lists of device tensors go to the HIP kernel (functional.depth_loss_func_new: no `nonzero`, no host
    synchronisation) and anything else to the original.  An unmodified `extract_feat` leaves `est_depth_crop` empty
    (mvsdet.py:400,698), so this matters once the caller fills that list.  Returns {name: original} for
    `unpatch_reference_depth_loss`."""
    cls = mvsdet_module.MVSDet
    original = cls.__dict__["depth_loss_func_new"]

    def depth_loss_func_new(self, est_depth, gt_depth):
        if len(est_depth) > 0 and all(getattr(t, "is_cuda", False) for t in est_depth):
            return F_.depth_loss_func_new(est_depth, gt_depth)
        return original(self, est_depth, gt_depth)

    depth_loss_func_new.__doc__ = original.__doc__
    cls.depth_loss_func_new = depth_loss_func_new
    return {"MVSDet.depth_loss_func_new": original}


def unpatch_reference_depth_loss(mvsdet_module, originals: dict) -> None:
    for name, fn in originals.items():
        setattr(mvsdet_module.MVSDet, name.split(".", 1)[1], fn)


def patch_reference_photometric(mvsdet_module) -> dict:
    """Opt-in (the import hook does not apply it): rebind `MVSDet.warp_img` (mvsdet.py:701-768) and `MVSDet.photometric_loss`
    (:845-874) of an imported reference `mvsdet` module so that device tensors go to the HIP kernels (functional.warp_img /
    functional.photometric_loss: no torch.inverse, no host synchronisation, no gathers) and anything else to the originals.  The
    reference ships both call sites commented out (mvsdet.py:687-692, 838-839): this matters once the caller re-enables them.
    Returns {name: original} for `unpatch_reference_photometric`."""
    cls = mvsdet_module.MVSDet
    originals = {"MVSDet.warp_img": cls.__dict__["warp_img"], "MVSDet.photometric_loss": cls.__dict__["photometric_loss"]}
    warp_original, loss_original = originals["MVSDet.warp_img"], originals["MVSDet.photometric_loss"]

    def warp_img(self, ref_imgs, neighbor_ids, ref_w2c, ref_feat_intrinsic, ref_depth):
        if getattr(ref_imgs, "is_cuda", False) and getattr(ref_depth, "is_cuda", False):
            return F_.warp_img(ref_imgs, neighbor_ids, ref_w2c, ref_feat_intrinsic, ref_depth)
        return warp_original(self, ref_imgs, neighbor_ids, ref_w2c, ref_feat_intrinsic, ref_depth)

    def photometric_loss(self, warped_img_list, mask_list, chose_ref_img_list):
        if len(warped_img_list) > 0 and all(getattr(t, "is_cuda", False) for t in warped_img_list):
            return F_.photometric_loss(warped_img_list, mask_list, chose_ref_img_list)
        return loss_original(self, warped_img_list, mask_list, chose_ref_img_list)

    warp_img.__doc__, photometric_loss.__doc__ = warp_original.__doc__, loss_original.__doc__
    cls.warp_img, cls.photometric_loss = warp_img, photometric_loss
    return originals


def unpatch_reference_photometric(mvsdet_module, originals: dict) -> None:
    for name, fn in originals.items():
        setattr(mvsdet_module.MVSDet, name.split(".", 1)[1], fn)


SPLATTING_EXTENSION = "diff_gaussian_rasterization"


def patch_reference_splatting(splatting_module=None) -> dict:
    """Opt-in (the import hook does not apply it): make `import diff_gaussian_rasterization` resolve to
    mvsdet_amd.diff_gaussian_rasterization when the real extension cannot be imported (it has no ROCm build), so that the reference's
    unmodified gs_src/model/decoder/cuda_splatting.py::render_cuda imports and runs on the HIP rasteriser.  A real, importable
    extension is left alone.  splatting_module: an already imported module that took the two classes by `from ... import` (a
    stand-in, or cuda_splatting itself imported against a stub) -- its `GaussianRasterizationSettings` / `GaussianRasterizer` are
    rebound too.  Returns what `unpatch_reference_splatting` needs."""
    import importlib

    from . import diff_gaussian_rasterization as shim
    state = {"registered": False, "module": splatting_module, "originals": {}}
    try:
        importlib.import_module(SPLATTING_EXTENSION)
    except ImportError:
        sys.modules[SPLATTING_EXTENSION] = shim
        state["registered"] = True
    if splatting_module is not None and sys.modules.get(SPLATTING_EXTENSION) is shim:
        for name in ("GaussianRasterizationSettings", "GaussianRasterizer"):
            state["originals"][name] = getattr(splatting_module, name, None)
            setattr(splatting_module, name, getattr(shim, name))
    return state


def unpatch_reference_splatting(state: dict) -> None:
    from . import diff_gaussian_rasterization as shim
    if state.get("registered") and sys.modules.get(SPLATTING_EXTENSION) is shim:
        del sys.modules[SPLATTING_EXTENSION]
    for name, original in state.get("originals", {}).items():
        if original is None:
            delattr(state["module"], name)
        else:
            setattr(state["module"], name, original)


def patch_reference_nms3d(head_module) -> dict:
    """Opt-in (the import hook does not apply it): rebind the module-global `nms3d` of an imported reference `nerfdet_head` module
    (mmcv.ops.nms3d, which ImVoxelHead_ARKit._single_scene_multiclass_nms calls) so that its unmodified predict runs the rotated
    NMS on the HIP kernel (ops.nms3d) for CUDA tensors and the original for anything else.  Returns {name: original} for
    `unpatch_reference_nms3d`."""
    from . import ops
    original = head_module.nms3d

    def nms3d(boxes, scores, iou_threshold):
        if boxes.is_cuda:
            return ops.nms3d(boxes, scores, iou_threshold)
        return original(boxes, scores, iou_threshold)

    nms3d.__doc__ = getattr(original, "__doc__", None)
    head_module.nms3d = nms3d
    return {"nms3d": original}


def unpatch_reference_nms3d(head_module, originals: dict) -> None:
    for name, fn in originals.items():
        setattr(head_module, name, fn)


def patch_reference_indoor_eval(metric_module, device="cuda") -> dict:
    """Opt-in (the import hook does not apply it): rebind the module-global `indoor_eval` of an imported reference module that
    calls it (mmdet3d.evaluation.metrics.indoor_metric, whose IndoorMetric.compute_metrics does; or
    mmdet3d.evaluation.functional.indoor_eval itself) to evaluation.indoor_eval, which scores the detections on `device`
    (csrc/evalmap.hip): the mathematical function of the reference's IoU, not mmcv's box_iou_rotated rounding.  Returns
    {name: original} for `unpatch_reference_indoor_eval`."""
    from . import evaluation
    original = metric_module.indoor_eval

    def indoor_eval(gt_annos, dt_annos, metric, label2cat, logger=None, box_mode_3d=None):
        return evaluation.indoor_eval(gt_annos, dt_annos, metric, label2cat, logger=logger, box_mode_3d=box_mode_3d, device=device)

    indoor_eval.__doc__ = getattr(original, "__doc__", None)
    metric_module.indoor_eval = indoor_eval
    return {"indoor_eval": original}


def unpatch_reference_indoor_eval(metric_module, originals: dict) -> None:
    for name, fn in originals.items():
        setattr(metric_module, name, fn)


def patch_reference_nvs_scores(mvsdet_module) -> dict:
    """Opt-in (the import hook does not apply it): rebind the module-globals `save_rendered_img_Image` and `save_rendered_depth` of an
    imported reference `mvsdet` module (imported at mvsdet.py:17 from nerf_utils/save_rendered_img.py, called by MVSDet.predict at
    :1020 and :1024).  With save_dir None the replacements score the scene on the tensors' device (functional.save_rendered_img_Image
    / save_rendered_depth over csrc/nvsmetric.hip: no per-view copies of the images to the host, no skimage) and return host numbers,
    because predict stores them on the data sample: one read-back per call.  With a save_dir (the pictures) they call the
    originals.  Returns {name: original} for `unpatch_reference_nvs_scores`."""
    originals = {"save_rendered_img_Image": mvsdet_module.save_rendered_img_Image,
                 "save_rendered_depth": mvsdet_module.save_rendered_depth}
    img_original, depth_original = originals["save_rendered_img_Image"], originals["save_rendered_depth"]

    def save_rendered_img_Image(pred, gt, img_meta, save_dir=None):
        if save_dir is not None:
            return img_original(pred, gt, img_meta, save_dir=save_dir)
        psnr, ssim, _ = F_.save_rendered_img_Image(pred, gt, img_meta)
        psnr, ssim = torch.stack((psnr, ssim)).cpu().tolist()
        return psnr, ssim, 0

    def save_rendered_depth(pred, gt, img_meta, save_dir=None):
        if save_dir is not None:
            return depth_original(pred, gt, img_meta, save_dir=save_dir)
        return float(F_.save_rendered_depth(pred, gt, img_meta).cpu())

    save_rendered_img_Image.__doc__ = getattr(img_original, "__doc__", None)
    save_rendered_depth.__doc__ = getattr(depth_original, "__doc__", None)
    mvsdet_module.save_rendered_img_Image, mvsdet_module.save_rendered_depth = save_rendered_img_Image, save_rendered_depth
    return originals


def unpatch_reference_nvs_scores(mvsdet_module, originals: dict) -> None:
    for name, fn in originals.items():
        setattr(mvsdet_module, name, fn)
