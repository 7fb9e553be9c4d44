"""The call form of the `diff_gaussian_rasterization` extension over the HIP rasteriser (csrc/splat.hip through ops.splat).

gs_src/model/decoder/cuda_splatting.py imports `GaussianRasterizationSettings` and `GaussianRasterizer` from an external CUDA
extension that has no ROCm build.  These two classes take what render_cuda hands them and run one view of `ops.splat.rasterize`.
`integration.patch_reference_splatting()` registers this module under the extension's name; nothing does so by itself.

The reference's own, unmodified render_depth_cuda runs through these classes too: it hands every Gaussian's mapped depth over as
`colors_precomp` in three equal channels and averages them, at the price of a second full rasterisation.  The fused form -- depth as a
fourth blended channel of the colour's pass, or alone -- is reached through `functional.render_depth_cuda` and
`functional.decode_splatting(depth_mode=...)`, not through this shim: the extension's call form has no depth output.

What is not here: `scales` / `rotations` (the covariance built inside the extension), `scale_modifier` other than 1 and the
orthographic form.  There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple, Union

import torch
from torch import Tensor, nn

from . import ops
from .ops._common import req


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: Union[float, Tensor]
    tanfovy: Union[float, Tensor]
    bg: Tensor
    scale_modifier: float
    viewmatrix: Tensor     # (4,4), transposed (row-vector form), as render_cuda passes it
    projmatrix: Tensor     # (4,4), the full projection, transposed
    sh_degree: int
    campos: Tensor
    prefiltered: bool = False
    debug: bool = False
    max_keys: Optional[int] = None   # ours: (Gaussian, tile) pairs the view may have (default 8 G)


def _cams(s: GaussianRasterizationSettings) -> Tensor:
    """(1,40) camera block of ops.splat from the settings, assembled on the device: no host read, scale 1."""
    dev = s.viewmatrix.device

    def scalar(v):
        return v.reshape(1).to(dev, torch.float32) if isinstance(v, Tensor) else torch.full((1,), float(v), dtype=torch.float32, device=dev)
    return torch.cat([s.viewmatrix.reshape(16), s.projmatrix.reshape(16), scalar(s.tanfovx), scalar(s.tanfovy), s.campos.reshape(3),
                      torch.ones(1, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.float32, device=dev)]).reshape(1, ops.splat.SPLAT_CAM)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D: Tensor, means2D: Optional[Tensor] = None, opacities: Optional[Tensor] = None, shs: Optional[Tensor] = None,
                colors_precomp: Optional[Tensor] = None, scales: Optional[Tensor] = None, rotations: Optional[Tensor] = None,
                cov3D_precomp: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """means3D (G,3), opacities (G,1), shs (G,d_sh,3) or colors_precomp (G,3), cov3D_precomp (G,6) the upper triangle ->
        (image (3,H,W), radii (G) int32).  means2D is accepted and gets no gradient."""
        s = self.raster_settings
        if scales is not None or rotations is not None or cov3D_precomp is None:
            raise NotImplementedError("mvsdet_amd.diff_gaussian_rasterization: pass cov3D_precomp (G,6); building the covariance from "
                                      "scales / rotations inside the rasteriser is not implemented")
        if (shs is None) == (colors_precomp is None):
            raise ValueError("mvsdet_amd.diff_gaussian_rasterization: pass exactly one of shs and colors_precomp")
        if float(s.scale_modifier) != 1.0:
            raise NotImplementedError("mvsdet_amd.diff_gaussian_rasterization: scale_modifier must be 1")
        if opacities is None:
            raise ValueError("mvsdet_amd.diff_gaussian_rasterization: opacities are required")
        for name, t in (("means3D", means3D), ("opacities", opacities), ("cov3D_precomp", cov3D_precomp), ("viewmatrix", s.viewmatrix),
                        ("projmatrix", s.projmatrix), ("campos", s.campos), ("bg", s.bg)):
            req(t, name)
        G = means3D.shape[0]
        if tuple(cov3D_precomp.shape) != (G, 6) or opacities.numel() != G:
            raise ValueError(f"mvsdet_amd.diff_gaussian_rasterization: cov3D_precomp {tuple(cov3D_precomp.shape)} must be ({G},6) and "
                             f"opacities {tuple(opacities.shape)} ({G},1)")
        if shs is not None:
            req(shs, "shs", dim=3)
            if shs.shape[1] != (int(s.sh_degree) + 1) ** 2:
                raise ValueError(f"mvsdet_amd.diff_gaussian_rasterization: shs {tuple(shs.shape)} for sh_degree {s.sh_degree}")
            harmonics = shs.permute(0, 2, 1)                     # (G,3,d_sh), read in place
        else:
            req(colors_precomp, "colors_precomp", dim=2)
            harmonics = colors_precomp[:, :, None]
        row, col = torch.triu_indices(3, 3, device=means3D.device)
        cov = torch.zeros((G, 3, 3), dtype=torch.float32, device=means3D.device)
        cov = cov.index_put((torch.arange(G, device=means3D.device)[:, None], row[None], col[None]), cov3D_precomp)
        keys = ops.splat.default_max_keys(G) if s.max_keys is None else int(s.max_keys)
        image, workspace = ops.splat.rasterize(means3D, cov, harmonics, opacities.reshape(G), _cams(s), s.bg.reshape(1, 3),
                                               int(s.image_height), int(s.image_width), keys, shs is not None)
        return image[0], ops.splat.radii(workspace, 1, G)[0]
