"""The 2D Gaussian surfel ("2DGS") operator behind the import name `diff_surfel_rasterization`: the settings tuple, the
nn.Module front door and the autograd Function that gaustudio/renderers/surfel_renderer.py uses.

    color [3,H,W], radii [P] int32, allmap [7,H,W] = GaussianRasterizer(settings)(means3D, means2D, opacities, shs | colors_precomp,
                                                                               scales [P,2], rotations [P,4])
    allmap = [expected depth, alpha, normal xyz (view space), median depth, depth distortion]

Everything numeric happens in libgsrast.so (gsr_surfel.hip, hand-written HIP for gfx950) through the torch adapter
(csrc/torch_binding.cpp: rasterize_surfels / rasterize_surfels_backward).  The semantics and the constants they pin are
listed in INTEGRATION.md ("2D Gaussian surfels"); tests/surfel_model.py restates them in float64.
"""
import torch
import torch.nn as nn

from . import _C
from .options import clear_grad_mode as _clear_grad_mode, for_forward as _options_for_forward, note_grad_mode as _note_grad_mode
from .rasterizer import GaussianRasterizationSettings, _absent  # noqa: F401  (the same 12 fields, in the same order)


def _check_inputs(means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp):
    """Argument validation, before any native call.  Every failure names the problem."""
    if (shs is None) == (colors_precomp is None):
        raise ValueError('diff_surfel_rasterization: provide exactly one of either SHs or precomputed colors')
    if cov3D_precomp is not None:
        raise ValueError("diff_surfel_rasterization: cov3D_precomp is not supported. In 2DGS that slot holds a precomputed 3x3 "
                         "splat-to-pixel matrix, not a 3D covariance (got shape %s; a [P,6] tensor is a 3D-Gaussian covariance, "
                         "e.g. from compute_cov3D_python=True). Pass scales [P,2] and rotations [P,4] instead."
                         % (tuple(cov3D_precomp.shape),))
    if scales is None or rotations is None:
        raise ValueError("diff_surfel_rasterization: scales [P,2] and rotations [P,4] are required")
    if means3D.ndim != 2 or means3D.shape[1] != 3:
        raise ValueError("diff_surfel_rasterization: means3D must have dimensions (num_points, 3), got %s" % (tuple(means3D.shape),))
    P = means3D.shape[0]
    if scales.ndim != 2 or tuple(scales.shape) != (P, 2):
        raise ValueError("diff_surfel_rasterization: scales must be [P,2] (two surfel scales per Gaussian), got %s for P = %d"
                         % (tuple(scales.shape), P))
    if rotations.ndim != 2 or tuple(rotations.shape) != (P, 4):
        raise ValueError("diff_surfel_rasterization: rotations must be [P,4] quaternions, got %s for P = %d" % (tuple(rotations.shape), P))
    if opacities.numel() != P:
        raise ValueError("diff_surfel_rasterization: opacities must hold one value per Gaussian, got %d for P = %d" % (opacities.numel(), P))


class _RasterizeSurfels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, raster_settings):
        rs = raster_settings
        opts = _options_for_forward(any(ctx.needs_input_grad))
        num_rendered, color, radii, allmap, geom_buf, binning_buf, img_buf = _C.native().rasterize_surfels(
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, float(rs.scale_modifier), rs.viewmatrix, rs.projmatrix,
            int(rs.image_height), int(rs.image_width), sh, int(rs.sh_degree), rs.campos, bool(rs.debug), list(opts))
        ctx.raster_settings = rs
        ctx.gsr_options = opts
        ctx.num_rendered = num_rendered
        ctx.opacity_shape = opacities.shape
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, radii, sh, color, allmap, geom_buf, binning_buf, img_buf)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return color, radii, allmap

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_allmap):
        rs = ctx.raster_settings
        colors_precomp, means3D, scales, rotations, radii, sh, color, allmap, geom_buf, binning_buf, img_buf = ctx.saved_tensors
        e = _absent()
        (g_means2D, g_colors, g_opacities, g_means3D, g_sh, g_scales, g_rotations) = _C.native().rasterize_surfels_backward(
            means3D, radii, colors_precomp, scales, rotations, float(rs.scale_modifier), color, allmap,
            e if grad_color is None else grad_color, e if grad_allmap is None else grad_allmap, sh, int(rs.sh_degree), geom_buf,
            ctx.num_rendered, binning_buf, img_buf, bool(rs.debug), list(ctx.gsr_options))
        g_opacities = g_opacities.reshape(ctx.opacity_shape)
        if sh.numel() == 0:
            g_sh = None
        if colors_precomp.numel() == 0:
            g_colors = None
        return g_means3D, g_means2D, g_sh, g_colors, g_opacities, g_scales, g_rotations, None


def rasterize_surfels(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, raster_settings):
    _note_grad_mode(torch.is_grad_enabled())
    try:
        return _RasterizeSurfels.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, raster_settings)
    finally:
        _clear_grad_mode()


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """bool[P]: Gaussians passing the near-plane test for this camera."""
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        _check_inputs(means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_surfels(means3D, means2D, shs if shs is not None else _absent(),
                                 colors_precomp if colors_precomp is not None else _absent(), opacities, scales, rotations,
                                 self.raster_settings)
