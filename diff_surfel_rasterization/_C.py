"""Native entry points of the surfel operator (csrc/torch_binding.cpp, over gsr_surfel_forward / gsr_surfel_backward of
include/gsrast.h).  No CPU fallback: without the built libraries or a ROCm device the calls raise.

    rasterize_surfels(...)           -> (num_rendered, color [3,H,W], radii [P], allmap [7,H,W], geomBuffer, binningBuffer, imgBuffer)
    rasterize_surfels_backward(...)  -> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dsh, dL_dscales, dL_drotations)
    mark_visible(means3D, viewmatrix, projmatrix) -> bool[P]
"""
from gaustudio_amd import _C as _gsr


def rasterize_surfels(*args, **kwargs):
    return _gsr.native().rasterize_surfels(*args, **kwargs)


def rasterize_surfels_backward(*args, **kwargs):
    return _gsr.native().rasterize_surfels_backward(*args, **kwargs)


def mark_visible(means3D, viewmatrix, projmatrix):
    return _gsr.mark_visible(means3D, viewmatrix, projmatrix)
