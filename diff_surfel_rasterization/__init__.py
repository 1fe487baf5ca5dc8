"""Import name of the 2D Gaussian surfel rasterizer for GauStudio (gaustudio/renderers/surfel_renderer.py does
`from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer`).

Nothing lives here: the operator is gaustudio_amd.surfel (hand-written HIP for MI355X in libgsrast.so); this package re-exports it
under the 2DGS module name, with the `_C` submodule holding its native entry points.
"""
from . import _C  # noqa: F401
from gaustudio_amd.surfel import (  # noqa: F401
    GaussianRasterizationSettings,
    GaussianRasterizer,
    _RasterizeSurfels,
    rasterize_surfels,
)

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_surfels", "_RasterizeSurfels", "_C"]
