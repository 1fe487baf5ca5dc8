"""gaustudio_amd: MI355X-native (gfx950) differentiable 3D-Gaussian rasterizer behind GauStudio's
`gaustudio_diff_gaussian_rasterization` operator interface.  See DESIGN.md."""
from .rasterizer import (  # noqa: F401
    GaussianRasterizationSettings,
    GaussianRasterizer,
    _RasterizeGaussians,
    rasterize_gaussians,
)
from .options import options  # noqa: F401,E402  (per-call options: tile band, fast_exp, kernel A/B switches)
from .tsdf_rgbd import ColorTSDFVolume, fuse_rgbd  # noqa: F401,E402  (coloured TSDF fusion of posed RGB-D frames)
from .visual_hull import VisualHull, carve, visual_hull_init  # noqa: F401,E402  (silhouette carving and Gaussian seeds)
from .voxelize import VoxelGrid, closest_on_mesh, voxel_init, voxel_seeds, voxelize_mesh  # noqa: F401,E402  (mesh -> voxels -> Gaussian seeds)
# point cloud -> Gaussian seeds; `gaustudio_amd.pcd_init` stays the module (its function of that name is pcd_init.pcd_init)
from .pcd_init import depth_seeds, mean_dist2, pcd_init_from_ply, point_seeds, sky_seeds  # noqa: F401,E402
# Scaffold-GS: anchors + MLPs + camera -> Gaussians -> render (the anchor-based family of the reference)
from .scaffold import (ScaffoldGaussians, ScaffoldModel, decode, decode_torch, render_scaffold,  # noqa: F401,E402
                       visible_anchors)
# the training loss: (1 - lambda) L1 + lambda (1 - SSIM), fused forward and backward
from .losses import l1_loss, photometric_loss, photometric_loss_with_parts, ssim, ssim_map  # noqa: F401,E402
# the optimiser half of training: a one-launch (visibility-sparse) Adam and adaptive density control
from .optim import DensifyReport, DensityControl, GaussianAdam  # noqa: F401,E402
# Scaffold-GS anchor control: grow anchors by voxel level, prune them, carry a torch Adam's moments
from .anchor_control import AnchorControl, AnchorReport  # noqa: F401,E402
# the geometric regularisers of 2D Gaussian surfel training: normal consistency + depth distortion on the surfel allmap
from .surfel_losses import (intrinsics_from_settings, surfel_geometric_loss, surfel_geometric_loss_with_parts,  # noqa: F401,E402
                            surfel_maps)

__version__ = "0.1.0"
