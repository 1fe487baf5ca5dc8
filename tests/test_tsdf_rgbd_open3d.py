"""Agreement with Open3D's ScalableTSDFVolume(color_type=RGB8).integrate / extract_triangle_mesh, where Open3D is installed (it
is not in the ROCm image; this skips otherwise, as the vdbfusion / PyTorch3D / mesh_clean pins do).  Until it runs, Open3D
parity of tests/tsdf_rgbd_model.py -- and with it of gaustudio_amd.tsdf_rgbd -- is unpinned.

What can agree: Open3D keeps 16^3-voxel units where the model keeps 8^3 blocks (only far-from-surface voxels holding
tsdf = 1 differ), uses its own marching-cubes triangulation, and places voxel (i, j, k) at (i, j, k) * voxel_length + half a
voxel like the model.  So the test compares the SURFACE: every vertex of either mesh lies within a fraction of a voxel of the
other mesh's vertex set, and the colours of nearest vertices agree to a few grey levels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_rgbd_model as M  # noqa: E402

o3d = pytest.importorskip("open3d")

VL, TR = 0.05, 0.15
K = (110.0, 110.0, 47.5, 35.5)
CENTRE = np.array([-1.3, -0.7, -2.1])


def _frames():
    import test_gpu_tsdf_rgbd as T
    out = []
    for n, axis in enumerate([(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]):
        E = T.look_at(CENTRE + 2.0 * np.asarray(axis, float) / np.sqrt(3.0), CENTRE, roll=0.2 * n)
        out.append(T.sphere_frame(72, 96, K, E) + (E,))
    return out


def _nearest(a, b):
    d = np.linalg.norm(a[:, None, :] - b[None, :, :], axis=2)
    return d.min(1), d.argmin(1)


def test_model_surface_equals_open3d():
    frames = _frames()
    model = M.ModelVolume(VL, TR)
    vol = o3d.pipelines.integration.ScalableTSDFVolume(voxel_length=VL, sdf_trunc=TR,
                                                       color_type=o3d.pipelines.integration.TSDFVolumeColorType.RGB8)
    intr = o3d.camera.PinholeCameraIntrinsic(96, 72, K[0], K[1], K[2], K[3])
    for d, c, E in frames:
        model.integrate(d, c, K, E, depth_trunc=5.0)
        rgbd = o3d.geometry.RGBDImage.create_from_color_and_depth(o3d.geometry.Image(np.ascontiguousarray(c)), o3d.geometry.Image(d),
                                                                  depth_scale=1.0, depth_trunc=5.0, convert_rgb_to_intensity=False)
        vol.integrate(rgbd, intr, E)
    mesh = vol.extract_triangle_mesh()
    ov, oc = np.asarray(mesh.vertices), np.asarray(mesh.vertex_colors)
    mv, _, mc = model.extract_triangle_mesh()
    assert len(ov) and len(mv)
    d1, i1 = _nearest(mv.astype(np.float64), ov)
    d2, _ = _nearest(ov, mv.astype(np.float64))
    assert d1.max() < 0.5 * VL and d2.max() < 0.5 * VL
    assert np.abs(mc - oc[i1]).max() < 8.0 / 255
