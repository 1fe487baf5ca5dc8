"""Parity of voxelize_mesh with Open3D's VoxelGrid.create_from_triangle_mesh_within_bounds, which the reference's
VoxelInitializer calls (mesh.py:354-379).  Open3D is not a dependency: the test runs where it is installed and the parity stays
unpinned elsewhere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_voxel_model as mm  # noqa: E402

o3d = pytest.importorskip("open3d")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["icosphere16", "ellipsoid24", "general"])
def test_same_voxels_and_centres_as_open3d(case):
    import torch
    from gaustudio_amd import voxelize_mesh
    if case == "general":
        v, f = mm.ellipsoid()
        vn = v.astype(np.float64) * 0.45 + np.array([0.55, 1.0, -1.25])
        vs, lo, hi = 0.1, (0.3, -0.2, 0.1), (1.3, 0.5, 1.3)
    else:
        v, f = mm.icosphere(1) if case == "icosphere16" else mm.ellipsoid()
        vn, _, _ = mm.normalize_mesh(v)
        vs, lo, hi = (1 / 16 if case == "icosphere16" else 1 / 24), (-0.5,) * 3, (0.5,) * 3
    grid = voxelize_mesh(torch.from_numpy(vn).cuda(), torch.from_numpy(f).cuda(), vs, lo, hi)
    mesh = o3d.geometry.TriangleMesh()
    mesh.vertices = o3d.utility.Vector3dVector(vn)
    mesh.triangles = o3d.utility.Vector3iVector(f)
    ref = o3d.geometry.VoxelGrid.create_from_triangle_mesh_within_bounds(mesh, voxel_size=vs, min_bound=np.array(lo, dtype=np.float64),
                                                                         max_bound=np.array(hi, dtype=np.float64))
    theirs = np.array([vox.grid_index for vox in ref.get_voxels()], dtype=np.int64).reshape(-1, 3)      # a hash map's order
    n1, n2 = grid.shape[1], grid.shape[2]
    order = np.argsort((theirs[:, 0] * n1 + theirs[:, 1]) * n2 + theirs[:, 2])
    theirs = theirs[order]
    ours = grid.grid_index.cpu().numpy()
    assert np.array_equal(ours, theirs)
    centres = np.array([ref.get_voxel_center_coordinate(g.astype(np.int32)) for g in theirs])
    assert np.array_equal(grid.centers().cpu().numpy(), centres)
