"""Agreement of mesh_seeds' default normals with Open3D's compute_vertex_normals, which the reference's MeshInitializer calls
(mesh.py:153).  Open3D is not a dependency: the test runs where it is installed and the parity stays unpinned elsewhere
(INTEGRATION.md s21).  Both are area-weighted sums of face normals; Open3D sums in float64."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_init_model as mi  # noqa: E402
import mesh_raster_model as rm  # noqa: E402
from gaustudio_amd import mesh_init  # noqa: E402,F401  (the module whose default normals this pins)

o3d = pytest.importorskip("open3d")


def test_vertex_normals_agree():
    v, f = rm.icosphere(2)
    mesh = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(v.astype(np.float64)), o3d.utility.Vector3iVector(f))
    mesh.compute_vertex_normals()
    theirs = np.asarray(mesh.vertex_normals)
    ours = rm.vertex_normals(v, f)
    assert np.abs(ours - theirs).max() <= 1e-5
    a = mi.seeds(v, f, ours, None, 1)["rot"]
    b = mi.seeds(v, f, theirs.astype(np.float32), None, 1)["rot"]
    well = a[:, 0] > 0.1                         # away from rotations by 180 degrees, where the quaternion is ill-conditioned
    assert np.abs(a[well] - b[well]).max() <= 1e-3
