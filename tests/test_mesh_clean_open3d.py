"""Agreement with Open3D's TriangleMesh.cluster_connected_triangles / remove_triangles_by_mask / remove_unreferenced_vertices,
where Open3D is installed (it is not in the ROCm image; this skips otherwise, as the vdbfusion / PyTorch3D pins do).  Until it
runs, Open3D parity of tests/mesh_clean_model.py -- and with it of gaustudio_amd.mesh_clean -- is unpinned."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_model as cm  # noqa: E402
import mesh_raster_model as mm  # noqa: E402

o3d = pytest.importorskip("open3d")


def o3d_mesh(verts, faces):
    return o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(np.asarray(verts, np.float64)),
                                     o3d.utility.Vector3iVector(np.asarray(faces, np.int32)))


def cases():
    rng = np.random.default_rng(0)
    out = {name: faces for name, (faces, _) in cm.hand_cases().items()}
    out["soup_small_V"] = cm.random_soup(rng, 3000, 60)
    out["soup_large_V"] = cm.random_soup(rng, 3000, 9000)
    vs, fs = mm.icosphere(3)
    out["icospheres"] = np.concatenate([fs, fs + len(vs), fs + 2 * len(vs)])[rng.permutation(3 * len(fs))]
    return out


@pytest.mark.parametrize("name", sorted(cases()))
def test_model_equals_open3d(name):
    faces = cases()[name]
    verts = np.random.default_rng(1).normal(size=(int(faces.max()) + 1, 3)).astype(np.float32)
    mesh = o3d_mesh(verts, faces)
    clusters, n_triangles, area = (np.asarray(x) for x in mesh.cluster_connected_triangles())
    labels, counts = cm.cluster_bfs(faces)
    assert np.array_equal(clusters, labels) and np.array_equal(n_triangles, counts)
    want = cm.cluster_areas(verts, faces, labels, counts.size)
    assert np.all(np.abs(area - want) <= len(faces) * 2.0 ** -52 * want)
    remove = ~cm.keep_clusters(counts, 0.5)[labels]
    mesh.remove_triangles_by_mask(remove)
    mesh.remove_unreferenced_vertices()
    v2, f2, _, _ = cm.remove_triangles_by_mask(verts, faces, remove)
    assert np.array_equal(np.asarray(mesh.triangles), f2) and np.array_equal(np.asarray(mesh.vertices).astype(np.float32), v2)


@pytest.mark.gpu
def test_device_equals_open3d():
    from gaustudio_amd import mesh_clean
    dev = torch.device("cuda", 0)
    for name, faces in cases().items():
        verts = np.random.default_rng(1).normal(size=(int(faces.max()) + 1, 3)).astype(np.float32)
        mesh = o3d_mesh(verts, faces)
        clusters, n_triangles, _ = (np.asarray(x) for x in mesh.cluster_connected_triangles())
        c, n, _ = mesh_clean.cluster_connected_triangles(torch.from_numpy(faces).to(dev), vertices=torch.from_numpy(verts).to(dev))
        assert np.array_equal(c.cpu().numpy(), clusters) and np.array_equal(n.cpu().numpy(), n_triangles), name
