"""CPU (-m "not gpu"): the model of the mesh cleaning stage (tests/mesh_clean_model.py) on hand-built cases, its two
clustering paths against each other, the round structure of the device algorithm, the Python boundary of
gaustudio_amd.mesh_clean and the PLY mesh container of gaustudio_amd.formats."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_model as cm  # noqa: E402


@pytest.mark.parametrize("name", sorted(cm.hand_cases()))
def test_hand_built_cases(name):
    faces, C = cm.hand_cases()[name]
    labels, counts = cm.cluster_bfs(faces)
    assert counts.size == C and counts.sum() == len(faces)
    l2, c2 = cm.cluster_scipy(faces)
    assert np.array_equal(labels, l2) and np.array_equal(counts, c2)


def test_shared_vertex_does_not_connect_shared_edge_does():
    labels, counts = cm.cluster_bfs(cm.hand_cases()["two_tets_sharing_a_vertex"][0])
    assert labels.tolist() == [0] * 4 + [1] * 4 and counts.tolist() == [4, 4]
    labels, counts = cm.cluster_bfs(cm.hand_cases()["two_tets_sharing_an_edge"][0])
    assert labels.tolist() == [0] * 8 and counts.tolist() == [8]
    labels, counts = cm.cluster_bfs(cm.hand_cases()["fan_of_three_on_one_edge"][0])
    assert counts.tolist() == [3]


def test_repeated_index_triangle_behaves_as_its_literal_edges():
    # (0,0,1) has the edges {0,0}, {0,1}, {0,1}: it joins (1,0,2) through {0,1} and (0,0,9) through {0,0}
    labels, counts = cm.cluster_bfs(cm.hand_cases()["repeated_index"][0])
    assert labels.tolist() == [0, 0, 1, 2, 0] and counts.tolist() == [3, 1, 1]


def test_empty_mesh():
    for fn in (cm.cluster_bfs, cm.cluster_scipy):
        labels, counts = fn(np.zeros((0, 3), np.int32))
        assert labels.shape == (0,) and counts.shape == (0,)
    v, f, vi, fi, removed = cm.remove_small_components(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert v.shape == (0, 3) and f.shape == (0, 3) and vi.shape == (0,) and fi.shape == (0,) and removed == 0


def test_cluster_numbering_follows_the_lowest_triangle_index_after_a_shuffle():
    rng = np.random.default_rng(3)
    faces = np.concatenate([np.array(cm.tetrahedron(*(4 * k + np.arange(4))), np.int32) for k in range(6)])
    perm = rng.permutation(len(faces))
    shuffled = faces[perm]
    for fn in (cm.cluster_bfs, cm.cluster_scipy):
        labels, counts = fn(shuffled)
        assert counts.tolist() == [4] * 6
        first = [int(np.nonzero(labels == c)[0][0]) for c in range(6)]
        assert first == sorted(first) and first[0] == 0
        # the same partition as before the shuffle
        assert all(len(set((perm[labels == c] // 4).tolist())) == 1 for c in range(6))


def test_keep_rule_is_strict_at_exactly_half():
    counts = np.array([3, 10, 5, 6, 10], np.int32)
    assert cm.keep_clusters(counts, 0.5).tolist() == [False, True, False, True, True]
    v = np.zeros((40, 3), np.float32)
    # clusters of 4 (a tetrahedron) and 2 (two triangles on one edge): 2 == 0.5 * 4 goes
    faces = np.array(cm.tetrahedron(0, 1, 2, 3) + [[10, 11, 12], [11, 10, 13]], np.int32)
    v2, f2, vi, fi, removed = cm.remove_small_components(v, faces, 0.5)
    assert removed == 2 and fi.tolist() == [0, 1, 2, 3] and vi.tolist() == [0, 1, 2, 3]
    assert cm.remove_small_components(v, faces, 0.49)[4] == 0


@pytest.mark.parametrize("F,V", [(1, 3), (50, 12), (400, 100), (400, 1200), (3000, 60), (3000, 750), (3000, 9000)])
def test_bfs_equals_scipy_on_random_soups(F, V):
    faces = cm.random_soup(np.random.default_rng(F + V), F, V)
    a, b = cm.cluster_bfs(faces), cm.cluster_scipy(faces)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the device algorithm's fixed point: every triangle labelled with the lowest triangle of its cluster
    u, w = cm.union_edges(faces)
    low, rounds = cm.fastsv(F, u, w)
    first = np.full(a[1].size, F)
    np.minimum.at(first, a[0], np.arange(F))
    assert np.array_equal(low, first[a[0]])
    assert rounds <= 4 * max(1, math.ceil(math.log2(F)))


@pytest.mark.parametrize("shuffle", [False, True])
def test_rounds_of_the_device_algorithm_do_not_follow_the_diameter(shuffle):
    F = 1 << 16
    faces = cm.strip(F)
    if shuffle:
        faces = faces[np.random.default_rng(1).permutation(F)]
    u, w = cm.union_edges(faces)
    low, rounds = cm.fastsv(F, u, w)
    assert (low == 0).all()
    assert rounds <= 4 * math.ceil(math.log2(F)), rounds


def test_areas_and_mask_removal():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 5, 5], [0, 0, 3]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 4], [0, 2, 4]], np.int32)
    assert cm.triangle_areas(v, faces).tolist() == [1.0, 1.5, 3.0]
    labels, counts = cm.cluster_bfs(faces)
    assert cm.cluster_areas(v, faces, labels, counts.size).tolist() == [5.5]
    v2, f2, vi, fi = cm.remove_triangles_by_mask(v, faces, np.array([False, True, False]))
    assert fi.tolist() == [0, 2] and vi.tolist() == [0, 1, 2, 4]
    assert f2.tolist() == [[0, 1, 2], [0, 2, 3]] and np.array_equal(v2, v[[0, 1, 2, 4]])


# ------------------------------------------------------------------------------------------------------ the Python boundary
def test_cpu_tensors_are_rejected():
    from gaustudio_amd import mesh_clean as mc
    v, f = torch.zeros(4, 3), torch.tensor(cm.tetrahedron(0, 1, 2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        mc.cluster_connected_triangles(f)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        mc.remove_triangles_by_mask(v, f, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        mc.remove_small_components(v, f)
    with pytest.raises(RuntimeError, match="ROCm devices only"):         # an empty mesh on the CPU is still refused
        mc.remove_small_components(torch.zeros(0, 3), torch.zeros((0, 3), dtype=torch.int32))


def test_bad_shapes_and_dtypes_are_rejected_before_the_device_check():
    from gaustudio_amd import mesh_clean as mc
    v, f = torch.zeros(4, 3), torch.tensor(cm.tetrahedron(0, 1, 2, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match=r"faces must have shape \[F, 3\]"):
        mc.cluster_connected_triangles(f.reshape(-1))
    with pytest.raises(ValueError, match=r"faces must have shape \[F, 3\]"):
        mc.remove_small_components(v, torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(TypeError, match="int32 or int64"):
        mc.cluster_connected_triangles(f.float())
    with pytest.raises(TypeError, match="torch tensor"):
        mc.cluster_connected_triangles(f.numpy())
    with pytest.raises(TypeError, match="torch tensor"):
        mc.remove_small_components(v.numpy(), f)


def test_keep_rule_of_the_module_equals_the_model():
    from gaustudio_amd import mesh_clean as mc
    rng = np.random.default_rng(0)
    for ratio in (0.5, 0.25, 0.0, 1.0):
        n = rng.integers(1, 40, size=30).astype(np.int32)
        n[7] = n[11] = 40
        n[3] = 20
        assert mc.keep_clusters(torch.from_numpy(n), ratio).numpy().tolist() == cm.keep_clusters(n, ratio).tolist()


def test_extract_triangle_mesh_device_takes_a_clean_ratio():
    import inspect
    from gaustudio_amd.tsdf import TSDFVolume
    p = inspect.signature(TSDFVolume.extract_triangle_mesh_device).parameters
    assert list(p) == ["self", "fill_holes", "min_weight", "clean_ratio"] and p["clean_ratio"].default is None


# ------------------------------------------------------------------------------------------------------ the PLY mesh container
def test_ply_mesh_round_trip_is_byte_exact(tmp_path):
    from gaustudio_amd import formats
    rng = np.random.default_rng(5)
    v = rng.normal(size=(37, 3)).astype(np.float32)
    v[0] = [np.float32(1e-42), -0.0, np.float32(3.4e38)]
    f = rng.integers(0, 37, size=(91, 3)).astype(np.int32)
    path = tmp_path / "fused_mesh.ply"
    formats.write_ply_mesh(path, v, f, comments=("made by a test",))
    v2, f2 = formats.read_ply_mesh(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    formats.write_ply_mesh(path, torch.from_numpy(v), torch.from_numpy(f).long())          # tensors, int64 faces
    v3, f3 = formats.read_ply_mesh(path)
    assert v3.tobytes() == v.tobytes() and np.array_equal(f3, f)
    assert np.array_equal(formats.read_ply_vertices(path)["y"], v[:, 1])                  # the vertex reader stops before the faces


def test_ply_mesh_header_and_layout(tmp_path):
    from gaustudio_amd import formats
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1]], np.int32)
    path = tmp_path / "m.ply"
    formats.write_ply_mesh(path, v, f, comments=("c1",))
    raw = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\ncomment c1\nelement vertex 4\nproperty float x\nproperty float y\n"
              b"property float z\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n")
    assert raw.startswith(header)
    body = raw[len(header):]
    assert len(body) == 4 * 12 + 2 * 13
    assert body[:48] == v.astype("<f4").tobytes()
    assert body[48:] == b"\x03" + f[0].astype("<i4").tobytes() + b"\x03" + f[1].astype("<i4").tobytes()
    with pytest.raises(formats.PlyFormatError):
        formats.write_ply_mesh(path, v, np.array([[0, 1, 4]], np.int32))
    empty = tmp_path / "e.ply"
    formats.write_ply_mesh(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v0, f0 = formats.read_ply_mesh(empty)
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
