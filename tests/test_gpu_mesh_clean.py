"""The HIP mesh cleaning stage (gaustudio_amd.mesh_clean over csrc/gsr_mesh_clean.hip) against its CPU model
(tests/mesh_clean_model.py).  Clusters, counts and every compaction output are compared exactly; cluster areas within the
fp64 summation bound F * 2^-52 (the device adds a cluster's triangle areas in a fixed tree, the model one after the other:
two orders of the same non-negative terms, each within (n - 1) * 2^-53 of the exact sum).

Figures on an MI355X (rounds of the 2^20-triangle strip, cap 4 * ceil(log2 F) = 80): see DESIGN.md s13."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_model as cm  # noqa: E402
import mesh_raster_model as mm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def mc():
    from gaustudio_amd import mesh_clean
    return mesh_clean


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_cluster(faces, vertices=None, num_verts=None):
    c, n, a = mc().cluster_connected_triangles(dev(faces), num_verts=num_verts, vertices=None if vertices is None else dev(vertices))
    return c.cpu().numpy(), n.cpu().numpy(), (None if a is None else a.cpu().numpy())


def assert_clusters(faces, model=cm.cluster_bfs, vertices=None, what=""):
    labels, counts = model(faces)
    c, n, a = gpu_cluster(faces, vertices, num_verts=None if vertices is not None else int(faces.max()) + 1 if len(faces) else 0)
    assert c.dtype == np.int32 and n.dtype == np.int32
    assert np.array_equal(c, labels), f"{what}: triangle_clusters differ from the model"
    assert np.array_equal(n, counts), f"{what}: cluster_n_triangles differ from the model"
    if vertices is not None:
        want = cm.cluster_areas(vertices, faces, labels, counts.size)
        F = len(faces)
        err = np.abs(a - want)
        print(f"{what}: F={F} C={counts.size} largest={counts.max()} rounds={mc().last_rounds} "
              f"max area rel err={np.max(err / np.maximum(want, 1e-300)):.3e} (bound {F * 2.0 ** -52:.3e})")
        assert a.dtype == np.float64 and (err <= F * 2.0 ** -52 * want).all(), f"{what}: cluster_area outside F * 2^-52"
    return labels, counts


def interleaved_icospheres(count, subdiv, rng):
    vs, fs = [], []
    base = 0
    for k in range(count):
        v, f = mm.icosphere(subdiv)
        vs.append(v * (0.5 + 0.1 * k) + [3.0 * k, 0, 0])
        fs.append(f + base)
        base += len(v)
    faces = np.concatenate(fs).astype(np.int32)
    return np.concatenate(vs).astype(np.float32), faces[rng.permutation(len(faces))]


@pytest.mark.parametrize("name", sorted(cm.hand_cases()))
def test_hand_built_cases(name):
    faces, C = cm.hand_cases()[name]
    rng = np.random.default_rng(0)
    verts = rng.normal(size=(int(faces.max()) + 1, 3)).astype(np.float32)
    _, counts = assert_clusters(faces, vertices=verts, what=name)
    assert counts.size == C


SOUPS = [(1, 3), (2, 6), (7, 2), (63, 40), (64, 16), (65, 195), (1000, 250), (1000, 3000), (4097, 1025), (12289, 12289),
         (50000, 12500), (50000, 50000), (50000, 150000),
         # few vertices: most triangles share an edge with another one -> one giant component and a tail of small ones
         (1000, 30), (20000, 150), (50000, 400)]


@pytest.mark.parametrize("F,V", SOUPS)
def test_random_index_soups(F, V):
    rng = np.random.default_rng(1000 * F + V)
    faces = cm.random_soup(rng, F, V)
    verts = rng.normal(size=(V, 3)).astype(np.float32)
    assert_clusters(faces, cm.cluster_bfs if F <= 20000 else cm.cluster_scipy, vertices=verts, what=f"soup F={F} V={V}")


def test_soups_cover_a_giant_component_and_thousands_of_singletons():
    sizes = {}
    for F, V in ((50000, 400), (50000, 150000)):
        _, counts = cm.cluster_scipy(cm.random_soup(np.random.default_rng(1000 * F + V), F, V))
        sizes[V] = counts
    assert sizes[400].max() > 25000 and (sizes[150000] == 1).sum() > 5000


def test_disjoint_icospheres_with_interleaved_faces():
    rng = np.random.default_rng(7)
    verts, faces = interleaved_icospheres(5, 3, rng)
    labels, counts = assert_clusters(faces, vertices=verts, what="icospheres")
    assert counts.tolist() == [1280] * 5
    # the area of a sphere of radius 0.5 + 0.1 k, from below
    _, _, a = gpu_cluster(faces, verts)
    sphere = 4 * np.pi * (0.5 + 0.1 * np.arange(5)) ** 2
    assert np.all(np.sort(a) < sphere) and np.all(np.sort(a) > 0.98 * sphere)


def test_non_manifold_edge_of_multiplicity_five():
    # five triangles on the edge (0, 1), each the seed of a strip of its own; two detached triangles
    faces = [[0, 1, 2 + k] for k in range(5)]
    nxt = 7
    for k in range(5):
        a, b = 1, 2 + k
        for _ in range(20):
            faces.append([a, b, nxt])
            a, b, nxt = b, nxt, nxt + 1
    faces += [[nxt, nxt + 1, nxt + 2], [nxt + 2, nxt + 3, nxt + 4]]
    faces = np.array(faces, np.int32)
    faces = faces[np.random.default_rng(2).permutation(len(faces))]
    verts = np.random.default_rng(3).normal(size=(nxt + 5, 3)).astype(np.float32)
    _, counts = assert_clusters(faces, vertices=verts, what="multiplicity 5")
    assert sorted(counts.tolist()) == [1, 1, 105]


@pytest.mark.parametrize("mask", ["random", "sparse", "all_kept", "all_removed"])
@pytest.mark.parametrize("F,V", [(1, 3), (300, 200), (5000, 9000), (40000, 15000)])
def test_compaction_equals_the_model(F, V, mask):
    rng = np.random.default_rng(F + len(mask))
    faces = cm.random_soup(rng, F, V)
    verts = rng.normal(size=(V, 3)).astype(np.float32)
    remove = {"random": rng.random(F) < 0.5, "sparse": rng.random(F) < 0.98, "all_kept": np.zeros(F, bool),
              "all_removed": np.ones(F, bool)}[mask]
    want = cm.remove_triangles_by_mask(verts, faces, remove)
    for m in (dev(remove), dev(remove.astype(np.uint8))):
        got = [t.cpu().numpy() for t in mc().remove_triangles_by_mask(dev(verts), dev(faces), m)]
        for name, g, w in zip(("vertices", "faces", "vertex_index", "face_index"), got, want):
            assert g.dtype == w.dtype and g.shape == w.shape, f"{name}: {g.dtype} {g.shape} against {w.dtype} {w.shape}"
            assert g.tobytes() == w.tobytes(), f"{name} differs from the model"


@pytest.mark.parametrize("shuffle", [False, True])
def test_round_cap_on_a_strip_of_2_20_triangles(shuffle):
    F = 1 << 20
    faces = cm.strip(F)
    if shuffle:
        faces = faces[np.random.default_rng(11).permutation(F)]
    c, n, _ = gpu_cluster(faces, num_verts=F + 2)
    rounds = mc().last_rounds
    print(f"strip of 2^20 triangles, shuffle={shuffle}: {rounds} rounds (cap {4 * math.ceil(math.log2(F))})")
    assert n.tolist() == [F] and not c.any()
    assert rounds <= 4 * math.ceil(math.log2(F))


def test_same_inputs_twice_give_identical_tensors():
    rng = np.random.default_rng(5)
    verts, faces = interleaved_icospheres(4, 4, rng)
    soup = cm.random_soup(rng, 30000, 300) + len(verts)
    faces = np.concatenate([faces, soup])
    faces = faces[rng.permutation(len(faces))]
    verts = np.concatenate([verts, rng.normal(size=(300, 3)).astype(np.float32)])
    runs = []
    for _ in range(2):
        c, n, a = mc().cluster_connected_triangles(dev(faces), vertices=dev(verts))
        out = mc().remove_small_components(dev(verts), dev(faces), 0.5, return_index=True)
        runs.append([c, n, a, out[0], out[1], out[3], out[4]] + [mc().last_rounds, out[2]])
    for x, y in zip(*runs):
        if torch.is_tensor(x):
            assert x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        else:
            assert x == y


def test_out_of_range_face_index_is_a_value_error():
    faces = np.array(cm.tetrahedron(0, 1, 2, 3), np.int32)
    verts = np.zeros((4, 3), np.float32)
    for bad in (4, -1):
        f = faces.copy()
        f[2, 1] = bad
        with pytest.raises(ValueError):
            mc().cluster_connected_triangles(dev(f), num_verts=4)
        with pytest.raises(ValueError):
            mc().cluster_connected_triangles(dev(f), vertices=dev(verts))
        with pytest.raises(ValueError):
            mc().remove_triangles_by_mask(dev(verts), dev(f), dev(np.zeros(4, bool)))
        with pytest.raises(ValueError):
            mc().remove_small_components(dev(verts), dev(f))
    with pytest.raises(ValueError):
        mc().remove_triangles_by_mask(dev(verts), dev(faces), dev(np.zeros(5, bool)))
    c, n, a = mc().cluster_connected_triangles(dev(faces).long(), vertices=dev(verts).double())     # int64 / float64 are converted
    assert c.tolist() == [0] * 4 and n.tolist() == [4] and a.tolist() == [0.0]


def test_empty_mesh_needs_no_launch():
    v, f = torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    c, n, a = mc().cluster_connected_triangles(f, vertices=v)
    assert c.shape == (0,) and n.shape == (0,) and a.shape == (0,) and a.dtype == torch.float64
    assert mc().cluster_connected_triangles(f)[2] is None
    v2, f2, removed = mc().remove_small_components(v, f)
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and f2.dtype == torch.int32 and removed == 0
    assert [t.shape[0] for t in mc().remove_triangles_by_mask(v, f, torch.zeros(0, dtype=torch.bool, device=DEV))] == [0] * 4


def _two_sphere_volume():
    from gaustudio_amd.tsdf import TSDFVolume
    rng = np.random.default_rng(0)
    vol = TSDFVolume(voxel_size=0.02, sdf_trunc=0.08, capacity_blocks=1 << 15)
    origins = [np.array(o, np.float32) for o in ((0, 0, -3), (3, 0, 0.5), (-3, 0.5, 0.5), (0, 3, 0.5), (0, -3, 0.5), (0.5, 0.5, 4))]
    for centre, radius, n in (((0.0, 0.0, 0.5), 0.5, 60000), ((1.4, 0.0, 0.5), 0.1, 6000)):
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        c = np.array(centre, np.float32)
        pts = (c + radius * d).astype(np.float32)
        for o in origins:
            vis = ((o - pts) * (pts - c)).sum(1) > 0.3 * np.linalg.norm(o - pts, axis=1) * radius
            vol.integrate(torch.from_numpy(pts[vis]).to(DEV), o)
    return vol


def test_end_to_end_on_a_tsdf_mesh_of_two_spheres():
    from gaustudio_amd.mesh_raster import MeshRasterizer
    vol = _two_sphere_volume()
    verts, faces = vol.extract_triangle_mesh_device(min_weight=1)
    v_np, f_np = verts.cpu().numpy(), faces.cpu().numpy()
    labels, counts = cm.cluster_scipy(f_np)
    c, n, _ = mc().cluster_connected_triangles(faces, vertices=verts)
    assert np.array_equal(c.cpu().numpy(), labels) and np.array_equal(n.cpu().numpy(), counts)
    assert counts.size >= 2
    print(f"TSDF mesh: {len(f_np)} triangles, {counts.size} clusters, largest {counts.max()}, rounds {mc().last_rounds}")
    want = cm.remove_small_components(v_np, f_np, 0.5, cluster=cm.cluster_scipy)
    v2, f2, removed, vidx, fidx = mc().remove_small_components(verts, faces, 0.5, return_index=True)
    got = (v2, f2, vidx, fidx)
    for name, g, w in zip(("vertices", "faces", "vertex_index", "face_index"), got, want[:4]):
        assert g.cpu().numpy().tobytes() == np.ascontiguousarray(w).tobytes(), f"{name} differs from the model"
    assert removed == want[4] and 0 < removed < len(f_np)
    # every kept triangle belongs to a cluster above the threshold; every output vertex is referenced
    assert (counts[labels[fidx.cpu().numpy()]] > 0.5 * counts.max()).all()
    assert torch.unique(f2).numel() == v2.shape[0]
    # on the small sphere's side nothing is left
    assert float(v2[:, 0].max()) < 0.6 < float(verts[:, 0].max())
    # the rasterizer takes the cleaned mesh
    E = mm.look_at([0.0, 0.0, -3.0], [0.0, 0.0, 0.5])
    K = np.array([[200, 0, 80], [0, 200, 60], [0, 0, 1]], dtype=np.float64)
    fr = MeshRasterizer(v2, f2).rasterize(K, E, 120, 160)
    assert int((fr.pix_to_face >= 0).sum()) > 1000
    v3, f3 = vol.extract_triangle_mesh_device(min_weight=1, clean_ratio=0.5)
    assert torch.equal(v3, v2) and torch.equal(f3, f2)
    v4, f4 = vol.extract_triangle_mesh_device(min_weight=1)
    assert torch.equal(v4, verts) and torch.equal(f4, faces)


def test_two_million_faces_against_the_scipy_path():
    rng = np.random.default_rng(21)
    v1, f1 = cm.subdivide_sphere(*mm.icosphere(3), times=4)     # 20 * 4^7 = 327 680 faces
    v0, f0 = cm.subdivide_sphere(v1, f1)                        # 20 * 4^8 = 1 310 720
    vs, fs, base = [v0, v1 * 0.5 + [3, 0, 0]], [f0, f1 + len(v0)], len(v0) + len(v1)
    vt, ft = mm.icosphere(1)                       # 80 faces each: 4000 small detached pieces
    for k in range(4000):
        vs.append(vt * 0.01 + rng.normal(size=3) * 5)
        fs.append(ft + base)
        base += len(vt)
    verts = np.concatenate(vs).astype(np.float32)
    faces = np.concatenate(fs).astype(np.int32)
    faces = faces[rng.permutation(len(faces))]
    assert 1.9e6 < len(faces) < 2.1e6
    labels, counts = assert_clusters(faces, cm.cluster_scipy, vertices=verts, what="2 M faces")
    assert counts.size == 4002
    want = cm.remove_small_components(verts, faces, 0.5, cluster=lambda f: (labels, counts))
    v2, f2, removed, vidx, fidx = mc().remove_small_components(dev(verts), dev(faces), 0.5, return_index=True)
    for name, g, w in zip(("vertices", "faces", "vertex_index", "face_index"), (v2, f2, vidx, fidx), want[:4]):
        assert g.cpu().numpy().tobytes() == np.ascontiguousarray(w).tobytes(), f"{name} differs from the model"
    assert removed == want[4] == len(faces) - len(f0)
