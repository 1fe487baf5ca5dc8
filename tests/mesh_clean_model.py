"""The CPU model of gaustudio_amd.mesh_clean (csrc/gsr_mesh_clean.hip): a numpy / pure-Python restatement of what
gaustudio/scripts/extract_mesh.py:149-186 takes from Open3D -- TriangleMesh::ClusterConnectedTriangles (an edge -> triangles
map, a breadth-first walk opened at the lowest unvisited triangle), the per-cluster triangle counts and fp64 areas
(GetTriangleArea), the keep rule of the script, RemoveTrianglesByMask and RemoveUnreferencedVertices.

Two clustering paths that must agree: `cluster_bfs` (the restatement) and `cluster_scipy` (scipy.sparse.csgraph, labels
renumbered by lowest triangle index) for meshes too large for a Python loop.  `fastsv` restates the round structure of the
device kernels (synchronous FastSV) so the round cap can be checked without a GPU.
"""
from collections import deque

import numpy as np


def edge_keys(faces):
    """[F,3,2] int64: the three undirected edges {min, max} of every face, (0,1), (1,2), (2,0)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b = f, f[:, [1, 2, 0]]
    return np.stack([np.minimum(a, b), np.maximum(a, b)], axis=-1)


def _counts(labels, C):
    return np.bincount(labels, minlength=C).astype(np.int32) if len(labels) else np.zeros(0, np.int32)


def cluster_bfs(faces):
    """(triangle_clusters [F] int32, cluster_n_triangles [C] int32).  Triangles sharing an undirected edge are adjacent (a
    shared vertex alone does not connect; an edge with more than two triangles connects all of them); clusters are numbered
    in the order a scan over the triangles opens them."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = f.shape[0]
    ek = edge_keys(f)
    e2t = {}
    for t in range(F):
        for k in range(3):
            e2t.setdefault((int(ek[t, k, 0]), int(ek[t, k, 1])), []).append(t)
    labels = np.full(F, -1, dtype=np.int32)
    C = 0
    for seed in range(F):
        if labels[seed] >= 0:
            continue
        labels[seed] = C
        queue = deque([seed])
        while queue:
            t = queue.popleft()
            for k in range(3):
                for n in e2t[(int(ek[t, k, 0]), int(ek[t, k, 1]))]:
                    if labels[n] < 0:
                        labels[n] = C
                        queue.append(n)
        C += 1
    return labels, _counts(labels, C)


def renumber_by_lowest_triangle(labels):
    """Any labelling -> cluster indices in ascending order of each cluster's lowest triangle index."""
    labels = np.asarray(labels)
    if labels.size == 0:
        return labels.astype(np.int32)
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.int32)


def union_edges(faces):
    """The (u, v) triangle pairs that are neighbours in the list of (edge key, triangle) pairs sorted stably by key: a chain
    through every edge's triangles (what the device code joins)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = f.shape[0]
    ek = edge_keys(f).reshape(-1, 2)
    V = int(f.max()) + 1 if F else 1
    key = ek[:, 0] * V + ek[:, 1]
    tri = np.repeat(np.arange(F, dtype=np.int64), 3)
    order = np.argsort(key, kind="stable")
    key, tri = key[order], tri[order]
    same = key[1:] == key[:-1]
    return tri[:-1][same], tri[1:][same]


def cluster_scipy(faces):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = f.shape[0]
    if F == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    u, v = union_edges(f)
    g = coo_matrix((np.ones(len(u), dtype=np.int8), (u, v)), shape=(F, F))
    C, lab = connected_components(g, directed=False)
    labels = renumber_by_lowest_triangle(lab)
    return labels, _counts(labels, C)


def fastsv(num_nodes, u, v, max_rounds=10000):
    """Synchronous FastSV (Zhang, Azad, Hu 2020) exactly as the device rounds run it: per round, with f the parents and gf the
    grandparents of the round before, next = gf (shortcutting), next[f[a]] = min(., gf[b]) (stochastic hooking) and
    next[a] = min(., gf[b]) (aggressive hooking) for both directions of every edge, then f = next, gf = f[f]; stops after the
    first round that leaves f and gf unchanged.  Returns (labels = lowest node of each component, rounds)."""
    f = np.arange(num_nodes, dtype=np.int64)
    gf = f.copy()
    a = np.concatenate([u, v]).astype(np.int64)
    b = np.concatenate([v, u]).astype(np.int64)
    rounds = 0
    while rounds < max_rounds:
        rounds += 1
        nxt = gf.copy()
        np.minimum.at(nxt, f[a], gf[b])
        np.minimum.at(nxt, a, gf[b])
        g2 = nxt[nxt]
        changed = not (np.array_equal(g2, gf) and np.array_equal(nxt, f))
        f, gf = nxt, g2
        if not changed:
            break
    return f, rounds


def triangle_areas(vertices, faces):
    """Open3D GetTriangleArea in fp64 from the float32 vertices: 0.5 |(v1 - v0) x (v2 - v0)|, the cross product as
    (e1.y e2.z - e1.z e2.y, ...), the norm as sqrt((x x + y y) + z z): the operation order of the kernel."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def cluster_areas(vertices, faces, labels, C):
    """[C] float64: the areas summed per cluster in ascending triangle order."""
    a = triangle_areas(vertices, faces)
    out = np.zeros(C, dtype=np.float64)
    if C <= 64 or len(a) <= 4096:
        for t in range(len(a)):
            out[labels[t]] += a[t]
        return out
    np.add.at(out, labels, a)            # unbuffered, in index order: the same sequence of additions
    return out


def keep_clusters(cluster_n_triangles, ratio_threshold=0.5):
    """bool [C]: cluster i stays when n_i > ratio_threshold * n_largest (strict, in float64)."""
    n = np.asarray(cluster_n_triangles)
    if n.size == 0:
        return np.zeros(0, dtype=bool)
    largest = n[int(np.argmax(n))]          # the first maximum
    return n.astype(np.float64) > np.float64(ratio_threshold) * np.float64(largest)


def remove_triangles_by_mask(vertices, faces, remove_mask):
    """RemoveTrianglesByMask + RemoveUnreferencedVertices: (vertices', faces', vertex_index, face_index), kept faces and
    referenced vertices in their original order, the maps new -> old as int32."""
    v = np.asarray(vertices).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    keep = ~np.asarray(remove_mask, dtype=bool).reshape(-1)
    face_index = np.nonzero(keep)[0].astype(np.int32)
    kf = f[face_index]
    ref = np.zeros(v.shape[0], dtype=bool)
    ref[kf.reshape(-1)] = True
    vertex_index = np.nonzero(ref)[0].astype(np.int32)
    vmap = np.cumsum(ref) - 1
    return v[vertex_index], vmap[kf].astype(np.int32).reshape(-1, 3), vertex_index, face_index


def remove_small_components(vertices, faces, ratio_threshold=0.5, cluster=cluster_bfs):
    """extract_mesh.py:152-182: (vertices', faces', vertex_index, face_index, number of removed triangles)."""
    labels, counts = cluster(faces)
    keep = keep_clusters(counts, ratio_threshold)
    remove = ~keep[labels] if len(labels) else np.zeros(0, dtype=bool)
    return (*remove_triangles_by_mask(vertices, faces, remove), int(remove.sum()))


# ------------------------------------------------------------------------------------------------------ meshes for the tests
def tetrahedron(i0, i1, i2, i3):
    return [[i0, i1, i2], [i0, i3, i1], [i1, i3, i2], [i2, i3, i0]]


def strip(num_triangles):
    """A triangle strip: triangle t = (t, t + 1, t + 2); consecutive triangles share an edge, the diameter is F - 1."""
    t = np.arange(num_triangles, dtype=np.int32)
    return np.stack([t, t + 1, t + 2], axis=1)


def subdivide_sphere(verts, faces, times=1):
    """The subdivision step of mesh_raster_model.icosphere (edge midpoints pushed onto the unit sphere, four faces per
    face), vectorised: icosphere(k + times) connectivity from icosphere(k) up to the numbering of the new vertices."""
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    for _ in range(times):
        e = edge_keys(f).reshape(-1, 2)
        uniq, inv = np.unique(e[:, 0] * len(v) + e[:, 1], return_inverse=True)
        m = v[uniq // len(v)] + v[uniq % len(v)]
        mid = (len(v) + inv.reshape(-1)).reshape(-1, 3)          # per face: the midpoints of (a,b), (b,c), (c,a)
        v = np.concatenate([v, m / np.linalg.norm(m, axis=1, keepdims=True)])
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
        f = np.stack([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)],
                     axis=1).reshape(-1, 3)
    return v.astype(np.float32), f.astype(np.int32)


def hand_cases():
    """name -> (faces, number of clusters)."""
    return {
        "two_tets_sharing_a_vertex": (np.array(tetrahedron(0, 1, 2, 3) + tetrahedron(3, 4, 5, 6), np.int32), 2),
        "two_tets_sharing_an_edge": (np.array(tetrahedron(0, 1, 2, 3) + tetrahedron(2, 3, 4, 5), np.int32), 1),
        "fan_of_three_on_one_edge": (np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int32), 1),
        "repeated_index": (np.array([[0, 0, 1], [1, 0, 2], [3, 3, 4], [5, 6, 7], [0, 0, 9]], np.int32), 3),
        "single": (np.array([[2, 1, 0]], np.int32), 1),
        "isolated_triangles": (np.array([[0, 1, 2], [2, 3, 4], [4, 5, 0]], np.int32), 3),
    }


def random_soup(rng, F, V):
    return rng.integers(0, V, size=(F, 3)).astype(np.int32)
