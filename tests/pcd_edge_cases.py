"""The small point clouds, queries and cleaning inputs shared by tests/test_pcd_fusion_model.py (CPU: the exact kNN model
and the absence of near-threshold events) and tests/test_gpu_knn_edges.py (the HIP kernels against that model).  Every
builder is deterministic and cached; the arrays are shared, so no test may write into them."""
import functools

import numpy as np


def _lattice(n, dims=3):
    axes = [np.arange(n)] * dims + [np.zeros(1, dtype=np.int64)] * (3 - dims)
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)


def _shuffled(rng, p):
    return np.ascontiguousarray(p[rng.permutation(len(p))].astype(np.float32))


@functools.lru_cache(maxsize=None)
def cloud(name):
    """float32 [N,3], N <= 4096."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "lattice":                    # 16^3 integers: ties across the k-th slot at nearly every query
        return _shuffled(rng, _lattice(16))
    if name == "lattice_offset":             # exact in float32, so the ties survive; extent 15/128 at offset 1024, points
        return _shuffled(rng, _lattice(16) * 2.0 ** -7 + np.array([1024.0, -1024.0, 0.5]))   # exactly on cell boundaries
    if name == "lattice17_holes":
        # 4096 sites of the 17^3 lattice, corners kept: extent 16 and N / 8 = 8^3 make a first cell size of exactly 2 for
        # k <= 16, so a site with odd coordinates sits in the centre of its cell and has its six nearest neighbours at
        # squared distance 1 = (distance to the cell's faces)^2, three of them inside the cell and three outside
        p = _lattice(17)
        corner = np.isin(p, (0.0, 16.0)).all(axis=1)
        rest = rng.permutation(np.nonzero(~corner)[0])[:4096 - int(corner.sum())]
        return _shuffled(rng, p[np.concatenate([np.nonzero(corner)[0], rest])])
    if name == "plane":
        return _shuffled(rng, _lattice(64, 2))
    if name == "line_axis":
        return _shuffled(rng, np.arange(2048.0)[:, None] * np.array([0.0, 1.0, 0.0]))
    if name == "line_diagonal":
        return _shuffled(rng, np.arange(2048.0)[:, None] * np.ones(3))
    if name == "duplicates":                 # 80 positions x 50 copies
        return _shuffled(rng, np.repeat(rng.uniform(size=(80, 3)).astype(np.float32), 50, axis=0))
    if name == "identical":                  # extent 0
        return np.tile(np.array([[0.25, -3.0, 7.5]], dtype=np.float32), (300, 1))
    if name == "single":
        return np.array([[1.5, 2.5, -3.5]], dtype=np.float32)
    if name == "n65":                        # k = 64 = N - 1: shells 0..2 cannot fill the list
        return rng.uniform(size=(65, 3)).astype(np.float32)
    if name == "two_clusters":               # 40 + 40 points 1e4 apart: k = 64 has to cross over
        p = rng.uniform(size=(80, 3))
        p[40:, 0] += 1e4
        return _shuffled(rng, p)
    if name == "far_1e30":                   # the cell size clamps at extent / 2^21: the unit cube is one cell
        return _shuffled(rng, np.concatenate([rng.uniform(size=(1000, 3)), np.full((1, 3), 1e30)]))
    if name == "far_pm3e38":
        return _shuffled(rng, np.concatenate([rng.uniform(size=(1000, 3)), [[3e38, 0.5, 0.5], [-3e38, 0.5, 0.5]]]))
    raise KeyError(name)


CLOUDS = ("lattice", "lattice_offset", "lattice17_holes", "plane", "line_axis", "line_diagonal", "duplicates", "identical",
          "single", "n65", "two_clusters", "far_1e30", "far_pm3e38")


@functools.lru_cache(maxsize=None)
def lattice_queries(name):
    """float32 [Q,3] against cloud("lattice") (integers 0..15 on each axis)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    sites = rng.integers(0, 16, size=(48, 3)).astype(np.float64)
    if name == "on_points":
        q = sites
    elif name == "midpoints":                # eight equidistant nearest neighbours
        q = rng.integers(0, 15, size=(48, 3)) + 0.5
    elif name == "outside_faces":            # a quarter of a lattice step outside each face of the bounding box
        q = np.concatenate([np.where(np.arange(3) == a, v, sites[:8] + off)
                            for a in range(3) for v in (-0.25, 15.25) for off in (0.0, 0.5)])
    elif name == "cells_outside":            # tens of cells outside it
        q = np.concatenate([np.where(np.arange(3) == a, v, sites[:8]) for a in range(3) for v in (-40.0, 75.0)]
                           + [[[-40.0, 75.0, 200.0], [300.0, 300.0, 300.0]]])
    elif name == "at_1e6":
        q = np.concatenate([np.where(np.arange(3) == a, v, sites[:4]) for a in range(3) for v in (-1e6, 1e6)]
                           + [[[1e6, 1e6, 1e6], [-1e6, 1e6, -1e6]]])
    elif name == "at_1e30":                  # beyond the clamp of the query's cell; every point is equally far in float64
        q = np.concatenate([np.where(np.arange(3) == a, v, sites[:4]) for a in range(3) for v in (-1e30, 1e30)]
                           + [[[1e30, 1e30, 1e30], [-1e30, 1e30, -1e30]]])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.asarray(q, dtype=np.float32))


LATTICE_QUERIES = ("on_points", "midpoints", "outside_faces", "cells_outside", "at_1e6", "at_1e30")


# ------------------------------------------------------------------------------------------------------------ cleaning
def _normals(rng, n, spread=0.5):
    v = np.array([0.0, 0.0, 1.0]) + spread * rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


CLEANING_SIZES = (1, 2, 255, 256, 257, 513)      # around the 256-element tiles of the mean / std reductions
CLEANING_NEIGHBORS = (1, 20, 50)


@functools.lru_cache(maxsize=None)
def cleaning_cloud(name):
    """(points float32 [n,3], normals float32 [n,3])."""
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    if name.startswith("n"):
        n = int(name[1:])
        p = rng.uniform(size=(n, 3))
        p[rng.uniform(size=n) < 0.05] *= 3.0             # a few statistical outliers
        return p.astype(np.float32), _normals(rng, n)
    if name == "identical":                               # no a_i > 0: 0 / 0 mean
        return np.tile(np.array([[1.0, 2.0, 3.0]], dtype=np.float32), (300, 1)), _normals(rng, 300)
    if name == "pairs_and_one":                           # at k = 2 exactly one a_i > 0: count - 1 = 0 under the std
        p = np.repeat(rng.uniform(size=(100, 3)), 2, axis=0)
        p = np.concatenate([p, [[0.5, 0.5, 2.0]]])
        o = rng.permutation(len(p))
        return p[o].astype(np.float32), _normals(rng, len(p))
    if name == "duplicated_fifth":                        # 20 % of the points are copies with other normals:
        base = rng.uniform(size=(800, 3))                 # "neighbour 0 is the point itself" is false for the higher index
        p = np.concatenate([base, base[rng.choice(800, size=200, replace=False)]])
        o = rng.permutation(len(p))
        return p[o].astype(np.float32), _normals(rng, len(p), 0.7)
    raise KeyError(name)


def cleaning_inputs():
    """[(cloud name, nb_neighbors)]: every (points, normals, k) the cleaning tests use."""
    cases = [(f"n{n}", nb) for n in CLEANING_SIZES for nb in CLEANING_NEIGHBORS]
    return cases + [("identical", 20), ("pairs_and_one", 2), ("duplicated_fifth", 20), ("duplicated_fifth", 1)]
