"""Parity of VisualHull.extract_mesh with the reference's extract_mesh (mask.py:82-93) on PyMCubes.  PyMCubes is not a
dependency: the test runs where it is installed and the parity stays unpinned elsewhere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import visual_hull_model as vm  # noqa: E402

mcubes = pytest.importorskip("mcubes")
pytestmark = pytest.mark.gpu


def test_same_surface_as_mcubes():
    import torch
    from gaustudio_amd import carve
    cameras, masks = vm.ring_scene(6, 64, 48, distance=3.0, fov_deg=40.0, disc=0.5, elevation=0.6, seed=2)
    translate, radius, R = np.array([0.05, -0.02, 0.03]), 0.9, 32
    hull = carve(cameras, [torch.from_numpy(m).cuda() for m in masks], resolution=R, translate=translate, radius=radius)
    v, f = (x.cpu().numpy() for x in hull.extract_mesh(0.5))
    # mask.py:82-93
    rv, rf = mcubes.marching_cubes(hull.filled.cpu().numpy(), 0.5)
    rf = np.fliplr(rf)
    rv = rv.dot(np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]]))
    rv = rv / (R - 1) * (2 * radius) - radius - translate
    # the same vertex set (order is each library's own) and the same orientation; the two tables may split an ambiguous cube
    # differently, which moves the enclosed volume by a fraction of a cell per such cube
    key = lambda a: np.unique(np.round(a * 1e4).astype(np.int64), axis=0)
    assert np.array_equal(key(v), key(rv))
    ours, theirs = vm.signed_volume(v + translate, f), vm.signed_volume(rv + translate, rf)
    assert ours > 0 and theirs > 0 and abs(ours - theirs) < 0.05 * theirs
