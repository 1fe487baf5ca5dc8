"""Agreement of the marching cubes of tests/sap_model.py (and with it of gaustudio_amd.sap.marching_cubes, which equals the
model exactly: tests/test_gpu_sap.py) with skimage.measure.marching_cubes, the reference's fallback mesher, where skimage is
installed (it is not in the ROCm image; this skips otherwise, as the Open3D / vdbfusion / PyTorch3D pins do).  Lewiner's
method triangulates ambiguous cubes differently, so what is compared is the surface, not the index lists: the same vertices
(one per crossing edge, at the same linear interpolation) and the same enclosed volume.  Until it runs, parity with skimage
and with cumcubes is unpinned."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sap_model as sm  # noqa: E402
from test_sap_model import fields  # noqa: E402

measure = pytest.importorskip("skimage.measure")


def volume(v, f):
    v = v.astype(np.float64)
    return np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_model_surface_equals_skimage(name):
    g = fields(29)[name].astype(np.float32)
    v, f = sm.marching_cubes(g, 0.0)
    sv, sf = measure.marching_cubes(g, 0.0)[:2]
    assert len(sv) == len(v)
    a = v[np.lexsort(v.T[::-1])]
    b = sv[np.lexsort(sv.T[::-1])]
    assert np.abs(a - b).max() < 1e-4
    assert abs(abs(volume(v, f)) - abs(volume(sv, sf))) < 1e-2 * abs(volume(v, f))
