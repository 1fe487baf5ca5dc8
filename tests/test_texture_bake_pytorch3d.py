"""Agreement of the bake's camera with PyTorch3D's, where PyTorch3D is installed (it has no ROCm build; this skips otherwise,
as tests/test_mesh_raster_pytorch3d.py does).  The camera is the one gaustudio/scripts/texture_mesh.py:77-91 arrives at (its
pose with the x and y camera axes negated) and the vertices go through transform_points as at :129.  PyTorch3D composes 4x4 matrices, which rounds differently from the
contract's x_c formula: the comparison is to 1e-3 px, and the parity stays unpinned elsewhere."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mesh_raster_model as rm  # noqa: E402
import texture_bake_model as tm  # noqa: E402
from gaustudio_amd import texture_bake  # noqa: E402,F401  (the module whose camera this pins)

p3d = pytest.importorskip("pytorch3d")


def test_transform_points_is_the_flipped_screen_camera():
    from pytorch3d.renderer import PerspectiveCameras
    W, H = 50, 33
    K = tm.intrinsics(41.0, 39.0, 21.3, 18.9)
    E = rm.look_at((0.4, -0.3, -3.0), (0.1, 0.05, 0.0))
    verts = np.random.default_rng(3).uniform(-1, 1, (200, 3)).astype(np.float32)
    # the camera the script hands to PyTorch3D: the pose with its x and y camera axes negated (OpenCV's right-down-forward
    # to PyTorch3D's left-up-forward), given as the row-vector rotation and the translation of the flipped world-to-camera
    flipped_w2c = np.diag([-1.0, -1.0, 1.0, 1.0]) @ np.asarray(E, dtype=np.float64)
    R = torch.from_numpy(flipped_w2c[:3, :3].T.copy()).float()[None]
    T = torch.from_numpy(flipped_w2c[:3, 3].copy()).float()[None]
    view = PerspectiveCameras(focal_length=((K[0, 0], K[1, 1]),), principal_point=((K[0, 2], K[1, 2]),), in_ndc=False,
                              image_size=((H, W),), R=R, T=T)
    pt = view.transform_points(torch.from_numpy(verts))[..., :2].numpy()
    x, y, _, _ = tm.screen_points(verts, K, E)
    assert np.abs(pt[:, 0] - x).max() <= 1e-3 and np.abs(pt[:, 1] - y).max() <= 1e-3
    near_far = view.unproject_points(torch.tensor([[0.0, 0.0, 0.1], [0.0, 0.0, 0.2]])).numpy()
    ray = near_far[1] - near_far[0]
    print("unproject_points direction", ray / np.linalg.norm(ray), "contract axis", tm.view_axis(E))
