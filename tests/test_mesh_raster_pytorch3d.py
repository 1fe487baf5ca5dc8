"""Agreement with PyTorch3D's MeshRasterizer, where PyTorch3D is installed (it has no ROCm build; this skips otherwise, as
the vdbfusion / Open3D pins do).  The camera is built exactly as gaustudio/scripts/render_mesh.py:285-304 builds it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_raster_model as mm  # noqa: E402

p3d = pytest.importorskip("pytorch3d")


def render_mesh_fragments(verts, faces, K, extrinsics, H, W, device):
    from pytorch3d.renderer import MeshRasterizer, PerspectiveCameras, RasterizationSettings
    from pytorch3d.structures import Meshes
    ext = torch.as_tensor(extrinsics, dtype=torch.float32)
    c2w = torch.inverse(ext)
    R, T = c2w[:3, :3], c2w[:3, 3:]
    R = torch.stack([-R[:, 0], -R[:, 1], R[:, 2]], 1)                     # RDF -> LUF
    new_c2w = torch.cat([R, T], 1)
    w2c = torch.linalg.inv(torch.cat((new_c2w, torch.Tensor([[0, 0, 0, 1]])), 0))
    R, T = w2c[:3, :3].permute(1, 0)[None], w2c[:3, 3][None]
    K = torch.as_tensor(K, dtype=torch.float32)
    cams = PerspectiveCameras(focal_length=((K[0, 0], K[1, 1]),), principal_point=((K[0, 2], K[1, 2]),), in_ndc=False,
                              image_size=((H, W),), R=R, T=T, device=device)
    rast = MeshRasterizer(cameras=cams, raster_settings=RasterizationSettings(image_size=(H, W), blur_radius=0.0, faces_per_pixel=1))
    mesh = Meshes(verts=[torch.as_tensor(verts).to(device)], faces=[torch.as_tensor(faces).long().to(device)])
    fr = rast(mesh)
    return fr.pix_to_face[0, ..., 0].cpu().numpy(), fr.zbuf[0, ..., 0].cpu().numpy(), fr.bary_coords[0, :, :, 0].cpu().numpy()


def test_fragments_agree_with_pytorch3d():
    v, f = mm.icosphere(3)
    H, W = 120, 160
    K = np.array([[150, 0, 80], [0, 150, 60], [0, 0, 1]], dtype=np.float64)
    E = mm.look_at([0.2, 0.3, -3.0], [0, 0, 0])
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    p2f_ref, z_ref, _ = render_mesh_fragments(v, f, K, E, H, W, dev)
    if torch.cuda.is_available():
        from gaustudio_amd import mesh_raster
        fr = mesh_raster.rasterize(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), K, E, H, W)
        p2f, z = fr.pix_to_face.cpu().numpy(), fr.zbuf.cpu().numpy()
    else:
        p2f, z, _ = mm.rasterize(v, f, K, E, H, W)
    both = (p2f >= 0) & (p2f_ref >= 0)
    assert ((p2f >= 0) == (p2f_ref >= 0)).mean() > 0.995
    assert (p2f[both] == p2f_ref[both]).mean() > 0.99
    assert np.allclose(z[both], z_ref[both], rtol=1e-4)
