#!/usr/bin/env python
"""Writes tests/golden/py_sap.npz: inputs and the outputs the REFERENCE's Python (gaustudio/utils/graphics_utils.py, imported
unmodified through ref_env.reference_modules(), run on the CPU) produced for them.  Data only.

    cloud      noisy ellipsoid (semi-axes 1, 0.7, 0.5; sigma 0.01; outward normals), seed below
    V          the unit-cube coordinates as ShapeAsPoints stores and recovers them: sigmoid(logit(transform(points)))
    ras_u/_w   point_rasterize(V, N, 32^3, weighted=False / True)
    phi_32     DPSR((32,32,32), sig=2)(V, N);  phi_nc: DPSR((20,24,36), sig=2)(V, N)
    fv_32      grid_interp(phi_32, V)
    eref_*     max |reference float32 phi - float64 model phi| (tests/sap_model.dpsr64): the reference's own error
    quirk_*    two points placed exactly on nodes of an 8^3 grid, three channels of ones (sums 6.0 and 0.75)
The generator also checks what the GPU tests rely on: phi_32[0,0,0] == 0.5, and the model's marching cubes of
tanh(phi_32) is closed with Euler characteristic 2."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_env  # noqa: E402
import sap_model as sm  # noqa: E402

N_POINTS, SEED, SIG = 4000, 7, 2
RES_32, RES_NC = (32, 32, 32), (20, 24, 36)


def main():
    pts, nrm = sm.ellipsoid_cloud(N_POINTS, seed=SEED)
    with ref_env.reference_modules():
        from gaustudio.utils import graphics_utils as gu
        P = torch.from_numpy(pts)
        center = P.mean(dim=0)
        scale = (P - center).abs().max() * 1.2
        unit = ((P - center) / scale + 1.) / 2.
        V = torch.sigmoid(torch.log(unit / (1 - unit)))
        Vb, Nb = V.unsqueeze(0), torch.from_numpy(nrm).unsqueeze(0)
        out = dict(points=pts, normals=nrm, V=V.numpy(), center=center.numpy(), scale=np.float32(scale))
        out["ras_u"] = gu.point_rasterize(Vb, Nb, RES_32, weighted=False)[0].numpy()
        out["ras_w"] = gu.point_rasterize(Vb, Nb, RES_32, weighted=True)[0].numpy()
        out["phi_32"] = gu.DPSR(RES_32, sig=SIG)(Vb, Nb)[0].numpy()
        out["phi_nc"] = gu.DPSR(RES_NC, sig=SIG)(Vb, Nb)[0].numpy()
        out["fv_32"] = gu.grid_interp(torch.from_numpy(out["phi_32"])[None, ..., None], Vb)[0, :, 0].numpy()
        q = torch.tensor([[[0.25, 0.5, 0.125], [0.75, 0.0, 0.875]]])
        out["quirk_pts"] = q[0].numpy()
        out["quirk_u"] = gu.point_rasterize(q, torch.ones(1, 2, 3), (8, 8, 8), weighted=False)[0].numpy()
        out["quirk_w"] = gu.point_rasterize(q, torch.ones(1, 2, 3), (8, 8, 8), weighted=True)[0].numpy()
    Vn = out["V"]
    out["sig"] = np.float64(SIG)
    out["eref_32"] = np.float64(np.abs(out["phi_32"] - sm.dpsr64(Vn, nrm, RES_32, SIG)).max())
    out["eref_nc"] = np.float64(np.abs(out["phi_nc"] - sm.dpsr64(Vn, nrm, RES_NC, SIG)).max())
    assert out["phi_32"][0, 0, 0] == 0.5, out["phi_32"][0, 0, 0]
    assert out["quirk_u"].sum() == 6.0 and out["quirk_w"].sum() == 0.75, (out["quirk_u"].sum(), out["quirk_w"].sum())
    v, f = sm.marching_cubes(np.tanh(out["phi_32"]), 0.0)
    chi = sm.euler_characteristic(v, f)
    assert sm.is_closed(f) and chi == 2, (sm.is_closed(f), chi)
    path = os.path.join(HERE, "py_sap.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; eref_32 = {out['eref_32']:.3e}, eref_nc = {out['eref_nc']:.3e}, "
          f"positive nodes = {(out['phi_32'] > 0).mean():.3f}, mesh {len(v)} vertices / {len(f)} faces, chi = {chi}")


if __name__ == "__main__":
    main()
