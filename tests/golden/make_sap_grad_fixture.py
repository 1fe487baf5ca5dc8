#!/usr/bin/env python
"""Writes tests/golden/py_sap_grad.npz: gradients the REFERENCE's Python (gaustudio/utils/graphics_utils.py, imported unmodified
through ref_env.reference_modules(), run on the CPU with torch autograd) produced.  Data only.  Inputs: the cloud of
py_sap.npz (V, normals) and the seeded weights of tests/sap_grad_model.loss_weights; grids 16^3 and (12, 10, 14) only.

    gV_16 / gN_16, gV_nc / gN_nc    V and N gradients of sum(tanh(DPSR(res, sig=2)(V, N)) * W), float32
    eref_grad_V_* / eref_grad_N_*   max |reference float32 gradient - float64 model| (sap_grad_model.dpsr_loss_grads)
    gscale_V_* / gscale_N_*         max |float64 model gradient|: the scale those errors are read against
    ras_{u,w}_gp / _gv              pts / vals gradients of sum(point_rasterize(P, vals, (12,10,14), weighted) * Wc), P = the
                                    first N_RAS points of V; quirk_{u,w}_gp / _gv: the same for the two node-aligned points of
                                    py_sap.npz on 8^3 with values of one and Wc = 1
    interp_gp / interp_gg           pts / grid gradients of sum(grid_interp(Wg, P) * go) at 16^3
The generator also runs the descent the GPU test repeats (20 Adam steps, lr 1e-2, 16^3, 2000 points) and prints its losses."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_env  # noqa: E402
import sap_grad_model as gm  # noqa: E402
import sap_model as sm  # noqa: E402

SIG, N_RAS = 2, 512
RES_16, RES_NC = (16, 16, 16), (12, 10, 14)


def main():
    fx = dict(np.load(os.path.join(HERE, "py_sap.npz")))
    V, N = fx["V"], fx["normals"]
    out = {}
    with ref_env.reference_modules():
        from gaustudio.utils import graphics_utils as gu
        for key, res in (("16", RES_16), ("nc", RES_NC)):
            W = gm.loss_weights(res)
            Vt = torch.from_numpy(V)[None].requires_grad_(True)
            Nt = torch.from_numpy(N)[None].requires_grad_(True)
            loss = (torch.tanh(gu.DPSR(res, sig=SIG)(Vt, Nt)[0]) * torch.from_numpy(W)).sum()
            loss.backward()
            out["gV_" + key], out["gN_" + key] = Vt.grad[0].numpy(), Nt.grad[0].numpy()
            want_loss, gV, gN = gm.dpsr_loss_grads(V, N, res, SIG, W)
            for name, ref, mod in (("V", out["gV_" + key], gV), ("N", out["gN_" + key], gN)):
                out[f"eref_grad_{name}_{key}"] = np.float64(np.abs(ref - mod).max())
                out[f"gscale_{name}_{key}"] = np.float64(np.abs(mod).max())
            print(f"DPSR {res}: loss {float(loss):.6f} (model {want_loss:.6f}); "
                  + ", ".join(f"eref_grad_{n} = {out[f'eref_grad_{n}_{key}']:.3e} of {out[f'gscale_{n}_{key}']:.3e}" for n in "VN"))

        P = V[:N_RAS]
        Wc = np.stack([gm.loss_weights(RES_NC, seed=21 + c) for c in range(3)])
        for weighted, tag in ((False, "u"), (True, "w")):
            for pts, vals, res, w, pre in ((P, N[:N_RAS], RES_NC, Wc, "ras_"),
                                           (fx["quirk_pts"], np.ones((2, 3), np.float32), (8, 8, 8), np.ones((3, 8, 8, 8), np.float32), "quirk_")):
                pt = torch.from_numpy(pts)[None].requires_grad_(True)
                vt = torch.from_numpy(vals)[None].requires_grad_(True)
                (gu.point_rasterize(pt, vt, res, weighted=weighted)[0] * torch.from_numpy(w)).sum().backward()
                out[f"{pre}{tag}_gp"], out[f"{pre}{tag}_gv"] = pt.grad[0].numpy(), vt.grad[0].numpy()
        Wg = gm.loss_weights(RES_16, seed=31)
        go = np.random.default_rng(32).normal(size=N_RAS).astype(np.float32)
        pt = torch.from_numpy(P)[None].requires_grad_(True)
        gt = torch.from_numpy(Wg)[None, ..., None].requires_grad_(True)
        (gu.grid_interp(gt, pt)[0, :, 0] * torch.from_numpy(go)).sum().backward()
        out["interp_gp"], out["interp_gg"] = pt.grad[0].numpy(), gt.grad[0, ..., 0].numpy()

        # the descent of the GPU test, on the reference alone
        start_w, nrm, target_w = gm.descent_clouds()
        start, center, scale = sm.unit_cube(start_w)
        target = ((target_w - center) / scale + np.float32(1.0)) / np.float32(2.0)
        dpsr = gu.DPSR(RES_16, sig=SIG)
        with torch.no_grad():
            tgt = torch.tanh(dpsr(torch.from_numpy(target)[None], torch.from_numpy(nrm)[None]))
        x = torch.log(torch.from_numpy(start) / (1 - torch.from_numpy(start))).requires_grad_(True)
        n = torch.from_numpy(nrm).clone().requires_grad_(True)
        opt = torch.optim.Adam([x, n], lr=1e-2)
        losses = []
        for _ in range(21):
            opt.zero_grad()
            loss = ((torch.tanh(dpsr(torch.sigmoid(x)[None], n[None])) - tgt) ** 2).mean()
            losses.append(float(loss))
            loss.backward()
            opt.step()
        print(f"descent on the reference: loss {losses[0]:.3e} -> {losses[20]:.3e} after 20 Adam steps "
              f"({100 * losses[20] / losses[0]:.1f} % of the initial loss)")
    assert np.abs(out["quirk_u_gp"] + 8 * 3).max() == 0, out["quirk_u_gp"]     # -R * sum_c g on every axis
    path = os.path.join(HERE, "py_sap_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
