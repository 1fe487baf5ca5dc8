#!/usr/bin/env python
"""A 2D Gaussian surfel training loop on the MI355X, on a synthetic scene (no dataset, no checkpoint):

    surfels on a sphere, their normals radial, a ring of cameras   ->  diff_surfel_rasterization: one target image per camera
    every second surfel, moved, turned, recoloured, enlarged, fainter ->  the start
    each step, one camera:  surfel rasterizer -> photometric_loss(color) + surfel_geometric_loss(allmap) -> backward
                            -> GaussianAdam.step(visible=radii)

The model keeps the [N,3] scale parameter of the optimiser's layout and hands the operator scale[:, :2].  Rasterizer, both
losses, all three backwards and the Adam step are HIP kernels; the activations are three torch element-wise ops.
    python examples/train_surfel_synthetic.py [steps]
Prints the three loss parts (photometric, normal consistency, distortion); the mean total over the last round of the ring has
to be below that of the first."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import (GaussianAdam, GaussianRasterizationSettings, intrinsics_from_settings, photometric_loss,  # noqa: E402
                           scenes, surfel_geometric_loss_with_parts)
from gaustudio_amd.surfel import GaussianRasterizer  # noqa: E402

RADIUS, VIEWS, WIDTH, HEIGHT = 3.0, 8, 160, 100
LAMBDA_NORMAL, LAMBDA_DIST = 0.05, 1000.0


def settings(cam, dev):
    return GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                         cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 3, cam.campos.to(dev), False, False)


def render(rs, p, means2D):
    """color [3,H,W], radii [N], allmap [7,H,W] of the raw parameters `p`."""
    return GaussianRasterizer(rs)(means3D=p["xyz"], means2D=means2D, opacities=torch.sigmoid(p["opacity"]),
                                  shs=torch.cat([p["f_dc"], p["f_rest"]], 1), scales=torch.exp(p["scaling"][:, :2]),
                                  rotations=p["rotation"])


def sphere_surfels(n, seed=0):
    """n surfels on the sphere of RADIUS: (r, x, y, z) quaternions that turn the z axis onto the radial direction."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    q = torch.cat([1.0 + d[:, 2:3], -d[:, 1:2], d[:, 0:1], torch.zeros(n, 1)], 1)       # (1 + <z, d>, z x d)
    q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-6)
    sh = torch.zeros(n, 16, 3)
    sh[:, 0] = (0.5 + 0.5 * torch.sin(3.0 * d)) / 0.28209479177387814 - 0.5 / 0.28209479177387814
    scaling = torch.log(0.12 * (0.7 + 0.6 * torch.rand(n, 3, generator=g)))
    return dict(xyz=RADIUS * d, f_dc=sh[:, :1].contiguous(), f_rest=sh[:, 1:].contiguous(),
                opacity=torch.full((n, 1), math.log(0.8 / 0.2)), scaling=scaling, rotation=q)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    dev = torch.device("cuda:0")
    rsets = [settings(c, dev) for c in scenes.ring_cameras(VIEWS, WIDTH, HEIGHT, radius=10.0)]
    intr = [intrinsics_from_settings(rs) for rs in rsets]         # Python floats: nothing below reads the device back
    truth = {k: v.to(dev) for k, v in sphere_surfels(4000).items()}
    with torch.no_grad():
        targets = [render(rs, truth, torch.zeros_like(truth["xyz"]))[0] for rs in rsets]

    g = torch.Generator().manual_seed(1)
    noise = lambda t, s: (s * torch.randn(t.shape, generator=g)).to(dev)
    start = {k: v[::2].contiguous() for k, v in truth.items()}
    start["xyz"] = start["xyz"] + noise(start["xyz"], 0.12)
    start["rotation"] = start["rotation"] + noise(start["rotation"], 0.4)
    start["f_dc"] = start["f_dc"] + noise(start["f_dc"], 0.3)
    start["scaling"] = start["scaling"] + math.log(1.3)
    start["opacity"] = torch.full_like(start["opacity"], math.log(0.6 / 0.4))
    params = {k: v.contiguous().requires_grad_(True) for k, v in start.items()}

    opt = GaussianAdam(params, lr=dict(xyz=1.6e-3, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3))
    parts = []
    for step in range(steps):
        v = step % VIEWS
        means2D = torch.zeros_like(params["xyz"], requires_grad=True)
        color, radii, allmap = render(rsets[v], params, means2D)
        photo = photometric_loss(color, targets[v])
        geo, normal, dist = surfel_geometric_loss_with_parts(allmap, intr[v], LAMBDA_NORMAL, LAMBDA_DIST)
        (photo + geo).backward()
        opt.step(visible=radii)
        opt.zero_grad()
        parts.append(torch.stack([photo.detach(), normal, dist]))
        if step % 20 == 0 or step == steps - 1:
            p = parts[-1].tolist()
            print(f"step {step:4d}: photometric = {p[0]:.5f}  normal = {p[1]:.5f}  distortion = {p[2]:.5f}  total = {sum(p):.5f}")
    parts = torch.stack(parts).cpu()
    assert bool(torch.isfinite(parts).all()), "a loss is not finite"
    assert all(bool(torch.isfinite(p).all()) for p in params.values()), "a parameter is not finite"
    first, last = parts[:VIEWS].mean(0), parts[-VIEWS:].mean(0)
    for name, a, b in zip(("photometric", "normal", "distortion"), first.tolist(), last.tolist()):
        print(f"{name:12s} {a:.5f} -> {b:.5f}")
    assert float(last.sum()) < float(first.sum()), f"the loss did not go down: {float(first.sum()):.5f} -> {float(last.sum()):.5f}"
    print(f"total loss {float(first.sum()):.5f} -> {float(last.sum()):.5f} in {steps} steps, {opt.num_rows} surfels")


if __name__ == "__main__":
    main()
