#!/usr/bin/env python
"""Fitting through the native photometric loss on the MI355X, on a synthetic scene (no dataset, no checkpoint):

    a small random cloud                  ->  GaussianRasterizer: the target image
    perturbed colours (SH) and opacities  ->  GaussianRasterizer  ->  photometric_loss to the target  ->  Adam

Forward and backward of the training step are HIP end to end: the rasterizer, the fused (1 - lambda) L1 + lambda (1 - SSIM)
loss, the loss's gradient, the rasterizer's backward.   python examples/fit_photometric_synthetic.py [steps]
Prints the loss every few steps; it has to go down."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, photometric_loss_with_parts, scenes  # noqa: E402


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    dev = torch.device("cuda:0")
    cam = scenes.make_camera(320, 200)
    sc = scenes.make_scene(8000, cam, seed=0, sigma_px_median=3.0)
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                       cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 3, cam.campos.to(dev), False, False)
    means3D, scales, rotations = sc.means3D.to(dev), sc.scales.to(dev), sc.rotations.to(dev)
    means2D = torch.zeros_like(means3D)

    def render(shs, opacity_logit):
        return GaussianRasterizer(rs)(means3D=means3D, means2D=means2D, opacities=torch.sigmoid(opacity_logit), shs=shs,
                                      scales=scales, rotations=rotations)[0]

    logit = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)).to(dev)
    with torch.no_grad():
        target = render(sc.shs.to(dev), logit)
    g = torch.Generator().manual_seed(1)
    shs = (sc.shs + 0.3 * torch.randn(sc.shs.shape, generator=g)).to(dev).requires_grad_(True)
    logit = (logit.cpu() + 1.0 * torch.randn(logit.shape, generator=g)).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([shs, logit], lr=2e-2)
    first = last = None
    for step in range(steps):
        opt.zero_grad()
        loss, l1, ssim = photometric_loss_with_parts(render(shs, logit), target)
        loss.backward()
        opt.step()
        if step % 10 == 0 or step == steps - 1:       # the only reads of the device
            last = float(loss)
            first = last if first is None else first
            print(f"step {step:3d}: loss = {last:.5f}  (l1 {float(l1):.5f}, ssim {float(ssim):.5f})")
    assert last < first, "the loss did not go down"
    print(f"loss {first:.5f} -> {last:.5f} in {steps} Adam steps through the HIP loss and the HIP rasterizer")


if __name__ == "__main__":
    main()
