#!/usr/bin/env python
"""Training through the Scaffold-GS decoder's HIP backward on the MI355X, on a synthetic scene (no dataset, no checkpoint):

    anchors on a sphere + random small MLPs  ->  render_scaffold: the target image
    perturbed anchor_feat and colour MLP     ->  render_scaffold(backward="hip")  ->  L1 to the target  ->  Adam

The forward is the inference path (the two HIP passes of decode); the gradient of the decoder comes from gsr_scaffold_backward
and that of the rasterizer from the operator's own backward.   python examples/scaffold_fit_synthetic.py [steps]
Prints the loss every few steps; it has to go down."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import GaussianRasterizationSettings, ScaffoldModel, render_scaffold, scenes  # noqa: E402


def synthetic_model(n, k, dev):
    g = torch.Generator().manual_seed(0)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
    d = torch.nn.functional.normalize(r(n, 3))
    anchor = d * (1.0 + 0.08 * torch.sin(5 * d[:, 0:1]) * torch.cos(4 * d[:, 1:2]))
    lin = lambda n_in, n_out, bias=0.0: (r(32, n_in, scale=0.2), r(32, scale=0.1), r(n_out, 32, scale=0.2), r(n_out, scale=0.1) + bias)
    scaling = torch.cat([torch.full((n, 3), 0.02), torch.full((n, 3), 0.012)], dim=1).to(dev)
    return ScaffoldModel(anchor, r(n, 32), r(n, k, 3), scaling, torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(n, 1),
                         lin(36, k, bias=1.5), lin(36, 7 * k), lin(36, 3 * k), lin(4, 3))


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    dev = torch.device("cuda:0")
    model = synthetic_model(60_000, 10, dev)
    cam = scenes.ring_cameras(1, 480, 360, radius=3.2, elevation=0.35)[0]
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                       cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 1, cam.campos.to(dev), False, False)
    with torch.no_grad():
        target = render_scaffold(model, rs)["render"]
    g = torch.Generator().manual_seed(1)
    model.anchor_feat = (model.anchor_feat + 0.5 * torch.randn(model.anchor_feat.shape, generator=g).to(dev)).requires_grad_(True)
    model.mlp_color = tuple((t + 0.1 * torch.randn(t.shape, generator=g).to(dev)).requires_grad_(True) for t in model.mlp_color)
    opt = torch.optim.Adam([model.anchor_feat, *model.mlp_color], lr=1e-2)
    first = last = None
    for step in range(steps):
        opt.zero_grad()
        out = render_scaffold(model, rs, backward="hip")
        loss = (out["render"] - target).abs().mean()
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if step % 10 == 0 or step == steps - 1:
            print(f"step {step:3d}: L1 = {last:.5f}  ({out['gaussians'].xyz.shape[0]} Gaussians of {int(out['gaussians'].visible.sum())} "
                  f"visible anchors)")
    assert last < first, "the loss did not go down"
    print(f"L1 {first:.5f} -> {last:.5f} in {steps} Adam steps through decode's HIP backward")


if __name__ == "__main__":
    main()
