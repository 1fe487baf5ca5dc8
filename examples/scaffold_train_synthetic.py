#!/usr/bin/env python
"""Scaffold-GS training with anchor control on the MI355X, on a synthetic scene (no dataset, no checkpoint):

    anchors on a sphere + random small MLPs, ring cameras            ->  render_scaffold: the target images
    the same model with one side thinned out and perturbed features  ->  render_scaffold(backward="hip") -> photometric_loss
                                                                         -> torch Adam -> AnchorControl.accumulate
    every `adjust_every` steps                                       ->  AnchorControl.adjust: anchors grow where the
                                                                         view-space gradient is large

Prints the loss and the anchor count; the loss has to fall and the anchor count has to rise.  The model has no opacity
parameter to starve an anchor with, so nothing is asserted about pruning.
The gradient threshold fits this scene's image size: the view-space gradient of a photometric loss scales with it.
    python examples/scaffold_train_synthetic.py [steps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import (AnchorControl, GaussianRasterizationSettings, ScaffoldModel, photometric_loss,  # noqa: E402
                           render_scaffold, scenes)

NAMES = ("anchor", "anchor_feat", "offset", "scale_raw", "rot_raw")


def synthetic(n, k, dev):
    g = torch.Generator().manual_seed(0)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
    d = torch.nn.functional.normalize(r(n, 3))
    anchor = d * (1.0 + 0.08 * torch.sin(5 * d[:, 0:1]) * torch.cos(4 * d[:, 1:2]))
    lin = lambda n_in, n_out, bias=0.0: (r(32, n_in, scale=0.2), r(32, scale=0.1), r(n_out, 32, scale=0.2), r(n_out, scale=0.1) + bias)
    params = dict(anchor=anchor, anchor_feat=r(n, 32), offset=r(n, k, 3),
                  scale_raw=torch.cat([torch.full((n, 3), 0.02), torch.full((n, 3), 0.012)], dim=1).log().to(dev),
                  rot_raw=torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(n, 1))
    mlps = dict(mlp_opacity=lin(36, k, bias=1.5), mlp_cov=lin(36, 7 * k), mlp_color=lin(36, 3 * k))
    return params, mlps, g


def main(steps=200, num_anchors=30_000, adjust_every=30, size=(320, 240), num_views=6, grad_threshold=4e-4, quiet=False):
    dev = torch.device("cuda:0")
    k = 6
    params, mlps, g = synthetic(num_anchors, k, dev)
    views = []
    for cam in scenes.ring_cameras(num_views, size[0], size[1], radius=3.2, elevation=0.35):
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                           cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 1, cam.campos.to(dev), False, False)
        with torch.no_grad():
            views.append((rs, render_scaffold(ScaffoldModel.from_raw(**params, **mlps), rs)["render"]))
    # the model to train: nine tenths of the anchors on one side are gone, the features are off
    thin = (params["anchor"][:, 0] > 0.2) & (torch.rand(num_anchors, generator=g).to(dev) < 0.9)
    params = {name: t[~thin].contiguous() for name, t in params.items()}
    params["anchor_feat"] = params["anchor_feat"] + 1.0 * torch.randn(params["anchor_feat"].shape, generator=g).to(dev)
    params = {name: t.requires_grad_(True) for name, t in params.items()}
    color = tuple((t + 0.1 * torch.randn(t.shape, generator=g).to(dev)).requires_grad_(True) for t in mlps["mlp_color"])
    mlps = dict(mlps, mlp_color=color)
    lr = dict(anchor=0.0, anchor_feat=7.5e-3, offset=1e-2, scale_raw=7e-3, rot_raw=2e-3)
    opt = torch.optim.Adam([dict(params=[params[name]], lr=lr[name]) for name in NAMES] + [dict(params=list(color), lr=4e-3)],
                           eps=1e-15)
    # two levels, 0.04 and 0.01: a new anchor's Gaussians start at the size of its voxel, and the sphere's own are about 0.01
    ctl = AnchorControl(params, voxel_size=0.01, optimizer=opt, update_depth=2, update_init_factor=4, update_hierarchy_factor=4)
    n0 = ctl.num_anchors
    losses = []
    for step in range(steps):
        rs, target = views[step % num_views]
        opt.zero_grad()
        out = render_scaffold(ScaffoldModel.from_raw(**params, **mlps), rs, backward="hip")
        loss = photometric_loss(out["render"], target)
        loss.backward()
        opt.step()
        ctl.accumulate(out["gaussians"], out["viewspace_points"].grad, out["radii"])
        losses.append(float(loss.detach()))
        if not quiet and (step % 10 == 0 or step == steps - 1):
            print(f"step {step:4d}: loss = {losses[-1]:.5f}  {ctl.num_anchors} anchors, {out['gaussians'].xyz.shape[0]} Gaussians")
        if (step + 1) % adjust_every == 0 and step + 1 <= 0.6 * steps:       # the last two fifths train the grown model
            rep = ctl.adjust(check_interval=adjust_every, success_threshold=0.8, grad_threshold=grad_threshold, min_opacity=0.005,
                             generator=torch.Generator(device=dev).manual_seed(step))
            if not quiet:
                print(f"step {step:4d}: adjust grew {rep.n_grown} and pruned {rep.n_pruned}: {rep.n_before} -> {rep.n_after} anchors")
    w = min(num_views, max(steps // 2, 1))                       # one round of the cameras at either end
    first, last = sum(losses[:w]) / w, sum(losses[-w:]) / w
    if not quiet:
        print(f"loss {first:.5f} -> {last:.5f} in {steps} steps; anchors {n0} -> {ctl.num_anchors}")
    assert last < first, "the loss did not fall"
    assert ctl.num_anchors > n0, "no anchor was grown"
    return first, last, n0, ctl.num_anchors


if __name__ == "__main__":
    main(steps=int(sys.argv[1]) if len(sys.argv) > 1 else 200)
