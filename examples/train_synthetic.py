#!/usr/bin/env python
"""A whole 3DGS training loop on the MI355X, on a synthetic scene (no dataset, no checkpoint):

    a ball of Gaussians, a ring of cameras                     ->  FusedGaussianRasterizer: one target image per camera
    every third Gaussian, moved, recoloured and made faint     ->  the start
    each step, one camera:  FusedGaussianRasterizer -> photometric_loss -> backward
                            -> DensityControl.accumulate -> GaussianAdam.step(visible=radii)
    every few dozen steps:  DensityControl.densify_and_prune (clone / split / prune), and one reset_opacity

Every kernel of the step is HIP: rasterizer, loss, both backwards, the statistics, the sparse Adam step, the compaction.
    python examples/train_synthetic.py [steps]
Prints loss and N; the mean loss over the last round of the ring has to be below that of the first."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import (DensityControl, GaussianAdam, GaussianRasterizationSettings, photometric_loss,  # noqa: E402
                           scenes)
from gaustudio_amd.fused import FusedGaussianRasterizer  # noqa: E402

RADIUS, VIEWS, WIDTH, HEIGHT = 3.0, 8, 160, 100


def settings(cam, dev):
    return GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                         cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 3, cam.campos.to(dev), False, False)


def render(rs, p, means2D):
    return FusedGaussianRasterizer(rs)(means3D=p["xyz"], means2D=means2D, raw_opacities=p["opacity"], f_dc=p["f_dc"],
                                       f_rest=p["f_rest"], raw_scales=p["scaling"], raw_rotations=p["rotation"])


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    every = max(steps // 5, 2 * VIEWS)                    # a densification every `every` steps, from the second interval on
    dev = torch.device("cuda:0")
    rsets = [settings(c, dev) for c in scenes.ring_cameras(VIEWS, WIDTH, HEIGHT, radius=10.0)]
    sc = scenes.make_ball_scene(3000, radius=RADIUS, seed=0, sigma=0.1)
    truth = dict(xyz=sc.means3D, f_dc=sc.shs[:, :1].contiguous(), f_rest=sc.shs[:, 1:].contiguous(),
                 opacity=torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)), scaling=torch.log(sc.scales), rotation=sc.rotations)
    truth = {k: v.to(dev) for k, v in truth.items()}
    with torch.no_grad():
        targets = [render(rs, truth, torch.zeros_like(truth["xyz"]))[0] for rs in rsets]

    g = torch.Generator().manual_seed(1)
    noise = lambda t, s: (s * torch.randn(t.shape, generator=g)).to(dev)
    start = {k: v[::3].contiguous() for k, v in truth.items()}
    start["xyz"] = start["xyz"] + noise(start["xyz"], 0.05)
    start["f_dc"] = start["f_dc"] + noise(start["f_dc"], 0.3)
    start["f_rest"] = torch.zeros_like(start["f_rest"])
    start["scaling"] = start["scaling"] + noise(start["scaling"], 0.2)
    start["opacity"] = torch.full_like(start["opacity"], math.log(0.1 / 0.9))
    params = {k: v.contiguous().requires_grad_(True) for k, v in start.items()}

    opt = GaussianAdam(params, lr=dict(xyz=1.6e-3, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3))
    xyz_lr = GaussianAdam.expon_lr(1.6e-3, 1.6e-5, max_steps=max(steps, 1))
    dc = DensityControl(opt, percent_dense=0.01)
    n_start = opt.num_rows
    losses, sizes = [], {n_start}
    for step in range(steps):
        v = step % VIEWS
        opt.set_lr("xyz", xyz_lr(step))
        means2D = torch.zeros_like(params["xyz"], requires_grad=True)
        color, radii = render(rsets[v], params, means2D)[:2]
        loss = photometric_loss(color, targets[v])
        loss.backward()
        dc.accumulate(means2D.grad, radii)
        opt.step(visible=radii)
        opt.zero_grad()
        losses.append(loss.detach())
        if step and step % every == 0 and step < steps - VIEWS and opt.num_rows < 4 * n_start:
            rep = dc.densify_and_prune(max_grad=2e-4, min_opacity=0.005, extent=RADIUS, max_screen_size=None, generator=None)
            sizes.add(rep.n_after)
            print(f"step {step:4d}: densify  +{rep.n_cloned} clones, {rep.n_split} split in two, -{rep.n_pruned} pruned:  "
                  f"N {rep.n_before} -> {rep.n_after}")
            if step == 2 * every:
                dc.reset_opacity(max_opacity=0.3)         # the published 0.01 needs thousands of steps to recover from
        if step % 20 == 0 or step == steps - 1:
            print(f"step {step:4d}: loss = {float(loss.detach()):.5f}  N = {opt.num_rows}")
    losses = torch.stack(losses).cpu()
    assert bool(torch.isfinite(losses).all()), "a loss is not finite"
    assert all(bool(torch.isfinite(p).all()) for p in params.values()), "a parameter is not finite"
    first, last = float(losses[:VIEWS].mean()), float(losses[-VIEWS:].mean())
    assert last < first, f"the loss did not go down: {first:.5f} -> {last:.5f}"
    print(f"loss {first:.5f} -> {last:.5f} in {steps} steps; N {n_start} -> {opt.num_rows} (sizes seen: {sorted(sizes)})")


if __name__ == "__main__":
    main()
