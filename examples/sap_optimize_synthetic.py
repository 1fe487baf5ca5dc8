#!/usr/bin/env python
"""Shape-as-Points as an optimisation: fit an optimisable cloud (gaustudio/models/sap.py registers it as `sap_pcd`) through the
differentiable Poisson solver and the differentiable mesh, every kernel forward and backward on the MI355X.

    oversized ellipsoid cloud -> ShapeAsPoints.requires_grad_() -> Adam on
        grid loss:   mean((tanh(DPSR(sigmoid(xyz), normals)) - target grid)^2)
        points loss: mean |vertex - nearest target point|^2 over the vertices of psr2mesh (nearest targets: pcd_fusion.knn)

Needs no dataset:
    python examples/sap_optimize_synthetic.py [out_dir] [--res 32] [--points 4000] [--steps 60] [--lr 1e-2]
Prints both losses as it goes and writes fitted_mesh.ply."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import formats, pcd_fusion, sap  # noqa: E402


def ellipsoid(n, axes, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    axes = torch.tensor(axes)
    nrm = torch.nn.functional.normalize(u / axes, dim=1)
    return (u * axes).to(dev).contiguous(), nrm.to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out", nargs="?", default="sap_optimize_out")
    ap.add_argument("--res", type=int, default=32)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--lr", type=float, default=1e-2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sap_optimize_synthetic.py runs on a ROCm GPU; none is visible")
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)

    target, target_n = ellipsoid(args.points, (1.0, 0.7, 0.5), 0, dev)
    start, start_n = ellipsoid(args.points, (1.0, 0.9, 0.8), 1, dev)           # shrinks towards the target
    shape = sap.ShapeAsPoints.from_pointcloud(start, start_n, dpsr_res=args.res, dpsr_sig=2)
    with torch.no_grad():
        target_unit = shape.transform(target, shape.center, shape.scale)
        target_grid = shape.dpsr(target_unit, target_n, apply_tanh=True)
    shape.requires_grad_()
    opt = torch.optim.Adam(shape.parameters(), lr=args.lr)
    for step in range(args.steps + 1):
        opt.zero_grad()
        grid = shape.psr_grid()
        grid_loss = ((grid - target_grid) ** 2).mean()
        v_unit, faces = sap.psr2mesh(grid)
        vertices = shape.transform(v_unit, shape.center, shape.scale, True)
        _, idx = pcd_fusion.knn(target, 1, queries=vertices.detach())
        points_loss = ((vertices - target[idx[:, 0]]) ** 2).sum(1).mean()
        if step % 10 == 0 or step == args.steps:
            print(f"step {step:4d}: grid loss {float(grid_loss.detach()):.4e}, points loss {float(points_loss.detach()):.4e}, "
                  f"{len(vertices)} vertices / {len(faces)} faces")
        if step == args.steps:
            break
        (grid_loss + points_loss).backward()
        opt.step()
    path = os.path.join(args.out, "fitted_mesh.ply")
    formats.write_ply_mesh(path, vertices.detach(), faces)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
