"""Times the 2D Gaussian surfel operator (diff_surfel_rasterization) at 1 M Gaussians / 1920x1080 / SH degree 3 -- forward alone
and forward + backward (colour and all seven allmap channels consumed) -- next to the 3DGS step of the same scene (config C3:
forward + backward of gaustudio_diff_gaussian_rasterization).  Same synthetic scene (scenes.make_scene, seed 0), surfels take
the first two scales.  Medians over K steps after W warm-up steps, CUDA events on the current stream.  Prints one JSON line.

    python tools/surfel_timing.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaustudio_amd import scenes  # noqa: E402


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    t = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=1_000_000)
    a = ap.parse_args()
    import diff_surfel_rasterization as ds
    import gaustudio_diff_gaussian_rasterization as g3
    dev = torch.device("cuda", 0)
    W, H, D = 1920, 1080, 3
    cam = scenes.make_camera(W, H)
    sc = scenes.make_scene(a.P, cam, seed=0)
    prm = {k: getattr(sc, k).to(dev).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    s2 = sc.scales[:, :2].contiguous().to(dev).requires_grad_(True)
    m2 = torch.zeros_like(prm["means3D"], requires_grad=True)
    args = (H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0, cam.viewmatrix.to(dev), cam.projmatrix.to(dev), D,
            cam.campos.to(dev), False, False)
    rs_s, rs_3 = ds.GaussianRasterizationSettings(*args), g3.GaussianRasterizationSettings(*args)
    gen = torch.Generator().manual_seed(1)
    gc, ga = torch.randn(3, H, W, generator=gen).to(dev), torch.randn(7, H, W, generator=gen).to(dev)
    grads3 = [t.to(dev) for t in scenes.make_output_grads(cam, seed=1)]
    surf = ds.GaussianRasterizer(rs_s)
    r3 = g3.GaussianRasterizer(rs_3)

    def surf_fwd():
        with torch.no_grad():
            surf(means3D=prm["means3D"], means2D=m2, opacities=prm["opacities"], shs=prm["shs"], scales=s2, rotations=prm["rotations"])

    def surf_step():
        c, r, am = surf(means3D=prm["means3D"], means2D=m2, opacities=prm["opacities"], shs=prm["shs"], scales=s2,
                        rotations=prm["rotations"])
        torch.autograd.backward([c, am], [gc, ga])

    def step3():
        c, r, d, m, o = r3(means3D=prm["means3D"], means2D=m2, opacities=prm["opacities"], shs=prm["shs"], scales=prm["scales"],
                           rotations=prm["rotations"])
        torch.autograd.backward([c, d, m, o], grads3)

    with torch.no_grad():
        _, radii, _ = surf(means3D=prm["means3D"], means2D=m2, opacities=prm["opacities"], shs=prm["shs"], scales=s2,
                           rotations=prm["rotations"])
    res = dict(P=a.P, W=W, H=H, D=D, steps=a.steps, visible_surfels=int((radii > 0).sum()),
               surfel_fwd_ms=round(_median_ms(surf_fwd, a.steps, a.warmup), 4),
               surfel_fwd_bwd_ms=round(_median_ms(surf_step, a.steps, a.warmup), 4),
               gs3d_c3_fwd_bwd_ms=round(_median_ms(step3, a.steps, a.warmup), 4))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
