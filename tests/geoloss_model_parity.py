"""The published 2DGS geometric loss restated in torch with autograd (`restatement`, any dtype and device), seeded smooth scenes,
and the error of the float32 model (tests/geoloss_model.py: the kernels' arithmetic) against the float64 restatement beside the
error of torch's own float32 evaluation of the same restatement.  tests/test_geoloss_model.py asserts on measure();
`python tests/geoloss_model_parity.py` writes the figures to profiles/geometric_loss_parity.json."""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import geoloss_model as gm  # noqa: E402

F32 = np.float32
SCENES = ("tilted_plane", "sphere_cap")
SHAPES = ((37, 53), (48, 80))
RHOS = (0.0, 0.5, 1.0)
LAMBDAS = (0.05, 100.0)          # lambda_normal, lambda_dist: both terms in play
C_FLOOR = 1e-3                   # |c| of every interior pixel of every scene stays above this (asserted by the test)


def restatement(allmap, intrinsics, lambda_normal=0.05, lambda_dist=0.0, depth_ratio=0.0, dtype=torch.float64, device="cpu"):
    """The definition: surfel_renderer.py's post-render block, the published depth_to_normal and the two loss terms, evaluated
    in camera space.  nan_to_num is the binding form (0 wherever the value is not finite) and is written so that autograd gives
    the pinned zero there instead of 0 * inf.  Returns a dict of tensors; `allmap` is the leaf, with .grad filled."""
    a = torch.as_tensor(allmap).detach().to(device=device, dtype=dtype).requires_grad_(True)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    H, W = a.shape[1:]
    alpha = a[1]
    q = a[0] / alpha
    fin = torch.isfinite(q)
    d_exp = torch.where(fin, a[0] / torch.where(fin, alpha, torch.ones_like(alpha)), torch.zeros_like(q))
    d_med = torch.where(torch.isfinite(a[5]), a[5], torch.zeros_like(a[5]))
    d = (1.0 - depth_ratio) * d_exp + depth_ratio * d_med
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype, device=device), torch.arange(W, dtype=dtype, device=device), indexing="ij")
    pts = torch.stack([d * ((xs - cx) / fx), d * ((ys - cy) / fy), d], -1)            # [H,W,3], camera space
    n = torch.zeros_like(pts)
    cnorm = None
    if H >= 3 and W >= 3:
        dy = pts[2:, 1:-1] - pts[:-2, 1:-1]
        dx = pts[1:-1, 2:] - pts[1:-1, :-2]
        c = torch.cross(dy, dx, dim=-1)
        cnorm = c.detach().norm(dim=-1)
        n[1:-1, 1:-1] = F.normalize(c, dim=-1)                                      # c / max(|c|, 1e-12)
    ns = n * alpha.detach()[..., None]
    err = 1.0 - (a[2:5].permute(1, 2, 0) * ns).sum(-1)
    normal_loss = lambda_normal * err.mean()
    dist_loss = lambda_dist * a[6].mean()
    loss = normal_loss + dist_loss
    loss.backward()
    return dict(loss=loss.detach(), normal_loss=normal_loss.detach(), dist_loss=dist_loss.detach(), normal_error=err.detach(),
                surf_normal=ns.detach().permute(2, 0, 1), surf_depth=d.detach(), grad=a.grad, cnorm=cnorm)


def intrinsics_of(H, W, fov_deg=60.0):
    f = W / (2.0 * math.tan(math.radians(fov_deg) / 2))
    return f, f, (W - 1) / 2.0, (H - 1) / 2.0


def scene(name, shape, seed=0):
    """(allmap [7,H,W] float32, intrinsics): a smooth depth surface seen by a 60-degree camera, alpha in (0.2, 1], the median
    depth = the depth plus N(0, 1e-3), the rendered normal = the surface's unit normal plus N(0, 0.05) per component,
    distortion in [0, 0.01)."""
    H, W = shape
    rng = np.random.default_rng([seed, SCENES.index(name), H, W])
    fx, fy, cx, cy = intr = intrinsics_of(H, W)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx)])
    if name == "tilted_plane":                       # <m, P> = k
        m = np.array([0.35, -0.25, -1.0])
        m /= np.linalg.norm(m)
        d = -4.0 / np.einsum("i,ihw->hw", m, ray)
        normal = np.broadcast_to(m[:, None, None], ray.shape)
    elif name == "sphere_cap":                       # the near side of a sphere of radius 7 centred at z = 10
        zc, r = 10.0, 7.0
        aa, bb, cc = (ray * ray).sum(0), -2.0 * zc * ray[2], zc * zc - r * r
        d = (-bb - np.sqrt(bb * bb - 4 * aa * cc)) / (2 * aa)
        normal = (d * ray - np.array([0, 0, zc])[:, None, None]) / r
    else:
        raise KeyError(name)
    alpha = 1.0 - 0.8 * rng.random((H, W))
    a = np.zeros((7, H, W))
    a[0], a[1] = d * alpha, alpha
    a[2:5] = normal + rng.normal(0, 0.05, normal.shape)
    a[5] = d + rng.normal(0, 1e-3, d.shape)
    a[6] = 0.01 * rng.random((H, W))
    return a.astype(F32), intr


def errors(got, r64):
    """|loss - loss64|, max |normal_error - its float64|, and per gradient group max |g - g64| / max |g64|: the depth planes
    (0, 1, 5) and the rendered normal's (2..4) have scales of their own."""
    g, g64 = np.asarray(got["grad"], dtype=np.float64), r64["grad"].numpy()
    rel = lambda idx: float(np.abs(g[idx] - g64[idx]).max() / np.abs(g64[idx]).max())
    return dict(loss=abs(float(got["loss"]) - float(r64["loss"])),
                normal_error=float(np.abs(np.asarray(got["normal_error"], dtype=np.float64) - r64["normal_error"].numpy()).max()),
                grad_depth_over_scale=rel([0, 1, 5]), grad_normal_over_scale=rel([2, 3, 4]))


def _numpy(r):
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def measure():
    out = {}
    ln, ld = LAMBDAS
    for s in SCENES:
        for shape in SHAPES:
            for rho in RHOS:
                a, intr = scene(s, shape)
                r64 = restatement(a, intr, ln, ld, rho, torch.float64)
                r32 = _numpy(restatement(a, intr, ln, ld, rho, torch.float32))
                out[f"{s}-{shape[0]}x{shape[1]}-rho{rho}"] = dict(model=errors(gm.loss_and_grad(a, intr, ln, ld, rho), r64),
                                                                   torch_float32=errors(r32, r64), min_c=float(r64["cnorm"].min()))
    return out


if __name__ == "__main__":
    rep = measure()
    for v in rep.values():
        v["ratio"] = {k: (v["model"][k] / v["torch_float32"][k] if v["torch_float32"][k] else None) for k in v["model"]}
    doc = dict(what="error against the float64 restatement (torch, autograd) of the published 2DGS normal-consistency + distortion "
                    "loss, lambda_normal 0.05, lambda_dist 100: the float32 model of the HIP kernels (tests/geoloss_model.py) "
                    "beside torch's float32 evaluation of the same restatement on the CPU",
               bound="model <= 2 x torch_float32 on each figure (tests/test_geoloss_model.py)", scenes=rep)
    path = os.path.join(os.path.dirname(HERE), "profiles", "geometric_loss_parity.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v["ratio"] for k, v in rep.items()}, indent=1))
