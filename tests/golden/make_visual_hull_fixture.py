#!/usr/bin/env python
"""Writes tests/golden/py_visual_hull.npz: a small carving scene and what the REFERENCE's Python produced for it on the CPU
(gaustudio/datasets/__init__.py Camera.insideView, gaustudio/datasets/utils.py getNerfppNorm, gaustudio/models/vanilla_sg.py
VanillaPointCloud.create_from_attribute, imported unmodified through ref_env.reference_modules()).  Data only.

    cam_R / cam_T / cam_fov     6 ring cameras + 1 camera without a mask, 48 x 36 (seeded)
    matrices                    each Camera's full_proj_transform (float32 [7,4,4])
    masks / has_mask            disc and off-centre blob silhouettes (uint8 [7,36,48]); the last camera has none
    translate / radius_norm / min_radius   getNerfppNorm's values as it returned them
    radius                      float(min_radius) * 1.2
    axis_x / axis_y / axis_z    the grid's per-axis tables read back from points_world (R = 24)
    inside                      per camera the vector the loop of mask.py:59-68 ANDs into `filled` (bool [7, 24^3])
    filled                      the flattened result
    seed_*                      create_from_attribute(xyz, rgb=0.5, opacity=0.1, scale=0.01) as build_model calls it
    meta                        text: the counts this script checked

The carve is the replay of mask.py:41-71 around those calls (its .cuda() calls are the only reason construct_visual_hull cannot
run as written on a box without a GPU).  translate and radius enter np.linspace / the subtraction as float64, the contract of
INTEGRATION.md s19 (numpy >= 2 would keep getNerfppNorm's float32 there; numpy 1 promoted to float64).

The script asserts what tests/test_visual_hull_model.py relies on: the float32 model disagrees with the reference on at
most 0.1 % of the grid's (voxel, camera) decisions, and every disagreement is attributed by the float64 replay to a decision
boundary closer than 1e-4."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import visual_hull_model as vm  # noqa: E402

SEED, R, W, H, RADIUS_SCALE = 11, 24, 48, 36, 1.2
FOV_X = np.radians(70.0)


def camera_params(rng):
    """(R camera-to-world [3,3], T world-to-camera [3], FoVx, FoVy) of the 7 cameras."""
    out = []
    fovy = 2 * np.arctan(np.tan(FOV_X / 2) * H / W)
    eyes = []
    for a in range(6):
        t = 2 * np.pi * a / 6 + rng.uniform(-0.15, 0.15)
        eyes.append(rng.uniform(2.8, 3.4) * np.array([np.cos(t), rng.uniform(-0.4, 0.4), np.sin(t)]))
    eyes.append(np.array([0.3, -3.6, 0.2]))                     # from above, no mask
    for eye in eyes:
        fwd = -eye / np.linalg.norm(eye)
        up = np.array([0.0, -1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
        right = np.cross(fwd, up)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        Rc2w = np.stack([right, down, fwd], axis=1)
        out.append((Rc2w, -Rc2w.T @ eye, FOV_X, fovy))
    return out


def silhouettes(rng):
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    masks = np.zeros((7, H, W), dtype=np.uint8)
    for c in range(6):
        disc = (u + 0.5 - W / 2) ** 2 + (v + 0.5 - H / 2) ** 2 <= rng.uniform(11.0, 14.0) ** 2
        bx, by = W / 2 + rng.uniform(-9, 9), H / 2 + rng.uniform(-6, 6)
        blob = ((u + 0.5 - bx) / 9.0) ** 2 + ((v + 0.5 - by) / 6.0) ** 2 <= 1.0
        masks[c] = disc | blob if c % 2 == 0 else disc
    return masks


def main():
    rng = np.random.default_rng(SEED)
    params = camera_params(rng)
    masks = silhouettes(rng)
    has_mask = np.array([1] * 6 + [0], dtype=np.uint8)
    out = dict(cam_R=np.stack([p[0] for p in params]), cam_T=np.stack([p[1] for p in params]),
               cam_fov=np.array([[p[2], p[3]] for p in params]), size=np.array([W, H]), masks=masks, has_mask=has_mask,
               resolution=np.int64(R), radius_scale=np.float64(RADIUS_SCALE))
    with ref_env.reference_modules():
        from gaustudio.datasets import Camera
        from gaustudio.datasets.utils import getNerfppNorm
        from gaustudio.models.vanilla_sg import VanillaPointCloud
        cams = [Camera(R=p[0], T=p[1], FoVx=p[2], FoVy=p[3], image_width=W, image_height=H) for p in params]
        for cam, m, h in zip(cams, masks, has_mask):
            cam.mask = torch.from_numpy(m.astype(np.float32)) if h else None
        norm = getNerfppNorm(cams)
        out["translate"], out["radius_norm"], out["min_radius"] = (np.asarray(norm[k]) for k in ("translate", "radius", "min_radius"))
        # ---- mask.py:41-71
        translate = np.asarray(norm["translate"], dtype=np.float64)
        radius = float(norm["min_radius"]) * RADIUS_SCALE
        x, y, z = np.meshgrid(np.linspace(-radius, radius, R), np.linspace(-radius, radius, R), np.linspace(-radius, radius, R))
        points = np.stack([x.flatten(), y.flatten(), z.flatten()], axis=-1)
        points_world = points - translate
        points_world = torch.from_numpy(points_world).float()
        filled = torch.ones((points_world.shape[0])).bool()
        inside = []
        for camera in cams:
            inside_view = camera.insideView(points_world)
            inside_view_idx = torch.where(inside_view)[0]
            inside_mask = camera.insideView(points_world[inside_view_idx], camera.mask)
            camera_filled = torch.zeros((points_world.shape[0])).bool()
            camera_filled[inside_view_idx] = inside_mask
            inside.append(camera_filled.numpy().copy())
            filled = filled & camera_filled
        out["matrices"] = np.stack([c.full_proj_transform.numpy() for c in cams]).astype(np.float32)
        # ---- mask.py:95-108 -> vanilla_sg.py:69-97
        xyz = torch.from_numpy(rng.uniform(-1, 1, (5, 3))).float()
        n = xyz.shape[0]
        model = VanillaPointCloud.__new__(VanillaPointCloud)
        model.max_sh_degree = 3
        model.create_from_attribute(xyz=xyz, rgb=torch.ones((n, 3)) * 0.5, opacity=torch.ones((n, 1)) * 0.1,
                                    scale=torch.ones((n, 3)) * 0.01)
        for k in ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot"):
            out["seed_" + k] = getattr(model, "_" + k).cpu().numpy()
    pw = points_world.numpy().reshape(R, R, R, 3)
    out["radius"] = np.float64(radius)
    out["axis_x"], out["axis_y"], out["axis_z"] = pw[0, :, 0, 0].copy(), pw[:, 0, 0, 1].copy(), pw[0, 0, :, 2].copy()
    out["inside"] = np.stack(inside)
    out["filled"] = filled.numpy()

    # what the CPU test relies on
    axes = (out["axis_x"], out["axis_y"], out["axis_z"])
    px, py, pz, _ = vm.grid_points(axes)
    assert np.array_equal(np.stack([px, py, pz], axis=1), points_world.numpy()), "the grid is not separable as assumed"
    cameras = [(M, W, H) for M in out["matrices"]]
    mlist = [m if h else None for m, h in zip(masks, has_mask)]
    m_filled, m_count, _, m_keep = vm.carve(axes, cameras, mlist, per_camera=True)
    _, margin = vm.replay64(axes, cameras, mlist)
    bad, ndiff = vm.unattributed(m_keep, out["inside"], margin, 1e-4)
    nvox_diff = int((m_filled.ravel() != out["filled"]).sum())
    assert ndiff <= 1e-3 * R ** 3, f"{ndiff} (voxel, camera) decisions differ: choose another seed"
    assert len(bad) == 0, f"{len(bad)} differing decisions are not near a boundary: {bad[:5]}"
    per_cam = out["inside"].sum(axis=1)
    out["meta"] = np.array(
        f"seed {SEED}; grid {R}^3 = {R ** 3} voxels; reference filled {int(out['filled'].sum())}, model filled {m_count}; "
        f"kept per camera {per_cam.tolist()}; (voxel, camera) decisions on which the float32 model and the reference "
        f"(torch.matmul) differ: {ndiff}; voxels whose filled differs: {nvox_diff}; unattributed: {len(bad)}; "
        f"numpy {np.__version__}, torch {torch.__version__.split('+')[0]}")
    path = os.path.join(HERE, "py_visual_hull.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes\n{out['meta']}")


if __name__ == "__main__":
    main()
