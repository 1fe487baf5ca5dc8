#!/usr/bin/env python
"""GPU times of the vertex-colour bake's per-view stages -- rasterize, visible, select, sample -- next to a torch restatement
of the script's per-view body on the same GPU in the same run.

    python tools/texture_bake_timing.py [--subdivisions 6] [--size 640 480] [--views 8] [--out profiles/texture_bake_timing.json]

Mesh: an icosphere of 20 * 4^subdivisions triangles (81 920 by default), ring cameras around it, random images.
Baseline: what gaustudio/scripts/texture_mesh.py:109-141 does per view behind the rasterizer, formulated with torch operations
for the same visible faces (PyTorch3D is not available, so the rasterization has no baseline): the face list, the face
normals and the cosine, the selection, the unique vertex list, the projection, grid_sample of the flipped image, the scatter
into the colour array.  It is the reference's formulation, not the code under test; its colours are compared with ours
(float32 rounding apart).  The four stage times are those of the kernels called one by one; add_view_*_ms time
TextureBaker.add_view as a whole, which adds the orientation mean, the statistics (small torch reductions) and, with strict,
a blocking read-back.
Times are HIP events on the stream around each stage after one warm-up pass over the views, per view, the median over
`--repeats` passes of the per-pass median over the views; a stage's time includes the read-back it ends with (rasterize:
the binned count; visible: the error flag; select and sample: none).  No threshold and no promised ratio: the JSON is the record."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaustudio_amd.texture_bake import TextureBaker  # noqa: E402
from mesh_voxel_timing import icosphere  # noqa: E402

STAGES = ("rasterize", "visible", "select", "sample")


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    eye, target, up = (np.asarray(x, dtype=np.float64) for x in (eye, target, up))
    zc = (target - eye) / np.linalg.norm(target - eye)
    xc = np.cross(zc, up)
    xc /= np.linalg.norm(xc)
    R = np.stack([xc, np.cross(zc, xc), zc])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ eye
    return E


def event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def ours(baker, views):
    """One pass over the views: per-stage milliseconds per view."""
    rows = []
    r = baker.raster
    for seq, (image, K, E) in enumerate(views):
        H, W = image.shape[:2]
        e0 = event()
        frags = r.rasterize(K, E, H, W)
        e1 = event()
        vis = r.visible_faces(frags)
        e2 = event()
        baker.select(vis, E, baker.num_views + seq, return_cos=False)
        e3 = event()
        baker.sample(image, K, E, baker.num_views + seq)
        e4 = event()
        torch.cuda.synchronize()
        rows.append(dict(zip(STAGES, (e0.elapsed_time(e1), e1.elapsed_time(e2), e2.elapsed_time(e3), e3.elapsed_time(e4)))))
        rows[-1]["visible_mask"] = vis
    baker.num_views += len(views)
    return rows


def torch_view(verts, faces, vis, image, K, E, out_colors):
    """The per-view body of the script behind the rasterizer, formulated with torch's own operations on the device (index
    lists through nonzero / unique, gathers, one grid_sample call with the script's arguments, one scatter)."""
    H, W = image.shape[:2]
    fid = torch.nonzero(vis).squeeze(1)
    p0, p1, p2 = (verts[faces[fid, k].long()] for k in range(3))
    nrm = torch.linalg.cross(p1 - p0, p2 - p0)
    axis = E[2, :3]
    cos = (nrm @ axis) / (torch.linalg.vector_norm(nrm, dim=1) * torch.linalg.vector_norm(axis))
    vid = torch.unique(faces[fid[cos < -0.05]].long())
    cam = torch.addmm(E[:3, 3], verts[vid], E[:3, :3].t())
    screen = torch.stack([K[0, 2] - K[0, 0] * cam[:, 0] / cam[:, 2], K[1, 2] - K[1, 1] * cam[:, 1] / cam[:, 2]], dim=1)
    g = 2 * screen / torch.tensor([W - 1, H - 1], dtype=screen.dtype, device=screen.device) - 1
    ok = (g.abs() <= 1).all(dim=1)
    flipped = torch.flip(image, dims=(0, 1)).permute(2, 0, 1).unsqueeze(0)
    looked_up = torch.nn.functional.grid_sample(flipped, g[ok].reshape(1, -1, 1, 2), mode="bilinear", padding_mode="reflection",
                                                align_corners=False)
    out_colors[vid[ok]] = looked_up[0, :, :, 0].t().clamp(0, 1)


def whole_views(v, f, views, strict, repeats):
    """add_view as a whole (rasterize, visible, select, the orientation mean, sample, the statistics): per-view milliseconds
    between HIP events, the median over `repeats` passes of the per-pass median, after a warm-up pass."""
    meds = []
    for it in range(repeats + 1):
        baker = TextureBaker(v, f)
        row = []
        for image, K, E in views:
            a = event()
            baker.add_view(image, K, E, strict=strict)
            b = event()
            torch.cuda.synchronize()
            row.append(a.elapsed_time(b))
        if it:
            meds.append(statistics.median(row))
    return statistics.median(meds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivisions", type=int, default=6)
    ap.add_argument("--size", type=int, nargs=2, default=[640, 480], metavar=("W", "H"))
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_bake_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H = args.size
    v, f, _ = (torch.from_numpy(a).to(dev) for a in icosphere(args.subdivisions))
    g = torch.Generator(device=dev).manual_seed(0)
    views = []
    for a in range(args.views):
        t = 2 * np.pi * a / args.views
        K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]])
        views.append((torch.rand((H, W, 3), device=dev, generator=g), K, look_at((3 * np.cos(t), 0.5, 3 * np.sin(t)))))
    baker = TextureBaker(v, f)
    passes = [ours(baker, views) for _ in range(args.repeats + 1)][1:]
    med = {s + "_ms": statistics.median(statistics.median(r[s] for r in p) for p in passes) for s in STAGES}
    per_view = [sum(statistics.median(r[s] for r in p) for s in STAGES) for p in passes]
    med["view_ms"] = statistics.median(per_view)
    med["view_ms_min_max"] = [min(per_view), max(per_view)]
    med["select_plus_sample_ms"] = med["select_ms"] + med["sample_ms"]
    med["add_view_strict_ms"] = whole_views(v, f, views, True, args.repeats)
    med["add_view_not_strict_ms"] = whole_views(v, f, views, False, args.repeats)

    tviews = [(img, torch.as_tensor(K, dtype=torch.float32, device=dev), torch.as_tensor(E, dtype=torch.float32, device=dev))
              for img, K, E in views]
    masks = [r["visible_mask"] for r in passes[-1]]
    base = []
    for it in range(args.repeats + 1):
        colors = torch.zeros_like(v)
        row = []
        for (img, K, E), vis in zip(tviews, masks):
            a = event()
            torch_view(v, f, vis, img, K, E, colors)
            b = event()
            torch.cuda.synchronize()
            row.append(a.elapsed_time(b))
        if it:
            base.append(statistics.median(row))
    fresh = TextureBaker(v, f)
    for img, K, E in views:
        fresh.add_view(img, K, E)
    out = {"device": torch.cuda.get_device_name(0), "triangles": int(f.shape[0]), "vertices": int(v.shape[0]), "image": [W, H],
           "views": args.views, "repeats": args.repeats, "sampling": "reference", **med,
           "visible_faces_per_view": statistics.median(int(m.sum()) for m in masks),
           "baseline_torch_select_sample_ms": statistics.median(base), "baseline_ms_min_max": [min(base), max(base)],
           "baseline_over_select_plus_sample": statistics.median(base) / med["select_plus_sample_ms"],
           "baseline_max_abs_colour_difference": float((colors - fresh.vertex_colors).abs().max()),
           "baseline_same_baked_set": bool(torch.equal(colors.any(dim=1), fresh.baked_by >= 0))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
