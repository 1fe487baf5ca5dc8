#!/usr/bin/env python
"""The gs-extract-pcd loop (gaustudio/scripts/extract_pcd.py:305-360 and its normal_fusion / clean_point_cloud) with every
stage on the MI355X:

    Gaussian PLY + cameras.json -> GaussianRasterizer (depth, median depth / id, opacity) -> masked_bilateral_filter
        -> depth_to_normals -> world normals -> view_records -> NormalFusion -> clean_point_cloud -> fused.ply

Runs on the synthetic shell of extract_mesh_synthetic.py, so it needs no dataset:
    python examples/extract_pcd_synthetic.py [out_dir] [--meshing {sap,None}] [--dpsr_res R]
--meshing sap (the reference's default mesher; here the default is None, the behaviour before the option existed) runs
gaustudio_amd.sap.mesh_sap on the cleaned cloud and writes fused_mesh.ply.  The other meshers of the script (NKSR, Open3D
Poisson, pymeshlab) are third-party packages and not part of this example.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extract_mesh_synthetic import write_inputs  # noqa: E402
from gaustudio_amd import GaussianRasterizationSettings, GaussianRasterizer, formats, pcd_fusion, postprocess as pp  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out", nargs="?", default="extract_pcd_out")
    ap.add_argument("--meshing", choices=["sap", "None"], default="None")
    ap.add_argument("--dpsr_res", type=int, default=256)
    args = ap.parse_args()
    out = args.out
    os.makedirs(out, exist_ok=True)
    write_inputs(out)
    dev = torch.device("cuda:0")
    pcd = formats.load_gaussian_ply(os.path.join(out, "point_cloud.ply"), device=dev)
    cameras = formats.load_cameras_json(os.path.join(out, "cameras.json"))
    act = pcd.activated()
    xyz = act["means3D"].contiguous()
    radius = pcd_fusion.scene_radius(torch.stack([rec.cam.campos for rec in cameras]))      # getNerfppNorm
    times = dict(render=0.0, filter_normals=0.0, records=0.0)
    fusion = pcd_fusion.NormalFusion(xyz)

    def tick():
        torch.cuda.synchronize()
        return time.perf_counter()

    for rec in cameras:
        cam = rec.cam
        t0 = tick()
        rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                           cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 0, cam.campos.to(dev), False, False)
        with torch.no_grad():
            _, _, depth, median, opacity = GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz),
                                                                  opacities=act["opacities"], shs=act["shs"],
                                                                  scales=act["scales"], rotations=act["rotations"])
        t1 = tick()
        f = cam.width / (2 * cam.tanfovx)
        K = torch.tensor([[f, 0, cam.width / 2], [0, f, cam.height / 2], [0, 0, 1]])
        w2c = cam.viewmatrix.t().contiguous()                                        # Camera.extrinsics
        filtered, fg = pp.masked_bilateral_filter(depth[0], opacity[0] > 0.1)         # :322-323
        cam_normals = pp.depth_to_normals(filtered, K)                                # :324
        cam_normals[~fg] = -1                                                         # :325
        world_normals = cam_normals @ w2c[:3, :3].to(dev).inverse().t()               # :327 normal2worldnormal
        t2 = tick()
        ids, normals, conf = pcd_fusion.view_records(median, opacity, world_normals, radius)   # :328-337
        fusion.add_view(ids, normals, conf, w2c[:3, 3])
        t3 = tick()
        times["render"] += t1 - t0
        times["filter_normals"] += t2 - t1
        times["records"] += t3 - t2
    t0 = tick()
    unique_ids, fused = fusion.finalize()
    t1 = tick()
    points = xyz[unique_ids.long()]
    kept = pcd_fusion.clean_point_cloud(points, fused)
    t2 = tick()
    times["fusion"], times["cleaning"] = t1 - t0, t2 - t1
    uid = unique_ids.long()[kept]
    p, n = points[kept].cpu().numpy(), fused[kept].cpu().numpy()
    colour = (pcd.f_dc.reshape(-1, 3)[uid] * 0.28209479177387814 + 0.5).clamp(0, 1).cpu().numpy()   # SH2RGB, clipped
    v = np.zeros(len(p), dtype=[(c, "f4") for c in ("x", "y", "z", "nx", "ny", "nz")] + [(c, "u1") for c in ("red", "green", "blue")])
    v["x"], v["y"], v["z"] = p[:, 0], p[:, 1], p[:, 2]
    v["nx"], v["ny"], v["nz"] = n[:, 0], n[:, 1], n[:, 2]
    rgb = np.round(colour * 255).astype(np.uint8)
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    formats.write_ply_vertices(os.path.join(out, "fused.ply"), v)
    outward = float(((n * p).sum(axis=1) > 0).mean()) if len(p) else 0.0
    print(f"{len(cameras)} views, {fusion.num_records} records -> {len(unique_ids)} fused points, {len(p)} after cleaning; "
          f"{100 * outward:.1f} % of the normals point outward")
    if args.meshing == "sap":
        from gaustudio_amd import sap
        t0 = tick()
        vertices, faces = sap.mesh_sap(points[kept].contiguous(), fused[kept].contiguous(), dpsr_res=args.dpsr_res)
        times["meshing"] = tick() - t0
        formats.write_ply_mesh(os.path.join(out, "fused_mesh.ply"), vertices, faces)
        print(f"sap meshing at {args.dpsr_res}^3: {len(vertices)} vertices, {len(faces)} faces -> fused_mesh.ply")
    print("stage times (ms): " + ", ".join(f"{k} {1e3 * t:.1f}" for k, t in times.items()))


if __name__ == "__main__":
    main()
