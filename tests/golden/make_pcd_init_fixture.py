#!/usr/bin/env python
"""Writes tests/golden/pcd_init_ref.npz: small point clouds and what the REFERENCE's Python produced for them on the CPU
(gaustudio/models/vanilla_sg.py calculate_dist2_python and VanillaPointCloud.create_from_attribute,
gaustudio/pipelines/initializers/pcd.py normal2rotation, gaussiansky.py fibonacci_sphere, imported unmodified through
ref_env.reference_modules() and the initializers-package stand-in of make_mesh_init_fixture.py).  Data only.

    cloud_<name> / dist2_<name>     the clouds of clouds() and calculate_dist2_python of each (float32)
    seed_in_* / seed_*              create_from_attribute(xyz, rgb, scale=None, opacity, rot) as PcdInitializer calls it on the
                                    random cloud (seed_in_rot = normal2rotation(seed_in_normals), random normals that are not
                                    unit; opacity = inverse_sigmoid(0.1 * ones) float64)
    bare_*                          create_from_attribute(xyz) alone: rgb, rot and opacity defaulted
    n2r_normals / n2r_rot           pcd.normal2rotation on the inward normals of a 100-point Fibonacci sphere and the sign() cases
    fib_<s>_points / fib_<s>_normals  fibonacci_sphere(s), s = 2, 9, 100 (float64)
    meta                            text: what this script measured

simple_knn is made unimportable inside the context, so that calculate_dist2() takes the scipy path the way it does on a box
without the extension (the attribute-sink stub of ref_env would otherwise "import")."""
import importlib
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import make_mesh_init_fixture as mmf  # noqa: E402
import pcd_init_model as pim  # noqa: E402
import mesh_init_model as mi  # noqa: E402


def clouds():
    """The five clouds of the CPU test, float32 [N,3]."""
    rng = np.random.default_rng(31)
    g = np.arange(5, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    dup = np.concatenate([np.repeat(np.float32([[0.25, -0.5, 0.75]]), 40, axis=0), rng.uniform(-1, 1, (10, 3))]).astype(np.float32)
    t = np.sort(rng.uniform(0, 1, 30)).astype(np.float32)
    line = np.stack([t, np.float32(2) * t, np.float32(-1) * t], axis=1).astype(np.float32)
    clusters = np.concatenate([rng.normal(0, 0.05, (60, 3)), rng.normal(0, 0.05, (60, 3)) + [3, 0, 0], [[400.0, -250.0, 90.0]]]).astype(np.float32)
    return dict(random=rng.uniform(-1, 1, (500, 3)).astype(np.float32), lattice=lattice, duplicates=dup, line=line, clusters=clusters)


def ulp_steps(a, b):
    """max number of float32 steps between two finite float32 arrays."""
    ia, ib = (np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return int(np.abs(ia - ib).max()), int((ia != ib).sum())


def main():
    warnings.simplefilter("ignore")
    out = {}
    cl = clouds()
    rng = np.random.default_rng(32)
    n = len(cl["random"])
    rgb = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    extra = {}
    for name in ("pycolmap", "torchvision"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:       # noqa: BLE001
                extra[name] = ref_env._Stub(name)
    with ref_env.reference_modules(), mmf.extra_stubs():
        sys.modules.update(extra)
        sys.modules["simple_knn"] = None
        sys.modules["simple_knn._C"] = None
        try:
            from gaustudio.models.vanilla_sg import VanillaPointCloud, calculate_dist2_python
            pcd = importlib.import_module("gaustudio.pipelines.initializers.pcd")
            sky = importlib.import_module("gaustudio.pipelines.initializers.gaussiansky")
            for name, p in cl.items():
                out[f"cloud_{name}"] = p
                out[f"dist2_{name}"] = calculate_dist2_python(torch.from_numpy(p)).numpy().copy()
            fib = {s: sky.fibonacci_sphere(s) for s in (2, 9, 100)}
            for s, (p, q) in fib.items():
                out[f"fib_{s}_points"], out[f"fib_{s}_normals"] = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
            n2r_normals = np.concatenate([fib[100][1].astype(np.float32), mmf.QUIRK_NORMALS])
            out["n2r_normals"] = n2r_normals
            out["n2r_rot"] = pcd.normal2rotation(torch.from_numpy(n2r_normals.copy())).numpy().copy()

            model = VanillaPointCloud.__new__(VanillaPointCloud)
            model.max_sh_degree = 3
            assert model.calculate_dist2() is calculate_dist2_python, "simple_knn must not import here"
            points = torch.from_numpy(cl["random"])
            rot = pcd.normal2rotation(torch.from_numpy(nrm.copy()))
            opacity = pcd.inverse_sigmoid(0.1 * np.ones((n, 1)))
            model.create_from_attribute(xyz=points, rgb=torch.from_numpy(rgb), scale=None, opacity=opacity, rot=rot)
            out.update(seed_in_rgb=rgb, seed_in_normals=nrm, seed_in_rot=rot.numpy().copy())
            for k in ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot"):
                out["seed_" + k] = getattr(model, "_" + k).cpu().numpy().copy()
            bare = VanillaPointCloud.__new__(VanillaPointCloud)
            bare.max_sh_degree = 3
            bare.create_from_attribute(xyz=points)
            for k in ("f_dc", "opacity", "scale", "rot"):
                out["bare_" + k] = getattr(bare, "_" + k).cpu().numpy().copy()
        finally:
            for name in ("simple_knn", "simple_knn._C", *extra):
                sys.modules.pop(name, None)

    # what tests/test_pcd_init_model.py relies on, measured here
    notes = []
    for name, p in cl.items():
        steps, count = ulp_steps(pim.mean_dist2(p), out[f"dist2_{name}"])
        notes.append(f"dist2 {name}: {count} of {len(p)} differ, at most {steps} float32 step(s)")
    m = pim.point_seeds(cl["random"], rgb=rgb, rot=out["seed_in_rot"], opacity=pim.PCD_OPACITY)
    steps, count = ulp_steps(m["scale"], out["seed_scale"])
    notes.append(f"seed scale: {count} of {m['scale'].size} differ, at most {steps} step(s)")
    for k in ("xyz", "f_dc", "f_rest", "opacity", "rot"):
        notes.append(f"seed {k}: {'equal' if np.array_equal(m[k], out['seed_' + k], equal_nan=True) else 'DIFFERS'}")
    notes.append("normal2rotation (mesh_init_model vs pcd.py) on the Fibonacci normals and the sign() cases: "
                 + ("equal" if np.array_equal(mi.normal2rotation(out["n2r_normals"]), out["n2r_rot"], equal_nan=True) else "DIFFERS"))
    got = mi.normal2rotation(nrm)
    notes.append(f"normal2rotation on the {n} random normals: {int((got != out['seed_in_rot']).any(axis=1).sum())} rows differ, "
                 f"{mmf.ulps(got, out['seed_in_rot']):.2f} ulp of the largest magnitude at most (torch's vectorised CPU kernels)")
    bare = pim.point_seeds(cl["random"])
    notes.append("bare f_dc / opacity / rot: " + ("equal" if all(np.array_equal(bare[k], out["bare_" + k]) for k in ("f_dc", "opacity", "rot")) else "DIFFERS"))
    out["meta"] = np.array("; ".join(notes) + f"; numpy {np.__version__}, torch {torch.__version__.split('+')[0]}")
    path = os.path.join(HERE, "pcd_init_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes\n" + "\n".join(notes))


if __name__ == "__main__":
    main()
