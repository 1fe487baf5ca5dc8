#!/usr/bin/env python
"""Writes tests/golden/py_mesh_init.npz: a small seeded mesh and what the REFERENCE's Python produced for it on the CPU
(gaustudio/pipelines/initializers/mesh.py normal2rotation, rotmat2quaternion and MeshInitializer's _compute_* methods,
gaustudio/models/vanilla_sg.py VanillaPointCloud.create_from_attribute, imported unmodified through
ref_env.reference_modules()).  Data only.

    verts / faces / normals / colors      the mesh of mesh_init_model.random_mesh() (F = 40, V = 30)
    bary_<n> / radius_<n>                 the initializer's barycentric table and circle radius, n = 1, 3, 4, 6
    pos_<n> / nrm_<n> / col_<n> / scl_<n> _compute_gaussian_positions / _surface_normals / _colors / _scales
    rot_<n>                               normal2rotation(nrm_<n>)
    quirk_normals / quirk_rot             the sign() cases of normal2rotation and what it returns for them
    rand_R / rand_q                       rotmat2quaternion of 16 seeded matrices
    seed_* / seed_nocolor_f_dc            create_from_attribute as build_model calls it (n = 1), with colours and with rgb=None
    meta                                  text: the figures this script measured and asserted

The script asserts what tests/test_mesh_init_model.py relies on: the float32 model of tests/mesh_init_model.py is within 4 ulp
of each output's scale of the reference's torch CPU arithmetic, and the sign() cases agree exactly."""
import contextlib
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import mesh_init_model as mi  # noqa: E402

QUIRK_NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, -1], [0.3, -0.5, 0.8], [0.6, 0.8, 0.0]], dtype=np.float32)


@contextlib.contextmanager
def extra_stubs():
    """The initializers package's __init__ imports every initializer (COLMAP, hloc, dust3r ... and their third-party packages,
    which are not dependencies of this project).  Only its mesh.py is run here: the package is entered through an empty
    stand-in that carries the real directory as __path__, a pass-through `register` and a plain BaseInitializer, so that
    mesh.py itself is imported unmodified."""
    import gaustudio
    names = ["gaustudio.pipelines", "gaustudio.pipelines.initializers", "gaustudio.pipelines.initializers.base"]
    root = os.path.join(os.path.dirname(gaustudio.__file__), "pipelines")
    pipelines, inits, base = (types.ModuleType(n) for n in names)
    pipelines.__path__ = [root]
    inits.__path__ = [os.path.join(root, "initializers")]
    inits.register = lambda name: (lambda cls: cls)
    base.BaseInitializer = type("BaseInitializer", (), {"__init__": lambda self, initializer_config=None: None})
    pipelines.initializers, inits.base = inits, base
    sys.modules.update(zip(names, (pipelines, inits, base)))
    try:
        yield importlib.import_module("gaustudio.pipelines.initializers.mesh")
    finally:
        for n in names:
            sys.modules.pop(n, None)


def ulps(got, want):
    """max |got - want| in units of the spacing of float32 at max |want| (finite entries; the others must coincide)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin], equal_nan=True)
    if not fin.any():
        return 0.0
    unit = np.spacing(np.float32(np.abs(want[fin]).max()))
    return float(np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)).max() / unit)


def main():
    warnings.simplefilter("ignore")
    v, f, nr, col = mi.random_mesh()
    out = dict(verts=v, faces=f, normals=nr, colors=col, quirk_normals=QUIRK_NORMALS)
    rng = np.random.default_rng(9)
    rand_R = rng.normal(size=(16, 3, 3)).astype(np.float32)
    out["rand_R"] = rand_R
    worst = {}
    with ref_env.reference_modules(), extra_stubs():
        from gaustudio.pipelines.initializers.mesh import MeshInitializer, normal2rotation, rotmat2quaternion, inverse_sigmoid
        from gaustudio.models.vanilla_sg import VanillaPointCloud
        faces = torch.from_numpy(f.astype(np.int64))
        faces_verts, faces_normals, vcol = torch.from_numpy(v)[faces], torch.from_numpy(nr)[faces], torch.from_numpy(col)
        for n in (1, 3, 4, 6):
            init = MeshInitializer.__new__(MeshInitializer)
            init.n_gaussians_per_surface_triangle = n
            init._setup_barycentric_coordinates()
            out[f"bary_{n}"] = init.surface_triangle_bary_coords[..., 0].numpy()
            out[f"radius_{n}"] = np.float64(init.surface_triangle_circle_radius)
            pos = init._compute_gaussian_positions(faces_verts)
            nrm = init._compute_surface_normals(faces_normals)
            colors = init._compute_colors(faces, vcol, True)
            scl = init._compute_scales(faces_verts)
            rot = normal2rotation(nrm)
            assert init._compute_colors(faces, vcol, False) is None
            for k, t in (("pos", pos), ("nrm", nrm), ("col", colors), ("scl", scl), ("rot", rot)):
                out[f"{k}_{n}"] = t.numpy().copy()
            if n == 1:
                opacity = inverse_sigmoid(np.ones((pos.shape[0], 1)))
                for name, rgb in (("seed_", colors), ("seed_nocolor_", None)):
                    model = VanillaPointCloud.__new__(VanillaPointCloud)
                    model.max_sh_degree = 3
                    model.create_from_attribute(xyz=pos, rgb=rgb, scale=scl, opacity=opacity, rot=rot)
                    if rgb is None:
                        out[name + "f_dc"] = model._f_dc.cpu().numpy()
                    else:
                        for k in ("xyz", "f_dc", "f_rest", "opacity", "scale", "rot"):
                            out[name + k] = getattr(model, "_" + k).cpu().numpy()
        out["quirk_rot"] = normal2rotation(torch.from_numpy(QUIRK_NORMALS.copy())).numpy().copy()
        out["rand_q"] = rotmat2quaternion(torch.from_numpy(rand_R)).numpy().copy()

    # what the CPU test relies on
    for n in (1, 3, 4, 6):
        assert np.array_equal(mi.bary_table(n), out[f"bary_{n}"]) and np.float32(mi.RADIUS[n]) == np.float32(out[f"radius_{n}"])
        m = mi.seeds(v, f, nr, col, n)
        got = dict(pos=m["xyz"], nrm=mi.surface_normals(nr, f, n), col=mi.bary_sum(col, f, n), scl=m["scale"], rot=m["rot"])
        for k, a in got.items():
            worst[k] = max(worst.get(k, 0.0), ulps(a, out[f"{k}_{n}"]))
    m1 = mi.seeds(v, f, nr, col, 1)
    worst["f_dc"] = max(ulps(m1["f_dc"], out["seed_f_dc"]), ulps(mi.seeds(v, f, nr, None, 1)["f_dc"], out["seed_nocolor_f_dc"]))
    assert np.array_equal(m1["opacity"], out["seed_opacity"]) and np.array_equal(m1["f_rest"], out["seed_f_rest"])
    q = mi.quaternion(rand_R[:, :, 0], rand_R[:, :, 1], rand_R[:, :, 2])
    worst["rotmat2quaternion"] = ulps(q, out["rand_q"])
    assert np.array_equal(mi.normal2rotation(QUIRK_NORMALS), out["quirk_rot"], equal_nan=True), "a sign() case differs"
    assert max(worst.values()) <= 4.0, f"the model is more than 4 ulp of scale from the reference: {worst}"
    out["meta"] = np.array(
        "mesh_init_model.random_mesh(): F = 40, V = 30; max |model - reference| in ulp of each output's largest magnitude, over "
        f"n = 1, 3, 4, 6: {', '.join(f'{k} {x:.2f}' for k, x in worst.items())} (asserted <= 4); the 7 sign() cases of "
        f"normal2rotation agree exactly; numpy {np.__version__}, torch {torch.__version__.split('+')[0]}")
    path = os.path.join(HERE, "py_mesh_init.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes\n{out['meta']}")


if __name__ == "__main__":
    main()
