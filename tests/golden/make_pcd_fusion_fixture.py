"""Writes tests/golden/py_pcd_fusion.npz (not ref_*: that prefix names the hipified-kernel fixtures) by EXECUTING the reference's own normal_fusion
(gaustudio/scripts/extract_pcd.py:108-183) on CPU tensors, through ref_env.reference_modules() (dev container only; the
reference checkout is needed).  Two cases:
  * coherent: noisy outward normals on a bumpy sphere (no NaN);
  * scattered: random unit normals, so ids without a consistent record fuse to NaN and the smoothing spreads it.
Run:  python tests/golden/make_pcd_fusion_fixture.py
"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the drop-in gaustudio_diff_gaussian_rasterization
import ref_env  # noqa: E402


def make_case(seed, scattered):
    rng = np.random.default_rng(seed)
    P = 3000
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (d * (1.0 + 0.05 * np.sin(4 * d[:, :1]))).astype(np.float32)
    views = []
    for v in range(6):
        n = 1200
        ids = rng.integers(0, P, size=n).astype(np.int32)
        if scattered:
            nrm = rng.normal(size=(n, 3))
        else:
            nrm = d[ids] + 0.25 * rng.normal(size=(n, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        conf = rng.uniform(0.5, 1.0, size=n).astype(np.float32)
        ang = 2 * np.pi * v / 6
        w2c = np.eye(4, dtype=np.float32)
        w2c[:3, 3] = [3.0 * np.cos(ang), 0.4 * (v - 2.5), 3.0 * np.sin(ang)]
        views.append((ids, nrm, conf, w2c))
    return xyz, views


def run_reference(xyz, views):
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    with ref_env.reference_modules():
        from gaustudio.scripts import extract_pcd
        pcd = SimpleNamespace(_xyz=torch.from_numpy(xyz))
        cams = [SimpleNamespace(extrinsics=torch.from_numpy(w2c)) for _, _, _, w2c in views]
        uids, normals = extract_pcd.normal_fusion(pcd, [torch.from_numpy(v[0]) for v in views],
                                                  [torch.from_numpy(v[1]) for v in views],
                                                  [torch.from_numpy(v[2]) for v in views], cams)
    return uids.numpy(), normals.numpy()


def main():
    out = {}
    for name, seed, scattered in (("coherent", 1, False), ("scattered", 2, True)):
        xyz, views = make_case(seed, scattered)
        uids, normals = run_reference(xyz, views)
        nan = np.isnan(normals).any(axis=1)
        assert nan.any() == scattered, (name, nan.sum())
        out[f"{name}_xyz"] = xyz
        out[f"{name}_ids"] = np.concatenate([v[0] for v in views])
        out[f"{name}_normals"] = np.concatenate([v[1] for v in views])
        out[f"{name}_conf"] = np.concatenate([v[2] for v in views])
        out[f"{name}_view_sizes"] = np.array([len(v[0]) for v in views], dtype=np.int64)
        out[f"{name}_w2c"] = np.stack([v[3] for v in views])
        out[f"{name}_unique_ids"] = uids
        out[f"{name}_fused_normals"] = normals
        print(f"{name}: {len(uids)} fused points, {int(nan.sum())} NaN")
    np.savez_compressed(os.path.join(HERE, "py_pcd_fusion.npz"), **out)


if __name__ == "__main__":
    main()
