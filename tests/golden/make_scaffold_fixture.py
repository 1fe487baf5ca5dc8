#!/usr/bin/env python
"""Writes tests/golden/py_scaffold.npz: two small seeded Scaffold-GS models (N = 300 anchors, k = 10 offsets; without and with
the feature bank) and what the REFERENCE's renderer produced for them on the CPU -- gaustudio/renderers/scaffold_renderer.py
ScaffoldRenderer.get_gaussians_properties, imported unmodified through ref_env.reference_modules() and handed a stub model
object (get_attribute, n_offsets, use_feat_bank, config) and a prefilter_voxel that returns the recorded mask.  Data only.

    <p>anchor / anchor_feat / offset / scaling / rot / campos / visible        the inputs (p = "plain_" or "bank_")
    <p>opacity_W1 ... <p>bank_b2                                               the nn.Linear tensors of the MLPs
    <p>f32_xyz / color / opacity / scales / rotations                          the five outputs, float32 run
    <p>f64_*                                                                   the same code with everything cast to float64
    <p>f64_logits                                                              the float64 opacity pre-activations [V, k]

Condition (asserted here and by the test that loads the file): in the float64 run no opacity logit lies within 1e-3 of 0, so
that no summation order can flip the mask.  Anchors that violate it get a fresh feature row until none does."""
import os
import sys
import warnings

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import scaffold_model as sm  # noqa: E402

N, K = 300, 10
MARGIN = 1e-3
OUTS = ("xyz", "color", "opacity", "scales", "rotations")


def sequential(w, last, dtype):
    l1, l2 = nn.Linear(w[0].shape[1], w[0].shape[0]), nn.Linear(w[2].shape[1], w[2].shape[0])
    with torch.no_grad():
        for lin, (wt, b) in ((l1, w[0:2]), (l2, w[2:4])):
            lin.weight.copy_(torch.from_numpy(wt))
            lin.bias.copy_(torch.from_numpy(b))
    return nn.Sequential(*([l1, nn.ReLU(True), l2] + ([last] if last is not None else []))).to(dtype)


class StubModel:
    """What get_gaussians_properties asks of a model."""

    def __init__(self, m, dtype):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        self.attrs = dict(anchor=t(m["anchor"]), anchor_feat=t(m["anchor_feat"]), offset=t(m["offset"]), scale=t(m["scaling"]),
                          rot=t(m["rot"]), mlp_opacity=sequential(m["mlp_opacity"], nn.Tanh(), dtype),
                          mlp_cov=sequential(m["mlp_cov"], None, dtype), mlp_color=sequential(m["mlp_color"], nn.Sigmoid(), dtype))
        self.use_feat_bank = m["bank"] is not None
        if self.use_feat_bank:
            self.attrs["mlp_feature_bank"] = sequential(m["bank"], nn.Softmax(dim=1), dtype)
        self.n_offsets = m["offset"].shape[1]
        self.config = {"activations": {"scale": "exp", "opacity": "sigmoid", "rot": "normalize"}}

    def get_attribute(self, name):
        return self.attrs[name]


class Camera:
    def __init__(self, campos, dtype):
        self.camera_center = torch.from_numpy(campos).to(dtype)


def run_reference(renderer_cls, m, campos, visible, dtype):
    r = renderer_cls.__new__(renderer_cls)
    r.prefilter_voxel = lambda cam, model: torch.from_numpy(visible)
    with torch.no_grad():
        xyz, shs, color, opacity, scales, rotations, cov = r.get_gaussians_properties(Camera(campos, dtype), StubModel(m, dtype))
    assert shs is None and cov is None
    return dict(zip(OUTS, (t.numpy().copy() for t in (xyz, color, opacity, scales, rotations))))


def logits64(m, campos, visible):
    """The float64 opacity pre-activations of the visible anchors, by the float64 modules."""
    s = StubModel(m, torch.float64)
    with torch.no_grad():
        a, f = s.attrs["anchor"][visible], s.attrs["anchor_feat"][visible]
        v = a - torch.from_numpy(campos).double()
        d = v.norm(dim=1, keepdim=True)
        v = v / d
        if s.use_feat_bank:
            w = s.attrs["mlp_feature_bank"](torch.cat([v, d], dim=1))
            f = f[:, ::4].repeat(1, 4) * w[:, 0:1] + f[:, ::2].repeat(1, 2) * w[:, 1:2] + f * w[:, 2:3]
        return s.attrs["mlp_opacity"][:3](torch.cat([f, v, d], dim=1)).numpy()


def main():
    warnings.simplefilter("ignore")
    out = {}
    meta = []
    with ref_env.reference_modules():
        from gaustudio.renderers.scaffold_renderer import ScaffoldRenderer
        for prefix, bank, seed in (("plain_", False, 11), ("bank_", True, 12)):
            m = sm.random_model(N, K, seed=seed, bank=bank)
            rng = np.random.default_rng(seed + 100)
            campos = np.array([0.3, -0.2, 4.0], dtype=np.float32)
            visible = rng.uniform(size=N) < 0.7
            redrawn = 0
            while True:
                lg = logits64(m, campos, visible)
                bad = np.nonzero(visible)[0][(np.abs(lg) < 2 * MARGIN).any(axis=1)]
                if bad.size == 0:
                    break
                m["anchor_feat"][bad] = rng.normal(size=(bad.size, sm.FEAT)).astype(np.float32)
                redrawn += bad.size
            assert np.abs(lg).min() >= MARGIN
            for name in ("anchor", "anchor_feat", "offset", "scaling", "rot"):
                out[prefix + name] = m[name]
            out[prefix + "campos"], out[prefix + "visible"] = campos, visible
            for mlp in ("opacity", "cov", "color") + (("bank",) if bank else ()):
                for nm, t in zip(("W1", "b1", "W2", "b2"), m["bank" if mlp == "bank" else "mlp_" + mlp]):
                    out[f"{prefix}{mlp}_{nm}"] = t
            for tag, dtype in (("f32_", torch.float32), ("f64_", torch.float64)):
                for name, a in run_reference(ScaffoldRenderer, m, campos, visible, dtype).items():
                    out[prefix + tag + name] = a
            out[prefix + "f64_logits"] = lg
            assert out[prefix + "f64_xyz"].shape[0] == int((lg > 0).sum()) == out[prefix + "f32_xyz"].shape[0]
            meta.append(f"{prefix[:-1]}: V = {int(visible.sum())} visible anchors, M = {int((lg > 0).sum())} Gaussians, min |logit| = "
                        f"{np.abs(lg).min():.3e}, {redrawn} feature rows redrawn")
    out["meta"] = np.array(f"N = {N}, k = {K}; " + "; ".join(meta) + f"; numpy {np.__version__}, torch {torch.__version__.split('+')[0]}")
    path = os.path.join(HERE, "py_scaffold.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes\n{out['meta']}")


if __name__ == "__main__":
    main()
