#!/usr/bin/env python
"""Writes tests/golden/py_scaffold_grad.npz: two small seeded Scaffold-GS models (k = 10 offsets; without and with the feature
bank), seeded cotangents of the five outputs, and the gradients the REFERENCE's renderer gives for them under torch.autograd on
the CPU -- gaustudio/renderers/scaffold_renderer.py ScaffoldRenderer.get_gaussians_properties, imported unmodified through
ref_env.reference_modules() and handed the stub model of make_scaffold_fixture.py with leaves that require grad.  Data only.

    <p>anchor / anchor_feat / offset / scaling / rot / campos / visible        the inputs (p = "plain_" or "bank_")
    <p>opacity_W1 ... <p>bank_b2                                               the nn.Linear tensors of the MLPs
    <p>kept                                                                    bool [N, k]: the float64 run's mask
    <p>cot_xyz / colors / opacity / scales / rotations                         the cotangents [M, .], float32 values
    <p>grad_<leaf>                                                             float64 gradients of every leaf: anchor, anchor_feat,
                                                                               offset, scaling, opacity_W1 ... (bank_b2)
    <p>eref_<leaf>, <p>gscale_<leaf>                                           max |float32 run - float64 run|, max |float64 gradient|

Conditions (asserted here and by the test that loads the file), in the float64 run over the visible anchors: no opacity logit
within 1e-3 of 0 (no summation order flips the mask), and no hidden pre-activation of any MLP within 1e-5 of 0 (a ReLU's
gradient is discontinuous: a unit whose sign differs between float32 and float64 changes the gradient by O(1)).  Anchors that
violate one get a fresh feature row -- a fresh position when it is the bank's hidden layer, which reads the view alone --
until none does."""
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
import scaffold_model as sm  # noqa: E402
from make_scaffold_fixture import Camera, StubModel  # noqa: E402

N, K = 300, 10
MARGIN = 1e-3
RELU_MARGIN = 1e-5
OUTS = ("xyz", "colors", "opacity", "scales", "rotations")
MLP_ATTR = (("opacity", "mlp_opacity"), ("cov", "mlp_cov"), ("color", "mlp_color"), ("bank", "mlp_feature_bank"))


def preactivations64(m, campos, visible):
    """float64: (opacity logits [V,k], hidden pre-activations of the three MLPs [V,96], of the bank [V,32] or None)."""
    s = StubModel(m, torch.float64)
    with torch.no_grad():
        a, f = s.attrs["anchor"][visible], s.attrs["anchor_feat"][visible]
        v = a - torch.from_numpy(campos).double()
        d = v.norm(dim=1, keepdim=True)
        v = v / d
        vd = torch.cat([v, d], dim=1)
        pre_bank = None
        if s.use_feat_bank:
            pre_bank = s.attrs["mlp_feature_bank"][0](vd).numpy()
            w = s.attrs["mlp_feature_bank"](vd)
            f = f[:, ::4].repeat(1, 4) * w[:, 0:1] + f[:, ::2].repeat(1, 2) * w[:, 1:2] + f * w[:, 2:3]
        x = torch.cat([f, vd], dim=1)
        pre = torch.cat([s.attrs[name][0](x) for name in ("mlp_opacity", "mlp_cov", "mlp_color")], dim=1).numpy()
        return s.attrs["mlp_opacity"][:3](x).numpy(), pre, pre_bank


def leaves_of(stub):
    res = dict(anchor=stub.attrs["anchor"], anchor_feat=stub.attrs["anchor_feat"], offset=stub.attrs["offset"], scaling=stub.attrs["scale"])
    for short, attr in MLP_ATTR:
        if attr in stub.attrs:
            seq = stub.attrs[attr]
            res.update({f"{short}_W1": seq[0].weight, f"{short}_b1": seq[0].bias, f"{short}_W2": seq[2].weight, f"{short}_b2": seq[2].bias})
    return res


def run_reference(renderer_cls, m, campos, visible, cot, dtype):
    """The reference under autograd: name -> gradient (numpy, of `dtype`)."""
    r = renderer_cls.__new__(renderer_cls)
    r.prefilter_voxel = lambda cam, model: torch.from_numpy(visible)
    stub = StubModel(m, dtype)
    lv = leaves_of(stub)
    for t in lv.values():
        t.requires_grad_(True)
    xyz, shs, color, opacity, scales, rotations, cov = r.get_gaussians_properties(Camera(campos, dtype), stub)
    assert shs is None and cov is None
    outs = dict(zip(OUTS, (xyz, color, opacity, scales, rotations)))
    grads = torch.autograd.grad([outs[n] for n in OUTS], list(lv.values()), [torch.from_numpy(cot[n]).to(dtype) for n in OUTS])
    return {k: g.numpy().copy() for k, g in zip(lv, grads)}, int(xyz.shape[0])


def main():
    warnings.simplefilter("ignore")
    out = {}
    meta = []
    with ref_env.reference_modules():
        from gaustudio.renderers.scaffold_renderer import ScaffoldRenderer
        for prefix, bank, seed in (("plain_", False, 21), ("bank_", True, 22)):
            m = sm.random_model(N, K, seed=seed, bank=bank)
            rng = np.random.default_rng(seed + 100)
            campos = np.array([0.3, -0.2, 4.0], dtype=np.float32)
            visible = rng.uniform(size=N) < 0.7
            vis_idx = np.nonzero(visible)[0]
            redrawn = 0
            while True:
                lg, pre, pre_bank = preactivations64(m, campos, visible)
                bad_feat = vis_idx[(np.abs(lg) < 2 * MARGIN).any(axis=1) | (np.abs(pre) < 2 * RELU_MARGIN).any(axis=1)]
                bad_pos = vis_idx[(np.abs(pre_bank) < 2 * RELU_MARGIN).any(axis=1)] if bank else bad_feat[:0]
                if bad_feat.size == 0 and bad_pos.size == 0:
                    break
                m["anchor_feat"][bad_feat] = rng.normal(size=(bad_feat.size, sm.FEAT)).astype(np.float32)
                m["anchor"][bad_pos] = rng.normal(size=(bad_pos.size, 3)).astype(np.float32)
                redrawn += bad_feat.size + bad_pos.size
            assert np.abs(lg).min() >= MARGIN and np.abs(pre).min() >= RELU_MARGIN
            assert not bank or np.abs(pre_bank).min() >= RELU_MARGIN
            kept = np.zeros((N, K), dtype=bool)
            kept[vis_idx] = lg > 0
            m_rows = int(kept.sum())
            cot = {name: rng.normal(size=(m_rows, c)).astype(np.float32) for name, c in zip(OUTS, (3, 3, 1, 3, 4))}
            for name in ("anchor", "anchor_feat", "offset", "scaling", "rot"):
                out[prefix + name] = m[name]
            out[prefix + "campos"], out[prefix + "visible"], out[prefix + "kept"] = campos, visible, kept
            for mlp in ("opacity", "cov", "color") + (("bank",) if bank else ()):
                for nm, t in zip(("W1", "b1", "W2", "b2"), m["bank" if mlp == "bank" else "mlp_" + mlp]):
                    out[f"{prefix}{mlp}_{nm}"] = t
            for name, c in cot.items():
                out[f"{prefix}cot_{name}"] = c
            g64, rows64 = run_reference(ScaffoldRenderer, m, campos, visible, cot, torch.float64)
            g32, rows32 = run_reference(ScaffoldRenderer, m, campos, visible, cot, torch.float32)
            assert rows64 == rows32 == m_rows
            ratios = []
            for name, g in g64.items():
                assert g.dtype == np.float64 and g32[name].dtype == np.float32
                out[f"{prefix}grad_{name}"] = g
                out[f"{prefix}eref_{name}"] = np.float64(np.abs(g32[name].astype(np.float64) - g).max())
                out[f"{prefix}gscale_{name}"] = np.float64(np.abs(g).max())
                ratios.append(out[f"{prefix}eref_{name}"] / out[f"{prefix}gscale_{name}"])
            meta.append(f"{prefix[:-1]}: V = {int(visible.sum())} visible anchors, M = {m_rows} Gaussians, min |logit| = "
                        f"{np.abs(lg).min():.3e}, min |hidden pre-activation| = {np.abs(pre).min():.3e}, {redrawn} rows redrawn, "
                        f"eref / gscale = {min(ratios):.1e} .. {max(ratios):.1e} over {len(ratios)} leaves")
    out["meta"] = np.array(f"N = {N}, k = {K}; " + "; ".join(meta) + f"; numpy {np.__version__}, torch {torch.__version__.split('+')[0]}")
    path = os.path.join(HERE, "py_scaffold_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes\n{out['meta']}")


if __name__ == "__main__":
    main()
