"""The error of the float32 loss model (tests/loss_model.py: the kernels' arithmetic) against the float64 restatement, beside
the error of torch's own float32 evaluation of the same formula, on three seeded scenes.  tests/test_loss_model.py asserts on
measure(); `python tests/loss_model_parity.py` writes the figures to profiles/photometric_loss_parity.json."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_model as lm  # noqa: E402

F32 = np.float32
SCENES = ("noise", "sinusoid", "flat_halves")
SHAPES = ((37, 53), (64, 64))
PLANES = 3


def scene(name, shape, seed=0):
    """(image, target), [3, H, W] float32."""
    H, W = shape
    rng = np.random.default_rng([seed, SCENES.index(name), H, W])
    if name == "noise":                      # noise against noise
        return rng.random((PLANES, H, W), dtype=F32), rng.random((PLANES, H, W), dtype=F32)
    if name == "sinusoid":                   # a smooth image against itself plus N(0, 0.05)
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([0.5 + 0.4 * np.sin(0.21 * xx + 0.5 * p) * np.cos(0.13 * yy - 0.3 * p) for p in range(PLANES)])
        return base.astype(F32), (base + rng.normal(0, 0.05, base.shape)).astype(F32)
    if name == "flat_halves":                # 0.9 | 0.1 against itself plus N(0, 1e-3): the worst cancellation in E[x^2] - mu^2
        base = np.full((PLANES, H, W), 0.9)
        base[:, :, W // 2:] = 0.1
        return base.astype(F32), (base + rng.normal(0, 1e-3, base.shape)).astype(F32)
    raise KeyError(name)


def errors(got, r64):
    return dict(loss=abs(float(got["loss"]) - r64["loss"]),
                ssim_map=float(np.abs(got["ssim_map"].astype(np.float64) - r64["ssim_map"]).max()),
                grad_over_scale=float(np.abs(got["grad"].astype(np.float64) - r64["grad"]).max() / np.abs(r64["grad"]).max()))


def measure(lambda_dssim=0.2):
    out = {}
    for s in SCENES:
        for shape in SHAPES:
            x, y = scene(s, shape)
            r64 = lm.reference(x, y, lambda_dssim, "float64")
            out[f"{s}-{shape[0]}x{shape[1]}"] = dict(model=errors(lm.loss_and_grad(x, y, lambda_dssim), r64),
                                                     torch_float32=errors(lm.reference(x, y, lambda_dssim, "float32"), r64))
    return out


if __name__ == "__main__":
    rep = measure()
    for v in rep.values():
        v["ratio"] = {k: (v["model"][k] / v["torch_float32"][k] if v["torch_float32"][k] else None) for k in v["model"]}
    doc = dict(what="error against the float64 restatement (F.conv2d, autograd) of the published 3DGS loss, lambda 0.2, 3 planes: "
                    "the float32 model of the HIP kernels (tests/loss_model.py) beside torch's float32 evaluation on the CPU",
               bound="model <= 2 x torch_float32 on each figure (tests/test_loss_model.py)", scenes=rep)
    path = os.path.join(os.path.dirname(HERE), "profiles", "photometric_loss_parity.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v["ratio"] for k, v in rep.items()}, indent=1))
