"""How far tests/optim_model.py's Adam (the float order of csrc/gsr_optim.hip) sits from torch.optim.Adam in float64, beside
torch.optim.Adam's own float32: 50 steps on random gradients.  tests/test_optim_model.py asserts on measure();
`python tests/optim_model_parity.py` writes the figures to profiles/optimizer_parity.json."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_model as om  # noqa: E402

STEPS, SIZE, LR, BETAS, EPS = 50, 4096, 1e-2, (0.9, 0.999), 1e-15


def measure(seed=0):
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(SIZE).astype(np.float32)
    grads = [(rng.standard_normal(SIZE) * np.exp(rng.uniform(-6.0, 0.0, SIZE))).astype(np.float32) for _ in range(STEPS)]

    def torch_adam(dtype):
        p = torch.tensor(p0, dtype=dtype, requires_grad=True)
        opt = torch.optim.Adam([p], lr=LR, betas=BETAS, eps=EPS)
        for g in grads:
            p.grad = torch.tensor(g, dtype=dtype)
            opt.step()
        return p.detach().double().numpy()

    ref64, ref32 = torch_adam(torch.float64), torch_adam(torch.float32)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        p, m, v = om.adam_update(p, g, m, v, om.adam_consts(LR, BETAS[0], BETAS[1], t), EPS)
    return dict(steps=STEPS, elements=SIZE, lr=LR, betas=list(BETAS), eps=EPS,
                model_max_abs_error_vs_float64=float(np.abs(p.astype(np.float64) - ref64).max()),
                torch_float32_max_abs_error_vs_float64=float(np.abs(ref32 - ref64).max()))


if __name__ == "__main__":
    out = measure()
    path = os.path.join(os.path.dirname(HERE), "profiles", "optimizer_parity.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
