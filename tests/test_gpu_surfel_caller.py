"""-m gpu: the surfel operator driven exactly the way GauStudio's SurfelRenderer drives it.  The replay
(tests/golden/surfel_call_record.py) is pinned to the unmodified renderer by tests/golden/py_surfel_calls.json; here it first
reproduces the recorded call on the GPU box, then pushes the same call through the real `diff_surfel_rasterization`, runs the
renderer's post-processing of the allmap (surfel_renderer.py:96-114: the normal rotated to world space, depth / alpha with
nan_to_num, len(allmap) == 7) and backpropagates through all of it to the raw point-cloud attributes."""
import json
import os
import sys

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import surfel_call_record as scr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", scr.CASES, ids=lambda c: c["name"])
def test_surfel_renderer_call_through_the_real_operator(case):
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    want = json.load(open(os.path.join(GOLD, "py_surfel_calls.json")))["cases"][case["name"]]
    got, _, _ = scr.replay_case(case, "cuda")
    assert json.loads(json.dumps(scr.comparable(got))) == scr.comparable(want)
    assert got["returns"] == want["returns"]

    _, pkg, raw = scr.replay_case(case, "cuda", Settings=GaussianRasterizationSettings, Rasterizer=GaussianRasterizer)
    for k, v in want["returns"].items():
        if v is None:
            assert pkg[k] is None, k                         # len(allmap) == 7: no median weight / id channels
            continue
        assert list(pkg[k].shape) == v["shape"] and str(pkg[k].dtype) == v["dtype"], k
        assert bool(torch.isfinite(pkg[k].float()).all()), k
    assert int(pkg["visibility_filter"].sum()) > 16
    assert float(pkg["rendered_final_opacity"].max()) > 0.1
    if case.get("no_grad"):
        assert not pkg["render"].requires_grad
        return
    g = torch.Generator().manual_seed(4)
    loss = sum((pkg[k] * torch.randn(pkg[k].shape, generator=g).to(pkg[k].device)).sum()
               for k in ("render", "rendered_normal", "rendered_depth", "rendered_median_depth", "rendered_final_opacity"))
    loss.backward()
    vp = pkg["viewspace_points"].grad                  # retained on the non-leaf carrier: the densification statistic
    assert vp is not None and torch.isfinite(vp).all() and float(vp[:, :2].abs().max()) > 0 and float(vp[:, 2].abs().max()) == 0
    for k in ("xyz", "opacity", "scale", "rot", "f_dc"):
        assert raw[k].grad is not None and torch.isfinite(raw[k].grad).all() and float(raw[k].grad.abs().max()) > 0, k
