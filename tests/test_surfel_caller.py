"""CPU: the restatement of GauStudio's SurfelRenderer (tests/golden/surfel_call_record.py) is pinned to the unmodified class.
tests/golden/py_surfel_calls.json records what `diff_surfel_rasterization` receives when the reference's SurfelRenderer runs
(tests/golden/make_surfel_call_fixture.py); replayed here with the same recording stand-in, the restatement must give the
identical record -- settings field by field, keyword set, None-ness, shapes, dtypes, contiguity, requires_grad / leaf /
retained grad, grad mode -- and a package with the recorded keys, dtypes and shapes."""
import json
import os
import sys

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import surfel_call_record as scr  # noqa: E402


def _fixture():
    return json.load(open(os.path.join(GOLD, "py_surfel_calls.json")))["cases"]


def test_fixture_covers_every_case():
    assert sorted(_fixture()) == sorted(c["name"] for c in scr.CASES)


@pytest.mark.parametrize("case", scr.CASES, ids=lambda c: c["name"])
def test_replay_equals_the_recorded_surfel_renderer_call(case):
    want = _fixture()[case["name"]]
    got, pkg, _ = scr.replay_case(case, "cpu")
    assert json.loads(json.dumps(scr.comparable(got))) == scr.comparable(want)
    assert got["returns"] == want["returns"]
    assert want["torch_factory_calls_with_device_cuda"][-1] == ["zeros_like", "cuda"]   # the screen-space carrier
    # what the operator must accept: a non-leaf means2D that retains its grad (training), [P,1] opacities, [P,2] scales, and
    # sh_degree 1 whenever the colours come precomputed
    args = want["arguments"]
    assert args["opacities"]["shape"] == [64, 1] and args["scales"]["shape"] == [64, 2] and args["cov3D_precomp"] is None
    if case["grad"]:
        assert args["means2D"]["is_leaf"] is False and args["means2D"]["retains_grad"] is True
    if args["shs"] is None:
        assert want["settings"]["sh_degree"]["value"] == 1
