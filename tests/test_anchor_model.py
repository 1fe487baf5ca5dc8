"""tests/anchor_model.py -- the float32 definition of AnchorControl -- against the float64 restatement of
the published anchor adjustment (tests/anchor_reference.py) on clouds whose decisions keep a margin; hand cases of every decision;
the Python boundary of gaustudio_amd.anchor_control; the host-side planning code under the host sanitizers.  No GPU."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import anchor_cases as ac  # noqa: E402
import anchor_model as am  # noqa: E402
import anchor_reference as aref  # noqa: E402
from gaustudio_amd import AnchorControl, AnchorReport, anchor_control  # noqa: E402

F32 = np.float32
CLOUDS = [(1500, 10, 21, 1.0), (900, 16, 22, 0.6), (2500, 1, 23, 0.5), (1200, 4, 24, 2.0)]


def run_both(params, stats, k, rand, moments, cfg=ac.CFG):
    model = am.adjust(params, moments, stats, k, rand=rand, **cfg)
    ref = aref.adjust_anchor({n: ac.t64(v) for n, v in params.items()}, {n: ac.t64(m[0]) for n, m in moments.items()},
                             {n: ac.t64(m[1]) for n, m in moments.items()}, {n: ac.t64(v) for n, v in stats.items()}, k,
                             rand=torch.tensor(rand), **cfg)
    return model, ref


@pytest.mark.parametrize("n,k,seed,extent", CLOUDS)
def test_model_matches_the_published_sequence(n, k, seed, extent):
    params, stats = ac.make_cloud(n, k, seed, extent)
    assert ac.margin(params, stats) >= ac.MARGIN                  # a condition on the inputs, measured on float64 alone
    rand, moments = ac.make_rand(n, k, seed), ac.make_moments(params, seed)
    (new_p, new_m, new_s, rep, levels), ref = run_both(params, stats, k, rand, moments)
    # which cells are added at which level in which order, the integer cells, the maximum features
    assert rep.n_grown == ref.n_grown and rep.n_grown[0] > 0 and sum(rep.n_grown[1:]) > 0
    assert len(levels) == len(ref.cells)
    for (cur, cells, feats), rcells, rfeats in zip(levels, ref.cells, ref.feats):
        assert np.array_equal(cells, rcells.numpy())
        assert np.array_equal(feats.astype(np.float64), rfeats.numpy())
    # the pruned set, the order of the rows (copied values identify their row), the surviving moments, the statistics
    assert rep.n_pruned == int(ref.prune_mask.sum()) > 0 and rep.n_after == ref.params["anchor"].shape[0]
    assert rep.n_after == rep.n_before - rep.n_pruned + sum(rep.n_grown)
    for name in ("anchor_feat", "offset", "rot_raw"):
        assert np.array_equal(new_p[name].astype(np.float64), ref.params[name].numpy()), name
    n_old = rep.n_before - rep.n_pruned
    for name in ("anchor", "scale_raw"):
        assert np.array_equal(new_p[name][:n_old].astype(np.float64), ref.params[name].numpy()[:n_old]), name
        # the new rows: float32(cell) * float32(cur) and float32(log(cur)) against their float64 forms, one or two roundings
        np.testing.assert_allclose(new_p[name][n_old:], ref.params[name].numpy()[n_old:], rtol=3 * 2.0 ** -24, atol=0)
    for name in am.NAMES:
        assert np.array_equal(new_m[name][0].astype(np.float64), ref.exp_avg[name].numpy()), name
        assert np.array_equal(new_m[name][1].astype(np.float64), ref.exp_avg_sq[name].numpy()), name
        assert not new_m[name][0][n_old:].any() and not new_m[name][1][n_old:].any()
    for name in am.STATS:
        assert np.array_equal(new_s[name].astype(np.float64), ref.stats[name].numpy()), name


def test_every_margin_holds_on_the_reference_alone():
    """The construction leaves no case out: every cloud of this file and of the GPU tests meets the margins as drawn."""
    for n, k, seed, extent in CLOUDS:
        assert ac.margin(*ac.make_cloud(n, k, seed, extent)) >= ac.MARGIN


# ------------------------------------------------------------------------------------------------------------ hand cases
def tiny(anchor, offsets, k=1, scale=0.0, feat=None):
    anchor = np.asarray(anchor, F32).reshape(-1, 3)
    n = anchor.shape[0]
    params = dict(anchor=anchor, anchor_feat=np.zeros((n, 32), F32) if feat is None else np.asarray(feat, F32),
                  offset=np.asarray(offsets, F32).reshape(n, k, 3), scale_raw=np.full((n, 6), scale, F32),
                  rot_raw=np.tile(np.array([1, 0, 0, 0], F32), (n, 1)))
    return params


def hot_stats(n, k, hot=None, denom=100, avg=1.0):
    st = am.zero_stats(n, k)
    hot = np.ones(n * k, bool) if hot is None else np.asarray(hot, bool)
    st["offset_denom"][hot] = denom
    st["offset_grad_accum"][hot] = F32(avg * denom)
    return st


ONES = lambda n, k, depth=3: np.full((depth, n * k), 0.999, F32)
# voxel_size 1 / 16 with the default factors 16, 4, 1: the level sizes are 1, 0.25 and 0.0625, all exact
UNIT = dict(voxel_size=1.0 / 16)


def exact_offset(target, scale=0.0):
    """The offset o with float32(o * gs_exp(scale)) == target: gs_exp(0) is 1 + 2^-23, not 1, so a tie needs a search."""
    s = am.gs_exp(np.array([scale], F32))[0]
    o = F32(F32(target) / s)
    for step in range(9):
        for cand in (o,) if step == 0 else (lo, hi):
            if F32(cand * s) == F32(target):
                return float(cand)
        lo = np.nextafter(o if step == 0 else lo, F32(-np.inf))
        hi = np.nextafter(o if step == 0 else hi, F32(np.inf))
    raise AssertionError(f"no float32 offset gives {target}")


def test_half_to_even_ties_and_negative_cells():
    xs = [0.5, -0.5, 1.5, 2.5, -1.5, -2.5, -7.25]
    y = exact_offset(50.0)                                # away from the anchors' own cell (0, 0, 0)
    params = tiny(np.zeros((len(xs), 3)), [[exact_offset(x), y, 0.0] for x in xs])
    assert am.slot_positions(params)[:, 0].tolist() == xs and (am.slot_positions(params)[:, 1] == 50.0).all()
    _, _, _, rep, levels = am.adjust(params, {}, hot_stats(len(xs), 1), 1, rand=ONES(len(xs), 1), update_depth=1, **UNIT)
    cells = levels[0][1]
    assert cells[:, 0].tolist() == [-7, -2, 0, 2] and rep.n_grown == (4,)     # 0.5, -0.5 -> 0; 1.5, 2.5 -> 2; -1.5, -2.5 -> -2
    assert (cells[:, 1:] == np.array([50, 0])).all()


def test_level_one_candidate_blocked_by_an_anchor_level_zero_added():
    # Anchor 0 (x = 50) has a slot at x = 0.1: level 0 adds cell 0, an anchor at the origin.  Anchor 1 (x = 60) has a slot at
    # x = 0.05 that the draw keeps out of level 0.  At level 1 (size 0.25) both slots fall into cell 0, which only the anchor that
    # level 0 added occupies: nothing is added.
    params = tiny([[50, 0, 0], [60, 0, 0]], [[-49.9, 0, 0], [-59.95, 0, 0]])
    rand = ONES(2, 1)
    rand[0, 1] = 0.1
    _, _, _, rep, levels = am.adjust(params, {}, hot_stats(2, 1), 1, rand=rand, update_depth=2, **UNIT)
    assert rep.n_grown == (1, 0) and levels[0][1].tolist() == [[0, 0, 0]]
    # the contrast: level 0 adds cell 3 instead (cell 12 at level 1), and cell 0 of level 1 is free for anchor 1's slot
    params["offset"][0] = [-46.9, 0, 0]
    _, _, _, rep, levels = am.adjust(params, {}, hot_stats(2, 1), 1, rand=rand, update_depth=2, **UNIT)
    assert rep.n_grown == (1, 1) and levels[0][1].tolist() == [[3, 0, 0]] and levels[1][1].tolist() == [[0, 0, 0]]


def test_skip_quirk_level_zero_adds_nothing():
    """Level 0 finds every candidate cell occupied, so levels 1 and 2 do not run although their slots are hot: the published
    behaviour, kept."""
    params = tiny([[0, 0, 0]], [[0.3, 0, 0]])            # cell 0 at size 1 (occupied), cell 1 at 0.25, cell 5 at 0.0625
    _, _, _, rep, levels = am.adjust(params, {}, hot_stats(1, 1), 1, rand=ONES(1, 1), **UNIT)
    assert rep.n_grown == (0, 0, 0) and levels == [] and rep.n_after == 1
    params = tiny([[0, 0, 0], [9, 9, 9]], [[0.3, 0, 0], [-7.3, 0, 0]])    # one more slot that level 0 does add: now they run
    _, _, _, rep, _ = am.adjust(params, {}, hot_stats(2, 1), 1, rand=ONES(2, 1), **UNIT)
    assert rep.n_grown[0] == 1 and rep.n_grown[1] >= 1


def test_zero_denominator_and_nan_average_are_no_candidates():
    params = tiny([[0, 0, 0]] * 3, [[5.2, 0, 0], [6.2, 0, 0], [7.2, 0, 0]])
    st = hot_stats(3, 1)
    st["offset_denom"][0] = 0                            # avg = 0 by definition, whatever the accumulator holds
    st["offset_grad_accum"][1] = np.nan
    new_p, _, new_s, rep, levels = am.adjust(params, {}, st, 1, rand=ONES(3, 1), update_depth=1, **UNIT)
    assert rep.n_grown == (1,) and levels[0][1].tolist() == [[7, 0, 0]]
    assert np.isnan(new_s["offset_grad_accum"][1]) is np.False_     # mature: reset to 0 with its denominator
    assert new_s["offset_denom"].tolist() == [0, 0, 0, 0] and new_s["offset_grad_accum"][0] == st["offset_grad_accum"][0]


def test_anchor_out_of_range_is_ignored_and_candidate_out_of_range_raises():
    far = float(2 ** 21)                                 # cell 2^21 at size 1: fits no field
    params = tiny([[far, 0, 0], [0, 0, 0]], [[1.0, 0, 0], [3.2, 0, 0]])
    st = hot_stats(2, 1, hot=[False, True])
    _, _, _, rep, levels = am.adjust(params, {}, st, 1, rand=ONES(2, 1), update_depth=1, **UNIT)
    assert rep.n_grown == (1,) and levels[0][1].tolist() == [[3, 0, 0]]
    st = hot_stats(2, 1)
    before = {k: v.copy() for k, v in {**params, **st}.items()}
    with pytest.raises(ValueError):
        am.adjust(params, {}, st, 1, rand=ONES(2, 1), update_depth=1, **UNIT)
    for k, v in {**params, **st}.items():
        assert np.array_equal(v, before[k], equal_nan=True)
    params = tiny([[0, 0, 0]], [[np.inf, 0, 0]])
    with pytest.raises(ValueError):
        am.adjust(params, {}, hot_stats(1, 1), 1, rand=ONES(1, 1), update_depth=1, **UNIT)


def test_cells_at_the_ends_of_the_range_fit():
    top = float(2 ** 20 - 1)
    params = tiny([[0, 0, 0], [0, 0, 0]], [[top, -top, top], [-top, top, -float(2 ** 20)]])
    _, _, _, rep, levels = am.adjust(params, {}, hot_stats(2, 1), 1, rand=ONES(2, 1), update_depth=1, **UNIT)
    assert levels[0][1].tolist() == [[-2 ** 20 + 1, 2 ** 20 - 1, -2 ** 20], [2 ** 20 - 1, -2 ** 20 + 1, 2 ** 20 - 1]]


def test_prune_rule_min_opacity_zero_and_everything_pruned():
    params = tiny([[i, 0, 0] for i in range(4)], [[0, 0, 0]] * 4)
    st = am.zero_stats(4, 1)
    st["anchor_denom"][:] = [81, 81, 80, 81]
    st["opacity_accum"][:] = [0.4, 0.41, 0.0, 0.0]       # 0.005f * 81 = 0.405: prune, keep, not settled, prune
    moments = ac.make_moments(params, 1)
    new_p, new_m, new_s, rep, _ = am.adjust(params, moments, st, 1, rand=ONES(4, 1), **UNIT)
    assert rep == am.Report((0, 0, 0), 2, 4, 2) and new_p["anchor"][:, 0].tolist() == [1.0, 2.0]
    assert np.array_equal(new_m["offset"][0], moments["offset"][0][1:3])
    assert new_s["anchor_denom"].tolist() == [0, 80] and new_s["opacity_accum"].tolist() == [0.0, 0.0]
    _, _, _, rep, _ = am.adjust(params, moments, st, 1, rand=ONES(4, 1), min_opacity=0, **UNIT)
    assert rep.n_pruned == 0                              # nothing is below 0
    st["opacity_accum"][:] = -1.0
    st["anchor_denom"][:] = 200
    new_p, new_m, new_s, rep, _ = am.adjust(params, moments, st, 1, rand=ONES(4, 1), **UNIT)
    assert rep == am.Report((0, 0, 0), 4, 4, 0)
    assert all(new_p[n].shape == (0,) + params[n].shape[1:] for n in am.NAMES) and new_s["offset_denom"].shape == (0,)


def test_maximum_feature_over_a_cell_and_new_rows():
    feat = np.zeros((3, 32), F32)
    feat[0, :], feat[1, :], feat[2, :] = -1.0, np.arange(32) - 16.0, -0.0
    params = tiny([[0, 0, 0]] * 3, [[4.1, 0, 0], [4.2, 0, 0], [3.9, 0, 0]], feat=feat)
    new_p, _, _, rep, _ = am.adjust(params, {}, hot_stats(3, 1), 1, rand=ONES(3, 1), update_depth=1, voxel_size=0.125)
    assert rep.n_grown == (1,)                            # size 2: all three slots in cell 2
    want = np.maximum(np.arange(32) - 16.0, 0.0).astype(F32)
    assert np.array_equal(new_p["anchor_feat"][3], want) and not np.signbit(new_p["anchor_feat"][3][16])
    assert new_p["anchor"][3].tolist() == [4.0, 0.0, 0.0] and new_p["rot_raw"][3].tolist() == [1, 0, 0, 0]
    assert (new_p["scale_raw"][3] == F32(math.log(2.0))).all() and not new_p["offset"][3].any()


def test_accumulate_model():
    st = am.zero_stats(3, 2)
    aidx, oidx = np.array([0, 0, 2]), np.array([0, 1, 1])
    op = np.array([[0.25], [0.5], [0.125]], F32)
    vg = np.array([[3, 4, 9], [0, 0, 9], [1, 0, 9]], F32)
    am.accumulate(st, 2, aidx, oidx, op, vg, np.array([2, 0, 1]), np.array([True, True, False]))
    assert st["offset_grad_accum"].tolist() == [5, 0, 0, 0, 0, 1] and st["offset_denom"].tolist() == [1, 0, 0, 0, 0, 1]
    assert st["opacity_accum"].tolist() == [0.75, 0, 0.125] and st["anchor_denom"].tolist() == [1, 1, 0]


# ------------------------------------------------------------------------------------------------------------ the Python boundary
def cpu_params(n=4, k=2):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).requires_grad_(True)
    return dict(anchor=r(n, 3), anchor_feat=r(n, 32), offset=r(n, k, 3), scale_raw=r(n, 6), rot_raw=r(n, 4))


def test_argument_checks_run_in_order_and_end_at_the_device():
    p = cpu_params()
    with pytest.raises(TypeError):
        AnchorControl([1], 0.01)
    with pytest.raises(TypeError):
        AnchorControl(p, "0.01")
    with pytest.raises(TypeError):
        AnchorControl(p, 0.01, optimizer=torch.optim.SGD(list(p.values()), lr=0.1))
    with pytest.raises(TypeError):
        AnchorControl(p, 0.01, update_depth=2.0)
    with pytest.raises(KeyError):
        AnchorControl({k: v for k, v in p.items() if k != "offset"}, 0.01)
    with pytest.raises(KeyError):
        AnchorControl({**p, "opacity": p["anchor"]}, 0.01)
    with pytest.raises(TypeError):                         # a type error comes before the shape error of another entry
        AnchorControl({**p, "anchor": torch.zeros(4, 2), "rot_raw": None}, 0.01)
    with pytest.raises(ValueError):                        # a shape before a dtype
        AnchorControl({**p, "anchor": torch.zeros(4, 2), "rot_raw": torch.zeros(4, 4, dtype=torch.float64)}, 0.01)
    with pytest.raises(ValueError):
        AnchorControl({**p, "offset": torch.zeros(4, 17, 3)}, 0.01)
    with pytest.raises(TypeError):                         # a dtype before contiguity
        AnchorControl({**p, "rot_raw": torch.zeros(4, 4, dtype=torch.float64), "anchor_feat": torch.zeros(32, 4).t()}, 0.01)
    with pytest.raises(ValueError, match="contiguous"):
        AnchorControl({**p, "anchor_feat": torch.zeros(32, 4).t()}, 0.01)
    with pytest.raises(ValueError, match="leaf"):
        AnchorControl({**p, "anchor": p["anchor"] * 1.0}, 0.01)
    for bad in (dict(voxel_size=0.0), dict(voxel_size=0.01, update_depth=0), dict(voxel_size=0.01, update_depth=9),
                dict(voxel_size=0.01, update_init_factor=4, update_hierarchy_factor=4, update_depth=3)):
        with pytest.raises(ValueError):
            AnchorControl(p, **bad)
    with pytest.raises(RuntimeError, match="ROCm"):        # everything passed: the CPU tensors are the last thing refused
        AnchorControl(p, 0.01)


def test_the_limits_are_checked_on_shapes_alone():
    anchor_control.check_limits(2 ** 24, 16)
    with pytest.raises(ValueError):
        anchor_control.check_limits(2 ** 24 + 1, 1)
    with pytest.raises(ValueError):
        anchor_control.check_limits(2 ** 27, 16)


def test_optimizer_wiring_is_checked_before_the_device():
    p = cpu_params()
    mlp = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="no param group"):
        AnchorControl(p, 0.01, optimizer=torch.optim.Adam([p["anchor"], *mlp.parameters()], lr=1e-3))
    with pytest.raises(ValueError, match="amsgrad"):
        AnchorControl(p, 0.01, optimizer=torch.optim.Adam(list(p.values()), lr=1e-3, amsgrad=True))
    opt = torch.optim.Adam([dict(params=[p[n]], lr=1e-3, name=n) for n in am.NAMES] + [dict(params=list(mlp.parameters()), lr=1e-2)])
    where = anchor_control.check_optimizer(opt, p)
    assert {n: g["name"] for n, (g, _) in where.items()} == {n: n for n in am.NAMES}
    with pytest.raises(RuntimeError, match="ROCm"):
        AnchorControl(p, 0.01, optimizer=opt)


def test_level_plan_matches_the_model():
    got = anchor_control.level_plan(0.01, 2e-4, 3, 16, 4)
    want = am.level_plan(0.01, 2e-4, 3, 16, 4)
    assert [tuple(float(v) for v in lv) for lv in want] == [tuple(lv) for lv in got]
    assert AnchorReport._fields == ("n_grown", "n_pruned", "n_before", "n_after")


# ------------------------------------------------------------------------------------------------------------ host planning code
def test_planning_code_under_the_host_sanitizers(tmp_path):
    """csrc/gsr_anchor_plan.h -- the size limits and the sort key of a level (rebased cells, packed x-major, as many bits as the
    occupied range needs) -- in a stand-alone program built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's torch adapter: it has to be here"
    exe = str(tmp_path / "anchor_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gaustudio_amd", "csrc"), os.path.join(HERE, "anchor_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out.stdout.splitlines()}
    assert got["sizes"] == [1, 1, 0, 0, 0, 1, 0]
    assert got["full"] == [63, 42, 21, 0]                  # the whole 21-bit range: the key of the contract
    assert got["small"] == [3 + 1 + 7, 8, 7, 0]
    assert got["order"] == [1] and got["roundtrip"] == [1]
