"""tests/optim_model.py -- the float32 definition of GaussianAdam and DensityControl -- against
torch.optim.Adam and against the float64 restatement of the published densification (tests/optim_reference.py); hand cases of
every decision; the Python boundary of gaustudio_amd.optim; the host-side planning code under the host sanitizers.  No GPU."""
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
import optim_cases as oc  # noqa: E402
import optim_model as om  # noqa: E402
import optim_model_parity as parity  # noqa: E402
import optim_reference as oref  # noqa: E402
from gaustudio_amd import optim  # noqa: E402

F32 = np.float32
ULP = 2.0 ** -23


def run_model(params, stats, noise, n_split, mss, moments_seed=7):
    adam = om.AdamModel(params, oc.LR)
    rng = np.random.default_rng(moments_seed)
    for k in om.GROUPS:                       # moments that identify their row
        adam.exp_avg[k] = rng.standard_normal(params[k].shape).astype(F32)
        adam.exp_avg_sq[k] = rng.random(params[k].shape).astype(F32)
    before = {k: (adam.exp_avg[k].copy(), adam.exp_avg_sq[k].copy()) for k in om.GROUPS}
    rep, new_stats = om.densify_and_prune(adam, stats, oc.CFG["max_grad"], oc.CFG["min_opacity"], oc.CFG["extent"], mss, n_split,
                                          noise, oc.CFG["percent_dense"])
    return adam, rep, new_stats, before


def run_reference(params, stats, noise, n_split, mss, before):
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    return oref.densify_and_prune({k: t64(v) for k, v in params.items()}, {k: t64(before[k][0]) for k in om.GROUPS},
                                  {k: t64(before[k][1]) for k in om.GROUPS}, t64(stats["grad_accum"]), t64(stats["denom"]),
                                  torch.tensor(stats["max_radii"]), oc.CFG["max_grad"], oc.CFG["min_opacity"], oc.CFG["extent"],
                                  mss, n_split, torch.tensor(noise), oc.CFG["percent_dense"])


CLOUDS = [(3000, 3, 11, 2, 20), (2500, 0, 12, 1, None), (2000, 15, 13, 3, 20), (3000, 8, 14, 2, None)]


@pytest.mark.parametrize("n,k,seed,n_split,mss", CLOUDS)
def test_classification_matches_the_published_sequence(n, k, seed, n_split, mss):
    params, stats = oc.make_cloud(n, k, seed, n_split, mss)
    assert oc.margin(params, stats, n_split, mss) >= 1e-3          # a condition on the inputs, not a tolerance
    noise = oc.make_noise(n, n_split, seed)
    adam, rep, _, before = run_model(params, stats, noise, n_split, mss)
    st = run_reference(params, stats, noise, n_split, mss, before)
    assert st.n == rep.n_after == adam.params["xyz"].shape[0]
    assert rep.n_cloned > 0 and rep.n_pruned > 0 and (rep.n_split > 0)
    # rows are identified by what is copied: f_dc and the rotation of the source, in order
    for name in ("f_dc", "rotation", "opacity", "f_rest"):
        assert np.array_equal(adam.params[name].astype(np.float64), st.p[name].numpy()), name
    # the moments: carried by the survivors, zero for every clone and child
    for name in om.GROUPS:
        assert np.array_equal(adam.exp_avg[name].astype(np.float64), st.m[name].numpy()), name
        assert np.array_equal(adam.exp_avg_sq[name].astype(np.float64), st.v[name].numpy()), name
    n_children = n_split * rep.n_split
    assert rep.n_after == rep.n_before - rep.n_pruned - rep.n_split + rep.n_cloned + n_children


@pytest.mark.parametrize("n,k,seed,n_split,mss", CLOUDS)
def test_values_match_the_published_sequence(n, k, seed, n_split, mss):
    """Bounds from the operation count, u = 2^-23.  A child's position: q / |q| costs 4 roundings for |q|^2, one for the
    root and one for the division, < 3 u per component; an entry of R is 3 to 4 more operations on products of two components,
    < 10 u absolute; gs_exp is within 2 u of exp and the product with the noise adds half; so each of the three terms
    R s noise is within 13 u of |s noise| (|R| <= 1), and the two additions and the addition to xyz round once each on a
    magnitude of at most |xyz| + sum |s noise|: 16 u (|xyz| + sum_j |s_j noise_j|) covers it.  A child's scaling:
    scaling - f32(log(0.8 n)) against log(exp(scaling) / (0.8 n)) in float64: one rounding of the constant, one of the
    difference, and the float64 detour's own error: 2 u (|scaling| + |d_split|).  Everything else is copied: exact."""
    params, stats = oc.make_cloud(n, k, seed, n_split, mss)
    noise = oc.make_noise(n, n_split, seed)
    adam, rep, _, before = run_model(params, stats, noise, n_split, mss)
    st = run_reference(params, stats, noise, n_split, mss, before)
    n_keep = rep.n_after - n_split * rep.n_split
    xyz, ref_xyz = adam.params["xyz"].astype(np.float64), st.p["xyz"].numpy()
    sc, ref_sc = adam.params["scaling"].astype(np.float64), st.p["scaling"].numpy()
    assert np.array_equal(xyz[:n_keep], ref_xyz[:n_keep]) and np.array_equal(sc[:n_keep], ref_sc[:n_keep])
    if rep.n_split:
        # the children's own terms, from the reference's rows: parent scaling = child scaling + log(0.8 n)
        parent_s = np.exp(ref_sc[n_keep:] + math.log(0.8 * n_split))
        fa, fb, fc, _, _ = om.classify(params["scaling"], params["opacity"], stats, oc.CFG["max_grad"],
                                       om.thresholds(oc.CFG["percent_dense"], oc.CFG["extent"], oc.CFG["min_opacity"], n_split), mss)
        zn = np.concatenate([noise[fc, c] for c in range(n_split)], axis=0).astype(np.float64)
        parent_xyz = np.concatenate([params["xyz"][fc]] * n_split, axis=0).astype(np.float64)
        bound = 16 * ULP * (np.abs(parent_xyz) + np.abs(parent_s * zn).sum(axis=1, keepdims=True))
        err = np.abs(xyz[n_keep:] - ref_xyz[n_keep:])
        assert (err <= bound).all(), f"child xyz: worst error / bound = {(err / bound).max():.3f}"
        bound_s = 2 * ULP * (np.abs(ref_sc[n_keep:]) + abs(math.log(0.8 * n_split)) + np.abs(ref_sc[n_keep:] + math.log(0.8 * n_split)))
        err_s = np.abs(sc[n_keep:] - ref_sc[n_keep:])
        assert (err_s <= bound_s).all(), f"child scaling: worst error / bound = {(err_s / bound_s).max():.3f}"


def test_adam_is_as_close_to_float64_as_torch_float32():
    """The same margin test_loss_model.py uses for a float32 restatement against torch's own float32: twice its error."""
    r = parity.measure()
    print(r)
    assert r["torch_float32_max_abs_error_vs_float64"] > 0
    assert r["model_max_abs_error_vs_float64"] <= 2 * r["torch_float32_max_abs_error_vs_float64"], r


def test_adam_first_step_moves_by_lr():
    c = om.adam_consts(1e-2, 0.9, 0.999, 1)
    p, m, v = om.adam_update(F32([1.0, -2.0]), F32([0.5, -3.0]), F32([0, 0]), F32([0, 0]), c, 1e-15)
    assert np.allclose(p, [1.0 - 1e-2, -2.0 + 1e-2], rtol=1e-6)
    assert np.allclose(m, [0.05, -0.3], rtol=1e-6) and np.allclose(v, [0.00025, 0.009], rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------ hand cases
def hand_model(scaling_max, opacity, k=0):
    """Rows with the given largest log-scale and opacity logit; everything else identifies the row."""
    n = len(scaling_max)
    p = oc.make_params(n, k, seed=5)
    p["scaling"] = np.stack([np.asarray(scaling_max, F32), np.asarray(scaling_max, F32) - F32(1), np.asarray(scaling_max, F32) - F32(2)], 1)
    p["opacity"] = np.asarray(opacity, F32).reshape(n, 1)
    return p


TH = om.thresholds(0.01, 4.0, 0.05, 2)          # t_big = log(0.04), t_world = log(0.4), t_op = logit(0.05), d_split = log(1.6)


def classes(params, stats, max_grad=F32(2e-4), mss=None, th=TH):
    fa, fb, fc, clone, split = om.classify(params["scaling"], params["opacity"], stats, max_grad, th, mss)
    return fa.tolist(), fb.tolist(), fc.tolist(), clone.tolist(), split.tolist()


def test_never_seen_row_and_nan_accumulator_select_nothing():
    p = hand_model([-5.0, -5.0, -5.0], [0.0, 0.0, 0.0])
    stats = dict(grad_accum=F32([1.0, np.nan, 1.0]), denom=np.int32([0, 3, 1]), max_radii=np.int32([0, 0, 0]))
    fa, fb, fc, clone, split = classes(p, stats)
    assert clone == [False, False, True] and split == [False, False, False]
    assert fa == [True, True, True] and fb == [False, False, True]


def test_average_on_the_threshold_selects():
    g = F32(2e-4)
    p = hand_model([-5.0, -5.0], [0.0, 0.0])
    stats = dict(grad_accum=F32([g * F32(2), np.nextafter(g * F32(2), F32(0))]), denom=np.int32([2, 2]), max_radii=np.int32([0, 0]))
    assert classes(p, stats, max_grad=g)[3] == [True, False]


def test_scale_on_the_threshold_clones():
    t_big = TH[0]
    p = hand_model([t_big, np.nextafter(t_big, F32(0))], [0.0, 0.0])
    stats = dict(grad_accum=F32([1.0, 1.0]), denom=np.int32([1, 1]), max_radii=np.int32([0, 0]))
    _, _, _, clone, split = classes(p, stats)
    assert clone == [True, False] and split == [False, True]


def test_clone_source_below_the_opacity_threshold_emits_nothing():
    p = hand_model([-5.0, -5.0], [float(TH[2]) - 1.0, 0.0])
    stats = dict(grad_accum=F32([1.0, 1.0]), denom=np.int32([1, 1]), max_radii=np.int32([0, 0]))
    fa, fb, fc, clone, _ = classes(p, stats)
    assert clone == [True, True] and fa == [False, True] and fb == [False, True] and fc == [False, False]
    adam = om.AdamModel(p, oc.LR)
    rep, _ = om.densify_and_prune(adam, stats, 2e-4, 0.05, 4.0, None, 2, oc.make_noise(2, 2))
    assert rep == om.Report(n_cloned=1, n_split=0, n_pruned=1, n_before=2, n_after=2)
    assert np.array_equal(adam.params["f_dc"], np.stack([p["f_dc"][1], p["f_dc"][1]]))


def test_child_that_fails_the_world_size_test():
    t_world, d = TH[1], TH[3]
    # row 0: the child's scale smax - d_split is still beyond t_world; row 1: the source is beyond it, its children are not
    p = hand_model([t_world + d + F32(0.1), t_world + F32(0.1)], [0.0, 0.0])
    stats = dict(grad_accum=F32([1.0, 1.0]), denom=np.int32([1, 1]), max_radii=np.int32([0, 0]))
    fa, fb, fc, _, split = classes(p, stats, mss=20)
    assert split == [True, True] and fc == [False, True] and fa == [False, False]
    assert classes(p, stats, mss=None)[2] == [True, True]          # without max_screen_size there is no world-size test


def test_screen_size_test_reads_the_saved_radii_and_spares_children():
    p = hand_model([-5.0, -5.0, -2.0], [0.0, 0.0, 0.0])
    stats = dict(grad_accum=F32([1.0, 0.0, 1.0]), denom=np.int32([1, 1, 1]), max_radii=np.int32([21, 20, 50]))
    fa, fb, fc, _, _ = classes(p, stats, mss=20)
    assert fa == [False, True, False] and fb == [False, False, False] and fc == [False, False, True]


@pytest.mark.parametrize("n_split", [1, 3])
def test_split_counts_and_order(n_split):
    params, stats = oc.make_cloud(300, 3, 21, n_split, None)
    noise = oc.make_noise(300, n_split)
    adam = om.AdamModel(params, oc.LR)
    rep, new_stats = om.densify_and_prune(adam, stats, noise=noise, n_split=n_split, max_screen_size=None, **oc.CFG)
    fa, fb, fc, _, _ = om.classify(params["scaling"], params["opacity"], stats, oc.CFG["max_grad"],
                                   om.thresholds(0.01, 4.0, 0.05, n_split), None)
    assert rep.n_after == fa.sum() + fb.sum() + n_split * fc.sum() and rep.n_split == fc.sum() > 0
    want = np.concatenate([params["f_dc"][fa], params["f_dc"][fb]] + [params["f_dc"][fc]] * n_split)
    assert np.array_equal(adam.params["f_dc"], want)
    d = om.thresholds(0.01, 4.0, 0.05, n_split)[3]
    assert np.array_equal(adam.params["scaling"][rep.n_after - fc.sum():], (params["scaling"][fc] - d).astype(F32))
    assert all(not v.any() and v.shape == (rep.n_after,) for v in new_stats.values())


def test_sparse_step_leaves_unseen_rows_and_matches_the_dense_step_elsewhere():
    params = oc.make_params(257, 3, seed=3)
    grads = oc.make_grads(params)
    vis = (np.arange(257) % 3 - 1).astype(np.int32)                 # -1, 0, 1, ...
    dense, sparse = om.AdamModel(params, oc.LR), om.AdamModel(params, oc.LR)
    for _ in range(3):
        dense.step(grads)
        sparse.step(grads, visible=vis)
    assert sparse.step_count == 3
    seen = vis > 0
    for k in om.GROUPS:
        for a, b, start in ((sparse.params, dense.params, params[k]), (sparse.exp_avg, dense.exp_avg, np.zeros_like(params[k])),
                            (sparse.exp_avg_sq, dense.exp_avg_sq, np.zeros_like(params[k]))):
            assert om.same_bits(a[k][~seen], start[~seen]) and om.same_bits(a[k][seen], b[k][seen])
    one = om.AdamModel(params, oc.LR)
    one.step({k: (None if k == "rotation" else g) for k, g in grads.items()})
    assert om.same_bits(one.params["rotation"], params["rotation"]) and not om.same_bits(one.params["xyz"], params["xyz"])


def test_accumulate_and_prune_carry_statistics():
    stats = om.new_stats(4)
    mg = F32([[3, 4, 9], [1, 0, 9], [0, 0, 9], [6, 8, 9]])
    om.accumulate(stats, mg, np.int32([5, 0, -1, 2]))
    om.accumulate(stats, mg, np.int32([3, 0, 0, 7]))
    assert stats["grad_accum"].tolist() == [10.0, 0.0, 0.0, 20.0] and stats["denom"].tolist() == [2, 0, 0, 2]
    assert stats["max_radii"].tolist() == [5, 0, 0, 7]
    adam = om.AdamModel(oc.make_params(4, 0), oc.LR)
    rep, kept = om.prune(adam, stats, np.array([True, False, False, False]))
    assert rep.n_after == 3 and kept["grad_accum"].tolist() == [0.0, 0.0, 20.0] and kept["max_radii"].tolist() == [0, 0, 7]


# ------------------------------------------------------------------------------------------------------------ Python boundary
def cpu_params(n=4, k=3):
    return {name: torch.zeros((n,) + oc.tail(name, k), requires_grad=True) for name in om.GROUPS}


def test_boundary_params():
    p = cpu_params()
    p["scaling"] = p["scaling"].detach().double().requires_grad_(True)
    with pytest.raises(TypeError, match="float32"):
        optim.GaussianAdam(p, oc.LR)
    p = cpu_params()
    del p["opacity"]
    with pytest.raises(KeyError, match="opacity"):
        optim.GaussianAdam(p, oc.LR)
    p = cpu_params()
    p["rotation"] = torch.zeros(5, 4, requires_grad=True)
    with pytest.raises(ValueError, match="rotation"):
        optim.GaussianAdam(p, oc.LR)
    p = cpu_params(k=3)
    p["f_rest"] = torch.zeros(4, 4, 3, requires_grad=True)
    with pytest.raises(ValueError, match="K in"):
        optim.GaussianAdam(p, oc.LR)
    with pytest.raises(TypeError):
        optim.GaussianAdam([1, 2], oc.LR)
    with pytest.raises(RuntimeError, match="ROCm"):                  # everything before the devices passed
        optim.GaussianAdam(cpu_params(), oc.LR)
    with pytest.raises(RuntimeError, match="ROCm"):
        optim.GaussianAdam(cpu_params(k=0), oc.LR)


def test_boundary_row_limit_without_an_allocation():
    n = 2 ** 31 // 45 + 1
    p = {name: torch.empty((n,) + oc.tail(name, 15), device="meta", requires_grad=True) for name in om.GROUPS}
    with pytest.raises(ValueError, match="2\\^31"):
        optim.GaussianAdam(p, oc.LR)
    optim.check_rows(n - 1)
    with pytest.raises(ValueError, match="2\\^31"):
        optim.check_rows(n)


def test_boundary_noise_mask_visible():
    with pytest.raises(ValueError, match="noise"):
        optim.check_noise(torch.zeros(4, 3, 3), 4, 2)
    with pytest.raises(TypeError, match="noise"):
        optim.check_noise(torch.zeros(4, 2, 3, dtype=torch.float64), 4, 2)
    optim.check_noise(torch.zeros(4, 2, 3), 4, 2)
    with pytest.raises(ValueError, match="mask"):
        optim.check_mask(torch.zeros(5, dtype=torch.bool), 4)
    with pytest.raises(TypeError, match="mask"):
        optim.check_mask(torch.zeros(4, dtype=torch.uint8), 4)
    with pytest.raises(TypeError, match="visible"):
        optim.check_visible(torch.zeros(4, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="visible"):
        optim.check_visible(torch.zeros(3, dtype=torch.int32), 4)
    with pytest.raises(TypeError):
        optim.DensityControl(object())


def test_expon_lr():
    f = optim.GaussianAdam.expon_lr(1.6e-4, 1.6e-6, delay_steps=0, delay_mult=0.01, max_steps=30000)
    assert f(0) == pytest.approx(1.6e-4) and f(30000) == pytest.approx(1.6e-6) and f(15000) == pytest.approx(1.6e-5)
    assert f(-1) == 0.0 and optim.GaussianAdam.expon_lr(0.0, 0.0)(5) == 0.0
    g = optim.GaussianAdam.expon_lr(1e-2, 1e-4, delay_steps=100, delay_mult=0.1, max_steps=1000)
    assert g(0) == pytest.approx(1e-3) and g(100) == pytest.approx(1e-2 * math.exp(math.log(1e-2) * 0.1))


# ------------------------------------------------------------------------------------------------------------ host planning code
def test_planning_code_under_the_host_sanitizers(tmp_path):
    """csrc/gsr_optim_plan.h -- threshold rounding, limit checks, sizes from the totals -- in a stand-alone program built with
    -fsanitize=address,undefined; the program compares with the values this process computes (tests/optim_model.py)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's torch adapter: it has to be here"
    exe = str(tmp_path / "optim_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gaustudio_amd", "csrc"), os.path.join(HERE, "optim_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {}
    for line in out.stdout.splitlines():
        key, *vals = line.split()
        got[key] = vals
    th = om.thresholds(0.01, 4.0, 0.05, 2)
    assert [float.fromhex(v) for v in got["thresholds"]] == [float(v) for v in th]
    assert [float.fromhex(v) for v in got["thresholds0"]][2] == -math.inf
    c = om.adam_consts(1.6e-4, 0.9, 0.999, 1000)
    assert [float.fromhex(v) for v in got["adam1000"]] == [float(v) for v in c]
    c = om.adam_consts(5e-2, 0.9, 0.999, 1)
    assert [float.fromhex(v) for v in got["adam1"]] == [float(v) for v in c]
    limit = 2 ** 31 // 45 + 1                                  # the first row count that is refused
    assert [int(v) for v in got["rows"]] == [1, 1, 0, 0]       # 0, limit - 1, limit, -1
    assert [int(v) for v in got["after"]] == [10 + 5 + 3 * 7, -1, limit - 1, -1, -1]
    assert [int(v) for v in got["units"]] == [0, 1, 1, 2, 2, 3]
