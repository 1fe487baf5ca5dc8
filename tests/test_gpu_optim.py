"""gaustudio_amd.optim on the GPU against tests/optim_model.py: every comparison is exact (the same bytes, NaN in the same
places).  Sizes: the edges of a wave (63 | 64 | 65), of a 256-lane workgroup, of the scan's 1024-row tile, a multi-tile carry."""
import math
import os
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
from gaustudio_amd import DensityControl, GaussianAdam  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = torch.device("cuda", 0)


def leaf(a, offset=0):
    """A leaf tensor with a's values whose storage starts `offset` floats into a larger buffer."""
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.tensor(a, device=DEV).requires_grad_(True)
    buf = torch.zeros(a.size + offset, dtype=torch.float32, device=DEV)
    t = buf[offset:].view(a.shape)
    t.copy_(torch.tensor(a))
    return t.requires_grad_(True)


def to_device(params, offset=0):
    return {k: leaf(v, offset) for k, v in params.items()}


def set_grads(dparams, grads, offset=0):
    for k, p in dparams.items():
        g = grads.get(k)
        p.grad = None if g is None else leaf(g, offset).detach()


def host(t):
    return t.detach().cpu().numpy()


def assert_state(opt, model, what=""):
    for k in om.GROUPS:
        assert om.same_bits(host(opt.params[k]), model.params[k]), f"{what}: {k}"
        assert om.same_bits(host(opt.exp_avg[k]), model.exp_avg[k]), f"{what}: exp_avg {k}"
        assert om.same_bits(host(opt.exp_avg_sq[k]), model.exp_avg_sq[k]), f"{what}: exp_avg_sq {k}"


def pair(params, lr=oc.LR, offset=0):
    return GaussianAdam(to_device(params, offset), lr), om.AdamModel(params, lr)


def both_step(opt, model, grads, visible=None, grad_offset=0):
    set_grads(opt.params, grads, grad_offset)
    opt.step(visible=None if visible is None else torch.tensor(visible, device=DEV))
    model.step(grads, visible=visible)


# ------------------------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("k", [0, 3, 8, 15])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1025])
def test_adam_step_1_and_1000(n, k):
    params = oc.make_params(n, k, seed=n + k)
    opt, model = pair(params)
    both_step(opt, model, oc.make_grads(params, seed=1))
    assert_state(opt, model, "step 1")
    both_step(opt, model, oc.make_grads(params, seed=2))
    assert_state(opt, model, "step 2")
    opt.step_count = model.step_count = 999
    both_step(opt, model, oc.make_grads(params, seed=3))
    assert opt.step_count == 1000
    assert_state(opt, model, "step 1000")


def test_adam_skips_a_group_without_grad_and_takes_lr_zero():
    params = oc.make_params(257, 3, seed=1)
    lr = dict(oc.LR, scaling=0.0)
    opt, model = pair(params, lr)
    grads = oc.make_grads(params)
    grads["rotation"] = None
    for _ in range(2):
        both_step(opt, model, grads)
    assert_state(opt, model)
    assert om.same_bits(host(opt.params["rotation"]), params["rotation"]) and not host(opt.exp_avg["rotation"]).any()
    assert om.same_bits(host(opt.params["scaling"]), params["scaling"]) and host(opt.exp_avg["scaling"]).any()
    opt.zero_grad()
    assert all(p.grad is None for p in opt.params.values())
    opt.step()                                   # no gradient anywhere: nothing moves, the count advances
    model.step({})
    assert_state(opt, model)
    assert opt.step_count == 3


def test_adam_special_gradients():
    n, k = 65, 3
    params = oc.make_params(n, k, seed=2)
    opt, model = pair(params)
    grads = oc.make_grads(params)
    special = F32([0.0, -0.0, 1e-42, -3e-45, np.inf, -np.inf, np.nan, 1e-30, 3e38])
    for name, g in grads.items():
        flat = g.reshape(-1)
        flat[:min(len(special), flat.size)] = special[:flat.size]
        flat[-1] = F32(1e-40)
    for i in range(3):
        both_step(opt, model, grads if i != 1 else oc.make_grads(params, seed=9))
        assert_state(opt, model, f"step {i + 1}")
    assert np.isnan(host(opt.params["xyz"])).any()


def visibility_patterns(n, k):
    rows = np.arange(n)
    pats = dict(none=np.zeros(n), all=np.ones(n), alternating=rows % 2, negative=-(rows % 2) * 7 + (rows % 3 == 0) * 3,
                upto63=rows < 64, from64=rows >= 64)
    # K = 15: row 5 holds floats 225 .. 269 of f_rest, across the 16-byte vector 224 .. 227 and the wave boundary at 256
    pats.update(upto5=rows <= 5, from5=rows >= 5, only5=rows == 5, not5=rows != 5)
    return {name: v.astype(np.int32) for name, v in pats.items()}


@pytest.mark.parametrize("n,k", [(129, 15), (257, 3), (65, 0)])
def test_adam_sparse_step(n, k):
    params = oc.make_params(n, k, seed=4)
    for name, vis in visibility_patterns(n, k).items():
        opt, model = pair(params)
        both_step(opt, model, oc.make_grads(params, seed=5))                 # moments that are not zero
        before = {g: (host(opt.params[g]), host(opt.exp_avg[g]), host(opt.exp_avg_sq[g])) for g in om.GROUPS}
        both_step(opt, model, oc.make_grads(params, seed=6), visible=vis)
        assert_state(opt, model, name)
        assert opt.step_count == 2
        unseen = vis <= 0
        for g in om.GROUPS:
            for a, b in zip(before[g], (host(opt.params[g]), host(opt.exp_avg[g]), host(opt.exp_avg_sq[g]))):
                assert om.same_bits(a[unseen], b[unseen]), f"{name}: unseen rows of {g} changed"
        both_step(opt, model, oc.make_grads(params, seed=7))                 # the dense step after it
        assert_state(opt, model, name + " then dense")


@pytest.mark.parametrize("grad_offset", [0, 1])
@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("n,k", [(1, 0), (65, 15), (257, 3)])
def test_adam_unaligned_storage(n, k, offset, grad_offset):
    """Parameters that start 1 .. 3 floats past a 16-byte boundary (the moments follow them): with a gradient at the same
    offset the 16-byte path runs with a head and a tail, with an aligned gradient the group takes the element path."""
    params = oc.make_params(n, k, seed=8)
    opt, model = pair(params, offset=offset)
    assert opt.params["xyz"].data_ptr() % 16 == 4 * offset and opt.exp_avg["xyz"].data_ptr() % 16 == 4 * offset
    goff = offset if grad_offset else 0
    vis = (np.arange(n) % 3 != 1).astype(np.int32)
    both_step(opt, model, oc.make_grads(params, seed=1), grad_offset=goff)
    both_step(opt, model, oc.make_grads(params, seed=2), visible=vis, grad_offset=goff)
    assert_state(opt, model)


def test_adam_state_dict_round_trip():
    params = oc.make_params(65, 3, seed=3)
    opt, model = pair(params)
    both_step(opt, model, oc.make_grads(params, seed=1))
    state = opt.state_dict()
    other = GaussianAdam({k: v.detach().clone().requires_grad_(True) for k, v in opt.params.items()}, dict(oc.LR, xyz=1.0))
    other.load_state_dict(state)
    assert other.step_count == 1 and other.lr == opt.lr
    both_step(other, model, oc.make_grads(params, seed=2))
    assert_state(other, model)
    with pytest.raises(TypeError):
        opt.step(visible=torch.zeros(65, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        opt.step(visible=torch.zeros(64, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="ROCm"):
        opt.step(visible=torch.zeros(65, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ accumulate
def dev_stats(dc):
    return dict(grad_accum=host(dc.grad_accum), denom=host(dc.denom), max_radii=host(dc.max_radii))


def assert_stats(dc, stats, what=""):
    got = dev_stats(dc)
    for k in stats:
        assert om.same_bits(got[k], stats[k]), f"{what}: {k}"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1025])
def test_accumulate(n):
    params = oc.make_params(n, 0, seed=n)
    dc = DensityControl(GaussianAdam(to_device(params), oc.LR))
    stats = om.new_stats(n)
    rng = np.random.default_rng(n)
    for call in range(3):
        mg = (rng.standard_normal((n, 3)) * 1e-3).astype(F32)
        mg[0, 0] = F32(1e-30)                                       # a square that underflows
        radii = rng.integers(-3, 30, n).astype(np.int32) // (call + 1)         # zero, negative, positive; shrinking
        if call == 2:
            mg[-1, 1] = np.nan
        dc.accumulate(torch.tensor(mg, device=DEV), torch.tensor(radii, device=DEV))
        om.accumulate(stats, mg, radii)
        assert_stats(dc, stats, f"call {call}")
    assert stats["max_radii"].max() > 0 or n == 1


# ------------------------------------------------------------------------------------------------------------------ densify
PATTERNS = ("nothing", "all_cloned", "all_split", "all_pruned", "last_row", "rows_1023_1024", "mix")


def pattern_cloud(n, k, pattern, n_split, mss):
    """(params, stats): the decisions of a pattern are forced through the statistics, the scales and the opacities."""
    if pattern == "mix":
        return oc.make_cloud(n, k, seed=n % 1000 + 3 * n_split, n_split=n_split, max_screen_size=mss)
    params = oc.make_params(n, k, seed=n % 1000)
    stats = dict(grad_accum=np.zeros(n, F32), denom=np.ones(n, np.int32), max_radii=np.zeros(n, np.int32))
    params["opacity"][:] = 2.0
    hot = np.zeros(n, bool)
    if pattern in ("all_cloned", "all_split", "all_pruned"):
        hot[:] = True
    elif pattern == "last_row":
        hot[-1] = True
    elif pattern == "rows_1023_1024":
        hot[[i for i in (1023, 1024) if i < n]] = True
    stats["grad_accum"][hot] = 1.0
    params["scaling"][:] = F32(-5.0) + params["scaling"] * F32(0.01)          # small: clone-class where hot
    if pattern == "all_split":
        params["scaling"][:] = F32(-2.0) + params["scaling"] * F32(0.01)
    elif pattern in ("last_row", "rows_1023_1024"):
        sel = np.nonzero(hot)[0]
        params["scaling"][sel[::2]] += F32(3.0)                                # every other selected row splits
    if pattern == "all_pruned":
        params["opacity"][:] = -10.0
    return params, stats


def run_densify(params, stats, noise, n_split, mss, generator=None, stream=None):
    opt, model = pair(params)
    for k in om.GROUPS:                                           # moments that identify their row
        model.exp_avg[k] = (params[k] * F32(0.5) + F32(1)).astype(F32)
        model.exp_avg_sq[k] = (params[k] * params[k]).astype(F32)
        opt.exp_avg[k].copy_(torch.tensor(model.exp_avg[k]))
        opt.exp_avg_sq[k].copy_(torch.tensor(model.exp_avg_sq[k]))
    dc = DensityControl(opt, oc.CFG["percent_dense"])
    dc.grad_accum.copy_(torch.tensor(stats["grad_accum"]))
    dc.denom.copy_(torch.tensor(stats["denom"]))
    dc.max_radii.copy_(torch.tensor(stats["max_radii"]))
    old = {k: opt.params[k] for k in om.GROUPS}
    rep = dc.densify_and_prune(oc.CFG["max_grad"], oc.CFG["min_opacity"], oc.CFG["extent"], mss, n_split,
                               None if noise is None else torch.tensor(noise, device=DEV), generator)
    return opt, model, dc, rep, old


def check_densify(n, k, pattern, n_split, mss):
    what = f"N={n} K={k} {pattern} n_split={n_split} mss={mss}"
    params, stats = pattern_cloud(n, k, pattern, n_split, mss)
    noise = oc.make_noise(n, n_split, seed=n % 97)
    opt, model, dc, rep, old = run_densify(params, stats, noise, n_split, mss)
    mrep, mstats = om.densify_and_prune(model, stats, oc.CFG["max_grad"], oc.CFG["min_opacity"], oc.CFG["extent"], mss, n_split,
                                        noise, oc.CFG["percent_dense"])
    assert tuple(rep) == tuple(int(v) for v in mrep), what
    assert opt.num_rows == rep.n_after == opt.params["xyz"].shape[0]
    assert_state(opt, model, what)
    assert_stats(dc, mstats, what)
    for name in om.GROUPS:
        p = opt.params[name]
        assert p.is_leaf and p.requires_grad and p.grad is None and p.shape[1:] == old[name].shape[1:]
        assert om.same_bits(host(old[name]), params[name]), f"{what}: the old {name} changed"
    expect = dict(nothing=(0, 0, 0), all_cloned=(n, 0, 0), all_split=(0, n, 0), all_pruned=(0, 0, n)).get(pattern)
    if expect:
        assert (rep.n_cloned, rep.n_split, rep.n_pruned) == expect, what
    # a step on the new tensors
    grads = oc.make_grads(model.params, seed=11)
    both_step(opt, model, grads, visible=(np.arange(rep.n_after) % 4 != 0).astype(np.int32) if rep.n_after else None)
    assert_state(opt, model, what + ", the step after")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049, 131073])
def test_densify(n, pattern):
    """1023 | 1024 | 1025: the edges of the scan's 1024-value tile (the scan runs over 3 N flags); 131073: a multi-tile carry."""
    for k in (0, 15):
        for mss in (None, 20):
            for n_split in (1, 2, 3):
                check_densify(n, k, pattern, n_split, mss)


def test_densify_generator_noise_and_determinism():
    n, k, n_split = 1025, 3, 2
    params, stats = oc.make_cloud(n, k, seed=31, n_split=n_split, max_screen_size=20)
    runs = []
    for _ in range(2):
        g = torch.Generator(device=DEV)
        g.manual_seed(5)
        opt, _, _, rep, _ = run_densify(params, stats, None, n_split, 20, generator=g)
        runs.append({name: host(opt.params[name]) for name in om.GROUPS})
    assert all(om.same_bits(runs[0][name], runs[1][name]) for name in om.GROUPS)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    noise = host(torch.randn((n, n_split, 3), dtype=torch.float32, device=DEV, generator=g))
    opt, model, _, rep, _ = run_densify(params, stats, noise, n_split, 20)
    om.densify_and_prune(model, stats, noise=noise, n_split=n_split, max_screen_size=20, **oc.CFG)
    assert_state(opt, model)
    assert all(om.same_bits(runs[0][name], host(opt.params[name])) for name in om.GROUPS)
    assert rep.n_split > 0
    with pytest.raises(ValueError, match="noise"):
        run_densify(params, stats, np.zeros((n, 3, 3), F32), n_split, 20)


def test_densify_on_a_side_stream():
    n, k, n_split = 2049, 15, 2
    params, stats = oc.make_cloud(n, k, seed=41, n_split=n_split, max_screen_size=None)
    noise = oc.make_noise(n, n_split)
    grads = oc.make_grads(params, seed=3)
    vis = (np.arange(n) % 2).astype(np.int32)
    side = torch.cuda.Stream(device=DEV)
    results = []
    for stream in (None, side, side):
        torch.cuda.synchronize()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(DEV)):
            opt, model = pair(params)
            both_step(opt, model, grads, visible=vis)
            dc = DensityControl(opt)
            dc.accumulate(torch.tensor(grads["xyz"] * F32(0.5), device=DEV), torch.tensor(vis * 9, device=DEV))
            rep = dc.densify_and_prune(1e-4, 0.05, 4.0, None, n_split, torch.tensor(noise, device=DEV))
            mask = torch.tensor(np.arange(rep.n_after) % 5 == 0, device=DEV)
            dc.prune(mask)
            torch.cuda.current_stream(DEV).synchronize()
        results.append({name: (host(opt.params[name]), host(opt.exp_avg[name])) for name in om.GROUPS})
    for other in results[1:]:
        for name in om.GROUPS:
            assert om.same_bits(results[0][name][0], other[name][0]) and om.same_bits(results[0][name][1], other[name][1])
    assert results[0]["xyz"][0].shape[0] != n


# ------------------------------------------------------------------------------------------------------------------ prune, reset
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049, 131073])
def test_prune_carries_moments_and_statistics(n):
    k = 15 if n < 5000 else 3
    params = oc.make_params(n, k, seed=n % 1000)
    stats = oc.make_stats(n, seed=5)
    rng = np.random.default_rng(n)
    masks = [np.zeros(n, bool), np.ones(n, bool), rng.random(n) < 0.3, np.arange(n) == n - 1, np.isin(np.arange(n), (1023, 1024))]
    for i, mask in enumerate(masks):
        opt, model = pair(params)
        both_step(opt, model, oc.make_grads(params, seed=1))
        dc = DensityControl(opt)
        dc.grad_accum.copy_(torch.tensor(stats["grad_accum"]))
        dc.denom.copy_(torch.tensor(stats["denom"]))
        dc.max_radii.copy_(torch.tensor(stats["max_radii"]))
        old = opt.params["xyz"]
        rep = dc.prune(torch.tensor(mask, device=DEV))
        mrep, kept = om.prune(model, {k_: v.copy() for k_, v in stats.items()}, mask)
        assert tuple(rep) == tuple(int(v) for v in mrep), f"mask {i}"
        assert_state(opt, model, f"mask {i}")
        assert_stats(dc, kept, f"mask {i}")
        assert om.same_bits(host(old), model_start(params, model, "xyz", 1)) and opt.num_rows == n - int(mask.sum())
        if rep.n_after:
            both_step(opt, model, oc.make_grads(model.params, seed=2))
            assert_state(opt, model, f"mask {i}, the step after")
    with pytest.raises(ValueError, match="mask"):
        dc.prune(torch.zeros(opt.num_rows + 1, dtype=torch.bool, device=DEV))


def model_start(params, model, name, steps):
    """What the tensor a prune left behind holds: the parameters after `steps` model steps on seed-1 gradients."""
    ref = om.AdamModel(params, oc.LR)
    for _ in range(steps):
        ref.step(oc.make_grads(params, seed=1))
    return ref.params[name]


def test_reset_opacity():
    params = oc.make_params(257, 3, seed=6)
    params["opacity"][3, 0] = np.nan
    params["opacity"][4, 0] = np.inf
    opt, model = pair(params)
    both_step(opt, model, oc.make_grads(params, seed=1))
    dc = DensityControl(opt)
    tensor = opt.params["opacity"]
    dc.reset_opacity(0.01)
    om.reset_opacity(model, 0.01)
    assert opt.params["opacity"] is tensor and tensor.is_leaf and tensor.requires_grad
    assert_state(opt, model)
    assert not host(opt.exp_avg["opacity"]).any() and host(opt.exp_avg["xyz"]).any()
    assert np.nanmax(host(tensor)) == F32(math.log(0.01 / 0.99))
    both_step(opt, model, oc.make_grads(params, seed=2))
    assert_state(opt, model, "the step after")


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_one_autograd_round():
    """FusedGaussianRasterizer -> photometric_loss -> backward -> accumulate -> sparse step on a 64 x 48 image with 500
    Gaussians: the model, given the device's own gradients, against the device."""
    from gaustudio_amd import GaussianRasterizationSettings, photometric_loss, scenes
    from gaustudio_amd.fused import FusedGaussianRasterizer
    cam = scenes.make_camera(64, 48)
    sc = scenes.make_scene(500, cam, seed=3, sigma_px_median=2.0)
    sc.means3D[::7, 2] = -5.0                                       # behind the camera: never visible
    params = dict(xyz=sc.means3D, f_dc=sc.shs[:, :1], f_rest=sc.shs[:, 1:], opacity=torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)),
                  scaling=torch.log(sc.scales), rotation=sc.rotations)
    params = {k: np.ascontiguousarray(v.numpy(), dtype=F32) for k, v in params.items()}
    opt, model = pair(params)
    dc = DensityControl(opt)
    stats = om.new_stats(500)
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=DEV), 1.0,
                                       cam.viewmatrix.to(DEV), cam.projmatrix.to(DEV), 3, cam.campos.to(DEV), False, False)
    target = torch.rand(3, cam.height, cam.width, generator=torch.Generator().manual_seed(0)).to(DEV)
    for step in range(2):
        p = opt.params
        means2D = torch.zeros_like(p["xyz"], requires_grad=True)
        color, radii = FusedGaussianRasterizer(rs)(means3D=p["xyz"], means2D=means2D, raw_opacities=p["opacity"], f_dc=p["f_dc"],
                                                   f_rest=p["f_rest"], raw_scales=p["scaling"], raw_rotations=p["rotation"])[:2]
        photometric_loss(color, target).backward()
        grads = {k: host(v.grad) for k, v in p.items()}
        dc.accumulate(means2D.grad, radii)
        opt.step(visible=radii)
        opt.zero_grad()
        om.accumulate(stats, host(means2D.grad), host(radii))
        model.step(grads, visible=host(radii))
        assert_state(opt, model, f"step {step}")
        assert_stats(dc, stats, f"step {step}")
    seen = host(radii) > 0
    assert seen.any() and not seen.all() and stats["grad_accum"][seen].max() > 0
    assert om.same_bits(host(opt.params["xyz"])[~seen], params["xyz"][~seen])


def test_the_training_example():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "64"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("loss ") and "N 1000 -> " in last, last
    n_end = int(last.split("N 1000 -> ")[1].split()[0])
    assert n_end != 1000, last

