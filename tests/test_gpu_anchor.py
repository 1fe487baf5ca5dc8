"""gaustudio_amd.AnchorControl on the GPU against tests/anchor_model.py, bit for bit: parameters, moments, statistics and the
report, at the sizes where the scan and sort tiles end, on degenerate candidate sets, through a real torch.optim.Adam, on a side
stream, and in one autograd round with render_scaffold."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import anchor_cases as ac  # noqa: E402
import anchor_model as am  # noqa: E402
import test_anchor_model as hand  # noqa: E402  (the hand cases' builders)

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need a ROCm device"
    return torch.device("cuda", 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def build(params, stats, k, moments, cfg, dev, step=7.0):
    from gaustudio_amd import AnchorControl
    tp = {n: torch.tensor(params[n], device=dev).requires_grad_(True) for n in am.NAMES}
    opt = None
    if moments:
        opt = torch.optim.Adam([dict(params=[tp[n]], lr=1e-3) for n in am.NAMES])
        for n in moments:
            opt.state[tp[n]] = dict(step=torch.tensor(step), exp_avg=torch.tensor(moments[n][0], device=dev),
                                    exp_avg_sq=torch.tensor(moments[n][1], device=dev))
    ctl = AnchorControl(tp, cfg["voxel_size"], optimizer=opt, update_depth=cfg.get("update_depth", 3),
                        update_init_factor=cfg.get("update_init_factor", 16), update_hierarchy_factor=cfg.get("update_hierarchy_factor", 4))
    for name in am.STATS:
        getattr(ctl, name).copy_(torch.tensor(stats[name], device=dev))
    return ctl, tp, opt


def adjust_kwargs(cfg):
    return {key: cfg[key] for key in ("check_interval", "success_threshold", "grad_threshold", "min_opacity") if key in cfg}


def run_and_compare(params, stats, k, rand, moments, cfg, dev):
    """GPU against the model on one case; returns the report."""
    model_cfg = dict(cfg)
    rand = np.ascontiguousarray(rand[:cfg.get("update_depth", 3)])   # a draw per level that can run
    want_p, want_m, want_s, want_rep, _ = am.adjust(params, moments, stats, k, rand=rand, **model_cfg)
    ctl, tp, opt = build(params, stats, k, moments, cfg, dev)
    tp = dict(tp)                                                    # the old leaves: adjust replaces the entries of ctl.params
    before = {n: t.detach().clone() for n, t in tp.items()}
    rep = ctl.adjust(rand=torch.tensor(rand, device=dev), **adjust_kwargs(cfg))
    assert tuple(rep) == tuple(want_rep), (rep, want_rep)
    for n in am.NAMES:
        new = ctl.params[n]
        assert new.is_leaf and new.requires_grad and new.grad is None and new is not tp[n]
        assert same(new.detach().cpu().numpy(), want_p[n]), n
        assert torch.equal(tp[n].detach(), before[n]), f"the old {n} was modified"
        if opt is not None:
            assert any(p is new for g in opt.param_groups for p in g["params"]) and tp[n] not in opt.state
            if n in moments:
                st = opt.state[new]
                assert float(st["step"]) == 7.0
                assert same(st["exp_avg"].cpu().numpy(), want_m[n][0]) and same(st["exp_avg_sq"].cpu().numpy(), want_m[n][1]), n
    for name in am.STATS:
        assert same(getattr(ctl, name).cpu().numpy(), want_s[name]), name
    assert ctl.num_anchors == want_rep.n_after
    return rep


def all_hot(n, k, seed, extent):
    """Every slot a candidate at every level: the candidate count is N k, the size the scan and sort tiles see."""
    params, stats = ac.make_cloud(n, k, seed, extent)
    stats["offset_denom"][:] = 90
    stats["offset_grad_accum"][:] = F32(90 * 1e-2)
    return params, stats, np.full((3, n * k), 0.999, F32)


EDGES = [(nk, 1) for nk in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)] + [(26, 10), (410, 10), (16, 16), (64, 16), (256, 16)]


@pytest.mark.parametrize("n,k", EDGES)
def test_tile_edges_with_every_slot_a_candidate(dev, n, k):
    params, stats, rand = all_hot(n, k, 100 + n + k, extent=0.4)
    rep = run_and_compare(params, stats, k, rand, ac.make_moments(params, n), ac.CFG, dev)
    assert sum(rep.n_grown) > 0


def test_many_sort_tiles(dev):
    n = 131073
    params, stats, rand = all_hot(n, 1, 5, extent=3.0)
    rep = run_and_compare(params, stats, 1, rand, {}, ac.CFG, dev)
    assert rep.n_grown[2] > 4096


@pytest.mark.parametrize("n,k,seed,extent", [(1500, 10, 21, 1.0), (900, 16, 22, 0.6), (2500, 1, 23, 0.5)])
def test_mixed_cloud_with_moments(dev, n, k, seed, extent):
    params, stats = ac.make_cloud(n, k, seed, extent)
    rep = run_and_compare(params, stats, k, ac.make_rand(n, k, seed), ac.make_moments(params, seed), ac.CFG, dev)
    assert rep.n_grown[0] > 0 and sum(rep.n_grown[1:]) > 0 and rep.n_pruned > 0


def test_zero_candidates(dev):
    params, stats = ac.make_cloud(300, 10, 31)
    stats["offset_denom"][:] = 10                                    # nothing is mature
    rep = run_and_compare(params, stats, 10, ac.make_rand(300, 10, 31), ac.make_moments(params, 31), ac.CFG, dev)
    assert rep.n_grown == (0, 0, 0)


def one_cell(n, k, occupied):
    """Every slot of every anchor decodes into the cell of the origin (level size 0.16); the anchors sit elsewhere, or one of
    them at the origin."""
    rng = np.random.default_rng(7)
    anchor = rng.uniform(2.0, 3.0, (n, 3)).astype(F32)
    if occupied:
        anchor[n // 2] = 0.01
    target = rng.uniform(-0.05, 0.05, (n, k, 3))
    params = dict(anchor=anchor, anchor_feat=rng.standard_normal((n, 32)).astype(F32),
                  offset=((target - anchor[:, None, :]) / 0.1).astype(F32), scale_raw=np.full((n, 6), np.log(0.1), F32),
                  rot_raw=rng.standard_normal((n, 4)).astype(F32))
    stats = am.zero_stats(n, k)
    stats["offset_denom"][:] = 90
    stats["offset_grad_accum"][:] = F32(90 * 1e-2)
    return params, stats, np.full((1, n * k), 0.999, F32)


def test_all_candidates_in_one_cell(dev):
    params, stats, rand = one_cell(500, 10, occupied=False)          # one run of 5000, longer than any tile
    cfg = dict(ac.CFG, update_depth=1)
    rep = run_and_compare(params, stats, 10, rand, {}, cfg, dev)
    assert rep.n_grown == (1,)


def test_every_candidate_cell_already_holds_an_anchor(dev):
    params, stats, rand = one_cell(500, 10, occupied=True)
    rep = run_and_compare(params, stats, 10, rand, {}, dict(ac.CFG, update_depth=1), dev)
    assert rep.n_grown == (0,)


def test_cells_at_the_ends_of_the_range(dev):
    top = float(2 ** 20 - 1)
    params = hand.tiny([[0, 0, 0], [0, 0, 0]], [[top, -top, top], [-top, top, -float(2 ** 20)]])
    rep = run_and_compare(params, hand.hot_stats(2, 1), 1, hand.ONES(2, 1), ac.make_moments(params, 3),
                          dict(hand.UNIT, update_depth=1), dev)
    assert rep.n_grown == (2,)


def test_candidate_out_of_range_raises_and_changes_nothing(dev):
    params, stats = ac.make_cloud(400, 4, 41)
    stats["offset_denom"][:] = 90
    stats["offset_grad_accum"][:] = F32(90 * 1e-2)
    params["offset"][123, 2, 1] = 1e9                                 # level 0 is fine with the draw below, level 1 is not
    rand = np.full((3, 1600), 0.999, F32)
    rand[0, 123 * 4 + 2] = 0.0
    moments = ac.make_moments(params, 41)
    with pytest.raises(ValueError):
        am.adjust(params, moments, stats, 4, rand=rand, **ac.CFG)
    ctl, tp, opt = build(params, stats, 4, moments, ac.CFG, dev)
    tp = dict(tp)
    with pytest.raises(ValueError, match="nothing was changed"):
        ctl.adjust(rand=torch.tensor(rand, device=dev), **adjust_kwargs(ac.CFG))
    for n in am.NAMES:
        assert ctl.params[n] is tp[n] and same(tp[n].detach().cpu().numpy(), params[n])
        assert same(opt.state[tp[n]]["exp_avg"].cpu().numpy(), moments[n][0])
        assert same(opt.state[tp[n]]["exp_avg_sq"].cpu().numpy(), moments[n][1])
    for name in am.STATS:
        assert same(getattr(ctl, name).cpu().numpy(), stats[name]), name
    params["offset"][123, 2, 1] = np.nan                              # a position that is not finite, at level 0
    rand[0, :] = 0.999
    ctl, tp, opt = build(params, stats, 4, {}, ac.CFG, dev)
    with pytest.raises(ValueError, match="nothing was changed"):
        ctl.adjust(rand=torch.tensor(rand, device=dev), **adjust_kwargs(ac.CFG))


def hand_cases():
    y = hand.exact_offset(50.0)
    xs = [0.5, -0.5, 1.5, 2.5, -1.5, -2.5, -7.25]
    out = {"ties": (hand.tiny(np.zeros((len(xs), 3)), [[hand.exact_offset(x), y, 0.0] for x in xs]), hand.hot_stats(len(xs), 1),
                    hand.ONES(len(xs), 1), dict(hand.UNIT, update_depth=1))}
    rand = hand.ONES(2, 1)
    rand[0, 1] = 0.1
    out["blocked"] = (hand.tiny([[50, 0, 0], [60, 0, 0]], [[-49.9, 0, 0], [-59.95, 0, 0]]), hand.hot_stats(2, 1), rand,
                      dict(hand.UNIT, update_depth=2))
    out["unblocked"] = (hand.tiny([[50, 0, 0], [60, 0, 0]], [[-46.9, 0, 0], [-59.95, 0, 0]]), hand.hot_stats(2, 1), rand,
                        dict(hand.UNIT, update_depth=2))
    out["quirk"] = (hand.tiny([[0, 0, 0]], [[0.3, 0, 0]]), hand.hot_stats(1, 1), hand.ONES(1, 1), dict(hand.UNIT))
    st = hand.hot_stats(3, 1)
    st["offset_denom"][0] = 0
    st["offset_grad_accum"][1] = np.nan
    out["denom0_nan"] = (hand.tiny([[0, 0, 0]] * 3, [[5.2, 0, 0], [6.2, 0, 0], [7.2, 0, 0]]), st, hand.ONES(3, 1),
                         dict(hand.UNIT, update_depth=1))
    out["far_anchor"] = (hand.tiny([[float(2 ** 21), 0, 0], [0, 0, 0]], [[1.0, 0, 0], [3.2, 0, 0]]),
                         hand.hot_stats(2, 1, hot=[False, True]), hand.ONES(2, 1), dict(hand.UNIT, update_depth=1))
    p4 = hand.tiny([[i, 0, 0] for i in range(4)], [[0, 0, 0]] * 4)
    st = am.zero_stats(4, 1)
    st["anchor_denom"][:] = [81, 81, 80, 81]
    st["opacity_accum"][:] = [0.4, 0.41, 0.0, 0.0]
    out["prune"] = (p4, st, hand.ONES(4, 1), dict(hand.UNIT))
    out["min_opacity_0"] = (p4, st, hand.ONES(4, 1), dict(hand.UNIT, min_opacity=0))
    st = am.zero_stats(4, 1)
    st["anchor_denom"][:] = 200
    st["opacity_accum"][:] = -1.0
    out["all_pruned"] = (p4, st, hand.ONES(4, 1), dict(hand.UNIT))
    feat = np.zeros((3, 32), F32)
    feat[0, :], feat[1, :], feat[2, :] = -1.0, np.arange(32) - 16.0, -0.0
    out["max_feature"] = (hand.tiny([[0, 0, 0]] * 3, [[4.1, 0, 0], [4.2, 0, 0], [3.9, 0, 0]], feat=feat), hand.hot_stats(3, 1),
                          hand.ONES(3, 1), dict(voxel_size=0.125, update_depth=1))
    return out


@pytest.mark.parametrize("name", ["ties", "blocked", "unblocked", "quirk", "denom0_nan", "far_anchor", "prune", "min_opacity_0",
                                  "all_pruned", "max_feature"])
def test_hand_cases(dev, name):
    params, stats, rand, cfg = hand_cases()[name]
    rep = run_and_compare(params, stats, 1, rand, ac.make_moments(params, 9), cfg, dev)
    if name == "all_pruned":
        assert rep.n_after == 0
    if name == "quirk":
        assert rep.n_grown == (0, 0, 0)


# ------------------------------------------------------------------------------------------------------------ accumulate
class G:
    """What accumulate reads of a ScaffoldGaussians."""

    def __init__(self, aidx, oidx, opacity, visible, dev):
        self.anchor_index = torch.tensor(aidx, dtype=torch.int32, device=dev)
        self.offset_index = torch.tensor(oidx, dtype=torch.int32, device=dev)
        self.opacity = torch.tensor(opacity, dtype=torch.float32, device=dev).reshape(-1, 1)
        self.visible = torch.tensor(visible, dtype=torch.bool, device=dev)


def random_view(n, k, seed):
    """Anchors with 0, 1, some and k kept offsets, in anchor-major order; radii <= 0 rows among them."""
    rng = np.random.default_rng(seed)
    visible = rng.random(n) < 0.7
    kept = rng.random((n, k)) < 0.5
    kept[rng.random(n) < 0.15] = False
    kept[rng.random(n) < 0.15] = True
    one = rng.random(n) < 0.15
    kept[one] = False
    kept[one, rng.integers(0, k, int(one.sum()))] = True
    kept[~visible] = False
    aidx, oidx = np.nonzero(kept)
    m = len(aidx)
    return (aidx, oidx, rng.random(m).astype(F32), (rng.standard_normal((m, 3)) * 1e-3).astype(F32),
            rng.integers(-1, 4, m).astype(np.int32), visible)


@pytest.mark.parametrize("n,k", [(1, 1), (300, 1), (257, 10), (1000, 16)])
def test_accumulate_matches_the_model(dev, n, k):
    from gaustudio_amd import AnchorControl
    params, _ = ac.make_cloud(n, k, 50 + n)
    ctl, _, _ = build(params, am.zero_stats(n, k), k, {}, ac.CFG, dev)
    want = am.zero_stats(n, k)
    for view in range(3):                                            # accumulators that already hold something
        aidx, oidx, op, vg, radii, visible = random_view(n, k, 10 * n + view)
        am.accumulate(want, k, aidx, oidx, op, vg, radii, visible)
        ctl.accumulate(G(aidx, oidx, op, visible, dev), torch.tensor(vg, device=dev), torch.tensor(radii, device=dev))
    for name in am.STATS:
        assert same(getattr(ctl, name).cpu().numpy(), want[name]), name
    empty = G(np.zeros(0), np.zeros(0), np.zeros(0), np.ones(n, bool), dev)       # M = 0: the visible anchors still count
    ctl.accumulate(empty, torch.zeros((0, 3), device=dev), torch.zeros(0, dtype=torch.int32, device=dev))
    want["anchor_denom"] += 1
    for name in am.STATS:
        assert same(getattr(ctl, name).cpu().numpy(), want[name]), name
    assert isinstance(ctl, AnchorControl)


# ------------------------------------------------------------------------------------------------------------ with the renderer
def scene(dev, n=3000, k=4, seed=0):
    from gaustudio_amd import GaussianRasterizationSettings, scenes
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
    anchor = torch.nn.functional.normalize(r(n, 3))
    params = dict(anchor=anchor, anchor_feat=r(n, 32), offset=r(n, k, 3),
                  scale_raw=torch.cat([torch.full((n, 3), 0.03), torch.full((n, 3), 0.02)], dim=1).log().to(dev),
                  rot_raw=torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(n, 1))
    params = {name: t.contiguous().requires_grad_(True) for name, t in params.items()}
    lin = lambda n_in, n_out, bias=0.0: tuple(t.requires_grad_(True) for t in (r(32, n_in, scale=0.2), r(32, scale=0.1),
                                                                                r(n_out, 32, scale=0.2), r(n_out, scale=0.1) + bias))
    mlps = dict(mlp_opacity=lin(36, k, bias=1.0), mlp_cov=lin(36, 7 * k), mlp_color=lin(36, 3 * k))
    cam = scenes.ring_cameras(1, 160, 120, radius=3.2, elevation=0.35)[0]
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0,
                                       cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 1, cam.campos.to(dev), False, False)
    return params, mlps, rs


def render(params, mlps, rs, backward):
    from gaustudio_amd import ScaffoldModel, render_scaffold
    return render_scaffold(ScaffoldModel.from_raw(**params, **mlps), rs, backward=backward)


@pytest.mark.parametrize("backward", ["hip", "torch"])
def test_accumulate_takes_the_outputs_of_both_backward_modes(dev, backward):
    from gaustudio_amd import AnchorControl
    params, mlps, rs = scene(dev)
    ctl = AnchorControl(params, 0.01)
    out = render(params, mlps, rs, backward)
    out["render"].square().mean().backward()
    g = out["gaussians"]
    ctl.accumulate(g, out["viewspace_points"].grad, out["radii"])
    want = am.zero_stats(3000, 4)
    am.accumulate(want, 4, g.anchor_index.cpu().numpy(), g.offset_index.cpu().numpy(), g.opacity.detach().cpu().numpy(),
                  out["viewspace_points"].grad.cpu().numpy(), out["radii"].cpu().numpy(), g.visible.cpu().numpy())
    assert want["offset_denom"].sum() > 100 and want["anchor_denom"].sum() > 100
    for name in am.STATS:
        assert same(getattr(ctl, name).cpu().numpy(), want[name]), name


def test_autograd_round_through_a_real_adam(dev):
    """render -> loss -> Adam step -> accumulate -> adjust -> Adam step -> render with the new N: survivors keep their moments
    bit for bit, new rows start at zero, `step` is kept and the MLP group is left alone."""
    from gaustudio_amd import AnchorControl
    params, mlps, rs = scene(dev)
    weights = [t for w in mlps.values() for t in w]
    opt = torch.optim.Adam([dict(params=[params[n]], lr=1e-3) for n in ("anchor", "anchor_feat", "offset", "scale_raw")] +
                           [dict(params=weights, lr=1e-3), dict(params=[params["rot_raw"]], lr=1e-3)])
    ctl = AnchorControl(params, 0.01, optimizer=opt)
    for _ in range(3):
        opt.zero_grad()
        out = render(params, mlps, rs, "hip")
        out["render"].square().mean().backward()
        params["rot_raw"].grad = torch.zeros_like(params["rot_raw"])          # decode treats rot as a constant
        opt.step()
        ctl.accumulate(out["gaussians"], out["viewspace_points"].grad, out["radii"])
    old = dict(params)
    stats = {name: getattr(ctl, name).cpu().numpy().copy() for name in am.STATS}
    moments = {n: (opt.state[old[n]]["exp_avg"].cpu().numpy().copy(), opt.state[old[n]]["exp_avg_sq"].cpu().numpy().copy())
               for n in am.NAMES}
    mlp_state = [(opt.state[w]["exp_avg"].clone(), opt.state[w]["exp_avg_sq"].clone()) for w in weights]
    rand = torch.rand((3, 3000 * 4), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    cfg = dict(check_interval=3, success_threshold=0.8, grad_threshold=1e-7, min_opacity=0.005)
    rep = ctl.adjust(rand=rand, **cfg)
    want_p, want_m, want_s, want_rep, _ = am.adjust({n: old[n].detach().cpu().numpy() for n in am.NAMES}, moments, stats, 4,
                                                    voxel_size=0.01, rand=rand.cpu().numpy(), **cfg)
    assert tuple(rep) == tuple(want_rep) and sum(rep.n_grown) > 0
    n_old = rep.n_before - rep.n_pruned
    for n in am.NAMES:
        st = opt.state[params[n]]
        assert params[n] is ctl.params[n] and params[n] is not old[n] and old[n] not in opt.state
        assert same(params[n].detach().cpu().numpy(), want_p[n]), n
        assert same(st["exp_avg"].cpu().numpy(), want_m[n][0]) and same(st["exp_avg_sq"].cpu().numpy(), want_m[n][1]), n
        assert not st["exp_avg"][n_old:].any() and not st["exp_avg_sq"][n_old:].any() and float(st["step"]) == 3.0
    assert [g["params"] for g in opt.param_groups][4] == weights
    for w, (m, v) in zip(weights, mlp_state):
        assert torch.equal(opt.state[w]["exp_avg"], m) and torch.equal(opt.state[w]["exp_avg_sq"], v)
    for name in am.STATS:
        assert same(getattr(ctl, name).cpu().numpy(), want_s[name]), name
    opt.zero_grad()
    out = render(params, mlps, rs, "hip")                                        # the new N renders and trains
    assert out["gaussians"].visible.shape[0] == rep.n_after
    out["render"].square().mean().backward()
    assert params["anchor_feat"].grad.shape[0] == rep.n_after
    params["rot_raw"].grad = torch.zeros_like(params["rot_raw"])
    opt.step()
    assert float(opt.state[params["anchor"]]["step"]) == 4.0 and torch.isfinite(params["anchor"]).all()
    ctl.accumulate(out["gaussians"], out["viewspace_points"].grad, out["radii"])


def test_two_runs_and_a_side_stream_give_the_same_bits(dev):
    params, stats = ac.make_cloud(1500, 10, 21, 1.0)
    rand, moments = ac.make_rand(1500, 10, 21), ac.make_moments(params, 21)
    results = []
    for stream in (None, None, torch.cuda.Stream(device=dev)):
        ctl, tp, opt = build(params, stats, 10, moments, ac.CFG, dev)
        r = torch.tensor(rand, device=dev)
        torch.cuda.synchronize(dev)
        if stream is None:
            rep = ctl.adjust(rand=r, **adjust_kwargs(ac.CFG))
        else:
            with torch.cuda.stream(stream):
                rep = ctl.adjust(rand=r, **adjust_kwargs(ac.CFG))
            stream.synchronize()
        torch.cuda.synchronize(dev)
        results.append((rep, {n: ctl.params[n].detach().cpu().numpy() for n in am.NAMES},
                        {n: opt.state[ctl.params[n]]["exp_avg"].cpu().numpy() for n in am.NAMES},
                        {name: getattr(ctl, name).cpu().numpy() for name in am.STATS}))
    for rep, p, m, s in results[1:]:
        assert rep == results[0][0]
        assert all(same(p[n], results[0][1][n]) and same(m[n], results[0][2][n]) for n in am.NAMES)
        assert all(same(s[name], results[0][3][name]) for name in am.STATS)


def test_default_draw_is_reproducible_with_a_generator(dev):
    params, stats = ac.make_cloud(500, 4, 61)
    reps = []
    for _ in range(2):
        ctl, _, _ = build(params, stats, 4, {}, ac.CFG, dev)
        reps.append((ctl.adjust(generator=torch.Generator(device=dev).manual_seed(11), **adjust_kwargs(ac.CFG)),
                     ctl.params["anchor"].detach().cpu().numpy()))
    assert reps[0][0] == reps[1][0] and same(reps[0][1], reps[1][1]) and sum(reps[0][0].n_grown) > 0


def test_the_example_at_a_reduced_step_count(dev):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import scaffold_train_synthetic as ex
    first, last, n0, n1 = ex.main(steps=30, num_anchors=4000, adjust_every=8, size=(160, 120), grad_threshold=2e-3, quiet=True)
    assert last < first and n1 > n0
