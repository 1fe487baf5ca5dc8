"""GPU (-m gpu): the 2D Gaussian surfel operator at the shapes where its four kernels can go wrong and tests/test_gpu_surfel.py's
five well-behaved scenes cannot tell: images that are no multiple of the tile (1 x 1 included), tile lists of several 256-entry
batches and of every sort size class (<= 1024, radix, > 8192), the near plane and every cull, depth ties, and -- free of any
tolerance -- bit-identity under a permutation of the surfels and under appended culled ones.  The scenes come from
tests/surfel_scenes.py; tests/test_surfel_scenes.py asserts on the CPU, with the model alone, that each still exercises its path.

Every case runs forward and backward against the float64 model (tests/surfel_model.py) fed the operator's radii, after the
radii themselves are checked against the model's own.  Images as in test_gpu_surfel.py (_check_images: 1e-4, at most 0.1 % of the
pixels beyond, each an event of the model); gradients within 1e-3 relative L2 per tensor, and, surfel by surfel,

    |g_i - ref_i| / (|ref_i| + 1e-3 median_j |ref_j|) <= PER_SURFEL_TOL      (surfel_checks.per_surfel_error)

over the visible surfels whose rect holds no event pixel (at most a quarter may be excluded).  PER_SURFEL_TOL is not chosen: it
is 4 x the largest such error of the model run in float32 against the model run in float64 (both on the CPU, same tile lists),
measured on three of the scenes below -- the kernel sums in another order than torch's float32 ops, and both orders obey the same
n u sum|x| bound, hence the factor.  Measured maxima (tests/test_surfel_scenes.py re-derives them and fails if they drift):

    ragged 129 x 65      1.37e-3   (recorded as 1.4e-3)
    near plane / culls   4.1e-4    (recorded as 4.2e-4)
    long list, P = 1025  2.08e-3   (recorded as 2.1e-3)           ->  PER_SURFEL_TOL = 4 x 2.1e-3 = 8.4e-3"""
import numpy as np
import pytest
import torch

import surfel_checks as ck
import surfel_model as sm
import surfel_scenes as ss
import test_gpu_surfel as base
from test_surfel_scenes import check_long_preconditions

pytestmark = pytest.mark.gpu

DEV = base.DEV
MEASURED_F32_MODEL = {"ragged_129x65": 1.4e-3, "near_and_culls": 4.2e-4, "long_1025": 2.1e-3}
PER_SURFEL_TOL = 4 * max(MEASURED_F32_MODEL.values())


def _setup(sc, leaves=None):
    from diff_surfel_rasterization import GaussianRasterizationSettings
    cam = sc.cam
    lv = {k: v.to(DEV).requires_grad_(True) for k, v in (sc.leaves if leaves is None else leaves).items()}
    bgt = sc.bg.to(DEV)
    rs = GaussianRasterizationSettings(sc.H, sc.W, cam.tanfovx, cam.tanfovy, bgt, 1.0, cam.viewmatrix.to(DEV), cam.projmatrix.to(DEV),
                                       sc.D, cam.campos.to(DEV), False, False)
    return lv, rs, bgt


def _output_grads(sc):
    gc, ga = ck.output_grads(sc.W, sc.H)
    return gc.to(DEV), ga.to(DEV)


def _check_case(sc, fast_exp, label, min_visible=None):
    """Forward and backward against the float64 model: radii, images, gradients (global and per surfel).  Returns what the
    case-specific assertions need."""
    import gaustudio_amd
    W, H, D = sc.W, sc.H, sc.D
    P = sc.leaves["means3D"].shape[0]
    leaves, rs, bgt = _setup(sc)
    gc, ga = _output_grads(sc)
    with gaustudio_amd.options(fast_exp=fast_exp):
        color, radii, allmap, g = base._grads(leaves, rs, gc, ga)
    assert radii.dtype == torch.int32 and int((radii > 0).sum()) > (P // 4 if min_visible is None else min_visible)
    own, boundary = sm.own_radii(leaves["means3D"], leaves["scales"], leaves["rotations"], rs.viewmatrix, rs.projmatrix, W, H,
                                 rs.scale_modifier)
    differ = own != radii.cpu().numpy()
    assert not (differ & ~boundary).any(), f"radii differ from the model at {np.nonzero(differ & ~boundary)[0][:8].tolist()}"
    assert int(differ.sum()) <= max(2, P // 1000)
    ml, out = base._model(sc.cam, leaves, rs, bgt, radii, W, H, D)
    assert torch.equal(out["radii"].to(radii.device), radii.long())
    ours, ref_img = torch.cat([color, allmap]), torch.cat([out["color"], out["allmap"]])
    diff = (ours.double() - ref_img.detach()).abs().amax(0)
    nev = int(out["events"].sum())
    print(f"{label}: events {nev} (share {nev / (W * H):.2e}), max image diff {float(diff.max()):.3g}, "
          f"off events {float(diff[~out['events']].max()) if nev < W * H else 0.0:.3g}, n_contrib max {int(out['n_contrib'].max())}")
    base._check_images(ours, ref_img, out["events"])
    ref = sm.grads(out, ml, gc.double(), ga.double(), W=W, H=H)
    worst, where, share = ck.per_surfel_error(g, ref, out)
    print(f"{label}: per-surfel max {worst:.3g} at {where}, excluded {share:.2%}; rel L2 " +
          ", ".join(f"{k} {base._rel(v, ref[k]):.2g}" for k, v in g.items()))
    for k, v in g.items():
        assert torch.isfinite(v).all(), k
        assert base._rel(v, ref[k]) < 1e-3, f"grad {k}: rel L2 {base._rel(v, ref[k]):.3g}"
    assert share <= 0.25, f"{share:.0%} of the visible surfels lie on an event pixel: the per-surfel check would be vacuous"
    assert worst <= PER_SURFEL_TOL, f"per-surfel gradient error {worst:.3g} at {where}"
    return dict(leaves=leaves, radii=radii, g=g, out=out, color=color, allmap=allmap)


def _modes(dagger):
    return [False, True] if dagger else [False]


# ---- (a) ragged images ------------------------------------------------------------------------------------------------------
RAGGED_CASES = [(W, H, fx) for (W, H) in ss.RAGGED for fx in _modes((W, H) in ((17, 33), (129, 65)))]


@pytest.mark.parametrize("W,H,fast_exp", RAGGED_CASES, ids=[f"{W}x{H}" + ("_fast" if fx else "") for W, H, fx in RAGGED_CASES])
def test_ragged_images(W, H, fast_exp):
    sc = ss.ragged(W, H)
    r = _check_case(sc, fast_exp, f"ragged {W}x{H}")
    if W * H == 1:
        assert int(r["out"]["events"].sum()) == 0
    # T_f bg is seen: the background shows through somewhere, and is not black
    assert float((1 - r["allmap"][1]).max()) > 0.1 and float(sc.bg.min()) > 0


# ---- (b) long lists ---------------------------------------------------------------------------------------------------------
LONG_CASES = [(16, 16, P, fx) for P in ss.LONG_P_16 for fx in _modes(P in (288, 1500))] + [(33, 17, 1100, False)]


@pytest.mark.parametrize("W,H,P,fast_exp", LONG_CASES, ids=[f"{W}x{H}_P{P}" + ("_fast" if fx else "") for W, H, P, fx in LONG_CASES])
def test_long_lists(W, H, P, fast_exp):
    """The per-surfel check is what found surfel_composite_bwd's loss of accuracy deep in a list: it formed what lies behind an
    entry as the forward's total minus the running prefix, and from P = 1023 on the opacity gradient of entries reached with
    T ~ 1e-3 was off by 1e-2 .. 0.32 of its size (P = 1023 2.3e-2, 1025 1.0e-2, 1500 3.9e-2, 8192 0.32, 8193 8.7e-2, 9000 0.14;
    tolerance 8.4e-3) while images and global norms passed.  The kernel now walks back to front and accumulates the remainder
    itself; measured since: at most 6.7e-3 (P = 1025), every other case below 4e-3."""
    sc = ss.long_list(W, H, P)
    r = _check_case(sc, fast_exp, f"long {W}x{H} P={P}")
    # the preconditions (tests/test_surfel_scenes.py asserts them on the CPU), here from the model fed the operator's radii
    check_long_preconditions(sc, r["out"], P, False)
    assert int(r["out"]["events"].sum()) == 0
    # opacities below 1/255 never contribute: no gradient at all
    assert float(r["g"]["opacities"][sc.groups["low"].to(DEV)].abs().max()) == 0.0


# ---- (c) near plane and culls -----------------------------------------------------------------------------------------------
def test_near_plane_and_culls():
    sc = ss.near_and_culls()
    P = sc.leaves["means3D"].shape[0]
    r = _check_case(sc, False, "near/culls")
    radii, g, grp = r["radii"].cpu(), {k: v.cpu() for k, v in r["g"].items()}, sc.groups
    # the intended culls, kind by kind (tests/test_surfel_scenes.py asserts the same counts of the model's own radii)
    assert int((radii[grp["behind"]] > 0).sum()) == 0 and int((radii[grp["offscreen"]] > 0).sum()) == 0
    pz = sc.leaves["means3D"][:, 2]
    assert torch.equal(radii[grp["z_span"]] > 0, pz[grp["z_span"]] > 0.2)
    k = len(grp["z_ulp"]) // 3
    assert torch.equal(radii[grp["z_ulp"]] > 0, torch.arange(3 * k) >= 2 * k)       # below and AT 0.2f: culled; one ulp above: kept
    for name in ("near_tilted", "tiny", "whole_grid", "opaque", "faint", "quat_big", "quat_small", "edge_on"):
        assert bool((radii[grp[name]] > 0).all()), name
    culled = radii == 0
    assert int(culled.sum()) >= 60
    assert len(g) == 6       # means3D, opacities, scales, rotations, shs or colors_precomp, means2D
    for name, v in g.items():
        assert float(v[culled].abs().max()) == 0.0, f"{name}: a culled surfel has a gradient"
    assert float(g["opacities"][grp["faint"]].abs().max()) == 0.0
    assert float(g["opacities"][grp["z_ulp"]].abs().max()) == 0.0                     # (opacity 0.0019: binned, never contributes)
    # opacity 1: where o G > 0.99 the clamp passes no gradient, elsewhere it does -- the rows are checked against the model above;
    # here only that the group is not silent
    assert float(g["opacities"][grp["opaque"]].abs().max()) > 0.0


# ---- (d) depth ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", ss.TIE_P)
def test_depth_ties(P):
    """The order within a tie shows in the images (a wrong order: differences far above 1e-4)."""
    sc = ss.long_list(16, 16, P, ties=True)
    key = ss.view_keys(sc).reshape(-1, 10)
    assert (key == key[:, :1]).all()                    # the float32 sort keys really tie, ten at a time
    r = _check_case(sc, False, f"ties P={P}")
    check_long_preconditions(sc, r["out"], P, True)
    assert int(r["out"]["events"].sum()) == 0


# ---- (e) bit-identity under permutation and padding ------------------------------------------------------------------------
def _run_plain(sc, leaves_cpu):
    leaves, rs, bgt = _setup(sc, leaves_cpu)
    gc, ga = _output_grads(sc)
    color, radii, allmap, g = base._grads(leaves, rs, gc, ga)
    return color, radii, allmap, g


@pytest.mark.parametrize("P", ss.PERM_P)
def test_bit_identical_under_permutation(P):
    sc = ss.plain(64, 48, P, seed=P)
    color, radii, allmap, g = _run_plain(sc, sc.leaves)
    key = ss.view_keys(sc)[radii.cpu().numpy() > 0]
    assert len(np.unique(key)) == len(key) and int((radii > 0).sum()) > P // 4
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(P))
    color2, radii2, allmap2, g2 = _run_plain(sc, {k: v[perm] for k, v in sc.leaves.items()})
    assert torch.equal(color2, color) and torch.equal(allmap2, allmap)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(P)
    assert torch.equal(radii2.cpu()[inv], radii.cpu())
    assert len(g) == 6       # means3D, opacities, scales, rotations, shs or colors_precomp, means2D
    for k in g:
        assert torch.equal(g2[k].cpu()[inv], g[k].cpu()), k


@pytest.mark.parametrize("P", ss.PERM_P)
def test_bit_identical_under_culled_padding(P):
    sc = ss.plain(64, 48, P, seed=P)
    color, radii, allmap, g = _run_plain(sc, sc.leaves)
    pad = ss.culled_padding(sc)
    color2, radii2, allmap2, g2 = _run_plain(sc, {k: torch.cat([v, pad[k]]) for k, v in sc.leaves.items()})
    assert torch.equal(color2, color) and torch.equal(allmap2, allmap)
    assert torch.equal(radii2[:P], radii) and int(radii2[P:].abs().max()) == 0 and radii2.numel() == P + 300
    assert len(g) == 6       # means3D, opacities, scales, rotations, shs or colors_precomp, means2D
    for k in g:
        assert torch.equal(g2[k][:P], g[k]), k
        assert float(g2[k][P:].abs().max()) == 0.0, k
