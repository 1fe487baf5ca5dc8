"""GPU (-m gpu): the 2D Gaussian surfel operator (diff_surfel_rasterization -> gsr_surfel.hip) against the float64 model of
tests/surfel_model.py, run on the GPU in float64 with the operator's radii (so that the tile lists agree).  Images within 1e-4;
at most 0.1 % of the pixels beyond, each of them an event of the model (surfel_model._composite): one of the contract's four
threshold events (alpha vs 1/255, T vs 1e-4, rho3 vs rho2, z vs 0.2) or -- a deliberate widening of that list -- o G vs the
0.99 clamp, T vs 0.5 at the median, or an ill-conditioned contributor (surfel_model._eval_f32: a splat seen almost edge-on, whose
float32 alpha or depth is off by more than 2e-5).  The radii are checked against the model's own culls and radius formula
(surfel_model.own_radii) before the operator's radii are fed to the model so that the tile lists agree.  Gradients within 1e-3
relative (L2) of the model's autograd gradients."""
import numpy as np
import pytest
import torch

import surfel_model as sm
from gaustudio_amd import scenes

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _setup(W, H, P, D, seed=0, precomp=False, modifier=1.0, bg="black", sigma=3.0):
    cam = scenes.make_camera(W, H)
    sc = scenes.make_scene(P, cam, seed=seed, sigma_px_median=sigma)
    leaves = dict(means3D=sc.means3D, opacities=sc.opacities, scales=sc.scales[:, :2].contiguous(), rotations=sc.rotations * 1.7)
    if precomp:
        leaves["colors_precomp"] = torch.sigmoid(sc.shs[:, 0, :]).contiguous()
    else:
        leaves["shs"] = sc.shs.contiguous()
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in leaves.items()}
    bgt = {"black": torch.zeros(3), "white": torch.ones(3), "device": torch.tensor([0.2, 0.4, 0.7], device=DEV)}[bg]
    from diff_surfel_rasterization import GaussianRasterizationSettings
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, bgt, modifier, cam.viewmatrix.to(DEV), cam.projmatrix.to(DEV),
                                       D, cam.campos.to(DEV), False, False)
    return cam, leaves, rs, bgt


def _run(leaves, rs):
    from diff_surfel_rasterization import GaussianRasterizer
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, radii, allmap = GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"],
                                                 shs=leaves.get("shs"), colors_precomp=leaves.get("colors_precomp"),
                                                 scales=leaves["scales"], rotations=leaves["rotations"])
    return color, radii, allmap, means2D


def _grads(leaves, rs, gc, ga):
    for v in leaves.values():
        v.grad = None
    color, radii, allmap, means2D = _run(leaves, rs)
    outs, gs = [], []
    if gc is not None:
        outs.append(color); gs.append(gc)
    if ga is not None:
        outs.append(allmap); gs.append(ga)
    torch.autograd.backward(outs, gs)
    torch.cuda.synchronize()
    g = {k: v.grad.clone() for k, v in leaves.items()}
    g["means2D"] = means2D.grad.clone()
    return color.detach(), radii, allmap.detach(), g


def _model(cam, leaves, rs, bgt, radii, W, H, D):
    d = torch.float64
    ml = {k: v.detach().to(d).requires_grad_(True) for k, v in leaves.items()}
    out = sm.render(ml["means3D"], ml["opacities"], ml["scales"], ml["rotations"], rs.viewmatrix, rs.projmatrix, rs.campos, W, H,
                    bgt.to(DEV), scale_modifier=rs.scale_modifier, sh_degree=D, shs=ml.get("shs"), colors_precomp=ml.get("colors_precomp"),
                    radii=radii)
    return ml, out


def _check_images(ours, ref, events, tol=1e-4):
    diff = (ours.double() - ref.detach()).abs().amax(0)
    bad = diff > tol
    nbad = int(bad.sum())
    assert nbad <= max(1, int(1e-3 * bad.numel())), f"{nbad} pixels beyond {tol} (max {float(diff.max()):.3g})"
    unexplained = bad & ~events
    if unexplained.any():
        ys, xs = torch.nonzero(unexplained, as_tuple=True)
        detail = [(int(y), int(x), [f"{float(a):.6g}/{float(b):.6g}" for a, b in zip(ours[:, y, x], ref[:, y, x].detach())])
                  for y, x in zip(ys[:4], xs[:4])]
        raise AssertionError(f"{int(unexplained.sum())} pixel(s) beyond {tol} are no threshold events: {detail}")


def _rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


CASES = [
    dict(W=64, H=48, P=200, D=0, bg="black"),
    dict(W=128, H=96, P=1500, D=1, bg="white"),
    dict(W=160, H=128, P=3000, D=2, bg="device", modifier=1.3),
    dict(W=256, H=160, P=5000, D=3, bg="black"),
    dict(W=128, H=96, P=1000, D=3, bg="white", precomp=True, modifier=0.8),
]


@pytest.mark.parametrize("fast_exp", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['W']}x{c['H']}_P{c['P']}_D{c['D']}_{c['bg']}" + ("_precomp" if c.get("precomp") else ""))
def test_surfel_forward_backward_vs_model(case, fast_exp):
    import gaustudio_amd
    W, H, D = case["W"], case["H"], case["D"]
    cam, leaves, rs, bgt = _setup(W, H, case["P"], D, seed=case["P"], precomp=case.get("precomp", False),
                                  modifier=case.get("modifier", 1.0), bg=case["bg"])
    gen = torch.Generator().manual_seed(5)
    gc = torch.randn(3, H, W, generator=gen).to(DEV)
    ga = torch.randn(7, H, W, generator=gen).to(DEV)
    with gaustudio_amd.options(fast_exp=fast_exp):
        color, radii, allmap, g = _grads(leaves, rs, gc, ga)
    assert radii.dtype == torch.int32 and int((radii > 0).sum()) > case["P"] // 4
    # the kernel's culls and radius formula against the model's own (not fed back: a radius too small, or a wrong cull, would
    # shrink both sides' tile lists alike below)
    own, boundary = sm.own_radii(leaves["means3D"], leaves["scales"], leaves["rotations"], rs.viewmatrix, rs.projmatrix, W, H,
                                 rs.scale_modifier)
    differ = own != radii.cpu().numpy()
    assert not (differ & ~boundary).any(), f"radii differ from the model at {np.nonzero(differ & ~boundary)[0][:8].tolist()}"
    assert int(differ.sum()) <= max(2, case["P"] // 1000)
    ml, out = _model(cam, leaves, rs, bgt, radii, W, H, D)
    assert torch.equal(out["radii"].to(radii.device), radii.long())
    _check_images(torch.cat([color, allmap]), torch.cat([out["color"], out["allmap"]]), out["events"])
    ref = sm.grads(out, ml, gc.double(), ga.double(), W=W, H=H)
    for k, v in g.items():
        assert torch.isfinite(v).all(), k
        assert _rel(v, ref[k]) < 1e-3, f"grad {k}: rel L2 {_rel(v, ref[k]):.3g}"


@pytest.mark.parametrize("channel", ["color"] + [f"allmap{c}" for c in range(7)])
def test_surfel_single_output_losses(channel):
    W, H, D = 96, 64, 2
    cam, leaves, rs, bgt = _setup(W, H, 800, D, seed=11)
    gen = torch.Generator().manual_seed(7)
    gc = ga = None
    if channel == "color":
        gc = torch.randn(3, H, W, generator=gen).to(DEV)
    else:
        ga = torch.zeros(7, H, W)
        ga[int(channel[-1])] = torch.randn(H, W, generator=gen)
        ga = ga.to(DEV)
    color, radii, allmap, g = _grads(leaves, rs, gc, None if ga is None else ga)
    ml, out = _model(cam, leaves, rs, bgt, radii, W, H, D)
    ref = sm.grads(out, ml, None if gc is None else gc.double(), None if ga is None else ga.double(), W=W, H=H)
    # a gradient that is zero in exact arithmetic (the median depth along a pixel ray does not depend on the in-plane scales, nor on
    # opacities) is measured on the scale of the geometry gradients of the same loss, not against its own rounding noise
    floor = 1e-3 * max(float(ref[k].norm()) for k in ("means3D", "scales", "rotations"))
    for k, v in g.items():
        if float(ref[k].norm()) == 0.0:
            assert float(v.abs().max()) == 0.0, k
        else:
            err = float((v.double() - ref[k]).norm()) / max(float(ref[k].norm()), floor)
            assert err < 1e-3, f"{channel}: grad {k}: rel L2 {err:.3g}"


@pytest.mark.parametrize("fast_exp", [False, True])
def test_surfel_backward_is_bit_identical(fast_exp):
    import gaustudio_amd
    W, H, D = 256, 160, 3
    cam, leaves, rs, bgt = _setup(W, H, 5000, D, seed=3)
    gen = torch.Generator().manual_seed(9)
    gc, ga = torch.randn(3, H, W, generator=gen).to(DEV), torch.randn(7, H, W, generator=gen).to(DEV)
    with gaustudio_amd.options(fast_exp=fast_exp):
        runs = [_grads(leaves, rs, gc, ga) for _ in range(2)]
    for k in runs[0][3]:
        assert torch.equal(runs[0][3][k], runs[1][3][k]), k
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])


def test_surfel_1080p_1M_forward_backward_finite():
    W, H = 1920, 1080
    cam = scenes.make_camera(W, H)
    sc = scenes.make_scene(1_000_000, cam, seed=1, sigma_px_median=1.5)
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in dict(
        means3D=sc.means3D, opacities=sc.opacities, scales=sc.scales[:, :2].contiguous(), rotations=sc.rotations, shs=sc.shs).items()}
    from diff_surfel_rasterization import GaussianRasterizationSettings
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=DEV), 1.0, cam.viewmatrix.to(DEV),
                                       cam.projmatrix.to(DEV), 3, cam.campos.to(DEV), False, False)
    color, radii, allmap, means2D = _run(leaves, rs)
    (color.sum() + allmap.sum()).backward()
    torch.cuda.synchronize()
    assert int((radii > 0).sum()) > 500_000
    assert torch.isfinite(color).all() and torch.isfinite(allmap).all()
    assert float(allmap[1].detach().max()) > 0.9
    for k, v in leaves.items():
        assert torch.isfinite(v.grad).all(), k
    assert torch.isfinite(means2D.grad).all()


def test_surfel_mark_visible_and_empty():
    from diff_surfel_rasterization import GaussianRasterizer
    W, H = 64, 48
    cam, leaves, rs, bgt = _setup(W, H, 100, 0)
    vis = GaussianRasterizer(rs).markVisible(leaves["means3D"].detach())
    assert vis.dtype == torch.bool and bool(vis.all())
    e = {k: v[:0].detach().requires_grad_(True) for k, v in leaves.items()}
    color, radii, allmap, _ = _run(e, rs)
    assert color.shape == (3, H, W) and allmap.shape == (7, H, W) and radii.numel() == 0
    assert float(color.detach().abs().max()) == 0.0 and float(allmap.detach().abs().max()) == 0.0
