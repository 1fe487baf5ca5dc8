"""CPU: the float64 surfel model (tests/surfel_model.py) against closed forms, and the Python boundary of
diff_surfel_rasterization (argument validation before any native call, the settings fields)."""
import math

import pytest
import torch

import surfel_model as sm
from gaustudio_amd import scenes

W = H = 33          # odd: the splat centre (0, 0, z) projects onto pixel (16, 16) exactly
CX = CY = 16


def _cam():
    return scenes.make_camera(W, H, fovx_deg=60.0)


def _render(means, opac, scales, rots, colors, bg=(0.0, 0.0, 0.0)):
    cam = _cam()
    d = torch.float64
    return sm.render(torch.tensor(means, dtype=d), torch.tensor(opac, dtype=d).reshape(-1, 1), torch.tensor(scales, dtype=d),
                     torch.tensor(rots, dtype=d), cam.viewmatrix, cam.projmatrix, cam.campos, W, H, torch.tensor(bg, dtype=d),
                     colors_precomp=torch.tensor(colors, dtype=d))


def _m(z):
    return sm.FAR / (sm.FAR - sm.NEAR) * (1 - sm.NEAR / z)


@pytest.mark.parametrize("o", [0.4, 0.995])
def test_fronto_parallel_splat(o):
    z0 = 5.0
    out = _render([[0.0, 0.0, z0]], [o], [[0.3, 0.2]], [[1.0, 0.0, 0.0, 0.0]], [[0.2, 0.5, 0.9]], bg=(1.0, 1.0, 1.0))
    a = min(0.99, o)
    am = out["allmap"][:, CY, CX]
    assert am[1].item() == pytest.approx(a, abs=1e-12)
    assert am[0].item() == pytest.approx(a * z0, rel=1e-12)
    assert am[2:5].tolist() == pytest.approx([0.0, 0.0, -a], abs=1e-12)      # normal (0, 0, -1), weighted
    assert am[5].item() == pytest.approx(z0, rel=1e-12)                      # median: entered with T = 1 > 0.5
    assert am[6].item() == pytest.approx(0.0, abs=1e-15)                     # one splat: no distortion
    assert out["color"][:, CY, CX].tolist() == pytest.approx([a * c + (1 - a) for c in (0.2, 0.5, 0.9)], rel=1e-12)
    assert int(out["radii"][0]) > 0


def test_two_splats_distortion():
    z1, z2, o1, o2 = 4.0, 7.0, 0.5, 0.7
    out = _render([[0.0, 0.0, z1], [0.0, 0.0, z2]], [o1, o2], [[0.3, 0.3], [0.3, 0.3]], [[1.0, 0, 0, 0], [1.0, 0, 0, 0]],
                  [[1.0, 0, 0], [0, 1.0, 0]])
    w1, w2 = o1, o2 * (1 - o1)
    am = out["allmap"][:, CY, CX]
    assert am[6].item() == pytest.approx(w1 * w2 * (_m(z1) - _m(z2)) ** 2, rel=1e-10)
    assert am[0].item() == pytest.approx(w1 * z1 + w2 * z2, rel=1e-12)
    assert am[1].item() == pytest.approx(1 - (1 - o1) * (1 - o2), rel=1e-12)


@pytest.mark.parametrize("o1,expect_first", [(0.3, False), (0.6, True)])
def test_median_rule(o1, expect_first):
    z1, z2 = 4.0, 7.0
    out = _render([[0.0, 0.0, z1], [0.0, 0.0, z2]], [o1, 0.5], [[0.3, 0.3], [0.3, 0.3]], [[1.0, 0, 0, 0], [1.0, 0, 0, 0]],
                  [[1.0, 0, 0], [0, 1.0, 0]])
    # the second splat is entered with T = 1 - o1: it becomes the median only while that is still > 0.5
    assert out["allmap"][5, CY, CX].item() == pytest.approx(z1 if expect_first else z2, rel=1e-12)


def test_edge_on_splat_takes_the_low_pass_branch():
    z0, o = 5.0, 0.8
    t = math.radians(89.9) / 2      # rotation about x by 89.9 degrees: the surfel plane almost contains the view rays
    out = _render([[0.0, 0.0, z0]], [o], [[0.3, 0.3]], [[math.cos(t), math.sin(t), 0.0, 0.0]], [[1.0, 1.0, 1.0]])
    cam = _cam()
    M, _ = sm.splat_matrix(torch.tensor([[0.0, 0.0, z0]], dtype=torch.float64), torch.tensor([[0.3, 0.3]], dtype=torch.float64),
                           torch.tensor([[math.cos(t), math.sin(t), 0.0, 0.0]], dtype=torch.float64), 1.0,
                           cam.projmatrix.to(torch.float64), W, H)
    Tu, Tv, Tw = M[0]
    x, y = float(CX), float(CY + 1)     # one pixel off the centre across the (edge-on) v axis
    k, l = x * Tw - Tu, y * Tw - Tv
    q = torch.cross(k, l, dim=0)
    u, v = q[0] / q[2], q[1] / q[2]
    rho3 = float(u * u + v * v)
    f = torch.tensor([9.0, 9.0, -1.0], dtype=torch.float64) / (Tw * Tw * torch.tensor([9.0, 9.0, -1.0], dtype=torch.float64)).sum()
    cx, cy = float((f * Tu * Tw).sum()), float((f * Tv * Tw).sum())
    rho2 = 2.0 * ((cx - x) ** 2 + (cy - y) ** 2)
    assert rho2 < rho3                                   # the ray meets the plane far outside the splat: low-pass wins
    a = o * math.exp(-0.5 * rho2)
    am = out["allmap"][:, CY + 1, CX]
    assert am[1].item() == pytest.approx(a, rel=1e-9)
    assert (am[0] / am[1]).item() == pytest.approx(float(Tw[2]), rel=1e-9)   # depth = Tw.z in the low-pass branch


def test_model_gradients_reach_every_input():
    cam = scenes.make_camera(48, 32)
    sc = scenes.make_scene(40, cam, seed=3, sigma_px_median=3.0)
    d = torch.float64
    leaves = dict(means3D=sc.means3D.to(d).requires_grad_(), opacities=sc.opacities.to(d).requires_grad_(),
                  scales=sc.scales[:, :2].to(d).contiguous().requires_grad_(), rotations=sc.rotations.to(d).requires_grad_(),
                  shs=sc.shs.to(d).requires_grad_())
    out = sm.render(leaves["means3D"], leaves["opacities"], leaves["scales"], leaves["rotations"], cam.viewmatrix, cam.projmatrix,
                    cam.campos, 48, 32, torch.zeros(3, dtype=d), sh_degree=3, shs=leaves["shs"])
    g = sm.grads(out, leaves, torch.ones(3, 32, 48, dtype=d), torch.ones(7, 32, 48, dtype=d), W=48, H=32)
    for k in ("means3D", "opacities", "scales", "rotations", "shs", "means2D"):
        assert torch.isfinite(g[k]).all() and g[k].abs().sum() > 0, k
    assert (g["means2D"][:, 2] == 0).all()


# ---- the Python boundary of diff_surfel_rasterization (no GPU needed: validation runs before any native call) ----
def _rasterizer():
    from diff_surfel_rasterization import GaussianRasterizationSettings as S, GaussianRasterizer
    return GaussianRasterizer(S(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False))


def test_settings_fields_and_public_names():
    import diff_surfel_rasterization as d
    assert d.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix", "sh_degree",
        "campos", "prefiltered", "debug")
    for fn in ("rasterize_surfels", "rasterize_surfels_backward", "mark_visible"):
        assert callable(getattr(d._C, fn))
    assert hasattr(d.GaussianRasterizer, "markVisible")


def test_argument_validation():
    r = _rasterizer()
    m, o = torch.zeros(2, 3), torch.zeros(2, 1)
    s2, q = torch.ones(2, 2), torch.ones(2, 4)
    with pytest.raises(Exception, match="exactly one of either SHs or precomputed colors"):
        r(m, m, o, scales=s2, rotations=q)
    with pytest.raises(Exception, match="exactly one of either SHs or precomputed colors"):
        r(m, m, o, shs=torch.zeros(2, 1, 3), colors_precomp=torch.zeros(2, 3), scales=s2, rotations=q)
    with pytest.raises(ValueError, match=r"scales must be \[P,2\]"):
        r(m, m, o, shs=torch.zeros(2, 1, 3), scales=torch.ones(2, 3), rotations=q)
    with pytest.raises(ValueError, match=r"rotations must be \[P,4\]"):
        r(m, m, o, shs=torch.zeros(2, 1, 3), scales=s2, rotations=torch.ones(2, 3))
    with pytest.raises(ValueError, match="scales .* and rotations .* are required"):
        r(m, m, o, shs=torch.zeros(2, 1, 3), scales=s2)


def test_cov3D_precomp_is_refused():
    r = _rasterizer()
    m, o = torch.zeros(2, 3), torch.zeros(2, 1)
    with pytest.raises(ValueError, match=r"cov3D_precomp is not supported.*\(2, 6\).*3D-Gaussian covariance"):
        r(m, m, o, colors_precomp=torch.zeros(2, 3), cov3D_precomp=torch.zeros(2, 6))


# ---- n_contrib, stopped and the float32 mode (used by the scene preconditions and the per-surfel tolerance) ----
def test_two_splats_n_contrib_and_stopped():
    out = _render([[0.0, 0.0, 4.0], [0.0, 0.0, 7.0]], [0.5, 0.7], [[0.3, 0.3], [0.3, 0.3]], [[1.0, 0, 0, 0], [1.0, 0, 0, 0]],
                  [[1.0, 0, 0], [0, 1.0, 0]])
    nc, st = out["n_contrib"], out["stopped"]
    assert nc.dtype == torch.int64 and st.dtype == torch.bool and nc.shape == (H, W) == st.shape
    assert int(nc[CY, CX]) == 2 and not bool(st.any())           # both contribute at the centre; T never nears 1e-4
    assert int(nc[0, 0]) == 0                                     # a corner far outside both footprints (the tile lists hold them)
    assert set(nc.unique().tolist()) <= {0, 1, 2}
    assert bool(((nc > 0) == (out["allmap"][1] > 0)).all())
    assert out["rects"].shape == (2, 4) and bool((out["rects"][:, 2] > out["rects"][:, 0]).all())


def test_stop_rule_sets_stopped_and_ends_n_contrib():
    # four splats of alpha 0.99 at the centre: T = 1e-2, 1e-4, then T (1 - alpha) = 1e-6 < 1e-4 at the third: the walk stops there,
    # the third and fourth do not contribute
    z = [3.0, 4.0, 5.0, 6.0]
    out = _render([[0.0, 0.0, v] for v in z], [1.0] * 4, [[0.3, 0.3]] * 4, [[1.0, 0, 0, 0]] * 4, [[1.0, 0, 0]] * 4)
    assert int(out["n_contrib"][CY, CX]) == 2 and bool(out["stopped"][CY, CX])
    assert out["allmap"][1, CY, CX].item() == pytest.approx(1 - 0.01 * 0.01, rel=1e-12)
    assert not bool(out["stopped"][0, 0])


@pytest.mark.parametrize("o1,expect_first", [(0.3, False), (0.6, True)])
def test_median_rule_n_contrib_and_float32_mode(o1, expect_first):
    args = ([[0.0, 0.0, 4.0], [0.0, 0.0, 7.0]], [o1, 0.5], [[0.3, 0.3], [0.3, 0.3]], [[1.0, 0, 0, 0], [1.0, 0, 0, 0]], [[1.0, 0, 0], [0, 1.0, 0]])
    out = _render(*args)
    assert int(out["n_contrib"][CY, CX]) == 2 and not bool(out["stopped"].any())    # the median moves, the last contributor does not
    cam = _cam()
    f = torch.float32
    t = [torch.tensor(a, dtype=f) for a in args]
    o32 = sm.render(t[0], t[1].reshape(-1, 1), t[2], t[3], cam.viewmatrix, cam.projmatrix, cam.campos, W, H, torch.zeros(3, dtype=f),
                    colors_precomp=t[4], dtype=f)
    assert o32["color"].dtype == f and o32["allmap"].dtype == f and o32["M"].dtype == f
    assert torch.equal(o32["n_contrib"], out["n_contrib"]) and torch.equal(o32["radii"], out["radii"])
    assert o32["allmap"][5, CY, CX].item() == pytest.approx(4.0 if expect_first else 7.0, rel=1e-6)
    d = (o32["allmap"].double() - out["allmap"]).abs().max().item()
    assert 0 < d < 1e-5                                           # float32 arithmetic: close, and not the float64 result recast
