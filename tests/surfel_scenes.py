"""TEST INFRASTRUCTURE: the scenes of tests/test_gpu_surfel_edges.py, plain torch/numpy on the CPU.  tests/test_surfel_scenes.py
runs the float64 model (surfel_model.py) alone on them and asserts the precondition that makes each GPU test meaningful; the
seeds below were chosen so that those preconditions hold (the event share of surfel_model._composite, the walk lengths).

A scene is a SurfelScene: the camera, float32 leaves (means3D, opacities [P,1], scales [P,2], rotations [P,4], shs [P,16,3] or
colors_precomp [P,3]), the SH degree, the background and `groups`, name -> index tensor, for the tests that look at one kind.

Why the long-list scenes look the way they do.  A threshold event of the model is a pixel within 1e-3 of a decision; a smooth
Gaussian footprint of pixel sigma s crosses alpha = 1/255 on a contour whose event band has the area pi s^2 4e-3, whatever its
opacity, and T = 0.5 likewise: a tile list of a thousand ordinary surfels has several event pixels at any seed, and in a
one-tile image one event pixel takes every surfel out of the per-surfel gradient check.  So these scenes are built from two
kinds whose alpha does not vary smoothly over the image:
  flat    a surfel facing the camera with a sigma of 2000-4000 pixels: G is 1 to within 1e-4 over the image, so every pixel's T
          crosses 0.5 at the same entry and by the same step (the ray-splat
          branch, every pixel), so alpha ~ o and the opacity ranges of the issue keep it off 1/255;
  blade   scales (0.05, 400) pixels, centred on one of two pixel CORNERS, the long axis along y to within 0.01 rad: no pixel
          centre comes within 0.4 pixel of the line, so every pixel takes the low-pass branch with G = exp(-d^2), d its distance
          from the corner -- the same four pixels around it for every blade, at G = exp(-0.5) -- or sees nothing.  The rect is
          still the whole image.  Opacities that would bring G o within 1 % of 1/255 are redrawn (_opacity_mix).
The flats give every pixel a walk to the end of the list (sum of alpha ~ 3), the blades end the walk of the four pixels around
each corner after a few hundred entries."""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from gaustudio_amd import scenes

ALPHA_MIN = 1.0 / 255.0


class SurfelScene(NamedTuple):
    cam: scenes.Cam
    W: int
    H: int
    leaves: dict            # name -> float32 CPU tensor
    D: int
    bg: torch.Tensor        # [3]
    groups: dict            # name -> int64 index tensor


def _leaves(means, opac, scales2, rot, shs=None, precomp=None):
    d = dict(means3D=means, opacities=opac.reshape(-1, 1), scales=scales2, rotations=rot)
    if precomp is not None:
        d["colors_precomp"] = precomp
    else:
        d["shs"] = shs
    return {k: v.float().contiguous() for k, v in d.items()}


def _shs(P, g):
    shs = torch.randn(P, 16, 3, generator=g) * 0.1
    shs[:, 0, :] = (torch.rand(P, 3, generator=g) * 2 - 1) / 0.28209479177387814
    return shs


def _unproject(cam, W, H, cx, cy, z):
    """World point (camera at the origin, looking down +z) that projects onto pixel coordinates (cx, cy) at view depth z."""
    return torch.stack([z * cam.tanfovx * (cx - (W - 1) / 2) * 2 / W, z * cam.tanfovy * (cy - (H - 1) / 2) * 2 / H, z], 1)


def _px(cam, W, z):
    """World length of one pixel at view depth z."""
    return z * 2 * cam.tanfovx / W


BG = torch.tensor([0.2, 0.4, 0.7])


# ---- (a) ragged images -----------------------------------------------------------------------------------------------------
# (W, H) -> P, SH degree (None: colors_precomp), sigma in pixels, opacity scale, spread, seed
RAGGED = {
    (1, 1): dict(P=50, D=0, sigma=1.0, oscale=0.1, spread=3.0, seed=0),
    (15, 16): dict(P=300, D=3, sigma=0.8, oscale=0.45, spread=2.5, seed=2),
    (17, 33): dict(P=300, D=1, sigma=1.0, oscale=0.45, spread=2.0, seed=19),
    (31, 47): dict(P=300, D=None, sigma=1.0, oscale=0.45, spread=2.0, seed=3),
    (129, 65): dict(P=400, D=2, sigma=1.0, oscale=0.45, spread=1.6, seed=2),
}


def ragged(W, H, seed=None):
    """A scenes.make_scene cloud on an image that is no multiple of the tile.  Opacities are scaled below 0.5 (a single surfel
    does not cross T = 0.5 on a contour of its own), and the cloud is drawn for a frustum `spread` times as wide as the
    camera's: fewer surfels lie in the image (the event share), more of them straddle its border (what the case is about)."""
    c = RAGGED[(W, H)]
    cam = scenes.make_camera(W, H)
    wide = cam._replace(tanfovx=cam.tanfovx * c["spread"], tanfovy=cam.tanfovy * c["spread"])
    sc = scenes.make_scene(c["P"], wide, seed=c["seed"] if seed is None else seed, sigma_px_median=c["sigma"] / c["spread"])
    D = c["D"]
    lv = _leaves(sc.means3D, sc.opacities * c["oscale"], sc.scales[:, :2], sc.rotations * 1.7, shs=sc.shs,
                 precomp=torch.sigmoid(sc.shs[:, 0, :]) if D is None else None)
    return SurfelScene(cam, W, H, lv, 0 if D is None else D, BG.clone(), {})


# ---- (b), (d) long lists ----------------------------------------------------------------------------------------------------
# seeds per (W, H, P, ties): chosen event-free (tests/test_surfel_scenes.py asserts it)
LONG_SEEDS = {(16, 16, 255, False): 1, (16, 16, 257, False): 1, (16, 16, 1023, False): 5, (16, 16, 8193, False): 2,
              (16, 16, 9000, False): 1, (16, 16, 8200, True): 4}      # (every other case: seed 0)
LONG_P_16 = [255, 256, 257, 288, 1023, 1024, 1025, 1500, 8192, 8193, 9000]
TIE_P = [300, 1100, 8200]


def _opacity_mix(P, g, forbidden_G=()):
    """About a third in [0.002, 0.0039] (below 1/255: never contribute), the rest in [0.004, 0.05]; values whose product with one
    of `forbidden_G` is within 1 % of 1/255 are redrawn, and so are those that would contribute at all through a G < 0.3 (the
    second ring of pixels around a blade centre, G = 0.082: it would take steps of 0.002 through T = 0.5, a certain event)."""
    low = torch.rand(P, generator=g) < 1.0 / 3.0
    o = torch.where(low, 0.002 + 0.0019 * torch.rand(P, generator=g), 0.004 + 0.046 * torch.rand(P, generator=g))
    for _ in range(64):
        bad = torch.zeros(P, dtype=torch.bool)
        for G in forbidden_G:
            bad |= (o * G > 0.99 * ALPHA_MIN) if G < 0.3 else ((o * G / ALPHA_MIN - 1).abs() < 0.01)
        bad &= ~low
        if not bad.any():
            break
        o = torch.where(bad, 0.004 + 0.046 * torch.rand(P, generator=g), o)
    assert not bad.any()
    return o, low


def blade_G(c0):
    """exp(-d^2) of the pixels around c0 that a blade of opacity <= 0.05 can reach (alpha >= 1/255 needs G >= 0.078)."""
    out = {}
    for ix in range(int(c0[0]) - 2, int(c0[0]) + 4):
        for iy in range(int(c0[1]) - 2, int(c0[1]) + 4):
            G = math.exp(-((ix - c0[0]) ** 2 + (iy - c0[1]) ** 2))
            if G * 0.05 >= ALPHA_MIN * 0.9:
                out[(ix, iy)] = G
    return out


def long_list(W, H, P, seed=None, ties=False):
    """Every rect covers the whole image; flats and blades (module docstring).  `ties`: groups of 10 share one means3D row
    (so one sort key), and within a group colour, opacity, scales and rotation differ."""
    if seed is None:
        seed = LONG_SEEDS.get((W, H, P, ties), 0)
    g = torch.Generator().manual_seed(1000 * seed + P)
    cam = scenes.make_camera(W, H)
    # blade centres on pixel corners: four pixels at d^2 = 0.5 each (G = 0.607), the next ring at d^2 = 2.5 (G = 0.082)
    c0, c1 = ((W - 1.5, H - 1.5), (15.5, 8.5)) if W > 16 else ((8.5, 8.5), (3.5, 12.5))    # W > 16: c0's pixels lie in four tiles
    n_flat = min(P // 2, 200)
    nrow = P // 10 if ties else P
    assert not ties or P % 10 == 0
    row_flat = torch.zeros(nrow, dtype=torch.bool)
    row_flat[torch.randperm(nrow, generator=g)[:max(1, n_flat * nrow // P)]] = True
    z = 2.0 + 18.0 * torch.rand(nrow, generator=g)
    second = torch.rand(nrow, generator=g) < 0.3
    cx = torch.where(row_flat, torch.rand(nrow, generator=g) * W - 0.37, torch.where(second, c1[0], c0[0]))
    cy = torch.where(row_flat, torch.rand(nrow, generator=g) * H - 0.41, torch.where(second, c1[1], c0[1]))
    means_rows = _unproject(cam, W, H, cx.double(), cy.double(), z.double()).float()
    rep = 10 if ties else 1
    means = means_rows.repeat_interleave(rep, 0)
    flat = row_flat.repeat_interleave(rep, 0)
    zz = z.repeat_interleave(rep, 0)
    px = _px(cam, W, zz)
    s_flat = (2000.0 + 2000.0 * torch.rand(P, 2, generator=g)) * px[:, None]
    s_blade = torch.stack([torch.full((P,), 0.05), 300.0 + 200.0 * torch.rand(P, generator=g)], 1) * px[:, None]
    scales2 = torch.where(flat[:, None], s_flat, s_blade)
    # (a flat leans by less than 1e-3 rad: 3 sigma of it must stay in front of the camera plane, or the footprint is no ellipse)
    phi = torch.rand(P, generator=g) * (2 * math.pi)
    q_flat = torch.stack([torch.cos(phi / 2), 1e-4 * torch.randn(P, generator=g), 1e-4 * torch.randn(P, generator=g), torch.sin(phi / 2)], 1)
    th = (torch.rand(P, generator=g) * 2 - 1) * 0.01
    q_blade = torch.stack([torch.cos(th / 2), torch.zeros(P), torch.zeros(P), torch.sin(th / 2)], 1)
    rot = torch.where(flat[:, None], q_flat, q_blade) * (0.5 + torch.rand(P, 1, generator=g))
    o, low = _opacity_mix(P, g, forbidden_G=sorted(set(round(v, 6) for v in blade_G(c0).values())) + [1.0])
    lv = _leaves(means, o, scales2, rot, shs=_shs(P, g))
    groups = dict(flat=torch.nonzero(flat)[:, 0], blade=torch.nonzero(~flat)[:, 0], low=torch.nonzero(low)[:, 0])
    return SurfelScene(cam, W, H, lv, 1, BG.clone(), groups)


# ---- (c) near plane and culls -----------------------------------------------------------------------------------------------
NEAR_SEED = 19
NEAR_W, NEAR_H = 80, 48


def _rand_q(n, g):
    q = torch.randn(n, 4, generator=g)
    return q / q.norm(dim=1, keepdim=True)


def near_and_culls(seed=None, counts=None):
    """80 x 48: a plain make_scene(zmin=0.5) background plus the groups of the issue's item (c).  `counts` overrides the group
    sizes (name -> n)."""
    seed = NEAR_SEED if seed is None else seed
    W, H = NEAR_W, NEAR_H
    cam = scenes.make_camera(W, H)
    g = torch.Generator().manual_seed(7000 + seed)
    n = dict(background=300, z_span=30, z_ulp=21, near_tilted=4, behind=30, offscreen=30, tiny=20, whole_grid=2, opaque=20,
             faint=30, quat_big=20, quat_small=20, edge_on=20)
    n.update(counts or {})
    parts, groups, at = [], {}, 0

    def add(name, means, opac, scales2, rot):
        nonlocal at
        k = means.shape[0]
        parts.append((means.float(), opac.float().reshape(-1, 1), scales2.float(), rot.float()))
        groups[name] = torch.arange(at, at + k)
        at += k

    def cloud(k, zlo, zhi, sigma_px=0.35):
        z = zlo + (zhi - zlo) * torch.rand(k, generator=g)
        cx, cy = torch.rand(k, generator=g) * W - 0.5, torch.rand(k, generator=g) * H - 0.5
        s = sigma_px * _px(cam, W, z)[:, None] * (0.6 + 0.8 * torch.rand(k, 2, generator=g))
        return _unproject(cam, W, H, cx, cy, z), s

    bgs = scenes.make_scene(n["background"], cam, seed=seed, sigma_px_median=0.35, sigma_px_logstd=0.3, zmin=0.5)
    add("background", bgs.means3D, bgs.opacities * 0.45, bgs.scales[:, :2], bgs.rotations * 1.7)
    faint = lambda k: 0.05 + 0.4 * torch.rand(k, generator=g)
    # view z in [0.15, 0.25]: spans the cull pv.z <= 0.2 (not within 0.01 of it: a visible surfel there is an event of every pixel
    # it covers; the z_ulp group below probes the cull at the plane itself)
    m, s = cloud(n["z_span"], 0.15, 0.25)
    close = (m[:, 2] - 0.2).abs() < 0.01
    m[close] = m[close] * ((0.2 + 0.01 * torch.sign(m[close, 2] - 0.2 + 1e-9)) / m[close, 2])[:, None]
    add("z_span", m, faint(len(m)), s, _rand_q(len(m), g))
    # view z exactly 0.2 (float32) and one ulp either side
    k = n["z_ulp"] // 3
    near32 = np.float32(0.2)
    zs = np.concatenate([np.full(k, np.nextafter(near32, np.float32(0))), np.full(k, near32), np.full(k, np.nextafter(near32, np.float32(1)))])
    zt = torch.tensor(zs, dtype=torch.float32)
    m = _unproject(cam, W, H, (torch.rand(3 * k, generator=g) * W).double(), (torch.rand(3 * k, generator=g) * H).double(), zt.double())
    m = m.float()
    m[:, 2] = zt
    # (opacity below half of 1/255: the group probes the cull, radii 0 or not; visible at the plane it would be all events)
    add("z_ulp", m, torch.full((3 * k,), 0.0019), 0.6 * _px(cam, W, zt)[:, None] * torch.ones(3 * k, 2), _rand_q(3 * k, g))
    # large, steeply tilted surfels at z in [0.3, 0.6]: the ray depth falls below 0.2 over part of the footprint
    k = n["near_tilted"]
    # (the long axis is sized so that 3 sigma of it stays in front of the camera plane: z - 3 s_u sin(tilt) = 0.08)
    z = 0.35 + 0.15 * torch.rand(k, generator=g)
    m = _unproject(cam, W, H, W * (0.2 + 0.6 * torch.rand(k, generator=g)), H * (0.2 + 0.6 * torch.rand(k, generator=g)), z)
    tilt = math.radians(75.0) + math.radians(10.0) * torch.rand(k, generator=g)
    q = torch.stack([torch.cos(tilt / 2), torch.zeros(k), torch.sin(tilt / 2), torch.zeros(k)], 1)     # about y: t_u leans into z
    add("near_tilted", m, 0.15 + 0.3 * torch.rand(k, generator=g),
        torch.stack([(z - 0.08) / (3.0 * torch.sin(tilt)), (4.0 + 4.0 * torch.rand(k, generator=g)) * _px(cam, W, z)], 1), q)
    # behind the camera
    m, s = cloud(n["behind"], -10.0, -0.5)
    add("behind", m, faint(len(m)), s.abs(), _rand_q(len(m), g))
    # in front, but off-screen: an empty rect
    k = n["offscreen"]
    z = 2.0 + 8.0 * torch.rand(k, generator=g)
    side = torch.rand(k, generator=g) < 0.5
    cx = torch.where(side, -40.0 - 100 * torch.rand(k, generator=g), W + 40.0 + 100 * torch.rand(k, generator=g))
    m = _unproject(cam, W, H, cx, torch.rand(k, generator=g) * H, z)
    add("offscreen", m, faint(k), 0.6 * _px(cam, W, z)[:, None] * torch.ones(k, 2), _rand_q(k, g))
    # scales 1e-4: the extent floor, the low-pass branch everywhere
    m, _ = cloud(n["tiny"], 2.0, 10.0)
    add("tiny", m, faint(len(m)), torch.full((len(m), 2), 1e-4), _rand_q(len(m), g))
    # one rect = the whole 5 x 3 tile grid; faint and flat (sigma >= 300 pixels), so that alpha does not cross 1/255 in the image
    k = n["whole_grid"]
    z = 3.0 + 5.0 * torch.rand(k, generator=g)
    m = _unproject(cam, W, H, torch.rand(k, generator=g) * W, torch.rand(k, generator=g) * H, z)
    add("whole_grid", m, 0.02 + 0.03 * torch.rand(k, generator=g), (300.0 + 200.0 * torch.rand(k, 2, generator=g)) * _px(cam, W, z)[:, None],
        torch.cat([torch.ones(k, 1), 0.002 * torch.randn(k, 2, generator=g), torch.randn(k, 1, generator=g)], 1))
    # opacity exactly 1: the 0.99 clamp
    # (centred 0.06 pixel off a pixel centre: that pixel has G = 0.993 > 0.99, clamped and clear of the clamp's event band, the
    # next ones G <= 0.41)
    k = n["opaque"]
    z = 2.0 + 10.0 * torch.rand(k, generator=g)
    cx, cy = torch.floor(torch.rand(k, generator=g) * W) + 0.05, torch.floor(torch.rand(k, generator=g) * H) + 0.03
    add("opaque", _unproject(cam, W, H, cx, cy, z), torch.ones(k), 0.35 * _px(cam, W, z)[:, None] * (0.6 + 0.8 * torch.rand(k, 2, generator=g)),
        _rand_q(k, g))
    # opacity 0.003 < 1/255: binned, never contributes
    m, s = cloud(n["faint"], 1.0, 8.0, sigma_px=3.0)
    add("faint", m, torch.full((len(m),), 0.003), s, _rand_q(len(m), g))
    # quaternions of norm 1e3 and 1e-3
    m, s = cloud(n["quat_big"], 2.0, 12.0)
    add("quat_big", m, faint(len(m)), s, _rand_q(len(m), g) * 1e3)
    m, s = cloud(n["quat_small"], 2.0, 12.0)
    add("quat_small", m, faint(len(m)), s, _rand_q(len(m), g) * 1e-3)
    # tilted to within 1e-3 rad of edge-on (the normal perpendicular to the view ray through the centre)
    k = n["edge_on"]
    z = 2.0 + 10.0 * torch.rand(k, generator=g)
    m = _unproject(cam, W, H, torch.rand(k, generator=g) * W, torch.rand(k, generator=g) * H, z).double()
    ray = m / m.norm(dim=1, keepdim=True)
    a = torch.linalg.cross(ray, torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float64).expand_as(ray))
    a = a / a.norm(dim=1, keepdim=True)
    eps = (torch.rand(k, generator=g).double() * 2 - 1) * 1e-3
    nrm = a * torch.cos(eps)[:, None] + ray * torch.sin(eps)[:, None]          # within 1e-3 rad of perpendicular to the ray
    tu = ray - (ray * nrm).sum(1, keepdim=True) * nrm
    tu = tu / tu.norm(dim=1, keepdim=True)
    tv = torch.linalg.cross(nrm, tu)
    add("edge_on", m, faint(k), 0.6 * _px(cam, W, z)[:, None] * (0.6 + 0.8 * torch.rand(k, 2, generator=g)),
        _quat_from_R(torch.stack([tu, tv, nrm], 1)))      # (rotmat_columns: t_u, t_v, t_n are the ROWS of the usual R(q))
    means, opac, scales2, rot = (torch.cat([p[i] for p in parts]) for i in range(4))
    P = means.shape[0]
    lv = _leaves(means, opac, scales2, rot, shs=_shs(P, g))
    return SurfelScene(cam, W, H, lv, 2, BG.clone(), groups)


def _quat_from_R(R):
    """(r, x, y, z) of rotation matrices R [n,3,3] (columns t_u, t_v, t_n), float64."""
    out = []
    for M in R.numpy():
        t = np.trace(M)
        if t > 0:
            s = math.sqrt(t + 1.0) * 2
            q = [0.25 * s, (M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s]
        else:
            i = int(np.argmax(np.diag(M)))
            j, k = (i + 1) % 3, (i + 2) % 3
            s = math.sqrt(1.0 + M[i, i] - M[j, j] - M[k, k]) * 2
            q = [0.0, 0.0, 0.0, 0.0]
            q[0] = (M[k, j] - M[j, k]) / s
            q[1 + i] = 0.25 * s
            q[1 + j] = (M[j, i] + M[i, j]) / s
            q[1 + k] = (M[k, i] + M[i, k]) / s
        out.append(q)
    return torch.tensor(np.array(out), dtype=torch.float64)


# ---- (e) permutation and padding --------------------------------------------------------------------------------------------
PERM_P = [255, 256, 257, 513]


def plain(W, H, P, seed=0, D=3):
    """The cloud of test_gpu_surfel.py's _setup."""
    cam = scenes.make_camera(W, H)
    sc = scenes.make_scene(P, cam, seed=seed, sigma_px_median=3.0)
    lv = _leaves(sc.means3D, sc.opacities, sc.scales[:, :2], sc.rotations * 1.7, shs=sc.shs)
    return SurfelScene(cam, W, H, lv, D, BG.clone(), {})


def culled_padding(sc: SurfelScene, n=300, seed=0):
    """n surfels that are all culled: a third behind the camera, a third at view z <= 0.2, a third with an empty rect."""
    g = torch.Generator().manual_seed(90 + seed)
    cam, W, H = sc.cam, sc.W, sc.H
    k = n // 3
    z = torch.cat([-0.5 - 10 * torch.rand(k, generator=g), 0.01 + 0.19 * torch.rand(k, generator=g), 2.0 + 8.0 * torch.rand(n - 2 * k, generator=g)])
    cx = torch.rand(n, generator=g) * W
    cx[2 * k:] = W + 60.0 + 100 * torch.rand(n - 2 * k, generator=g)
    m = _unproject(cam, W, H, cx, torch.rand(n, generator=g) * H, z)
    lv = _leaves(m, 0.1 + 0.8 * torch.rand(n, generator=g), 0.6 * _px(cam, W, z.abs())[:, None] * torch.ones(n, 2), _rand_q(n, g), shs=_shs(n, g))
    return lv


def view_keys(sc: SurfelScene):
    """The float32 sort keys (surfel_model._view_z_f32)."""
    import surfel_model as sm
    return sm._view_z_f32(sc.leaves["means3D"].numpy(), sc.cam.viewmatrix.float().numpy().reshape(-1))
