"""CPU: the preconditions of tests/test_gpu_surfel_edges.py, asserted on the float64 model alone (surfel_model.py with its own
radii) for every scene of surfel_scenes.py that is small enough -- a GPU test whose scene stops exercising its path fails here
first --, and the re-derivation of the per-surfel gradient tolerance: the float32 model against the float64 model."""
import functools

import numpy as np
import pytest
import torch

import surfel_checks as ck
import surfel_model as sm
import surfel_scenes as ss


@functools.lru_cache(maxsize=None)
def _ragged(W, H):
    sc = ss.ragged(W, H)
    with torch.no_grad():
        return sc, ck.run_model(sc)[1]


@functools.lru_cache(maxsize=None)
def _long(W, H, P, ties):
    sc = ss.long_list(W, H, P, ties=ties)
    with torch.no_grad():
        return sc, ck.run_model(sc)[1]


@functools.lru_cache(maxsize=None)
def _near():
    sc = ss.near_and_culls()
    with torch.no_grad():
        return sc, ck.run_model(sc)[1]


def _own(sc):
    lv = sc.leaves
    return sm.own_radii(lv["means3D"], lv["scales"], lv["rotations"], sc.cam.viewmatrix, sc.cam.projmatrix, sc.W, sc.H)[0]


@pytest.mark.parametrize("W,H", list(ss.RAGGED), ids=lambda v: str(v))
def test_ragged_scene_preconditions(W, H):
    sc, out = _ragged(W, H)
    P = sc.leaves["means3D"].shape[0]
    assert P == (50 if (W, H) == (1, 1) else P) and (P == 50 or 300 <= P <= 1500)
    assert W % 16 != 0 or H % 16 != 0
    nev = int(out["events"].sum())
    print(f"{W}x{H}: {nev} event pixel(s), share {nev / (W * H):.2e}")
    # (1 x 1: its one pixel must be no event, or the case compares nothing)
    assert nev <= (0 if W * H == 1 else ck.event_cap(W, H))
    assert int((_own(sc) > 0).sum()) > P // 4
    assert float(sc.bg.abs().min()) > 0 and float((1 - out["allmap"][1]).max()) > 0.1      # T_f bg is seen
    assert ck.per_surfel_error({}, {}, out)[2] <= 0.25


# (without autograd the model holds a one-tile list of 9000 in a few hundred MB and a second: every case is checked here)
LONG_CPU = [(16, 16, P, False) for P in ss.LONG_P_16] + [(33, 17, 1100, False)] + [(16, 16, P, True) for P in ss.TIE_P]


def check_long_preconditions(sc, out, P, ties):
    """Shared with the GPU test, which runs it on the model's outputs for the cases too large for the CPU suite."""
    W, H = sc.W, sc.H
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert torch.equal(out["rects"].cpu(), torch.tensor([[0, 0, gx, gy]]).expand(P, 4)), "a rect does not cover the whole image"
    o = sc.leaves["opacities"][:, 0]
    low = o < 1.0 / 255.0
    assert 0.25 < float(low.float().mean()) < 0.42 and float(o[low].min()) >= 0.002 and float(o[low].max()) <= 0.0039
    assert float(o[~low].min()) >= 0.004 and float(o[~low].max()) <= 0.05
    nc, st = out["n_contrib"].cpu(), out["stopped"].cpu()
    if P > 300:
        assert int(nc.max()) > 256
    if P >= 1500:
        assert int(nc.max()) > 1024
    if P >= 1024:
        assert bool(st.any()) and bool((~st & (nc > P - 256)).any()), "no stopped pixel, or none that walks to the list's last batch"
    if P == 288:
        assert bool(((nc > 256) & (nc <= 288)).any())
    if ties:
        key = ss.view_keys(sc).reshape(-1, 10)
        assert (key == key[:, :1]).all() and len(np.unique(key[:, 0])) == P // 10
        lv = sc.leaves
        for k in ("opacities", "scales", "rotations", "shs"):
            v = lv[k].reshape(P // 10, 10, -1)
            assert bool((v[:, 1:] != v[:, :1]).any(2).all()), k


@pytest.mark.parametrize("W,H,P,ties", LONG_CPU, ids=lambda v: str(v))
def test_long_list_scene_preconditions(W, H, P, ties):
    sc, out = _long(W, H, P, ties)
    nev = int(out["events"].sum())
    print(f"{W}x{H} P={P} ties={ties}: {nev} event pixel(s)")
    # one event pixel would take every surfel of a one-tile image out of the per-surfel gradient check: the seeds are event-free
    assert nev == 0
    assert int((_own(sc) > 0).sum()) == P
    check_long_preconditions(sc, out, P, ties)


def test_near_and_cull_scene_preconditions():
    sc, out = _near()
    W, H = sc.W, sc.H
    P = sc.leaves["means3D"].shape[0]
    assert 500 <= P <= 700
    nev = int(out["events"].sum())
    print(f"near/culls: {nev} event pixel(s), share {nev / (W * H):.2e}")
    assert nev <= ck.event_cap(W, H)
    own = torch.tensor(_own(sc))
    g = sc.groups
    vis = {k: int((own[v] > 0).sum()) for k, v in g.items()}
    pz = sc.leaves["means3D"][:, 2]                       # (the camera sits at the origin and looks down +z: view z = z)
    near32 = np.float32(0.2)
    # the intended culls, kind by kind
    assert vis["behind"] == 0 and vis["offscreen"] == 0
    assert bool((pz[g["offscreen"]] > 1).all()) and bool((pz[g["behind"]] < 0).all())
    n_front = int((pz[g["z_span"]] > 0.2).sum())
    assert vis["z_span"] == n_front and 5 <= n_front <= len(g["z_span"]) - 5
    zu = pz[g["z_ulp"]].numpy()
    k = len(zu) // 3
    assert (zu[:k] == np.nextafter(near32, np.float32(0))).all() and (zu[k:2 * k] == near32).all() and (zu[2 * k:] == np.nextafter(near32, np.float32(1))).all()
    assert vis["z_ulp"] == k and bool((own[g["z_ulp"]][2 * k:] > 0).all())
    for name in ("background", "near_tilted", "tiny", "whole_grid", "opaque", "faint", "quat_big", "quat_small", "edge_on"):
        assert vis[name] >= len(g[name]) - (30 if name == "background" else 0), name      # (the plain cloud reaches past the image)
    # what each kind is there for
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert (gx, gy) == (5, 3) and bool((out["rects"][g["whole_grid"]] == torch.tensor([0, 0, gx, gy])).all())
    assert bool((own[g["tiny"]] == 3).all())                                  # ceil(MIN_EXTENT): the floor, not the footprint
    assert bool((sc.leaves["opacities"][g["opaque"]] == 1.0).all()) and bool((sc.leaves["opacities"][g["faint"]] == 0.003).all())
    qn = sc.leaves["rotations"].norm(dim=1)
    assert float(qn[g["quat_big"]].min()) > 990 and float(qn[g["quat_small"]].max()) < 1.01e-3
    # per pixel: z, alpha and the branch of one kind, in float64
    def per_pixel(idx):
        lv = {k: v[idx].double() for k, v in sc.leaves.items()}
        M, tn = sm.splat_matrix(lv["means3D"], lv["scales"], lv["rotations"], 1.0, sc.cam.projmatrix.double(), W, H)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        px, py = xs.reshape(-1), ys.reshape(-1)
        Tu, Tv, Tw = M[:, 0], M[:, 1], M[:, 2]
        q = torch.cross(px[:, None, None] * Tw[None] - Tu[None], py[:, None, None] * Tw[None] - Tv[None], dim=2)
        u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
        f = torch.tensor([9.0, 9.0, -1.0], dtype=torch.float64)
        ff = f[None] / (Tw * Tw * f).sum(1)[:, None]
        cx, cy = (ff * Tu * Tw).sum(1), (ff * Tv * Tw).sum(1)
        rho3, rho2 = u * u + v * v, 2.0 * ((cx[None] - px[:, None]) ** 2 + (cy[None] - py[:, None]) ** 2)
        in3 = rho3 <= rho2
        z = torch.where(in3, u * Tw[None, :, 0] + v * Tw[None, :, 1] + Tw[None, :, 2], Tw[None, :, 2].expand_as(u))
        return z, lv["opacities"][:, 0][None] * torch.exp(-0.5 * torch.minimum(rho3, rho2)), in3, tn, lv["means3D"]
    # the per-pixel near skip: without it (same tile lists) the model's images change at many pixels -- the tilted surfels would
    # contribute where their ray depth is below 0.2 -- so an operator that drops the skip cannot pass
    with torch.no_grad():
        off = ck.run_model(sc, radii=out["radii"], near_skip=False)[1]
    d = (torch.cat([off["color"], off["allmap"]]) - torch.cat([out["color"], out["allmap"]])).abs().amax(0)
    assert int((d > 1e-3).sum()) >= 20
    z, a, in3, _, _ = per_pixel(g["near_tilted"])
    assert int(((z >= sm.NEAR) & (a >= sm.ALPHA_MIN)).sum()) >= 20                     # (and do contribute elsewhere)
    # scales of 1e-4: the low-pass branch wherever they contribute; opacity 1: the clamp is hit
    z, a, in3, _, _ = per_pixel(g["tiny"])
    assert int((a >= sm.ALPHA_MIN).sum()) > 0 and not bool((in3 & (a >= sm.ALPHA_MIN)).any())
    z, a, in3, _, _ = per_pixel(g["opaque"])
    assert int((a > sm.ALPHA_MAX).sum()) >= 5
    # edge-on: the normal within 1e-3 rad of perpendicular to the view ray through the centre
    z, a, in3, tn, p = per_pixel(g["edge_on"])
    cosv = ((p / p.norm(dim=1, keepdim=True)) * tn).sum(1).abs()
    assert float(cosv.max()) < 1.001e-3 and float(cosv.min()) > 0
    assert ck.per_surfel_error({}, {}, out)[2] <= 0.25


@pytest.mark.parametrize("P", ss.PERM_P)
def test_permutation_scene_preconditions(P):
    sc = ss.plain(64, 48, P, seed=P)
    own = _own(sc)
    key = ss.view_keys(sc)[own > 0]
    assert len(np.unique(key)) == len(key) and int((own > 0).sum()) > P // 4
    pad = ss.culled_padding(sc)
    padded = sc._replace(leaves={k: torch.cat([v, pad[k]]) for k, v in sc.leaves.items()})
    assert (_own(padded)[P:] == 0).all() and pad["means3D"].shape[0] == 300
    pz = pad["means3D"][:, 2]
    assert int((pz < 0).sum()) == 100 and int(((pz > 0) & (pz <= 0.2)).sum()) == 100 and int((pz > 1).sum()) == 100


# ---- the per-surfel gradient tolerance: measured model against model, recorded in test_gpu_surfel_edges.py -----------------------
def _f32_vs_f64(sc):
    gc, ga = ck.output_grads(sc.W, sc.H)
    l64, o64 = ck.run_model(sc, requires_grad=True)
    r64 = sm.grads(o64, l64, gc.double(), ga.double(), W=sc.W, H=sc.H)
    l32, o32 = ck.run_model(sc, dtype=torch.float32, radii=o64["radii"], requires_grad=True)
    r32 = sm.grads(o32, l32, gc, ga, W=sc.W, H=sc.H)
    assert torch.equal(o32["rects"], o64["rects"])
    worst, where, share = ck.per_surfel_error(r32, r64, o64)
    assert share <= 0.25
    return worst, where


@pytest.mark.parametrize("name", ["ragged_129x65", "near_and_culls", "long_1025"])
def test_per_surfel_tolerance_is_the_measured_one(name):
    import test_gpu_surfel_edges as edges
    sc = {"ragged_129x65": lambda: ss.ragged(129, 65), "near_and_culls": ss.near_and_culls, "long_1025": lambda: ss.long_list(16, 16, 1025)}[name]()
    worst, where = _f32_vs_f64(sc)
    print(f"{name}: float32 model against float64 model, max per-surfel error {worst:.4g} at {where}")
    assert 0.5 * edges.MEASURED_F32_MODEL[name] < worst <= edges.MEASURED_F32_MODEL[name]
    assert edges.PER_SURFEL_TOL == 4 * max(edges.MEASURED_F32_MODEL.values())
