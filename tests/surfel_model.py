"""TEST INFRASTRUCTURE: a float64 PyTorch restatement of the 2D Gaussian surfel operator (diff_surfel_rasterization), the
contract gsr_surfel.hip implements (INTEGRATION.md "2D Gaussian surfels").  Per pixel over the same square-rect tile lists and
the same (depth, index) order; gradients come from autograd, the documented stop-gradients are `.detach()`.

    out = render(...)            # dict: color [3,H,W], allmap [7,H,W], radii [P], M [P,3,3], events [H,W],
                                 #       n_contrib [H,W] (the kernel's `last`), stopped [H,W], rects [P,4] (tiles: x0 y0 x1 y1)
    grads(out, leaves, ...)      # autograd gradients, plus means2D from dL/dM (the 2DGS densification proxy)

Runs on any device; the GPU tests run it on the GPU in float64."""
import math

import numpy as np
import torch

# the compatibility contract (gsr_common.h GSR_SURF_*)
NEAR = float(np.float32(0.2))     # 0.2f, the kernel's constant: a surfel at exactly this view depth is culled on both sides
FAR = 100.0
LOWPASS = 2.0
CUTOFF = 3.0
MIN_EXTENT = 3.0 * 0.707106
ALPHA_MAX = 0.99
ALPHA_MIN = 1.0 / 255.0
T_MIN = 1e-4
MEDIAN_T = 0.5
BLOCK = 16

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435]


def eval_sh(deg, sh, d):
    """sh [P,>=(deg+1)^2,3], d [P,3] unit directions -> [P,3] (before +0.5)."""
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    r = SH_C0 * sh[:, 0]
    if deg > 0:
        r = r - SH_C1 * y * sh[:, 1] + SH_C1 * z * sh[:, 2] - SH_C1 * x * sh[:, 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            r = (r + SH_C2[0] * xy * sh[:, 4] + SH_C2[1] * yz * sh[:, 5] + SH_C2[2] * (2 * zz - xx - yy) * sh[:, 6]
                 + SH_C2[3] * xz * sh[:, 7] + SH_C2[4] * (xx - yy) * sh[:, 8])
            if deg > 2:
                r = (r + SH_C3[0] * y * (3 * xx - yy) * sh[:, 9] + SH_C3[1] * xy * z * sh[:, 10]
                     + SH_C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
                     + SH_C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + SH_C3[5] * z * (xx - yy) * sh[:, 14]
                     + SH_C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return r


def rotmat_columns(q):
    """Columns (t_u, t_v, t_n) of R(q), q = (r, x, y, z) normalised -- the convention of the 3DGS path (quat_to_R)."""
    r, x, y, z = q.unbind(1)
    tu = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1)
    tv = torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1)
    tn = torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)
    return tu, tv, tn


def splat_matrix(means3D, scales, rotations, scale_modifier, projmatrix, W, H):
    """M [P,3,3] with h = M (u, v, 1), rows Tu, Tv, Tw; also the normalised quaternion's columns."""
    q = rotations / rotations.norm(dim=1, keepdim=True).clamp_min(1e-12)
    tu, tv, tn = rotmat_columns(q)
    s = scale_modifier * scales[:, :2]
    N = torch.tensor([[W / 2, 0, 0, (W - 1) / 2], [0, H / 2, 0, (H - 1) / 2], [0, 0, 0, 1]], dtype=means3D.dtype, device=means3D.device)
    Q = N @ projmatrix.T                                  # h = Q (X, 1): clip c = (X, 1) @ projmatrix
    Q3, Qt = Q[:, :3], Q[:, 3]
    M = torch.stack([(s[:, 0:1] * tu) @ Q3.T, (s[:, 1:2] * tv) @ Q3.T, means3D @ Q3.T + Qt], 2)   # [P, row, col]
    return M, tn


def get_rect(cx, cy, r, gx, gy):
    """The reference's square getRect, in float32 arithmetic like the kernel."""
    cx, cy = np.float32(cx), np.float32(cy)
    r = np.float32(r)
    b = np.float32(BLOCK)
    f = lambda v, hi: min(hi, max(0, int(v)))
    return (f((cx - r) / b, gx), f((cy - r) / b, gy), f((cx + r + b - 1) / b, gx), f((cy + r + b - 1) / b, gy))


def _view_z_f32(p, v):
    """The sort key as the kernel forms it: view z in float32, fma(v10, z, fma(v6, y, v2 * x)) + v14 (the exact product + sum
    rounded once: float64 holds every product of two float32 exactly)."""
    f = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    x, y, z = (p[:, i].astype(np.float64) for i in range(3))
    t = f(v[2] * x)
    t = f(np.float64(v[6]) * y + t)
    t = f(np.float64(v[10]) * z + t)
    return f(t + np.float64(v[14]))


def own_radii(means3D, scales, rotations, viewmatrix, projmatrix, W, H, scale_modifier=1.0):
    """The model's own culls and radii, independent of the operator: -> (radii int64 [P] (0 = culled or an empty rect), boundary
    bool [P]).  `boundary` marks the Gaussians whose outcome float32 may legitimately decide the other way: the pre-ceil radius
    within 1e-4 relative of an integer, the view depth within 1e-5 of the near plane, the normal within 1e-6 of edge-on, or a rect
    that changes when the centre moves by 2e-5 of its magnitude."""
    dt = torch.float64
    with torch.no_grad():
        p, view, proj = means3D.detach().to(dt), viewmatrix.to(dt), projmatrix.to(dt)
        pv = p @ view[:3, :3] + view[3, :3]
        M, tn = splat_matrix(p, scales.detach().to(dt), rotations.detach().to(dt), scale_modifier, proj, W, H)
        n = tn @ view[:3, :3]
        cosv = -(pv * n).sum(1)
        Tu, Tv, Tw = M[:, 0], M[:, 1], M[:, 2]
        f = torch.tensor([CUTOFF ** 2, CUTOFF ** 2, -1.0], dtype=dt, device=p.device)
        dist = (Tw * Tw * f).sum(1)
        ff = f[None] / dist[:, None]
        cx, cy = (ff * Tu * Tw).sum(1), (ff * Tv * Tw).sum(1)
        tx, ty = (ff * Tu * Tu).sum(1), (ff * Tv * Tv).sum(1)
        ext = torch.sqrt(torch.clamp(torch.stack([cx * cx - tx, cy * cy - ty], 1), min=1e-4)).max(1).values
        pre = torch.clamp(ext, min=MIN_EXTENT)
        vis = (pv[:, 2] > NEAR) & (cosv != 0) & (dist != 0)
        boundary = ((pre - torch.round(pre)).abs() < 1e-4 * pre) | ((pv[:, 2] - NEAR).abs() < 1e-5) | \
                   (cosv.abs() < 1e-6 * pv.norm(dim=1) * n.norm(dim=1))
        pre, vis, boundary = pre.cpu().numpy(), vis.cpu().numpy(), boundary.cpu().numpy()
        cx, cy = cx.cpu().numpy(), cy.cpu().numpy()
    gx, gy = (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK
    radii = np.zeros(len(pre), np.int64)
    for i in range(len(pre)):
        if not vis[i]:
            continue
        r = int(math.ceil(pre[i]))
        rect = get_rect(cx[i], cy[i], r, gx, gy)
        e = 2e-5 * (1 + abs(cx[i]) + abs(cy[i]))
        if any(get_rect(cx[i] + a, cy[i] + b, r, gx, gy) != rect for a in (-e, e) for b in (-e, e)):
            boundary[i] = True
        if (rect[2] - rect[0]) * (rect[3] - rect[1]) > 0:
            radii[i] = r
    return radii, boundary


def render(means3D, opacities, scales, rotations, viewmatrix, projmatrix, campos, W, H, bg, scale_modifier=1.0, sh_degree=0,
           shs=None, colors_precomp=None, radii=None, dtype=torch.float64, near_skip=True):
    """Float64 forward.  Tensors may require grad.  `radii` (int, [P]): use these radii (visibility and rect size) instead of
    the model's own -- the GPU tests pass the operator's radii so that the tile lists agree.  `dtype`: the arithmetic of the
    whole model (the inputs are expected in it); torch.float32 gives a second, independently ordered float32 evaluation of the
    operator, against which the float64 one measures what float32 can hold.  The sort key is _view_z_f32 in either.

    Besides the images: `n_contrib` [H,W] int64, the 1-based list position of the pixel's last contributor (0: none), and
    `stopped` [H,W] bool, true where the walk ended on the T (1 - alpha) < T_MIN rule rather than at the list's end.
    `near_skip=False` drops the per-pixel skip z < NEAR (not the cull): a scene on which that changes nothing does not test it."""
    dt = dtype
    dev = means3D.device
    view = viewmatrix.to(dt)
    proj = projmatrix.to(dt)
    P = means3D.shape[0]
    pv = means3D @ view[:3, :3] + view[3, :3]
    M, tn = splat_matrix(means3D, scales, rotations, scale_modifier, proj, W, H)
    n = tn @ view[:3, :3]
    cosv = -(pv * n).sum(1)
    sgn = torch.where(cosv.detach() > 0, 1.0, -1.0).to(dt)
    n = n * sgn[:, None]
    Tu, Tv, Tw = M[:, 0], M[:, 1], M[:, 2]
    f = torch.tensor([CUTOFF ** 2, CUTOFF ** 2, -1.0], dtype=dt, device=dev)
    dist = (Tw * Tw * f).sum(1)
    ff = f[None] / dist[:, None]
    cx, cy = (ff * Tu * Tw).sum(1), (ff * Tv * Tw).sum(1)
    tx, ty = (ff * Tu * Tu).sum(1), (ff * Tv * Tv).sum(1)
    ext = torch.sqrt(torch.clamp(torch.stack([cx * cx - tx, cy * cy - ty], 1), min=1e-4))
    rad = torch.ceil(torch.clamp(ext.max(1).values, min=MIN_EXTENT)).detach()
    gx, gy = (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK
    if shs is not None:
        d = means3D - campos.to(dt)[None]
        d = d / d.norm(dim=1, keepdim=True)
        rgb = torch.clamp_min(eval_sh(sh_degree, shs, d) + 0.5, 0.0)
    else:
        rgb = colors_precomp
    op = opacities.reshape(P)
    cxd, cyd = cx.detach().cpu().numpy(), cy.detach().cpu().numpy()
    own_vis = ((pv[:, 2] > NEAR) & (cosv != 0) & (dist != 0)).detach().cpu().numpy()
    rad_np = rad.cpu().numpy()
    if radii is not None:
        radii = np.asarray(radii.cpu() if torch.is_tensor(radii) else radii).astype(np.int64)
    out_radii = np.zeros(P, np.int64)
    rects = {}
    for i in range(P):
        if radii is not None:
            if radii[i] <= 0:
                continue
            r = int(radii[i])
        else:
            if not own_vis[i]:
                continue
            r = int(rad_np[i])
        rect = get_rect(cxd[i], cyd[i], r, gx, gy)
        if (rect[2] - rect[0]) * (rect[3] - rect[1]) == 0:
            continue
        rects[i] = rect
        out_radii[i] = r
    color = torch.zeros(3, H, W, dtype=dt, device=dev)
    allmap = torch.zeros(7, H, W, dtype=dt, device=dev)
    color = color + bg.to(dt).reshape(3, 1, 1)
    events = torch.zeros(H, W, dtype=torch.bool, device=dev)
    n_contrib = torch.zeros(H, W, dtype=torch.int64, device=dev)
    stopped = torch.zeros(H, W, dtype=torch.bool, device=dev)
    ids = np.array(sorted(rects), dtype=np.int64)
    key = _view_z_f32(means3D.detach().float().cpu().numpy(), viewmatrix.float().cpu().numpy().reshape(-1))
    order = ids[np.lexsort((ids, key[ids]))] if len(ids) else ids
    imgs_c, imgs_a, idx_pix = [], [], []
    for ty in range(gy):
        for tx in range(gx):
            lst = [i for i in order if rects[i][0] <= tx < rects[i][2] and rects[i][1] <= ty < rects[i][3]]
            ys, xs = torch.meshgrid(torch.arange(ty * BLOCK, min(H, ty * BLOCK + BLOCK), device=dev),
                                    torch.arange(tx * BLOCK, min(W, tx * BLOCK + BLOCK), device=dev), indexing="ij")
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            if not lst:
                continue
            L = torch.tensor(lst, device=dev)
            c_out, a_out, ev, nc, st = _composite(xs.to(dt), ys.to(dt), Tu[L], Tv[L], Tw[L], cx[L].detach(), cy[L].detach(), op[L], n[L], rgb[L],
                                          bg.to(dt), M[L].detach(), near_skip)
            imgs_c.append(c_out)
            imgs_a.append(a_out)
            idx_pix.append(ys * W + xs)
            events[ys, xs] = ev
            n_contrib[ys, xs] = nc
            stopped[ys, xs] = st
    if idx_pix:
        pix = torch.cat(idx_pix)
        color = color.reshape(3, H * W).index_copy(1, pix, torch.cat(imgs_c, 1)).reshape(3, H, W)
        allmap = allmap.reshape(7, H * W).index_copy(1, pix, torch.cat(imgs_a, 1)).reshape(7, H, W)
    rect_t = torch.zeros(P, 4, dtype=torch.int64)
    for i, r in rects.items():
        rect_t[i] = torch.tensor(r)
    return dict(color=color, allmap=allmap, radii=torch.tensor(out_radii), M=M, events=events, n_contrib=n_contrib, stopped=stopped,
                rects=rect_t)


def _excl_cumprod(x):
    return torch.cat([torch.ones_like(x[:, :1]), torch.cumprod(x, 1)[:, :-1]], 1)


def _excl_cumsum(x):
    return torch.cat([torch.zeros_like(x[:, :1]), torch.cumsum(x, 1)[:, :-1]], 1)


def _eval_f32(px, py, M, o):
    """alpha and z of every (pixel, entry) evaluated in float32 from the float32-rounded splat matrix (centre included): where
    these differ from the float64 values the evaluation itself is ill-conditioned (a splat seen almost edge-on, a centre from a
    near-singular denominator) and the operator's float32 result may differ from the model's at that pixel."""
    M = M.float()
    Tu, Tv, Tw = M[:, 0], M[:, 1], M[:, 2]
    f = torch.tensor([CUTOFF ** 2, CUTOFF ** 2, -1.0], dtype=torch.float32, device=M.device)
    ff = f[None] / (Tw * Tw * f).sum(1)[:, None]
    cx, cy = (ff * Tu * Tw).sum(1), (ff * Tv * Tw).sum(1)
    px, py = px.float(), py.float()
    k = px[:, None, None] * Tw[None] - Tu[None]
    l = py[:, None, None] * Tw[None] - Tv[None]
    q = torch.cross(k, l, dim=2)
    qz = torch.where(q[..., 2] != 0, q[..., 2], torch.ones_like(q[..., 2]))
    u, v = q[..., 0] / qz, q[..., 1] / qz
    rho3 = u * u + v * v
    rho2 = LOWPASS * ((cx[None] - px[:, None]) ** 2 + (cy[None] - py[:, None]) ** 2)
    in3 = rho3 <= rho2
    z = torch.where(in3, u * Tw[None, :, 0] + v * Tw[None, :, 1] + Tw[None, :, 2], Tw[None, :, 2].expand_as(u))
    alpha = torch.clamp(o.detach().float()[None] * torch.exp(-0.5 * torch.where(in3, rho3, rho2)), max=ALPHA_MAX)
    return alpha.double(), z.double()


def _composite(px, py, Tu, Tv, Tw, cx, cy, o, n, rgb, bg, M, near_skip=True):
    """One tile: pixels [n] x list entries [L] (front to back).  Returns colour [3,n], allmap [7,n], the per-pixel flag of a
    threshold event, the 1-based position of the pixel's last contributor (0: none) and whether the T_MIN rule ended its walk.
    A threshold event is a decision within 1e-3 relative of its threshold.  The four of the contract -- alpha vs 1/255, T vs 1e-4,
    rho3 vs rho2, z vs NEAR -- and, a DELIBERATE WIDENING beyond them, three more: o G vs the 0.99 clamp, T vs 0.5 at the median,
    and an ill-conditioned contributor (_eval_f32: its float32 alpha or depth is off by more than 2e-5 -- a splat seen almost
    edge-on; measured: 3 of the 4 pixels beyond 1e-4 in the GPU tests' two largest scenes were of this kind, the fourth a
    median depth off by 1.1e-4)."""
    k = px[:, None, None] * Tw[None] - Tu[None]
    l = py[:, None, None] * Tw[None] - Tv[None]
    q = torch.cross(k, l, dim=2)
    qz = q[..., 2]
    ok = qz.detach() != 0
    qzs = torch.where(ok, qz, torch.ones_like(qz))
    u, v = q[..., 0] / qzs, q[..., 1] / qzs
    rho3 = u * u + v * v
    rho2 = LOWPASS * ((cx[None] - px[:, None]) ** 2 + (cy[None] - py[:, None]) ** 2)   # the centre is detached (stop-gradient)
    in3 = (rho3 <= rho2).detach()
    rho = torch.where(in3, rho3, rho2)
    z = torch.where(in3, u * Tw[None, :, 0] + v * Tw[None, :, 1] + Tw[None, :, 2], Tw[None, :, 2].expand_as(u))
    if near_skip:
        ok = ok & (z.detach() >= NEAR)
    G = torch.exp(-0.5 * rho)
    alpha = torch.clamp(o[None] * G, max=ALPHA_MAX)         # clamped: no gradient
    ok = ok & (alpha.detach() >= ALPHA_MIN)
    a_ok = torch.where(ok, alpha, torch.zeros_like(alpha))
    Tb = _excl_cumprod(1 - a_ok.detach())
    stop = ok & (Tb * (1 - alpha.detach()) < T_MIN)
    keep = torch.cumsum(stop.int(), 1) == 0
    con = ok & keep
    a_c = torch.where(con, alpha, torch.zeros_like(alpha))
    T = _excl_cumprod(1 - a_c)
    w = a_c * T
    Tf = torch.prod(1 - a_c, 1)
    zs = torch.where(con, z, torch.ones_like(z))
    m = FAR / (FAR - NEAR) * (1 - NEAR / zs)
    wm, wm2 = w * m, w * m * m
    dist = (w * (m * m * (1 - T) + _excl_cumsum(wm2) - 2 * m * _excl_cumsum(wm))).sum(1)
    C = w @ rgb + Tf[:, None] * bg[None]
    D = (w * zs).sum(1)
    Nn = w @ n
    med_mask = con & (T.detach() > MEDIAN_T)
    idx = torch.arange(alpha.shape[1], device=alpha.device)[None].expand_as(alpha)
    last = torch.where(med_mask, idx, torch.full_like(idx, -1)).max(1).values
    has = last >= 0
    median = torch.where(has, zs.gather(1, last.clamp_min(0)[:, None])[:, 0], torch.zeros_like(D))
    # threshold events (for the attribution of pixels beyond tolerance)
    rel = 1e-3
    ad, Tbd = alpha.detach(), T.detach()
    ev = (((ad - ALPHA_MIN).abs() < rel * ALPHA_MIN) & (ad > 0)) | ((o[None].detach() * G.detach() - ALPHA_MAX).abs() < rel)
    ev = ev | (((Tbd * (1 - ad) - T_MIN).abs() < rel * T_MIN) & ok & (torch.cumsum(stop.int(), 1) <= 1))
    ev = ev | (((rho3 - rho2).detach().abs() < rel * (rho2.detach() + 1e-6)) & (ad > ALPHA_MIN * 0.5))
    ev = ev | (((z.detach() - NEAR).abs() < rel) & (ad > ALPHA_MIN * 0.5))      # (an entry far below 1/255 contributes either way)
    ev = ev | (((Tbd - MEDIAN_T).abs() < rel) & con)
    a32, z32 = _eval_f32(px, py, M, o)
    ev = ev | (con & (((a32 - ad).abs() > 2e-5) | ((z32 - z.detach()).abs() > 2e-5)))
    ev = ev.any(1)
    allmap = torch.stack([D, 1 - Tf, Nn[:, 0], Nn[:, 1], Nn[:, 2], median, dist], 0)
    n_contrib = torch.where(con, idx + 1, torch.zeros_like(idx)).max(1).values
    return C.T, allmap, ev, n_contrib, stop.any(1)


def grads(out, leaves, g_color=None, g_allmap=None, W=None, H=None):
    """Autograd gradients of L = <g_color, color> + <g_allmap, allmap> for the dict of leaf tensors; adds 'means2D' from dL/dM."""
    loss = 0
    if g_color is not None:
        loss = loss + (out["color"] * g_color.to(out["color"])).sum()
    if g_allmap is not None:
        loss = loss + (out["allmap"] * g_allmap.to(out["allmap"])).sum()
    names = [k for k, v in leaves.items() if v is not None and v.requires_grad]
    gs = torch.autograd.grad(loss, [leaves[k] for k in names] + [out["M"]], allow_unused=True)
    res = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(names, gs[:-1])}
    gM = gs[-1] if gs[-1] is not None else torch.zeros_like(out["M"])
    M = out["M"].detach()
    m2 = torch.zeros(M.shape[0], 3, dtype=M.dtype, device=M.device)
    m2[:, 0] = gM[:, 0, 2] * M[:, 2, 2] * W / 2
    m2[:, 1] = gM[:, 1, 2] * M[:, 2, 2] * H / 2
    res["means2D"] = m2
    return res
