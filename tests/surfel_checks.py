"""TEST INFRASTRUCTURE: checks shared by tests/test_surfel_scenes.py (CPU, model against model) and tests/test_gpu_surfel_edges.py
(GPU, operator against model): running the float64 model on a surfel_scenes.SurfelScene, the per-surfel gradient error and the
event cap of the scenes."""
import torch

import surfel_model as sm

GRAD_NAMES = ("means3D", "opacities", "scales", "rotations", "shs", "colors_precomp", "means2D")
EVENT_SHARE = 5e-4          # of the pixels; half of the cap of test_gpu_surfel._check_images


def event_cap(W, H):
    return max(1, int(EVENT_SHARE * W * H))


def run_model(sc, dtype=torch.float64, device="cpu", radii=None, requires_grad=False, leaves=None, near_skip=True):
    """surfel_model.render on a scene (or on `leaves` in its place) -> (leaves of the model, out)."""
    src = sc.leaves if leaves is None else leaves
    ml = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(requires_grad) for k, v in src.items()}
    cam = sc.cam
    out = sm.render(ml["means3D"], ml["opacities"], ml["scales"], ml["rotations"], cam.viewmatrix.to(device), cam.projmatrix.to(device),
                    cam.campos.to(device), sc.W, sc.H, sc.bg.to(device=device, dtype=dtype), sh_degree=sc.D, shs=ml.get("shs"),
                    colors_precomp=ml.get("colors_precomp"), radii=radii, dtype=dtype, near_skip=near_skip)
    return ml, out


def output_grads(W, H, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=gen), torch.randn(7, H, W, generator=gen)


def excluded_by_events(out):
    """bool [P]: the surfel's rect (in tiles) holds a tile with an event pixel -- its gradient row may legitimately differ."""
    ev = out["events"].cpu()
    H, W = ev.shape
    gy, gx = (H + sm.BLOCK - 1) // sm.BLOCK, (W + sm.BLOCK - 1) // sm.BLOCK
    tile_ev = torch.zeros(gy, gx, dtype=torch.bool)
    ys, xs = torch.nonzero(ev, as_tuple=True)
    tile_ev[ys // sm.BLOCK, xs // sm.BLOCK] = True
    r = out["rects"]
    exc = torch.zeros(r.shape[0], dtype=torch.bool)
    for ty, tx in torch.nonzero(tile_ev).tolist():
        exc |= (r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3])
    return exc


def per_surfel_error(g, ref, out):
    """The per-surfel gradient check: for every visible surfel i whose rect holds no event pixel, and every gradient tensor,

        err_i = |g_i - ref_i| / (|ref_i| + floor),   floor = 1e-3 of the median row norm of `ref` over the visible surfels

    (row norms: L2 over the surfel's row).  Returns (the maximum, its (tensor, surfel), the share of visible surfels excluded).
    A global relative L2 cannot see one wrong row among thousands; this does."""
    vis = out["radii"].cpu() > 0
    exc = excluded_by_events(out)
    use = vis & ~exc
    share = float((vis & exc).sum()) / max(1, int(vis.sum()))
    worst, where = 0.0, None
    for k in g:
        a = g[k].detach().double().cpu().reshape(vis.numel(), -1)
        b = ref[k].detach().double().cpu().reshape(vis.numel(), -1)
        nb = b.norm(dim=1)
        floor = 1e-3 * float(nb[vis].median()) if vis.any() else 0.0
        err = (a - b).norm(dim=1) / (nb + floor).clamp_min(1e-300)
        err = torch.where(use, err, torch.zeros_like(err))
        if use.any() and float(err.max()) > worst:
            worst, where = float(err.max()), (k, int(err.argmax()))
    return worst, where, share
