"""A float64 torch restatement of the densification of the published 3DGS training loop, in its mask-and-cat form:
densify_and_clone, then densify_and_split on the padded gradients, then the prune of the split sources, then the final prune,
with the optimizer-state surgery of cat_tensors_to_optimizer and _prune_optimizer.  One deliberate change:
the screen-size test reads the radii saved before the pass (a clone inherits its source's, a child has none), where the
published code reads radii it has just zeroed.  The normal samples are passed in (noise [N, n_split, 3] by source row).

tests/test_optim_model.py compares tests/optim_model.py with this; tools/optimizer_timing.py times it as the torch baseline."""
import torch

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def build_rotation(r):
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype, device=r.device)
    r_, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r_ * z)
    R[:, 0, 2] = 2 * (x * z + r_ * y)
    R[:, 1, 0] = 2 * (x * y + r_ * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r_ * x)
    R[:, 2, 0] = 2 * (x * z - r_ * y)
    R[:, 2, 1] = 2 * (y * z + r_ * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


class State:
    """Parameters, the two Adam moments per group and the saved radii, all of one row count."""

    def __init__(self, params, exp_avg, exp_avg_sq, radii):
        self.p = {k: params[k] for k in GROUPS}
        self.m = {k: exp_avg[k] for k in GROUPS}
        self.v = {k: exp_avg_sq[k] for k in GROUPS}
        self.radii = radii

    @property
    def n(self):
        return self.p["xyz"].shape[0]

    def cat(self, new, new_radii):           # cat_tensors_to_optimizer + densification_postfix
        for k in GROUPS:
            self.m[k] = torch.cat((self.m[k], torch.zeros_like(new[k])), dim=0)
            self.v[k] = torch.cat((self.v[k], torch.zeros_like(new[k])), dim=0)
            self.p[k] = torch.cat((self.p[k], new[k]), dim=0)
        self.radii = torch.cat((self.radii, new_radii), dim=0)

    def prune(self, mask):                   # prune_points + _prune_optimizer
        keep = ~mask
        for k in GROUPS:
            self.m[k] = self.m[k][keep]
            self.v[k] = self.v[k][keep]
            self.p[k] = self.p[k][keep]
        self.radii = self.radii[keep]


def densify_and_prune(params, exp_avg, exp_avg_sq, grad_accum, denom, max_radii, max_grad, min_opacity, extent,
                      max_screen_size=None, n_split=2, noise=None, percent_dense=0.01):
    """Tensors of any float dtype (the tests pass float64).  Returns the State after the pass."""
    st = State(params, exp_avg, exp_avg_sq, max_radii.clone())
    grads = grad_accum / denom
    grads[grads.isnan()] = 0.0

    # densify_and_clone
    sel = grads >= max_grad
    sel = torch.logical_and(sel, torch.max(torch.exp(st.p["scaling"]), dim=1).values <= percent_dense * extent)
    st.cat({k: st.p[k][sel] for k in GROUPS}, st.radii[sel])

    # densify_and_split
    padded = torch.zeros(st.n, dtype=grads.dtype, device=grads.device)
    padded[:grads.shape[0]] = grads
    sel = padded >= max_grad
    sel = torch.logical_and(sel, torch.max(torch.exp(st.p["scaling"]), dim=1).values > percent_dense * extent)
    src = torch.nonzero(sel[:grads.shape[0]]).reshape(-1)           # split sources are original rows: clones have gradient 0
    stds = torch.exp(st.p["scaling"][sel]).repeat(n_split, 1)
    samples = stds * torch.cat([noise[src, c] for c in range(n_split)], dim=0).to(stds.dtype)
    rots = build_rotation(st.p["rotation"][sel]).repeat(n_split, 1, 1)
    new = dict(xyz=torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + st.p["xyz"][sel].repeat(n_split, 1),
               scaling=torch.log(torch.exp(st.p["scaling"][sel]).repeat(n_split, 1) / (0.8 * n_split)),
               rotation=st.p["rotation"][sel].repeat(n_split, 1), f_dc=st.p["f_dc"][sel].repeat(n_split, 1, 1),
               f_rest=st.p["f_rest"][sel].repeat(n_split, 1, 1), opacity=st.p["opacity"][sel].repeat(n_split, 1))
    n_new = new["xyz"].shape[0]
    st.cat(new, torch.zeros(n_new, dtype=st.radii.dtype, device=st.radii.device))
    st.prune(torch.cat((sel, torch.zeros(n_new, dtype=torch.bool, device=sel.device))))

    # the final prune
    mask = (torch.sigmoid(st.p["opacity"]) < min_opacity).squeeze(-1)
    if max_screen_size is not None:
        big_vs = st.radii > max_screen_size
        big_ws = torch.exp(st.p["scaling"]).max(dim=1).values > 0.1 * extent
        mask = torch.logical_or(torch.logical_or(mask, big_vs), big_ws)
    st.prune(mask)
    return st
