"""The published Scaffold-GS anchor adjustment (adjust_anchor / anchor_growing / prune_anchor) restated in torch float64, in the
published order of operations: torch.unique over rows with the inverse, the chunked all-pairs compare against every anchor, a
scatter maximum (scatter_reduce "amax" stands in for torch_scatter.scatter_max), one cat per tensor with the Adam state cut and
extended the same way, then the masked prune.  It runs on any device.  Two differences, both in the caller's favour: the draw
`rand` is an argument ([update_depth, N k]) where the publication calls torch.rand_like inside the loop, and the opacity of new
anchors is left out (this model family has no opacity parameter).

tests/test_anchor_model.py compares tests/anchor_model.py with it; tools/anchor_control_timing.py times it."""
import math
from collections import namedtuple

import torch

NAMES = ("anchor", "anchor_feat", "offset", "scale_raw", "rot_raw")
Result = namedtuple("Result", "params exp_avg exp_avg_sq stats n_grown cells feats prune_mask")


def _cat(state, new):
    """cat_tensors_to_optimizer: parameters and both moments, the moments of the new rows zero."""
    for name, ext in new.items():
        state["p"][name] = torch.cat([state["p"][name], ext], dim=0)
        for key in ("m", "v"):
            if name in state[key]:
                state[key][name] = torch.cat([state[key][name], torch.zeros_like(ext)], dim=0)


def anchor_growing(state, grads, threshold, offset_mask, rand, k, voxel_size, update_depth, update_init_factor,
                   update_hierarchy_factor, chunk_size=4096):
    p = state["p"]
    init_length = p["anchor"].shape[0] * k
    n_grown, cells, feats = [], [], []
    for i in range(update_depth):
        cur_threshold = threshold * ((update_hierarchy_factor // 2) ** i)
        candidate_mask = grads >= cur_threshold
        candidate_mask = torch.logical_and(candidate_mask, offset_mask)
        rand_mask = rand[i] > (0.5 ** (i + 1))
        candidate_mask = torch.logical_and(candidate_mask, rand_mask)
        length_inc = p["anchor"].shape[0] * k - init_length
        if length_inc == 0:
            if i > 0:
                n_grown.append(0)
                continue
        else:
            candidate_mask = torch.cat([candidate_mask, torch.zeros(length_inc, dtype=torch.bool, device=candidate_mask.device)], dim=0)
        scaling = torch.exp(p["scale_raw"])
        all_xyz = p["anchor"].unsqueeze(dim=1) + p["offset"] * scaling[:, :3].unsqueeze(dim=1)
        size_factor = update_init_factor // (update_hierarchy_factor ** i)
        cur_size = voxel_size * size_factor
        grid_coords = torch.round(p["anchor"] / cur_size).long()
        selected_xyz = all_xyz.view([-1, 3])[candidate_mask]
        selected_grid_coords = torch.round(selected_xyz / cur_size).long()
        selected_grid_coords_unique, inverse_indices = torch.unique(selected_grid_coords, return_inverse=True, dim=0)
        remove_duplicates = torch.zeros(selected_grid_coords_unique.shape[0], dtype=torch.bool, device=grads.device)
        max_iters = grid_coords.shape[0] // chunk_size + (1 if grid_coords.shape[0] % chunk_size != 0 else 0)
        for c in range(max_iters):
            cur = (selected_grid_coords_unique.unsqueeze(1) == grid_coords[c * chunk_size:(c + 1) * chunk_size, :]).all(-1).any(-1).view(-1)
            remove_duplicates = torch.logical_or(remove_duplicates, cur)
        remove_duplicates = ~remove_duplicates
        candidate_cells = selected_grid_coords_unique[remove_duplicates]
        candidate_anchor = candidate_cells * cur_size
        n_grown.append(int(candidate_anchor.shape[0]))
        if candidate_anchor.shape[0] > 0:
            new_scaling = torch.log(torch.ones_like(candidate_anchor).repeat([1, 2]) * cur_size)
            new_rotation = torch.zeros([candidate_anchor.shape[0], 4], dtype=candidate_anchor.dtype, device=candidate_anchor.device)
            new_rotation[:, 0] = 1.0
            feat_dim = p["anchor_feat"].shape[1]
            new_feat = p["anchor_feat"].unsqueeze(dim=1).repeat([1, k, 1]).view([-1, feat_dim])[candidate_mask]
            index = inverse_indices.unsqueeze(1).expand(-1, new_feat.size(1))
            new_feat = torch.full((selected_grid_coords_unique.shape[0], feat_dim), -math.inf, dtype=new_feat.dtype,
                                  device=new_feat.device).scatter_reduce(0, index, new_feat, "amax")[remove_duplicates]
            new_offsets = torch.zeros_like(candidate_anchor).unsqueeze(dim=1).repeat([1, k, 1])
            _cat(state, dict(anchor=candidate_anchor, scale_raw=new_scaling, rot_raw=new_rotation, anchor_feat=new_feat,
                             offset=new_offsets))
            cells.append(candidate_cells)
            feats.append(new_feat)
    return n_grown, cells, feats


def adjust_anchor(params, exp_avg, exp_avg_sq, stats, k, voxel_size, rand, check_interval=100, success_threshold=0.8,
                  grad_threshold=2e-4, min_opacity=0.005, update_depth=3, update_init_factor=16, update_hierarchy_factor=4):
    """params, exp_avg, exp_avg_sq: name -> float64 tensor (the moment dicts may lack names); stats: offset_grad_accum [N k],
    offset_denom [N k], opacity_accum [N], anchor_denom [N] as float64 tensors; rand [update_depth, N k]."""
    state = dict(p={n: params[n].clone() for n in NAMES}, m={n: t.clone() for n, t in exp_avg.items()},
                 v={n: t.clone() for n, t in exp_avg_sq.items()})
    accum, denom = stats["offset_grad_accum"].clone().view(-1, 1), stats["offset_denom"].clone().view(-1, 1)
    op_accum, a_denom = stats["opacity_accum"].clone().view(-1, 1), stats["anchor_denom"].clone().view(-1, 1)
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    grads_norm = torch.norm(grads, dim=-1)
    offset_mask = (denom > check_interval * success_threshold * 0.5).squeeze(dim=1)
    n_grown, cells, feats = anchor_growing(state, grads_norm, grad_threshold, offset_mask, rand, k, voxel_size, update_depth,
                                           update_init_factor, update_hierarchy_factor)
    n_all = state["p"]["anchor"].shape[0]
    pad = lambda t, rows: torch.cat([t, torch.zeros([rows - t.shape[0], 1], dtype=t.dtype, device=t.device)], dim=0)
    denom[offset_mask] = 0
    denom = pad(denom, n_all * k)
    accum[offset_mask] = 0
    accum = pad(accum, n_all * k)
    op_accum = pad(op_accum, n_all)
    a_denom = pad(a_denom, n_all)
    prune_mask = (op_accum < min_opacity * a_denom).squeeze(dim=1)
    anchors_mask = (a_denom > check_interval * success_threshold).squeeze(dim=1)
    prune_mask = torch.logical_and(prune_mask, anchors_mask)
    denom = denom.view([-1, k])[~prune_mask].view([-1, 1])
    accum = accum.view([-1, k])[~prune_mask].view([-1, 1])
    if anchors_mask.sum() > 0:
        op_accum[anchors_mask] = 0
        a_denom[anchors_mask] = 0
    op_accum, a_denom = op_accum[~prune_mask], a_denom[~prune_mask]
    if prune_mask.shape[0] > 0:                                   # prune_anchor: the mask on parameters and moments
        for key in ("p", "m", "v"):
            for name in state[key]:
                state[key][name] = state[key][name][~prune_mask]
    new_stats = dict(offset_grad_accum=accum.view(-1), offset_denom=denom.view(-1), opacity_accum=op_accum.view(-1),
                     anchor_denom=a_denom.view(-1))
    return Result(state["p"], state["m"], state["v"], new_stats, tuple(n_grown), cells, feats, prune_mask)
