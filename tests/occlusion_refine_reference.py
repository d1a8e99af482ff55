"""Host-side reference of the coarse-to-fine occlusion scan (tests only): the selection rule in numpy float32, the child variant list by
integer arithmetic on the COO lists, and the painting rule."""
import numpy as np
import torch

import occlusion_reference as R


def level_tile(tile, level):
    return (tile[0] >> level, tile[1] >> level)


def selected_rows(heat, index, keep, target="event"):
    """bool [V]: which variants of one level are refined.  heat: that level's heat map [B, 1 + P, Ht, Wt] (float32 values as the kernel
    stored them), index [V, 4].  score = |h|; group = the event, or the map (b, s) for target "prong"; selected iff
    score >= float32(keep) * max(group) (float32, one multiplication) and (keep == 0 or score > 0)."""
    heat = np.asarray(torch.as_tensor(heat).cpu().numpy(), dtype=np.float32)
    idx = np.asarray(torch.as_tensor(index).cpu().numpy(), dtype=np.int64).reshape(-1, 4)
    score = np.abs(heat[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]).astype(np.float32)
    per_map = isinstance(target, str) and target == "prong"
    group = idx[:, 0] * heat.shape[1] + idx[:, 1] if per_map else idx[:, 0]
    gmax = np.zeros(int(group.max()) + 1 if len(group) else 0, dtype=np.float32)
    np.maximum.at(gmax, group, score)
    bound = (np.float32(keep) * gmax[group]).astype(np.float32)
    assert bound.dtype == np.float32 and score.dtype == np.float32
    return (score >= bound) & ((np.float32(keep) == 0) | (score > 0))


def child_index(batch, parent_index, parent_selected, child_tile, shape, maps="all"):
    """int32 [V, 4]: the tiles (2 ty + i, 2 tx + j) at `child_tile` of the selected parent variants that hold at least one hit, ordered by
    (b, s, ty, tx).  All occupied tiles at the child tile come from the COO lists; a child is kept iff its parent was selected."""
    chosen = {tuple(r) for r, k in zip(torch.as_tensor(parent_index).cpu().tolist(), list(parent_selected)) if k}
    flat = R.expected_index(batch, child_tile, shape, maps).tolist()
    rows = [r for r in flat if (r[0], r[1], r[2] // 2, r[3] // 2) in chosen]
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


def keep0_levels(batch, tile, levels, shape, maps="all"):
    """The index of every level with keep = 0, built level by level with the rule above from constant heat maps: every variant has the
    score 1, so every one is selected.  Must equal the flat list at every level."""
    B, P = batch[7].shape
    out = []
    index = R.expected_index(batch, tile, shape, maps)
    for lv in range(levels):
        t = level_tile(tile, lv)
        if lv:
            heat = np.ones((B, 1 + P, *R.grid_of(shape, level_tile(tile, lv - 1))), dtype=np.float32)
            index = child_index(batch, out[-1], selected_rows(heat, out[-1], 0.0), t, shape, maps)
        out.append(index)
    return out


def occupied_cells(batch, tile, shape):
    """bool [B, 1 + P, Ht, Wt]: which cells of the grid at `tile` hold at least one hit."""
    B, P = batch[7].shape
    occ = torch.zeros(B, 1 + P, *R.grid_of(shape, tile), dtype=torch.bool)
    i = R.expected_index(batch, tile, shape).long()
    occ[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = True
    return occ


def paint(heats, indexes, occupied):
    """float32 on the last level's grid: a cell with a hit takes the value of the deepest evaluated variant whose tile contains it (level
    l's tiles are 2^(last - l) cells of the last grid wide), every other cell 0.  heats[l] [B, 1 + P, Ht_l, Wt_l], indexes[l] [V_l, 4]."""
    heats = [torch.as_tensor(h).cpu().float() for h in heats]
    last = len(heats) - 1
    evaluated = [{tuple(r) for r in torch.as_tensor(i).cpu().tolist()} for i in indexes]
    out = torch.zeros_like(heats[last])
    for b, s, y, x in occupied.nonzero().tolist():
        for lv in range(last, -1, -1):
            ty, tx = y >> (last - lv), x >> (last - lv)
            if (b, s, ty, tx) in evaluated[lv]:
                out[b, s, y, x] = heats[lv][b, s, ty, tx]
                break
    return out
