"""Host-side reference of the deletion / insertion curves (tests only): the ranking of every map's occupied tiles by a Python sort, the
variant list (b, s, k, m_k), the brute force "plain forward() of the same model on event b alone with the hits of the first m_k tiles
removed / kept", and the float64 curve and area from a result's own logits."""
import math

import torch

import occlusion_reference as R


def occupied_tiles(batch, tile, maps="all"):
    """{(b, s): {(ty, tx), ...}}: the tiles that hold a hit, for every scanned map that holds one."""
    ec, pc, pm = batch[2].cpu().long(), batch[5].cpu().long(), batch[7].cpu()
    pb, pp = R.prong_slots(pm)
    out = {}
    if maps in ("all", "event"):
        for img, y, x in ec.tolist():
            out.setdefault((img, 0), set()).add((y // tile[0], x // tile[1]))
    if maps in ("all", "prongs"):
        for img, y, x in pc.tolist():
            out.setdefault((pb[img], 1 + pp[img]), set()).add((y // tile[0], x // tile[1]))
    return out


def steps_of(n, K):
    return [(k * n + K - 1) // K for k in range(K + 1)]


def expected_rank_and_index(batch, relevance, tile, shape, steps, maps="all"):
    """-> (rank int32 [B, 1 + P, Ht, Wt], index int32 [V, 4] = (b, s, k, m_k) ascending): per map a Python sort by (-relevance, tile
    index); -0.0 == 0.0 in Python as in the ranking rule."""
    Ht, Wt = R.grid_of(shape, tile)
    B, P = batch[7].shape
    rel = relevance.cpu()
    rank = torch.full((B, 1 + P, Ht, Wt), -1, dtype=torch.int32)
    rows = []
    for (b, s), tiles in sorted(occupied_tiles(batch, tile, maps).items()):
        order = sorted(tiles, key=lambda t: (-float(rel[b, s, t[0], t[1]]), t[0] * Wt + t[1]))
        for r, (ty, tx) in enumerate(order):
            rank[b, s, ty, tx] = r
        rows += [(b, s, k, m) for k, m in enumerate(steps_of(len(order), steps))]
    return rank, torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


def single_event_variant(batch, b, s, rank_map, m, tile, mode):
    """The 8 forward() inputs of event b alone; the map of token slot s without (deletion) / with only (insertion) the hits of the tiles
    ranked below m in rank_map [Ht, Wt].  Hit order is kept."""
    f, x, e_c, e_v, em, p_c, p_v, pm = R.single_event(batch, b)
    slots = batch[7][b].cpu().nonzero().flatten().tolist()

    def survives(c):
        top = rank_map[c[:, 1].long() // tile[0], c[:, 2].long() // tile[1]] < m
        return ~top if mode == "deletion" else top

    if s == 0:
        keep = survives(e_c)
        e_c, e_v = e_c[keep].contiguous(), e_v[keep].contiguous()
    else:
        mine = p_c[:, 0] == slots.index(s - 1)
        keep = ~mine | survives(p_c)
        p_c, p_v = p_c[keep].contiguous(), p_v[keep].contiguous()
    return f, x, e_c, e_v, em, p_c, p_v, pm


def brute_force(model, batch, index, rank, tile, mode, device="cuda"):
    """forward() of `model` on event b alone for every variant of `index` -> (event logits [V, Ce], prong logits [V, P, Cp])."""
    evs, prs = [], []
    rank = rank.cpu()
    with torch.no_grad():
        for b, s, k, m in index.cpu().tolist():
            one = single_event_variant(batch, b, s, rank[b, s], m, tile, mode)
            ev, pr = model.forward(*[t.to(device) for t in one])
            evs.append(ev[0].cpu())
            prs.append(pr[0].cpu())
    return torch.stack(evs), torch.stack(prs)


def curve_reference(result, target="event"):
    """float64 (curve [B, 1 + P, K + 1], auc [B, 1 + P]) from the result's own logits; NaN where there is no variant."""
    ev, pr = result.event_logits.cpu().double(), result.prong_logits.cpu().double()
    sev, spr = result.step_event_logits.cpu().double(), result.step_prong_logits.cpu().double()
    B, P, K = pr.shape[0], pr.shape[1], result.steps
    curve = torch.full((B, 1 + P, K + 1), math.nan, dtype=torch.float64)
    for v, (b, s, k, m) in enumerate(result.index.cpu().tolist()):
        if isinstance(target, str) and target == "prong":
            if s == 0:
                continue
            c = int(pr[b, s - 1].argmax())
            p = torch.softmax(spr[v, s - 1], 0)[c]
        else:
            c = int(ev[b].argmax()) if isinstance(target, str) else int(torch.as_tensor(target).reshape(-1).expand(B)[b])
            p = torch.softmax(sev[v], 0)[c]
        curve[b, s, k] = p
    auc = (curve[..., 0] / 2 + curve[..., 1:K].sum(-1) + curve[..., K] / 2) / K
    return curve, auc
