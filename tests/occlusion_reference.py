"""Host-side reference of the occlusion scan (tests only): the variant list by integer arithmetic on the COO lists, the filtered inputs
of one variant, and the brute force "plain forward() of the same model on event b alone with that tile's hits removed"."""
import torch


def grid_of(shape, tile):
    return (-(-shape[0] // tile[0]), -(-shape[1] // tile[1]))


def prong_slots(prong_mask):
    """(b, p) of every packed prong image, in the packed order of the prong hit list."""
    b, p = prong_mask.cpu().nonzero(as_tuple=True)
    return b.tolist(), p.tolist()


def expected_index(batch, tile, shape, maps="all"):
    """int32 [V, 4] = (b, s, ty, tx), ascending: unique (image, y // th, x // tw) of both hit lists, prong images mapped through the mask."""
    ec, pc, pm = batch[2].cpu().long(), batch[5].cpu().long(), batch[7].cpu()
    pb, pp = prong_slots(pm)
    rows = set()
    if maps in ("all", "event"):
        for img, y, x in ec.tolist():
            rows.add((img, 0, y // tile[0], x // tile[1]))
    if maps in ("all", "prongs"):
        for img, y, x in pc.tolist():
            rows.add((pb[img], 1 + pp[img], y // tile[0], x // tile[1]))
    return torch.tensor(sorted(rows), dtype=torch.int32).reshape(-1, 4)


def single_event(batch, b, drop=None, tile=None):
    """The 8 forward() inputs of event b alone (same prong width, so the same sequence length).  drop = (s, ty, tx): the hits of that tile
    are removed from the map of token slot s; drop = (s, None, None): every hit of that map.  Hit order is kept."""
    f, x, ec, ev, em, pc, pv, pm = [t.cpu() for t in batch[:8]]
    counts = pm.sum(1).tolist()
    first = int(sum(counts[:b]))
    n = int(counts[b])
    slots = pm[b].nonzero().flatten().tolist()                    # slot of local prong image j

    def tile_hit(c):
        if drop[1] is None:
            return torch.ones(c.shape[0], dtype=torch.bool)
        return (c[:, 1] // tile[0] == drop[1]) & (c[:, 2] // tile[1] == drop[2])

    ke = ec[:, 0] == b
    e_c, e_v = ec[ke].clone(), ev[ke]
    e_c[:, 0] = 0
    if drop is not None and drop[0] == 0:
        keep = ~tile_hit(e_c)
        e_c, e_v = e_c[keep], e_v[keep]
    kp = (pc[:, 0] >= first) & (pc[:, 0] < first + n)
    p_c, p_v = pc[kp].clone(), pv[kp]
    p_c[:, 0] -= first
    if drop is not None and drop[0] > 0:
        j = slots.index(drop[0] - 1)
        keep = ~((p_c[:, 0] == j) & tile_hit(p_c))
        p_c, p_v = p_c[keep], p_v[keep]
    return (f[b:b + 1].clone(), x[b:b + 1].clone(), e_c.contiguous(), e_v.contiguous(), em[b:b + 1].clone(), p_c.contiguous(),
            p_v.contiguous(), pm[b:b + 1].clone())


def filtered_batch(batch, b, drop, tile):
    """The whole batch with the hits of one tile removed from one map of event b (inputs of the CPU oracle)."""
    f, x, ec, ev, em, pc, pv, pm = [t.cpu() for t in batch[:8]]
    s, ty, tx = drop
    if s == 0:
        hit = (ec[:, 0] == b) & (ec[:, 1] // tile[0] == ty) & (ec[:, 2] // tile[1] == tx)
        assert bool(hit.any())
        ec, ev = ec[~hit], ev[~hit]
    else:
        pb, pp = prong_slots(pm)
        img = [i for i in range(len(pb)) if pb[i] == b and pp[i] == s - 1][0]
        hit = (pc[:, 0] == img) & (pc[:, 1] // tile[0] == ty) & (pc[:, 2] // tile[1] == tx)
        assert bool(hit.any())
        pc, pv = pc[~hit], pv[~hit]
    return f, x, ec.contiguous(), ev.contiguous(), em, pc.contiguous(), pv.contiguous(), pm


def brute_force(model, batch, index, tile, whole_map=False, device="cuda"):
    """forward() of `model` on event b alone for every variant of `index` -> (event logits [V, Ce], prong logits [V, P, Cp])."""
    evs, prs = [], []
    with torch.no_grad():
        for b, s, ty, tx in index.cpu().tolist():
            one = single_event(batch, b, (s, None, None) if whole_map else (s, ty, tx), tile)
            ev, pr = model.forward(*[t.to(device) for t in one])
            evs.append(ev[0].cpu())
            prs.append(pr[0].cpu())
    return torch.stack(evs), torch.stack(prs)


def valid_rows(prong_logits, index, prong_mask):
    """Rows of the valid prong slots of every variant's event, stacked: [sum, Cp]."""
    pm = prong_mask.cpu()
    out = [prong_logits[v][pm[b]] for v, b in enumerate(index[:, 0].tolist())]
    return torch.cat(out) if out else prong_logits.reshape(0, prong_logits.shape[-1])


def heat_reference(result, target="event"):
    """float64 [B, 1 + P, Ht, Wt] from the result's own logits."""
    ev, pr = result.event_logits.cpu().double(), result.prong_logits.cpu().double()
    oev, opr = result.occluded_event_logits.cpu().double(), result.occluded_prong_logits.cpu().double()
    B, P = pr.shape[0], pr.shape[1]
    out = torch.zeros(B, 1 + P, *result.grid, dtype=torch.float64)
    for v, (b, s, ty, tx) in enumerate(result.index.cpu().tolist()):
        if isinstance(target, str) and target == "prong":
            if s == 0:
                continue
            c = int(pr[b, s - 1].argmax())
            d = torch.softmax(pr[b, s - 1], 0)[c] - torch.softmax(opr[v, s - 1], 0)[c]
        else:
            c = int(ev[b].argmax()) if isinstance(target, str) else int(torch.as_tensor(target).reshape(-1).expand(B)[b])
            d = torch.softmax(ev[b], 0)[c] - torch.softmax(oev[v], 0)[c]
        out[b, s, ty, tx] = d
    return out


# ---- the variant lists themselves (test_occlusion_lists_gpu.py) -------------------------------------------------------------------------
def list_reference(coords, n_img, shape, tile, img_bs, max_pass, keep_map=None, curve=None):
    """What tcvn_occlusion_variants / _refine_variants (keep_map uint8 [B, S, parent Ht, parent Wt]) / _curve_variants (curve =
    (relevance float32 [B, S, Ht, Wt], steps, mode)) return for one COO list, by the rules alone: a variant's hit list is its image's
    rows, in original order, filtered by the variant's predicate; voff, bounds, V and nh are prefix sums of the row counts; the ranking
    is sorted(occupied tiles, key=(-relevance with -0.0 as +0.0, tile index)).
    -> dict: header [V, unsorted, bad, nh]; bounds (every word of the host buffer behind the header: bounds[k] = first row of pass k,
    the end of the last pass, zero behind it); vimg int32 [V]; index int32 [V, 4]; rows: per variant the positions in `coords` of its
    hits (meaningful for a list with neither flag set); rank int32 [B, S, Ht, Wt] (curves only; -1 where nothing is ranked)."""
    c = coords.cpu().long().reshape(-1, 3)
    bs = img_bs.cpu().long().reshape(n_img, 2)
    (H, W), (th, tw) = shape, tile
    Ht, Wt = grid_of(shape, tile)
    T = Ht * Wt
    img, y, x = c[:, 0], c[:, 1], c[:, 2]
    unsorted = bool((img[:-1] > img[1:]).any())
    inside = (img >= 0) & (img < n_img) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
    cell = (y // th) * Wt + x // tw                                   # read only where `inside`
    admitted = inside.clone()                                          # the hits that make their tile a variant
    if keep_map is not None:
        km = keep_map.cpu()
        b, s = bs[img.clamp(0, n_img - 1)].unbind(1)
        py, px = y // (2 * th), x // (2 * tw)
        named = inside & (b >= 0) & (b < km.shape[0]) & (s >= 0) & (s < km.shape[1]) & (py < km.shape[2]) & (px < km.shape[3])
        admitted = torch.zeros_like(inside)
        admitted[named] = km[b[named], s[named], py[named], px[named]] != 0
    of_image = [((img == i) & inside).nonzero().flatten() for i in range(n_img)]      # original order
    occupied = [sorted(set(cell[admitted & (img == i)].tolist())) for i in range(n_img)]
    variants = []                                                      # (image, two index words, the kept positions)
    out = {}
    if curve is None:
        total = n_img * T
        for i in range(n_img):
            for t in occupied[i]:
                variants.append((i, t // Wt, t % Wt, of_image[i][cell[of_image[i]] != t]))
    else:
        relevance, steps, mode = curve
        rel = relevance.cpu()
        total = n_img * (steps + 1)
        rank = torch.full(tuple(rel.shape), -1, dtype=torch.int32)
        for i in range(n_img):
            b, s = bs[i].tolist()
            if not (0 <= b < rel.shape[0] and 0 <= s < rel.shape[1]) or not occupied[i]:
                continue
            flat = rel[b, s].reshape(-1)
            order = sorted(occupied[i], key=lambda t: (-(float(flat[t]) + 0.0), t))      # x + 0.0 turns -0.0 into +0.0
            rk = torch.full((T,), -1, dtype=torch.long)
            rk[torch.tensor(order)] = torch.arange(len(order))
            rank[b, s] = rk.reshape(Ht, Wt).int()
            mine = of_image[i]
            for k in range(steps + 1):
                m = (k * len(order) + steps - 1) // steps
                top = rk[cell[mine]] < m
                variants.append((i, k, m, mine[top if mode == 1 else ~top]))           # mode 1: insertion
        out["rank"] = rank
    V = len(variants)
    voff = [0]
    for v in variants:
        voff.append(voff[-1] + int(v[3].numel()))
    nb = -(-total // max_pass)
    bounds = [0] * (nb + 1)
    for k in range(-(-V // max_pass)):
        bounds[k] = voff[k * max_pass]
    bounds[-(-V // max_pass)] = voff[V]
    out.update(header=[V, int(unsorted), int(bool((~inside).any())), voff[V]], bounds=bounds,
               vimg=torch.tensor([v[0] for v in variants], dtype=torch.int32),
               index=torch.tensor([[*bs[v[0]].tolist(), v[1], v[2]] for v in variants], dtype=torch.int32).reshape(V, 4),
               rows=[v[3] for v in variants])
    return out


def pass_reference(ref, coords, values, first, count):
    """The rows tcvn_occlusion_build_pass / _curve_build_pass write for variants first .. first + count - 1 of list_reference's `ref`:
    (out_coords int32 [n, 3] = (variant - first, y, x), out_values [n, C])."""
    c, v = coords.cpu(), values.cpu()
    oc, ov = [], []
    for j in range(count):
        at = ref["rows"][first + j]
        rows = c[at].clone()
        rows[:, 0] = j
        oc.append(rows)
        ov.append(v[at])
    return torch.cat(oc).reshape(-1, 3), torch.cat(ov).reshape(-1, v.shape[1])
