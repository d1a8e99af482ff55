"""Host-side reference of the tile Shapley scan (tests only): the occupied tiles of every map by integer arithmetic, the permutations by
the Python Philox of detector_reference.py and a Python sort, the variant list (b, s, m, k), the brute force "plain forward() of the same
model on event b alone with only the coalition's hits kept", the float64 Shapley formulas on a result's own logits and permutations, and
the same formulas on a toy value function."""
import itertools
import math

import numpy as np
import torch

import occlusion_curves_reference as CR
import occlusion_reference as R
from detector_reference import philox4

STREAM = 0x54534850          # "TSHP": the Philox stream constant of the tile permutation keys


def occupied(batch, tile, shape, maps="all"):
    """{(b, s): ascending tile indices ty * Wt + tx that hold a hit}, for every scanned map that holds one."""
    Wt = R.grid_of(shape, tile)[1]
    return {bs: sorted(ty * Wt + tx for ty, tx in tiles) for bs, tiles in CR.occupied_tiles(batch, tile, maps).items()}


def scanned_maps(batch, maps="all"):
    """(b, s) of every scanned map, with or without hits."""
    pm = batch[7].cpu()
    B, P = pm.shape
    out = [(b, 0) for b in range(B)] if maps in ("all", "event") else []
    if maps in ("all", "prongs"):
        out += [(b, 1 + p) for b in range(B) for p in range(P) if bool(pm[b, p])]
    return sorted(out)


def permutation(tiles, m, map_id, seed):
    """The tiles sorted by (key, t), key = word 0 of philox4(t, m, map_id, STREAM; seed)."""
    if not tiles:
        return []
    t = np.asarray(tiles, dtype=np.uint64)
    key = philox4(t, np.full_like(t, m), np.full_like(t, map_id), np.full_like(t, STREAM), np.full_like(t, seed & 0xffffffff),
                  np.full_like(t, seed >> 32))[0]
    return [tile for _, tile in sorted(zip(key.tolist(), tiles))]


def expected_lists(batch, tile, shape, max_exact, samples, seed, maps="all"):
    """-> (index int32 [V, 4] = (b, s, m, k) ascending, exact bool [B, 1 + P], n_tiles int32 [B, 1 + P], permutations int32
    [B, 1 + P, samples, Ht * Wt]) by the rules alone."""
    B, P = batch[7].shape
    Ht, Wt = R.grid_of(shape, tile)
    occ = occupied(batch, tile, shape, maps)
    exact = torch.zeros(B, 1 + P, dtype=torch.bool)
    n_tiles = torch.full((B, 1 + P), -1, dtype=torch.int32)
    perms = torch.full((B, 1 + P, samples, Ht * Wt), -1, dtype=torch.int32)
    rows = []
    for b, s in scanned_maps(batch, maps):
        tiles = occ.get((b, s), [])
        n = len(tiles)
        n_tiles[b, s] = n
        exact[b, s] = 1 <= n <= max_exact
        for m in range(samples):
            perms[b, s, m, :n] = torch.tensor(permutation(tiles, m, b * (1 + P) + s, seed), dtype=torch.int32)
        if n == 0:
            continue
        if exact[b, s]:
            rows += [(b, s, 0, k) for k in range(2 ** n - 1)]
        else:
            rows += [(b, s, 0, 0)] + [(b, s, m, k) for m in range(samples) for k in range(1, n)]
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4), exact, n_tiles, perms


def coalition(row, exact, perms):
    """The tiles of variant row = (b, s, m, k), from exact [B, 1 + P] and permutations [B, 1 + P, M, T] (any permutation of an exact
    map lists its occupied tiles; bit i of k is the i-th of them in ascending order)."""
    b, s, m, k = row
    if bool(exact[b, s]):
        tiles = sorted(t for t in perms[b, s, 0].tolist() if t >= 0)
        return {t for i, t in enumerate(tiles) if (k >> i) & 1}
    return set(perms[b, s, m, :k].tolist())


def brute_force(model, batch, index, exact, perms, tile, shape, device="cuda"):
    """forward() of `model` on event b alone, map s with only the hits of the coalition's tiles, for every variant of `index`
    -> (event logits [V, Ce], prong logits [V, P, Cp])."""
    Ht, Wt = R.grid_of(shape, tile)
    exact, perms = exact.cpu(), perms.cpu()
    evs, prs = [], []
    with torch.no_grad():
        for row in index.cpu().tolist():
            member = torch.ones(Ht * Wt, dtype=torch.long)              # "rank" 0 inside the coalition, 1 outside: insertion with m = 1
            for t in coalition(row, exact, perms):
                member[t] = 0
            one = CR.single_event_variant(batch, row[0], row[1], member.reshape(Ht, Wt), 1, tile, "insertion")
            ev, pr = model.forward(*[t.to(device) for t in one])
            evs.append(ev[0].cpu())
            prs.append(pr[0].cpu())
    return torch.stack(evs), torch.stack(prs)


# ---- the formulas ------------------------------------------------------------------------------------------------------------------------
def exact_shapley(v, n):
    """v: the 2^n coalition values, indexed by the bit mask -> phi [n] by full enumeration, float64."""
    phi = [0.0] * n
    for i in range(n):
        for c in range(2 ** n):
            if not (c >> i) & 1:
                size = bin(c).count("1")
                w = math.factorial(size) * math.factorial(n - size - 1) / math.factorial(n)
                phi[i] += w * (float(v[c | (1 << i)]) - float(v[c]))
    return phi


def permutation_shapley(value_of, n):
    """Brute force of the definition: the mean marginal over all n! orders; value_of(frozenset of players)."""
    phi = [0.0] * n
    orders = list(itertools.permutations(range(n)))
    for order in orders:
        have = set()
        for i in order:
            before = value_of(frozenset(have))
            have.add(i)
            phi[i] += value_of(frozenset(have)) - before
    return [p / len(orders) for p in phi]


def sampled_shapley(prefix_values, perms):
    """prefix_values[m][k]: the value of the first k players of permutation m (k = 0..n); perms[m]: the players in that order
    -> (mean [n], stderr [n]) indexed by the position of the player in sorted(perms[0]); float64."""
    M, players = len(perms), sorted(perms[0])
    d = {t: [] for t in players}
    for m in range(M):
        for j, t in enumerate(perms[m]):
            d[t].append(float(prefix_values[m][j + 1]) - float(prefix_values[m][j]))
    mean = [sum(d[t]) / M for t in players]
    se = [math.sqrt(sum((x - mu) ** 2 for x in d[t]) / (M - 1) / M) if M > 1 else 0.0 for t, mu in zip(players, mean)]
    return mean, se


def _value(row, c, value):
    row = row.double()
    return float(torch.softmax(row, 0)[c]) if value == "prob" else float(row[c])


def values_reference(result, target="event", value="prob"):
    """float64 (phi, stderr [B, 1 + P, Ht, Wt], full, empty [B, 1 + P]) from the result's own logits, index, exact, n_tiles and
    permutations; NaN at padded slots, at maps not scanned and, with target "prong", in row s = 0."""
    ev, pr = result.event_logits.cpu(), result.prong_logits.cpu()
    cev, cpr = result.coalition_event_logits.cpu(), result.coalition_prong_logits.cpu()
    index, exact, n_tiles, perms = (t.cpu() for t in (result.index, result.exact, result.n_tiles, result.permutations))
    B, P = pr.shape[0], pr.shape[1]
    Ht, Wt = result.grid
    M = result.samples
    phi = torch.full((B, 1 + P, Ht * Wt), math.nan, dtype=torch.float64)
    se = phi.clone()
    full = torch.full((B, 1 + P), math.nan, dtype=torch.float64)
    empty = full.clone()
    first = {}
    for v, (b, s, m, k) in enumerate(index.tolist()):
        first.setdefault((b, s), v)
    prong = isinstance(target, str) and target == "prong"
    for b in range(B):
        for s in range(1 + P):
            n = int(n_tiles[b, s])
            if n < 0 or (prong and s == 0):
                continue
            if prong:
                c = int(pr[b, s - 1].argmax())
                base, of = pr[b, s - 1], (lambda v: cpr[v, s - 1])
            else:
                c = int(ev[b].argmax()) if isinstance(target, str) else int(torch.as_tensor(target).reshape(-1).expand(B)[b])
                base, of = ev[b], (lambda v: cev[v])
            full[b, s] = _value(base, c, value)
            phi[b, s], se[b, s] = 0.0, 0.0
            if n == 0:
                empty[b, s] = full[b, s]
                continue
            st = first[(b, s)]
            empty[b, s] = _value(of(st), c, value)
            if bool(exact[b, s]):
                tiles = sorted(t for t in perms[b, s, 0].tolist() if t >= 0)
                vals = [_value(of(st + k), c, value) for k in range(2 ** n - 1)] + [float(full[b, s])]
                for t, p in zip(tiles, exact_shapley(vals, n)):
                    phi[b, s, t] = p
            else:
                orders = [perms[b, s, m, :n].tolist() for m in range(M)]
                prefix = [[float(empty[b, s])] + [_value(of(st + 1 + m * (n - 1) + k - 1), c, value) for k in range(1, n)]
                          + [float(full[b, s])] for m in range(M)]
                mean, err = sampled_shapley(prefix, orders)
                for t, p, e in zip(sorted(orders[0]), mean, err):
                    phi[b, s, t], se[b, s, t] = p, e
    return phi.reshape(B, 1 + P, Ht, Wt), se.reshape(B, 1 + P, Ht, Wt), full, empty
