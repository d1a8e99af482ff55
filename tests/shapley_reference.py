"""CPU yardstick of the prong Shapley scan (tests only).  A listed coalition is evaluated by the walk of the model's own holder modules
(attention_reference.walk) plus the CPU copy of the event decoder, as attention_reference.leave_one_out uses them; the values are reduced
by the defining formulas in float64: brute force over subsets, and over given permutations."""
import itertools
import math

import torch

import attention_reference as R


# ---- the coalition list: host integer arithmetic on the mask ---------------------------------------------------------------------------
def valid_slots(mask):
    """mask [B, S] bool -> per event the valid prong slots in ascending order (slot p = token 1 + p)."""
    m = mask.cpu().bool()
    return [[p for p in range(m.shape[1] - 1) if m[b, 1 + p]] for b in range(m.shape[0])]


def coalition_list(mask, max_exact, samples, permutations=None):
    """-> (offsets [B+1], event [J], masks [J], exact [B]) as Python ints.  Exact events: compact index k = 0 .. 2^n-1, bit i = the i-th
    valid slot.  Sampled events: empty, full, then per permutation m the prefixes of length 1 .. n-1 (permutations [B, M, P])."""
    offsets, event, masks, exact = [0], [], [], []
    for b, slots in enumerate(valid_slots(mask)):
        n = len(slots)
        exact.append(n <= max_exact)
        if exact[-1]:
            mine = [sum(1 << slots[i] for i in range(n) if (k >> i) & 1) for k in range(1 << n)]
        else:
            mine = [0, sum(1 << p for p in slots)]
            for m in range(samples):
                perm = [int(x) for x in permutations[b, m, :n]]
                mine += [sum(1 << p for p in perm[:length]) for length in range(1, n)]
        masks += mine
        event += [b] * len(mine)
        offsets.append(len(masks))
    return offsets, event, masks, exact


def coalition_logits(holder, event_decoder, tokens, mask, event, masks, chunk=2048):
    """Event logits [J, Ce] (float32, CPU) of the listed coalitions: event[j]'s tokens with every prong outside masks[j] zeroed and
    padded as a key; token 0 as the mask has it."""
    dec = R._cpu_eval(event_decoder).hidden_layer
    tokens, mask = tokens.detach().cpu(), mask.cpu().bool()
    S = tokens.shape[1]
    ev = torch.tensor(event, dtype=torch.int64)
    bits = torch.tensor([[True] + [bool((c >> p) & 1) for p in range(S - 1)] for c in masks], dtype=torch.bool).reshape(len(masks), S)
    out = []
    with torch.no_grad():
        for lo in range(0, len(masks), chunk):
            e = ev[lo:lo + chunk]
            vm = mask[e] & bits[lo:lo + chunk]
            vt = tokens[e] * vm.unsqueeze(-1)
            out.append(dec(R.walk(holder, vt, vm)[0][0]))
    return torch.cat(out)


def values(logits, kind):
    """logits [..., Ce] -> float64 values: the logits themselves or their softmax formed in float64."""
    x = logits.detach().cpu().double()
    return x if kind == "logit" else torch.softmax(x, -1)


# ---- the formulas, float64 -------------------------------------------------------------------------------------------------------------
def exact_phi(v):
    """v [2^n, Ce] float64 indexed by the compact coalition index -> phi [n, Ce], brute force over subsets."""
    n = int(math.log2(v.shape[0]))
    assert 1 << n == v.shape[0]
    phi = torch.zeros(n, v.shape[1], dtype=torch.float64)
    for i in range(n):
        for k in range(1 << n):
            if (k >> i) & 1:
                continue
            c = bin(k).count("1")
            w = math.factorial(c) * math.factorial(n - c - 1) / math.factorial(n)
            phi[i] += w * (v[k | (1 << i)] - v[k])
    return phi


def exact_interaction(v):
    """v [2^n, Ce] -> interaction [n, n, Ce], SHAP convention: off-diagonal half the Shapley interaction index, diagonal phi_i minus the
    rest of row i."""
    n = int(math.log2(v.shape[0]))
    phi = exact_phi(v)
    inter = torch.zeros(n, n, v.shape[1], dtype=torch.float64)
    for i, j in itertools.combinations(range(n), 2):
        bi, bj = 1 << i, 1 << j
        for k in range(1 << n):
            if k & (bi | bj):
                continue
            c = bin(k).count("1")
            w = math.factorial(c) * math.factorial(n - c - 2) / math.factorial(n - 1)
            inter[i, j] += 0.5 * w * (v[k | bi | bj] - v[k | bi] - v[k | bj] + v[k])
        inter[j, i] = inter[i, j]
    for i in range(n):
        inter[i, i] = phi[i] - inter[i].sum(0)
    return inter


def sampled_phi(perms, value_of):
    """perms: M orders of the same n players (lists); value_of(frozenset of players) -> [Ce] float64.  -> (phi, stderr) as dicts
    player -> [Ce]: mean and sample standard deviation / sqrt(M) of the marginal contributions."""
    M = len(perms)
    contrib = {p: [] for p in perms[0]}
    for perm in perms:
        have = frozenset()
        before = value_of(have)
        for p in perm:
            have = have | {p}
            after = value_of(have)
            contrib[p].append(after - before)
            before = after
    phi, se = {}, {}
    for p, rows in contrib.items():
        x = torch.stack(rows)
        phi[p] = x.mean(0)
        se[p] = x.std(0, unbiased=True) / math.sqrt(M) if M > 1 else torch.zeros_like(phi[p])
    return phi, se


def reduce_result(v, mask, max_exact, samples, permutations, offsets, masks):
    """The whole reduction in float64 on coalition values v [J, Ce] listed as coalition_list lists them -> (phi [B, P, Ce], stderr,
    interaction [B, P, P, Ce]) with zeros at padded slots and NaN interactions between the valid slots of sampled events."""
    m = mask.cpu().bool()
    B, P, Ce = m.shape[0], m.shape[1] - 1, v.shape[1]
    phi = torch.zeros(B, P, Ce, dtype=torch.float64)
    se = torch.zeros_like(phi)
    inter = torch.zeros(B, P, P, Ce, dtype=torch.float64)
    for b, slots in enumerate(valid_slots(m)):
        n = len(slots)
        mine = v[offsets[b]:offsets[b + 1]]
        if n <= max_exact:
            if n:
                idx = torch.tensor(slots)
                phi[b, idx] = exact_phi(mine)
                inter[b, idx[:, None], idx[None, :]] = exact_interaction(mine)
            continue
        row = {c: j for j, c in enumerate(masks[offsets[b]:offsets[b + 1]])}           # coalition mask -> row of this event

        def value_of(have):
            return mine[row[sum(1 << p for p in have)]]
        perms = [[int(x) for x in permutations[b, k, :n]] for k in range(samples)]
        ph, s = sampled_phi(perms, value_of)
        for p in slots:
            phi[b, p], se[b, p] = ph[p], s[p]
        idx = torch.tensor(slots)
        inter[b, idx[:, None], idx[None, :]] = float("nan")
    return phi, se, inter
