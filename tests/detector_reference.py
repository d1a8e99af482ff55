"""Host-side reference of the detector-effect scan (tests only): the Philox draws restated with numpy integers, one effect applied to a
COO list in torch float32 in the documented order (drop, dead, scale, threshold, shift), the variant list and its passes by the rules
alone, the brute force "plain forward() of the same model on event b alone with the perturbed lists", and the float64 response from a
result's own logits."""
import math

import numpy as np
import torch

import occlusion_reference as R

M32 = np.uint64(0xFFFFFFFF)


def philox4(c0, c1, c2, c3, k0, k1):
    """philox4 of csrc/tcvn_common.h line by line: Philox-4x32-10 on uint64 arrays that hold 32-bit words -> the four output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0                     # both factors are below 2^32: the product fits 64 bits
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        n0, n2 = hi1 ^ c1 ^ k0, hi0 ^ c3 ^ k1
        c0, c1, c2, c3 = n0, lo1, n2, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def drop_draws(y, x, b, s, W, seed):
    """float32 u in [0, 1) of every hit: (philox4(y * W + x, b, s, 0x44455453, seed_lo, seed_hi).x >> 8) * 2^-24."""
    pix = np.asarray(y, dtype=np.uint64) * np.uint64(W) + np.asarray(x, dtype=np.uint64)
    w0 = philox4(pix, np.asarray(b, dtype=np.uint64), np.asarray(s, dtype=np.uint64), 0x44455453, seed & 0xFFFFFFFF, seed >> 32)[0]
    return (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def apply_effect(coords, values, img_bs, effect, shape):
    """One effect on a COO list (coords [nnz, 3] = (image, y, x), every hit inside the map; values [nnz, C] float32; img_bs [n_img, 2] =
    (b, s) of every image) -> (positions of the surviving hits in the list, ascending; their coords after the shift; their values)."""
    c, v = coords.cpu().long().reshape(-1, 3), values.cpu().float()
    bs = torch.as_tensor(img_bs).cpu().long().reshape(-1, 2)
    H, W = shape
    img, y, x = c[:, 0], c[:, 1], c[:, 2]
    alive = torch.ones(c.shape[0], dtype=torch.bool)
    if effect.drop > 0 and c.shape[0]:                                            # 1. drop
        u = drop_draws(y.numpy(), x.numpy(), bs[img, 0].numpy(), bs[img, 1].numpy(), W, effect.seed)
        alive &= ~torch.from_numpy(u < np.float32(effect.drop))
    if effect.dead_rows is not None:                                              # 2. dead
        alive &= ~((y >= effect.dead_rows[0]) & (y < effect.dead_rows[1]))
    if effect.dead_cols is not None:
        alive &= ~((x >= effect.dead_cols[0]) & (x < effect.dead_cols[1]))
    v = v * torch.tensor(effect.scale, dtype=torch.float32)                       # 3. scale: one float32 multiplication
    if effect.threshold > 0:                                                      # 4. threshold
        v = torch.where(v < torch.tensor(effect.threshold, dtype=torch.float32), torch.zeros_like(v), v)
        alive &= (v != 0).any(1)
    out = c.clone()                                                               # 5. shift
    out[:, 1] += effect.shift[0]
    out[:, 2] += effect.shift[1]
    alive &= (out[:, 1] >= 0) & (out[:, 1] < H) & (out[:, 2] >= 0) & (out[:, 2] < W)
    at = alive.nonzero().flatten()
    return at, out[at].int(), v[at]


def list_reference(coords, values, n_img, shape, img_bs, effects, max_pass):
    """What tcvn_detector_variants returns for one clean COO list, by the rules alone -> dict: header [V, 0, 0, nh]; bounds (every word
    behind the header); vimg int32 [V]; index int32 [V, 4] = (b, s, k, surviving hits); hits: per variant its (coords, values)."""
    c = coords.cpu().long().reshape(-1, 3)
    bs = img_bs.cpu().long().reshape(n_img, 2)
    K = len(effects)
    per_effect = [apply_effect(coords, values, img_bs, e, shape) for e in effects]
    variants = []
    for i in range(n_img):
        if not bool((c[:, 0] == i).any()):
            continue
        for k in range(K):
            at, oc, ov = per_effect[k]
            mine = c[at, 0] == i
            variants.append((i, k, oc[mine], ov[mine]))
    V = len(variants)
    voff = [0]
    for v in variants:
        voff.append(voff[-1] + int(v[2].shape[0]))
    nb = -(-(n_img * K) // max_pass)
    bounds = [0] * (nb + 1)
    for p in range(-(-V // max_pass)):
        bounds[p] = voff[p * max_pass]
    bounds[-(-V // max_pass)] = voff[V]
    return dict(header=[V, 0, 0, voff[V]], bounds=bounds, vimg=torch.tensor([v[0] for v in variants], dtype=torch.int32),
                index=torch.tensor([[*bs[v[0]].tolist(), v[1], int(v[2].shape[0])] for v in variants], dtype=torch.int32).reshape(V, 4),
                hits=[(v[2], v[3]) for v in variants])


def pass_reference(ref, first, count, channels):
    """The rows tcvn_detector_build_pass writes for variants first .. first + count - 1: (out_coords int32 [n, 3] = (variant - first,
    y + dy, x + dx), out_values [n, C])."""
    oc, ov = [], []
    for j in range(count):
        rows, vals = ref["hits"][first + j]
        rows = rows.clone()
        rows[:, 0] = j
        oc.append(rows)
        ov.append(vals)
    return torch.cat(oc).reshape(-1, 3), torch.cat(ov).reshape(-1, channels)


def scanned_slots(batch, b, maps="all"):
    """The token slots of event b whose maps a scan with `maps` perturbs."""
    slots = [0] if maps in ("all", "event") else []
    if maps in ("all", "prongs"):
        slots += [1 + p for p in batch[7][b].cpu().nonzero().flatten().tolist()]
    return slots


def single_event_variant(batch, b, effect, shape, slots):
    """The 8 forward() inputs of event b alone with the maps of the token slots in `slots` under `effect`; the draws use the event's
    original (b, s).  Hit order is kept.  -> (inputs, {s: surviving hits} for the perturbed slots)."""
    f, x, e_c, e_v, em, p_c, p_v, pm = R.single_event(batch, b)
    prong_slot = batch[7][b].cpu().nonzero().flatten().tolist()                  # slot of local prong image j
    left = {}
    if 0 in slots:
        at, oc, ov = apply_effect(e_c, e_v, [[b, 0]], effect, shape)
        left[0] = int(at.numel())
        e_c, e_v = oc.to(e_c.dtype).contiguous(), ov.to(e_v.dtype).contiguous()
    mine = [j for j, p in enumerate(prong_slot) if 1 + p in slots]
    if mine:
        at, oc, ov = apply_effect(p_c, p_v, [[b, 1 + p] for p in prong_slot], effect, shape)       # the effect on every prong map ...
        touched = torch.isin(p_c[:, 0].long(), torch.tensor(mine))                                 # ... taken for the maps in `slots` only
        survives = torch.zeros(p_c.shape[0], dtype=torch.bool)
        survives[at] = True
        new_c, new_v = p_c.clone(), p_v.clone()
        new_c[at[touched[at]]], new_v[at[touched[at]]] = oc[touched[at]].to(p_c.dtype), ov[touched[at]].to(p_v.dtype)
        keep = ~touched | survives
        for j in mine:
            left[1 + prong_slot[j]] = int((keep & (p_c[:, 0] == j)).sum())
        p_c, p_v = new_c[keep].contiguous(), new_v[keep].contiguous()
    return (f, x, e_c, e_v, em, p_c, p_v, pm), left


def brute_force(model, batch, cases, shape, device="cuda"):
    """forward() of `model` on event b alone for every case (b, effect, slots) -> (event logits [n, Ce], prong logits [n, P, Cp], the
    surviving hits of every case as single_event_variant returns them)."""
    evs, prs, lefts = [], [], []
    with torch.no_grad():
        for b, effect, slots in cases:
            one, left = single_event_variant(batch, b, effect, shape, slots)
            ev, pr = model.forward(*[t.to(device) for t in one])
            evs.append(ev[0].cpu())
            prs.append(pr[0].cpu())
            lefts.append(left)
    return torch.stack(evs), torch.stack(prs), lefts


def random_result(scope, B=5, P=4, K=6, Ce=4, Cp=5, seed=1, device=None):
    """A hand-made DetectorScan with seeded random logits (no model): the prong slots of event b beyond 1 + b % P are padded; every other
    varied row is the base row plus a little noise (the arg-max stays), the rest are fresh rows (it mostly moves).  Scope map: one
    variant per (valid slot, k) except every fifth, so some valid maps have no variant."""
    from transformercvn.hip.detector import DetectorEffect, DetectorScan
    g = torch.Generator().manual_seed(seed)
    ev, pr = torch.randn(B, Ce, generator=g), torch.randn(B, P, Cp, generator=g)
    valid = torch.full((B, 1 + P), -1, dtype=torch.int32)
    for b in range(B):
        valid[b, :2 + b % P] = 0
    effects = tuple(DetectorEffect(scale=1.0 - 0.01 * k) for k in range(K))

    def varied(base, n):
        near = base + 1e-3 * torch.randn(base.shape, generator=g)
        pick = (torch.arange(n) % 2 == 0).reshape(-1, *([1] * (base.dim() - 1)))
        return torch.where(pick, near, torch.randn(base.shape, generator=g)).contiguous()

    if scope == "event":
        vev = varied(ev.repeat(K, 1), K * B).reshape(K, B, Ce)
        vpr = varied(pr.repeat(K, 1, 1), K * B).reshape(K, B, P, Cp)
        res = DetectorScan(ev, pr, effects, scope, valid, vev, vpr, surviving=torch.zeros(K, B, 1 + P, dtype=torch.int32))
    else:
        rows = [(b, s, k, 1) for b in range(B) for s in range(1 + P) if valid[b, s] >= 0 for k in range(K)]
        rows = [r for i, r in enumerate(rows) if i % 5 != 4]
        index = torch.tensor(rows, dtype=torch.int32)
        at = index[:, 0].long()
        res = DetectorScan(ev, pr, effects, scope, valid, varied(ev[at], len(rows)), varied(pr[at], len(rows)), index=index)
    if device is not None:
        for name in ("event_logits", "prong_logits", "valid", "varied_event_logits", "varied_prong_logits", "surviving", "index"):
            if getattr(res, name) is not None:
                setattr(res, name, getattr(res, name).to(device))
    return res


def response_reference(result, target="event"):
    """float64 (prob, delta) and bool flipped from the result's own logits, in the shapes of DetectorScan.response; NaN / False where
    there is nothing to compare."""
    ev, pr = result.event_logits.cpu().double(), result.prong_logits.cpu().double()
    vev, vpr = result.varied_event_logits.cpu().double(), result.varied_prong_logits.cpu().double()
    valid = result.valid.cpu()
    B, P, K = pr.shape[0], pr.shape[1], len(result.effects)
    prong = isinstance(target, str) and target == "prong"
    by_map = result.scope == "map"
    shape = (K, B, 1 + P) if by_map else (K, B, P) if prong else (K, B)
    prob, delta = torch.full(shape, math.nan, dtype=torch.float64), torch.full(shape, math.nan, dtype=torch.float64)
    flipped = torch.zeros(shape, dtype=torch.bool)

    def compare(base, varied, c, at):
        c = int(base.argmax()) if c is None else c
        p, p0 = torch.softmax(varied, 0)[c], torch.softmax(base, 0)[c]
        prob[at], delta[at], flipped[at] = p, p - p0, int(varied.argmax()) != int(base.argmax())

    def event_class(b):
        return None if isinstance(target, str) else int(torch.as_tensor(target).reshape(-1).expand(B)[b])

    if by_map:
        for v, (b, s, k, _) in enumerate(result.index.cpu().tolist()):
            if prong:
                if s > 0:
                    compare(pr[b, s - 1], vpr[v, s - 1], None, (k, b, s))
            else:
                compare(ev[b], vev[v], event_class(b), (k, b, s))
    else:
        for k in range(K):
            for b in range(B):
                if prong:
                    for p in range(P):
                        if valid[b, 1 + p] >= 0:
                            compare(pr[b, p], vpr[k, b, p], None, (k, b, p))
                else:
                    compare(ev[b], vev[k, b], event_class(b), (k, b))
    return prob, delta, flipped
