"""Float64 references of the hit-gradient pieces (tests only): the conv0 gather at the hits as a plain loop, the integrated-gradients
weights and completeness arithmetic, the heat-map painting as a loop, and the gradient of the float64 oracle at three cuts."""
import math

import torch
import torch.nn.functional as F

from oracle import tcvn_oracle as O


def owners(coords, n_img, H, W):
    """list index -> True when the entry owns its pixel: inside the maps and the highest index listed at its coordinate."""
    last = {}
    for i, (n, y, x) in enumerate(coords.tolist()):
        if 0 <= n < n_img and 0 <= y < H and 0 <= x < W:
            last[(n, y, x)] = i
    own = [False] * len(coords)
    for i in last.values():
        own[i] = True
    return own


def pre_derivative(values, value_mode):
    v = values.double()
    if value_mode == 0:
        return torch.full_like(v, 1.0 / 255.0)
    if value_mode == 1:
        return 1.0 / (v + 1.0)
    if value_mode == 2:
        return torch.ones_like(v)
    raise ValueError("one-hot pixels have no gradient")


def gather(e0, w0, coords, values, shape, value_mode):
    """e0 [n, Hc, Wc, N], w0 [N, C, 7, 7], coords [nnz, 3], values [nnz, C] -> float64 [nnz, C]: conv0 (7x7, stride 2, pad 3) data
    gradient at the hits, times the value transform's derivative; non-owning and outside entries 0."""
    e0, w0 = e0.double(), w0.double()
    n_img, Hc, Wc, N = e0.shape
    H, W = shape
    out = torch.zeros(values.shape, dtype=torch.float64)
    pre = pre_derivative(values, value_mode)
    own = owners(coords, n_img, H, W)
    for i, (n, y, x) in enumerate(coords.tolist()):
        if not own[i]:
            continue
        acc = torch.zeros(values.shape[1], dtype=torch.float64)
        for ky in range(7):
            if (y + 3 - ky) % 2:
                continue
            oy = (y + 3 - ky) // 2
            if not 0 <= oy < Hc:
                continue
            for kx in range(7):
                if (x + 3 - kx) % 2:
                    continue
                ox = (x + 3 - kx) // 2
                if not 0 <= ox < Wc:
                    continue
                acc += e0[n, oy, ox] @ w0[:, :, ky, kx]
        out[i] = acc * pre[i]
    return out


def gather_autograd(e0, w0, coords, values, shape, value_mode):
    """The same by torch autograd through a scattered map and F.conv2d(stride=2, padding=3) (a list without duplicates)."""
    n_img = e0.shape[0]
    v = values.double().clone().requires_grad_(True)
    t = v / 255.0 if value_mode == 0 else torch.log(v + 1.0) if value_mode == 1 else v
    img = torch.zeros(n_img, *shape, values.shape[1], dtype=torch.float64)
    c = coords.long()
    img = img.index_put((c[:, 0], c[:, 1], c[:, 2]), t)
    out = F.conv2d(img.permute(0, 3, 1, 2), w0.double(), None, stride=2, padding=3)
    (out.permute(0, 2, 3, 1) * e0.double()).sum().backward()
    return v.grad


def ig_weights(steps):
    return [((k + 0.5) / steps, 1.0 / steps) for k in range(steps)]


def integrated_gradients(grad_fn, values, steps):
    """grad_fn(list of scaled value tensors) -> list of gradients; midpoint rule along alpha * values -> the attributions (float64)."""
    acc = [torch.zeros_like(v, dtype=torch.float64) for v in values]
    for alpha, w in ig_weights(steps):
        for a, g in zip(acc, grad_fn([alpha * v for v in values])):
            a += w * g.double()
    return [a * v.double() for a, v in zip(acc, values)]


def completeness_gap(event_attr, prong_attr, event_img, prong_event, value, baseline):
    B = value.shape[0]
    tot = [0.0] * B
    for a, b in zip(event_attr.double().sum(1).tolist(), event_img.tolist()):
        tot[b] += a
    for a, b in zip(prong_attr.double().sum(1).tolist(), prong_event.tolist()):
        tot[b] += a
    return torch.tensor([abs(t - (float(v) - float(z))) for t, v, z in zip(tot, value, baseline)], dtype=torch.float64)


def heatmap(event_attr, prong_attr, event_coords, prong_coords, prong_mask, shape, tile, reduce):
    B, P = prong_mask.shape
    H, W = shape
    out = torch.zeros(B, 1 + P, -(-H // tile[0]), -(-W // tile[1]), dtype=torch.float64)
    slots = [(b, p + 1) for b in range(B) for p in range(P) if prong_mask[b, p]]
    for attr, coords, where in ((event_attr, event_coords, [(b, 0) for b in range(B)]), (prong_attr, prong_coords, slots)):
        for a, (n, y, x) in zip(attr.double(), coords.tolist()):
            b, s = where[n]
            out[b, s, y // tile[0], x // tile[1]] += float(a.abs().sum() if reduce == "abs" else a.sum())
    for b in range(B):
        for p in range(P):
            if not prong_mask[b, p]:
                out[b, 1 + p] = math.nan
    return out


# ---- the float64 oracle, differentiated ----------------------------------------------------------------------------------------------
def cast_state(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def score(ev, pr, prong_mask, target, value):
    """The scalar whose gradient hit_gradients returns: sum over events of the target's value.  target: [B] event classes, "prong", or a
    pair of raw seeds."""
    if isinstance(target, (tuple, list)):
        return (target[0].to(ev.dtype) * ev).sum() + (target[1].to(pr.dtype) * pr)[prong_mask].sum()
    if isinstance(target, str):
        s = pr if value == "logit" else pr.softmax(2)
        cls = pr.detach().argmax(2)
        return s.gather(2, cls.unsqueeze(2)).squeeze(2)[prong_mask].sum()
    s = ev if value == "logit" else ev.softmax(1)
    return s.gather(1, target.long().view(-1, 1)).sum()


def oracle_hit_gradients(sd, cfg, batch8, target, value="prob", dtype=torch.float64, values=None, autocast=False):
    """d score / d (event_values, prong_values) through O.forward(training=False); values: other hit values on the same coordinates."""
    sd = cast_state(sd, dtype)
    b = list(batch8)
    ev_v = (b[3] if values is None else values[0]).to(dtype).clone().requires_grad_(True)
    pr_v = (b[6] if values is None else values[1]).to(dtype).clone().requires_grad_(True)
    b[3], b[6] = ev_v, pr_v
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ev, pr, ctx = O.forward(sd, cfg, tuple(b), training=False)
        ev, pr = ev.float(), pr.float()
    else:
        ev, pr, ctx = O.forward(sd, cfg, tuple(b), training=False)
    g = torch.autograd.grad(score(ev, pr, b[7], target, value), [ev_v, pr_v])
    return g[0].double(), g[1].double(), ev.detach(), pr.detach()


def rel_l2(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


def cosine(got, ref):
    a, b = got.double().cpu().reshape(-1), ref.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm()))


def per_map_rel_l2(got, ref, coords):
    """The largest relative L2 error over the maps of a hit list (maps whose reference gradient is exactly zero must be exactly zero)."""
    worst = 0.0
    for n in coords[:, 0].unique().tolist():
        m = coords[:, 0] == n
        r = ref[m].double()
        d = (got[m].double().cpu() - r).norm()
        worst = max(worst, float(d / r.norm()) if float(r.norm()) > 0 else (0.0 if float(d) == 0 else math.inf))
    return worst
