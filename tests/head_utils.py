"""GPU-side helpers shared by the token-path tests: a bound HeadEngine with seeded parameters, a seeded batch, one train step, and the
kernels' own dropout masks in the layout the CPU oracle's mask_provider wants."""
import ctypes as C

import numpy as np
import torch

from oracle import tcvn_oracle as O
from head_reference import head_shapes

ENC_LAYER = "network.encoder.encoder.layers."


def legacy_fill(name, numel, g):
    """N(0, 0.1) everywhere; '*norm*' weights and running variances 1 + |n|."""
    t = torch.randn(numel, generator=g) * 0.1
    if "norm" in name and name.endswith(("weight", "running_var")):
        t = 1.0 + t.abs()
    return t


def scaled_fill(cfg, in_dim):
    """fill() for head_engine from the oracle's layout of the same head: matrices N(0, 1/fan_in); norm weights and running variances
    1 + |0.1 n|; PReLU slopes near 0.25; biases and running means N(0, 0.1).  Nothing is zero and nothing is one, so no term of a
    gradient can hide behind a neutral parameter."""
    shapes = head_shapes(cfg, in_dim)
    layout = {"network." + k: v for k, v in shapes.items()}

    def fill(name, numel, g):
        kind = O.tensor_kind("network." + name, layout)
        assert int(np.prod(shapes[name])) == numel, (name, shapes[name], numel)
        n = torch.randn(numel, generator=g)
        if kind == "matrix":
            return n / shapes[name][1] ** 0.5
        if kind in ("gamma", "running_var"):
            return 1.0 + (0.1 * n).abs()
        if kind == "prelu":
            return 0.25 + 0.05 * n
        return 0.1 * n
    return fill


def head_engine(seed, hidden=128, heads=8, layers=2, in_dim=40, dec_dims=(32, 16), norm_first=False, dropout=0.1, bn=True, prelu=True,
                activation="gelu", gamma=2.0, event_weight=0.5, event_classes=4, prong_classes=5, dec_out_in=None, fill=legacy_fill):
    """A bound HeadEngine with random parameters -> (engine, data, grads).  fill(name, numel, generator): one slot's values; the slots
    are drawn in slot order from one generator seeded with `seed`.  dec_out_in: the output layer's input width (default: the last
    decoder width, as the reference builds it when no decoder layer is cut short)."""
    from transformercvn.hip.engine import HeadEngine
    from transformercvn.hip import _lib
    dec_dims = list(dec_dims)
    if dec_out_in is None:
        dec_out_in = dec_dims[-1] if dec_dims else hidden
    eng = HeadEngine(hidden, heads, layers, in_dim, event_classes, prong_classes, dec_dims, dec_out_in, activation == "gelu", norm_first,
                     dropout, gamma, event_weight, bn, prelu)
    g = torch.Generator().manual_seed(seed)
    data, grads = {}, {}
    for name, numel, kind in eng.slots():
        if kind == _lib.SLOT_COUNTER:
            continue
        data[name] = fill(name, numel, g).float().cuda()
        if kind == _lib.SLOT_PARAM:
            grads[name] = torch.zeros(numel, device="cuda")
    eng.bind(data, grads)
    return eng, data, grads


def head_batch(seed, counts, P, in_dim, event_classes=4, prong_classes=5, min_rows=5):
    """rows [B + nP, in_dim], tok_row [B, 1 + P], event targets [B], prong targets [B, P] (-1 on padding) for the prong counts.
    min_rows: every BatchNorm1d of a train step must see at least this many rows -- the combined embedding sees B + nP, the prong
    decoder B * P.  (With two rows x-hat is +-1 whatever the input: the float32 oracle alone is then 3e-4 off its float64 self.)"""
    from transformercvn.network.layers.packed_data import token_rows
    g = torch.Generator().manual_seed(seed)
    B, nP = len(counts), sum(counts)
    assert B * P >= min_rows and B + nP >= min_rows, (B, P, nP)
    mask = torch.arange(P).view(1, P) < torch.tensor(counts).view(B, 1)
    rows = torch.randn(B + nP, in_dim, generator=g).cuda()
    et = torch.randint(0, event_classes, (B,), generator=g).cuda()
    pt = torch.where(mask, torch.randint(0, prong_classes, (B, P), generator=g), torch.tensor(-1)).to(torch.int8).cuda()
    return rows, token_rows(mask.cuda(), B), et, pt, nP


def head_train_step(eng, grads, rows, tok_row, et, pt, nP, seed):
    """One forward + loss + backward from zeroed gradients -> {name: tensor} of everything the step computes."""
    for v in grads.values():
        v.zero_()
    B, S = tok_row.shape
    ev, pr = eng.forward(rows, tok_row, B, S - 1, nP, True, seed)
    losses, accs, d_ev, d_pr = eng.loss(ev, pr, et, pt)
    d_rows = eng.backward(rows, tok_row, d_ev, d_pr)
    torch.cuda.synchronize()
    out = {"event_logits": ev, "prong_logits": pr, "losses": losses, "d_rows": d_rows}
    out.update({"grad:" + k: v.clone() for k, v in grads.items()})
    return out


# ---- dropout masks of the kernels, replayed through the oracle's mask_provider ----------------------------------------------------
def keep(kind, p, seed, sid, rows, cols):
    """tcvn_dropout_keep: the keep scale (0 or 1/(1-p)) of one site as a [rows, cols] device tensor."""
    from transformercvn.hip._lib import lib, check
    out = torch.empty(rows, cols, device="cuda")
    check(lib.tcvn_dropout_keep(kind, float(p), C.c_uint64(seed), C.c_uint32(sid), rows, cols, C.c_void_p(out.data_ptr()),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dropout_keep")
    return out


def head_site_id(site):
    """Stream id of a token-path dropout site of the oracle (oracle.tcvn_oracle._Ctx), None for any other site: combined embedding
    0x5000, encoder layer l 0x6000 + 8 l + {attention probabilities 0, attention branch 1, FFN activation 2, FFN branch 3}, prong
    decoder block i 0x7000 + i."""
    if site.endswith("combined_embedding"):
        return 0x5000
    if site.startswith(ENC_LAYER):
        l, kind = site[len(ENC_LAYER):].split(":")
        return 0x6000 + 8 * int(l) + {"attn": 0, "sa": 1, "ffn_act": 2, "ffn": 3}[kind]
    if site.startswith("decoder."):
        return 0x7000 + int(site.split(".")[1])
    return None


def head_site_keep(site, shape, p, seed):
    """The kernels' keep scale at a token-path site, in the oracle's layout `shape` (row-major element numbering in both)."""
    n = int(np.prod(shape))
    return keep(0, p, seed, head_site_id(site), n // shape[-1], shape[-1]).view(shape).cpu()


def head_mask_provider(p, seed):
    return lambda site, shape: head_site_keep(site, shape, p, seed)
