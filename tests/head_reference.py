"""The token path alone (combined embedding -> transformer encoder -> decoders -> focal loss) on the CPU, in any dtype.

Nothing here is new arithmetic: the step is composed of the functions oracle/tcvn_oracle.py already has (linear_block, pack_indices,
encoder_forward, decoders_forward, training_loss, _Ctx with its mask_provider), which tests/test_oracle_golden.py pins to the
reference; tests/test_head_reference_cpu.py pins this composition to O.forward bit for bit.  The only step of its own is the gather of
the packed prong rows into [B, 1 + P, D] (what prong_embedding_forward does between its linear_block and the encoder).

Parameters come as {slot name: tensor} named as HeadEngine.slots() names them: state-dict keys minus "network.".  No GPU use."""
from types import SimpleNamespace

import torch

from oracle import tcvn_oracle as O

COMBINED = "network.prong_embedding.combined_embedding"
STAT_LEAVES = ("running_mean", "running_var", "num_batches_tracked")


def head_config(hidden=128, heads=8, layers=2, dec_layers=2, activation="gelu", norm_first=False, dropout=0.0, gamma=2.0,
                event_weight=0.5, event_classes=4, prong_classes=5, bn=True, prelu=True):
    """The oracle config of a head: only the keys the token path reads differ from the tutorial's."""
    return O.tutorial_config(hidden_dim=hidden, num_attention_heads=heads, num_encoder_layers=layers, num_prong_decoder_layers=dec_layers,
                             transformer_activation=activation, transformer_norm_first=norm_first, dropout=dropout, loss_gamma=gamma,
                             event_prong_loss_proportion=event_weight, num_event_classes=event_classes, num_prong_classes=prong_classes,
                             linear_batch_norm=bn, linear_prelu_activation=prelu)


def head_shapes(cfg, in_dim):
    """{slot name: shape} of every head tensor, from the oracle's state layout (the combined Linear reads in_dim columns)."""
    out = {}
    for k, shp in O.state_layout(cfg).items():
        if k.startswith(("network.encoder.", "network.event_decoder.", "network.prong_decoder.", COMBINED + ".")):
            out[k[len("network."):]] = (shp[0], in_dim) if k == COMBINED + ".linear.weight" else shp
    return out


def head_reference(params, cfg, rows, counts, P, event_targets=None, prong_targets=None, dtype=torch.float64, train=True,
                   mask_provider=None, seeds=None):
    """One head step in `dtype`.  params: {slot name: tensor} (any shape with the slot's element count); rows [B + nP, in_dim];
    counts: prongs per event; P: prong slots per event.  Dropout is applied only through mask_provider (cfg.dropout still decides
    the prong decoder's Sequential indices).  train: batch statistics, the loss and every gradient; else running statistics and logits.
    seeds = (d_ev [B, Ce], d_pr [B, P, Cp]) with train = False: the frozen backward -- d_rows is the gradient of
    sum d_ev * ev + sum over the valid prong slots of d_pr * pr on running statistics, no dropout, by torch autograd.
    -> namespace(event_logits [B, Ce], prong_logits [B, P, Cp], losses {total, event, prong}, d_rows, grads {slot name: tensor},
    new_running {slot name: tensor})."""
    B = len(counts)
    shapes = head_shapes(cfg, rows.shape[1])
    sd, leaves = {}, {}
    for name, shp in shapes.items():
        if name.endswith("num_batches_tracked"):
            continue
        t = params[name].detach().cpu().to(dtype).reshape(shp).clone()
        if train and not name.endswith(STAT_LEAVES):
            leaves[name] = t.requires_grad_(True)
        sd["network." + name] = t
    assert seeds is None or not train
    x = rows.detach().cpu().to(dtype).clone().requires_grad_(train or seeds is not None)
    ctx = O._Ctx(train, cfg.dropout if mask_provider is not None else 0.0, mask_provider)
    with torch.set_grad_enabled(train or seeds is not None):
        comb = O.linear_block(sd, COMBINED, cfg, x, ctx)
        prong_mask = torch.arange(P).view(1, P) < torch.tensor(counts).view(B, 1)
        I1, I2 = O.pack_indices(prong_mask)
        padded = torch.zeros(B, P, comb.shape[1], dtype=comb.dtype)
        padded[I1, I2] = comb[B:]
        tokens = torch.cat((comb[:B].view(B, 1, -1), padded), dim=1)
        mask = torch.cat((torch.ones(B, 1, dtype=torch.bool), prong_mask), dim=1)
        hidden = O.encoder_forward(sd, cfg, tokens, mask, ctx)
        ev, pr = O.decoders_forward(sd, cfg, hidden, ctx)
        out = SimpleNamespace(event_logits=ev.detach(), prong_logits=pr.detach(), losses=None, d_rows=None, grads={}, new_running={})
        if seeds is not None:
            d_ev, d_pr = (t.detach().cpu().to(dtype) for t in seeds)
            out.d_rows = torch.autograd.grad((d_ev * ev).sum() + (d_pr * pr)[prong_mask].sum(), x)[0]
        if not train:
            return out
        total, el, pl = O.training_loss(cfg, ev, pr, event_targets.cpu(), prong_targets.cpu())
    names = list(leaves)
    gs = torch.autograd.grad(total, [x] + [leaves[n] for n in names], allow_unused=True)
    out.losses = {"total": total.detach(), "event": el.detach(), "prong": pl.detach()}
    out.d_rows = gs[0]
    out.grads = {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs[1:])}
    out.new_running = {k[len("network."):]: v for k, v in ctx.new_running.items()}
    return out
