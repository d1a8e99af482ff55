"""CPU yardstick of the explanation features (tests only): the model's own holder modules (``network.encoder.encoder``, the stock
``nn.TransformerEncoder``, and ``network.event_decoder``) deep-copied to the CPU in eval mode and walked layer by layer through
``nn.MultiheadAttention(need_weights=True, average_attn_weights=False)``; the rollout formula in float64."""
import copy

import torch


def _cpu_eval(module, dtype=torch.float32):
    return copy.deepcopy(module).to("cpu", dtype).eval()


def walk(holder, tokens, mask, dtype=torch.float32):
    """holder: nn.TransformerEncoder; tokens [B, S, D]; mask [B, S] bool (True = valid) -> (hidden [S, B, D] masked like
    ProngCustomBertEncoder.forward, weights [L, B, H, S, S] with the rows of padded queries zeroed)."""
    enc = _cpu_eval(holder, dtype)
    mask = mask.cpu().bool()
    seq = mask.transpose(0, 1).unsqueeze(-1).to(dtype)
    x = tokens.detach().cpu().to(dtype).transpose(0, 1) * seq
    weights = []
    with torch.no_grad():
        for layer in enc.layers:
            if layer.norm_first:
                h = layer.norm1(x)
                a, w = layer.self_attn(h, h, h, key_padding_mask=~mask, need_weights=True, average_attn_weights=False)
                x = x + a
                x = x + layer.linear2(layer.activation(layer.linear1(layer.norm2(x))))
            else:
                a, w = layer.self_attn(x, x, x, key_padding_mask=~mask, need_weights=True, average_attn_weights=False)
                x = layer.norm1(x + a)
                x = layer.norm2(x + layer.linear2(layer.activation(layer.linear1(x))))
            weights.append(w * mask[:, None, :, None].to(dtype))
        if enc.norm is not None:
            x = enc.norm(x)
    return x * seq, torch.stack(weights)


def leave_one_out(holder, event_decoder, tokens, mask, dtype=torch.float32):
    """-> (event_logits [B, Ce], loo [B, S-1, Ce], n_variants): every valid prong of every event ablated (token zeroed, key padded);
    rows of padded slots are the unablated logits."""
    dec = _cpu_eval(event_decoder, dtype).hidden_layer
    tokens, mask = tokens.detach().cpu(), mask.cpu().bool()
    B, S, _ = tokens.shape
    with torch.no_grad():
        base = dec(walk(holder, tokens, mask, dtype)[0][0])
        where = [(b, s) for b in range(B) for s in range(1, S) if mask[b, s]]
        vt = torch.stack([tokens[b] for b, _ in where])
        vm = torch.stack([mask[b] for b, _ in where])
        for v, (_, s) in enumerate(where):
            vt[v, s] = 0
            vm[v, s] = False
        lg = dec(walk(holder, vt, vm, dtype)[0][0])
    loo = base[:, None, :].repeat(1, S - 1, 1)
    for v, (b, s) in enumerate(where):
        loo[b, s - 1] = lg[v]
    return base, loo, len(where)


def rollout(weights, mask, head_fusion="mean"):
    """float64: R = A^_{L-1} ... A^_0, A^_l = rownorm(0.5 fuse_h(weights[l]) + 0.5 I_valid)."""
    w = weights.detach().cpu().double()
    m = mask.cpu().double()
    L, B, H, S, _ = w.shape
    eye = torch.diag_embed(m)
    R = None
    for l in range(L):
        A = w[l].mean(1) if head_fusion == "mean" else w[l].max(1).values
        A = 0.5 * A + 0.5 * eye
        s = A.sum(-1, keepdim=True)
        A = torch.where(s > 0, A / s.clamp_min(1e-300), torch.zeros_like(A))
        R = A if R is None else A @ R
    return R


def ragged_mask(B, S, seed):
    """[B, S] bool: token 0 valid everywhere, event 0 without padding, event 1 with at least one padded slot, the rest random."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(B, S, generator=g) < 0.7
    mask[:, 0] = True
    mask[0] = True
    mask[1, S - 1] = False
    return mask
