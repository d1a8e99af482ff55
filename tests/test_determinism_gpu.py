"""Run-to-run reproducibility of the bf16 DenseNet forward (train mode) and of the head's train step on the GPU.

The forward has no atomics: every repetition of the same step must be bit-identical.  This is the regression test for a
hazard inside the hand-scheduled MFMA chain of the 3x3 tile kernel (a VALU copy landing directly in front of an inline-asm
MFMA), which corrupted about one wave-tile in 10^4 and only showed as a rare parity failure."""
import pytest
import torch

from golden_utils import load_case, train_cfg
from oracle import tcvn_oracle as O

pytestmark = pytest.mark.gpu


def test_bf16_forward_is_bit_reproducible():
    import test_densenet_gpu as T
    cfg, over, batch, g = load_case("tutorial_b2p4")
    cfg = train_cfg(over)
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    n_img = int(batch[7].sum())
    eng, data, grads = T._engine(cfg, sd, mode=1, with_grad=False)
    coords, values = batch[5].cuda(), batch[6].cuda()
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    names = [f"dense{i + 1}" for i in range(len(cfg.densenet_structure))]
    first = None
    for rep in range(60):
        eng.forward(coords, values, n_img, out, train=True, seed=1)
        cur = [eng.tap(n).clone().view(torch.int16) for n in names] + [out.clone().view(torch.int32)]
        if first is None:
            first = cur
            continue
        for n, a, b in zip(names + ["out"], cur, first):
            assert torch.equal(a, b), f"repetition {rep}: {n} differs in {(a != b).sum().item()} elements"


def test_bf16_dense_layer_weight_gradients_are_bit_reproducible():
    """Round 5: the per-workgroup weight-gradient slabs are reduced in a fixed order (one y-slice per job, no fp32 atomics between slices:
    csrc/elementwise_bwd.hip, slab_reduce_body), and the forward statistics are integer sums (csrc/bn_lf.h): repeating the same train
    step must reproduce the dense layers' convolution weight gradients bit for bit.  (Not claimed for the stem's conv0 gradient and the
    exact-zero convolution biases: those still end in LDS / global fp32 atomics.)"""
    import test_densenet_gpu as T
    cfg, over, batch, g = load_case("tutorial_b2p4")
    cfg = train_cfg(over)
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    n_img = int(batch[7].sum())
    eng, data, grads = T._engine(cfg, sd, mode=1, with_grad=True)
    coords, values = batch[5].cuda(), batch[6].cuda()
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    d_out = torch.randn(n_img, eng.out_dim, generator=torch.Generator().manual_seed(3)).cuda()
    keys = [k for k in grads if ".dense" in k and k.endswith(("conv1.weight", "conv2.weight"))]
    assert len(keys) == 2 * sum(cfg.densenet_structure)
    first = None
    for rep in range(6):
        for v in grads.values():
            v.zero_()
        eng.forward(coords, values, n_img, out, train=True, seed=1)
        eng.backward(d_out)
        torch.cuda.synchronize()
        cur = {k: grads[k].clone().view(torch.int32) for k in keys}
        assert all(torch.isfinite(grads[k]).all() and grads[k].abs().max() > 0 for k in keys)
        if first is None:
            first = cur
            continue
        diff = [k for k in keys if not torch.equal(cur[k], first[k])]
        assert not diff, f"repetition {rep}: {len(diff)} of {len(keys)} weight gradients differ, e.g. {diff[:3]}"


# ---- head (token path) ---------------------------------------------------------------------------------------------------------------
def head_engine(seed, hidden=128, heads=8, layers=2, in_dim=40, dec_dims=(32, 16), norm_first=False, dropout=0.1, bn=True, prelu=True):
    """A bound HeadEngine with random parameters (BatchNorm weights near one, running variances positive) -> (engine, data, grads)."""
    from transformercvn.hip.engine import HeadEngine
    from transformercvn.hip import _lib
    dec_dims = list(dec_dims)
    eng = HeadEngine(hidden, heads, layers, in_dim, 4, 5, dec_dims, dec_dims[-1] if dec_dims else hidden, True, norm_first, dropout,
                     2.0, 0.5, bn, prelu)
    g = torch.Generator().manual_seed(seed)
    data, grads = {}, {}
    for name, numel, kind in eng.slots():
        if kind == _lib.SLOT_COUNTER:
            continue
        t = torch.randn(numel, generator=g) * 0.1
        if "norm" in name and name.endswith(("weight", "running_var")):
            t = 1.0 + t.abs()
        data[name] = t.cuda()
        if kind == _lib.SLOT_PARAM:
            grads[name] = torch.zeros(numel, device="cuda")
    eng.bind(data, grads)
    return eng, data, grads


def head_batch(seed, counts, P, in_dim):
    """rows [B + nP, in_dim], tok_row [B, 1 + P], event targets [B], prong targets [B, P] (-1 on padding) for the prong counts."""
    from transformercvn.network.layers.packed_data import token_rows
    g = torch.Generator().manual_seed(seed)
    B, nP = len(counts), sum(counts)
    mask = torch.arange(P).view(1, P) < torch.tensor(counts).view(B, 1)
    rows = torch.randn(B + nP, in_dim, generator=g).cuda()
    et = torch.randint(0, 4, (B,), generator=g).cuda()
    pt = torch.where(mask, torch.randint(0, 5, (B, P), generator=g), torch.tensor(-1)).to(torch.int8).cuda()
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


@pytest.mark.parametrize("path", ["fused", "post_norm", "pre_norm"])
def test_head_step_is_bit_reproducible(path):
    """rows.hip, encoder.hip, encoder_fused.hip and head.hip contain no atomic operation and the dropout masks are a function of
    (seed, stream id, element): the same head train step (dropout 0.1) repeated from zeroed gradients reproduces logits, losses, the
    input gradient and every parameter gradient bit for bit, on each of the three encoder paths.  B = 3 with prong counts [1, 4, 2]
    of P = 4 (S = 5): padding in two sequences, more than one event, more than one prong."""
    from transformercvn.hip._lib import lib
    eng, data, grads = head_engine(11, norm_first=path == "pre_norm")
    if path == "post_norm":
        lib.tcvn_head_set_fused_encoder(eng.handle, 0)
    batch = head_batch(12, [1, 4, 2], 4, eng.cfg.in_dim)
    first = None
    for rep in range(3):
        cur = head_train_step(eng, grads, *batch, seed=77)
        for k, v in cur.items():
            assert torch.isfinite(v).all(), k
            if k.startswith("grad:") or k == "d_rows":
                assert v.abs().max() > 0, k
        if first is None:
            first = cur
            continue
        diff = [k for k in cur if not torch.equal(cur[k].view(torch.int32), first[k].view(torch.int32))]
        assert not diff, f"repetition {rep}: {len(diff)} of {len(cur)} tensors differ, e.g. {diff[:3]}"
