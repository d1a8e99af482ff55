"""HeadEngine (combined embedding, transformer encoder, decoders, focal loss: rows.hip, encoder.hip, encoder_fused.hip, head.hip)
against tests/head_reference.py in float64, one train step and one eval forward per case, on every encoder path, block option and
loss branch the project ships.

Metric: err(t) = ||hip - ref64|| / ||ref64|| per tensor.  Gauge: the same reference run in float32 on the CPU gives e32(t); the bound
is max(K * e32(t), 2e-6) (floor: about twice fp32 epsilon * sqrt(320), the rounding of one in_dim-long dot product).

Measured on an MI355X, largest err / e32 over the tensors whose err is above the floor (below it the floor decides, not K), per path:
    fused encoder (train)                  1.39   S9_layers8, layers.0.norm1.weight gradient (err 4.0e-6, e32 2.9e-6)
    row kernels, post-norm (train)         1.51   S9_layers8 with the fused encoder off, a prong decoder weight gradient (2.7e-6 / 1.8e-6)
    row kernels, pre-norm (train)          1.84   dropout_pre_norm_S9, event loss (2.5e-6 / 1.3e-6)
    eval logits, every path                none above the floor (largest err 8.0e-7)
    frozen d_rows, every path              none above the floor (largest err 8.5e-7, S9_layers8 with the fused encoder off; largest err / e32
                                           1.08, S23; frozen logits: largest err 5.3e-7, bit-equal to the eval forward's)
Largest err of any tensor: 4.4e-6 (d_rows, 8 layers); every 2-layer case stays under 1e-6 but for pre-norm with dropout.  The kernels'
summation orders, MFMA 16x16x4 f32 products and erff / expf sit as close to float64 as torch's float32 does.
K = 4: twice the largest ratio (1.84), rounded up to a power of two.
The frozen leg (test_head_frozen_backward_...: forward_frozen + input_gradient behind a train step on the same engine and workspace, all
17 cases, random logit seeds with the padded slots zeroed) holds d_rows to the same bound with the same K; it also asserts that the
frozen logits are the eval forward's bit for bit, that on the fused path switching the fused encoder off changes some bit, that the
bound gradient tensors (filled with a NaN pattern) and the running statistics keep their bits, and that the dropout cases give the
d_rows of an engine configured with dropout 0.

Two traps (both asserted):
  * the gradient of a Linear bias that feeds a train-mode BatchNorm1d is analytically zero (1e-17 in float64, 1e-8 in float32): such
    tensors are found by ||ref64|| < 1e-9 * (largest gradient norm of the case), must be exactly the prong decoder's Linear biases when
    the blocks have a BatchNorm1d and none otherwise, and must satisfy ||hip|| <= max(K * ||float32 oracle's value||, 1e-6 * g_max);
  * a BatchNorm1d over two rows has x-hat = +-1 for any input and is ill-conditioned in float32 already: head_batch refuses a batch whose
    BatchNorm1ds would see fewer than 5 rows."""
import pytest
import torch

from head_reference import head_config, head_reference, head_shapes
from head_utils import head_batch, head_engine, head_mask_provider, head_train_step, scaled_fill
from oracle import tcvn_oracle as O

pytestmark = pytest.mark.gpu

K = 4                       # twice the largest err / e32 measured (1.84), rounded up to a power of two; may not exceed 32
FLOOR = 2e-6
IN_DIM = 40
SEED = 77                   # dropout seed of the train step

# case -> engine options (defaults: hidden 128, 8 heads, 2 layers, GELU, post-norm, BatchNorm1d + PReLU blocks, gamma 2.0, event
# weight 0.5, 4 / 5 classes, dropout 0) and prong counts (P = max count).  path: the encoder kernels the case must reach.
CASES = {
    "S2": dict(layers=1, counts=[1, 0, 1, 1, 1], path="fused"),                    # smallest sequence with a prong; bucket 3 mostly padding
    "S6": dict(counts=[5, 0, 3], path="fused"),                                   # last length of bucket 3; zero-prong event
    "S7_heads4_relu": dict(heads=4, activation="relu", counts=[6, 1], path="fused"),      # first of bucket 5; <32, 5>; ReLU
    "S11": dict(counts=[10, 2, 0, 7], path="fused"),                              # first of bucket 8
    "S17_heads4": dict(heads=4, counts=[16, 1, 5], path="fused"),                 # <32, 11> backward
    "S22": dict(counts=[21, 3], path="fused"),                                    # last fused length
    "S23": dict(counts=[22, 3], path="rows"),                                     # first length of the row kernels
    "S64": dict(layers=1, counts=[63, 1, 30], path="rows"),                       # limit of k_attn_*
    "S9_unfused_relu": dict(activation="relu", counts=[8, 0, 4], fused=False, path="rows"),
    "S9_pre_norm": dict(norm_first=True, counts=[8, 0, 4], path="rows"),
    "S9_layers8": dict(layers=8, counts=[8, 2], path="fused"),                    # ENC_MAX_LAYERS
    "hidden64_heads2": dict(hidden=64, heads=2, dec_layers=3, counts=[4, 1, 2], path="rows"),     # head_dim 32 = MAXHD; decoder 32, 16, 8
    "no_bn_relu_blocks": dict(bn=False, prelu=False, counts=[4, 1, 2], path="fused"),      # Linear bias path, no statistics
    "gamma0": dict(layers=1, gamma=0.0, counts=[3, 2], path="fused"),             # cross-entropy branch of k_focal
    "dropout_fused_S6": dict(dropout=0.1, counts=[5, 0, 3], path="fused"),
    "dropout_rows_S23": dict(dropout=0.1, counts=[22, 3], path="rows"),
    "dropout_pre_norm_S9": dict(dropout=0.1, norm_first=True, counts=[8, 0, 4], path="rows"),
}


def _build(case, seed=5):
    """-> (cfg, engine, initial parameters on the CPU, data, grads)."""
    o = dict(CASES[case])
    counts, path, fused = o.pop("counts"), o.pop("path"), o.pop("fused", True)
    dec_layers = o.pop("dec_layers", 2)
    o.setdefault("dropout", 0.0)
    cfg = head_config(dec_layers=dec_layers, **o)
    dims, final = O.prong_decoder_dims(cfg)
    eng, data, grads = head_engine(seed, in_dim=IN_DIM, dec_dims=[w for _, w in dims], dec_out_in=final, fill=scaled_fill(cfg, IN_DIM), **o)
    if not fused:
        _fused(eng, False)
    return cfg, eng, {k: v.cpu().clone() for k, v in data.items()}, data, grads, counts, path


def _fused(eng, on):
    from transformercvn.hip._lib import lib
    lib.tcvn_head_set_fused_encoder(eng.handle, int(on))


def _rel(a, ref):
    a, ref = a.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    return ((a - ref).norm() / ref.norm()).item()


class _Report:
    """Collects err, e32 and their ratio per tensor; asserts the bound; remembers the largest ratio among tensors above the floor."""

    def __init__(self, case):
        self.case, self.worst, self.fail = case, 0.0, []

    def check(self, name, hip, ref64, ref32):
        assert torch.isfinite(hip).all(), (self.case, name)
        err, e32 = _rel(hip, ref64), _rel(ref32, ref64)
        ratio = err / e32 if e32 > 0 else float("inf")
        if err > FLOOR:
            self.worst = max(self.worst, ratio)
        print(f"  {self.case:22s} {name:60s} err {err:.2e} e32 {e32:.2e} ratio {ratio:8.2f}{'' if err > FLOOR else '  (under the floor)'}")
        if not err <= max(K * e32, FLOOR):
            self.fail.append((name, err, e32))

    def done(self):
        print(f"{self.case}: largest err / e32 above the floor: {self.worst:.2f}")
        assert not self.fail, (self.case, self.fail)


def _compare_step(rep, tag, out, data, r64, r32, valid, zero, g_max):
    rep.check(tag + "event_logits", out["event_logits"], r64.event_logits, r32.event_logits)
    rep.check(tag + "prong_logits[valid]", out["prong_logits"].cpu()[valid], r64.prong_logits[valid], r32.prong_logits[valid])
    for i, k in enumerate(("total", "event", "prong")):
        rep.check(tag + "loss." + k, out["losses"][i], r64.losses[k], r32.losses[k])
    rep.check(tag + "d_rows", out["d_rows"], r64.d_rows, r32.d_rows)
    compared = set()
    for k in r64.grads:
        hip = out["grad:" + k]
        compared.add(k)
        if k in zero:                                        # analytically zero: no relative error exists
            assert torch.isfinite(hip).all(), k
            n_hip, n32 = hip.double().norm().item(), r32.grads[k].double().norm().item()
            print(f"  {rep.case:22s} {tag + 'grad:' + k:60s} analytically zero: |hip| {n_hip:.2e} |fp32 oracle| {n32:.2e} g_max {g_max:.2e}")
            assert n_hip <= max(K * n32, 1e-6 * g_max), (rep.case, k, n_hip, n32, g_max)
            continue
        assert hip.abs().max() > 0, (rep.case, k)
        rep.check(tag + "grad:" + k, hip, r64.grads[k], r32.grads[k])
    for k in r64.new_running:
        rep.check(tag + k, data[k], r64.new_running[k], r32.new_running[k])
    return compared


@pytest.mark.parametrize("case", list(CASES))
def test_head_step_matches_the_float64_reference(case):
    from transformercvn.hip import _lib
    cfg, eng, p0, data, grads, counts, path = _build(case)
    P = max(counts)
    rows, tok_row, et, pt, nP = head_batch(6, counts, P, IN_DIM, cfg.num_event_classes, cfg.num_prong_classes)
    B = len(counts)
    valid = (pt >= 0).cpu()
    rep = _Report(case)

    # ---- eval forward, with the running statistics that were bound (before the train step moves them) ---------------------------
    ev, pr = eng.forward(rows, tok_row, B, P, nP, False, 0)
    torch.cuda.synchronize()
    e64 = head_reference(p0, cfg, rows, counts, P, dtype=torch.float64, train=False)
    e32 = head_reference(p0, cfg, rows, counts, P, dtype=torch.float32, train=False)
    rep.check("eval:event_logits", ev, e64.event_logits, e32.event_logits)
    rep.check("eval:prong_logits", pr, e64.prong_logits, e32.prong_logits)     # padded positions too: the decoder reads the masked hidden state

    # ---- one train step ------------------------------------------------------------------------------------------------------------
    provider = head_mask_provider(cfg.dropout, SEED) if cfg.dropout > 0 else None
    r64 = head_reference(p0, cfg, rows, counts, P, et, pt, torch.float64, True, provider)
    r32 = head_reference(p0, cfg, rows, counts, P, et, pt, torch.float32, True, provider)
    gnorm = {k: v.norm().item() for k, v in r64.grads.items()}
    g_max = max(gnorm.values())
    zero = {k for k, n in gnorm.items() if n < 1e-9 * g_max}
    shapes = head_shapes(cfg, IN_DIM)
    dec_bias = {k for k in shapes if k.startswith("prong_decoder.hidden_layers.") and k.endswith(".bias")
                and len(shapes[k[:-len("bias")] + "weight"]) == 2}
    assert len(dec_bias) == len(O.prong_decoder_dims(cfg)[0])
    assert zero == (dec_bias if cfg.linear_batch_norm else set()), (case, sorted(zero))

    out = head_train_step(eng, grads, rows, tok_row, et, pt, nP, SEED)
    compared = _compare_step(rep, "train:", out, data, r64, r32, valid, zero, g_max)
    params = {n for n, _, kind in eng.slots() if kind == _lib.SLOT_PARAM}
    buffers = {n for n, _, kind in eng.slots() if kind == _lib.SLOT_BUFFER}
    assert params == compared, (case, sorted(params ^ compared))
    assert buffers == set(r64.new_running), (case, sorted(buffers ^ set(r64.new_running)))

    # ---- the path the case is listed for ----------------------------------------------------------------------------------------------
    if path == "fused":
        # the row kernels at the same length, from the same start (running statistics back to what was bound)
        for k in buffers:
            data[k].copy_(p0[k])
        _fused(eng, False)
        out_rows = head_train_step(eng, grads, rows, tok_row, et, pt, nP, SEED)
        _compare_step(rep, "train(rows):", out_rows, data, r64, r32, valid, zero, g_max)
        same = all(torch.equal(out[k].view(torch.int32), out_rows[k].view(torch.int32)) for k in out)
        assert not same, f"{case}: the fused encoder was to run here, yet switching it off changes no bit"
    elif CASES[case].get("fused", True):
        # the switch is on and must not matter: this length / width / norm order belongs to the row kernels
        for k in buffers:
            data[k].copy_(p0[k])
        _fused(eng, False)
        out_rows = head_train_step(eng, grads, rows, tok_row, et, pt, nP, SEED)
        diff = [k for k in out if not torch.equal(out[k].view(torch.int32), out_rows[k].view(torch.int32))]
        assert not diff, f"{case}: fused encoder on / off differ in {diff[:3]}: the fused kernels ran where the row kernels must"
    rep.done()


ARENA_PATTERN = 0x7FA5C3E1   # bits of a NaN: the bound gradient tensors hold them while a frozen backward runs


def _frozen(eng, rows, tok_row, B, P, nP, d_ev, d_pr):
    ev, pr = eng.forward_frozen(rows, tok_row, B, P, nP)
    d_rows = eng.input_gradient(rows, tok_row, d_ev, d_pr)
    torch.cuda.synchronize()
    return ev, pr, d_rows


@pytest.mark.parametrize("case", list(CASES))
def test_head_frozen_backward_matches_the_float64_reference(case):
    """forward_frozen + input_gradient (the data-only backward of hit gradients: running statistics, dropout 0, no parameter gradient) on
    every case of the train test, behind one train step on the same engine and workspace."""
    from transformercvn.hip import _lib
    cfg, eng, p0, data, grads, counts, path = _build(case)
    P = max(counts)
    rows, tok_row, et, pt, nP = head_batch(6, counts, P, IN_DIM, cfg.num_event_classes, cfg.num_prong_classes)
    B = len(counts)
    valid = (pt >= 0)
    buffers = {n for n, _, kind in eng.slots() if kind == _lib.SLOT_BUFFER}
    head_train_step(eng, grads, rows, tok_row, et, pt, nP, SEED)             # the workspace now holds a train step's state
    for k in buffers:
        data[k].copy_(p0[k])                                                # running statistics back to what was bound
    g = torch.Generator().manual_seed(31)
    d_ev = torch.randn(B, cfg.num_event_classes, generator=g).cuda()
    d_pr = (torch.randn(B, P, cfg.num_prong_classes, generator=g).cuda() * valid.unsqueeze(2)).contiguous()      # padded slots zeroed, as the runtime does
    for t in grads.values():
        t.view(torch.int32).fill_(ARENA_PATTERN)
    ev, pr, d_rows = _frozen(eng, rows, tok_row, B, P, nP, d_ev, d_pr)
    assert all(bool((t.view(torch.int32) == ARENA_PATTERN).all()) for t in grads.values()), "a frozen backward wrote a parameter gradient"
    assert all(torch.equal(data[k].cpu(), p0[k]) for k in buffers), "running statistics moved"
    ev_e, pr_e = eng.forward(rows, tok_row, B, P, nP, False, 0)
    torch.cuda.synchronize()
    assert torch.equal(ev, ev_e) and torch.equal(pr, pr_e), "the frozen forward is the eval forward"
    r64 = head_reference(p0, cfg, rows, counts, P, dtype=torch.float64, train=False, seeds=(d_ev, d_pr))
    r32 = head_reference(p0, cfg, rows, counts, P, dtype=torch.float32, train=False, seeds=(d_ev, d_pr))
    rep = _Report(case)
    assert r64.d_rows.abs().max() > 0
    rep.check("frozen:event_logits", ev, r64.event_logits, r32.event_logits)
    rep.check("frozen:d_rows", d_rows, r64.d_rows, r32.d_rows)
    if path == "fused":
        _fused(eng, False)
        ev_r, pr_r, d_rows_r = _frozen(eng, rows, tok_row, B, P, nP, d_ev, d_pr)
        rep.check("frozen(rows):d_rows", d_rows_r, r64.d_rows, r32.d_rows)
        same = torch.equal(d_rows.view(torch.int32), d_rows_r.view(torch.int32)) and torch.equal(ev.view(torch.int32), ev_r.view(torch.int32))
        assert not same, f"{case}: the fused encoder was to run here, yet switching it off changes no bit"
        _fused(eng, True)
    if cfg.dropout > 0:
        # the frozen pass ignores dropout: an engine with dropout 0 and the same parameters gives the same bits
        o = dict(CASES[case], dropout=0.0)
        for k in ("counts", "path", "fused"):
            o.pop(k, None)
        dec_layers = o.pop("dec_layers", 2)
        cfg0 = head_config(dec_layers=dec_layers, **o)
        dims, final = O.prong_decoder_dims(cfg0)
        eng0, data0, _ = head_engine(5, in_dim=IN_DIM, dec_dims=[w for _, w in dims], dec_out_in=final, fill=scaled_fill(cfg0, IN_DIM), **o)
        assert [v.numel() for v in data0.values()] == [v.numel() for v in data.values()]
        for v0, v in zip(data0.values(), data.values()):
            v0.copy_(v)
        _, _, d_rows0 = _frozen(eng0, rows, tok_row, B, P, nP, d_ev, d_pr)
        assert torch.equal(d_rows0, d_rows), f"{case}: dropout {cfg.dropout} configured changes the frozen d_rows"
    assert all(bool((t.view(torch.int32) == ARENA_PATTERN).all()) for t in grads.values())
    rep.done()


def test_eval_without_any_prong_returns_the_event_logits():
    """P = 0 (S = 1): every event is its event token alone.  The reference has no prong loss there (mean over no row) and its
    decoder cannot reshape an empty matrix, so the reference is run with ONE all-padding slot per event: a padded key is masked out
    of every attention row and the event decoder reads token 0 only, so its event logits are those of P = 0."""
    cfg = head_config(dropout=0.0)
    dims, final = O.prong_decoder_dims(cfg)
    eng, data, grads = head_engine(5, in_dim=IN_DIM, dec_dims=[w for _, w in dims], dec_out_in=final, dropout=0.0,
                                   fill=scaled_fill(cfg, IN_DIM))
    p0 = {k: v.cpu().clone() for k, v in data.items()}
    rows, tok_row, et, pt, nP = head_batch(6, [0, 0, 0], 0, IN_DIM, min_rows=0)
    assert tok_row.shape == (3, 1) and nP == 0
    ev, pr = eng.forward(rows, tok_row, 3, 0, 0, False, 0)
    torch.cuda.synchronize()
    assert pr.shape == (3, 0, cfg.num_prong_classes)
    e64 = head_reference(p0, cfg, rows, [0, 0, 0], 1, dtype=torch.float64, train=False)
    e32 = head_reference(p0, cfg, rows, [0, 0, 0], 1, dtype=torch.float32, train=False)
    rep = _Report("P0_eval")
    rep.check("eval:event_logits", ev, e64.event_logits, e32.event_logits)
    rep.done()


# ---- host checks: refusals are return codes, no kernel is involved in what is refused ------------------------------------------------
def test_more_than_64_tokens_are_refused():
    eng, data, grads = head_engine(5, dropout=0.0)
    rows, tok_row, et, pt, nP = head_batch(6, [64, 1], 64, IN_DIM)
    with pytest.raises(RuntimeError, match="code -1"):
        eng.forward(rows, tok_row, 2, 64, nP, False, 0)


def test_head_dim_64_is_refused():
    eng, data, grads = head_engine(5, hidden=64, heads=1, dropout=0.0)
    rows, tok_row, et, pt, nP = head_batch(6, [4, 1, 2], 4, IN_DIM)
    with pytest.raises(RuntimeError, match="code -2"):
        eng.forward(rows, tok_row, 3, 4, nP, False, 0)
    torch.cuda.synchronize()


def test_decoder_output_width_mismatch_is_refused():
    eng, data, grads = head_engine(5, dec_dims=(32, 16), dec_out_in=8, dropout=0.0)
    rows, tok_row, et, pt, nP = head_batch(6, [4, 1, 2], 4, IN_DIM)
    with pytest.raises(RuntimeError, match="code -21"):
        eng.forward(rows, tok_row, 3, 4, nP, False, 0)
