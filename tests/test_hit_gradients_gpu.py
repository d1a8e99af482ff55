"""Hit gradients (model.hit_gradients) on the GPU against float64 torch autograd through the oracle (O.forward(training=False)).

  1. fp32 mode: event_grad / prong_grad, whole tensor and per map, relative L2 <= 1e-3 of float64 -- also with cfg.dropout = 0.1 (the
     frozen pass ignores dropout) and on all three encoder paths; case B (280-wide maps): target "prong" and raw seeds;
  2. bf16 mode against the oracle under torch.autocast (no more than 2x its relative L2, cosine no lower than 2 cos_autocast - 1);
  3. the stages: token path alone, one embedder alone;
  4. the gather kernel alone through its C entry (corners, a full row, duplicates, every value mode, fp32 and bf16 rows);
  5. integrated gradients against the oracle's own midpoint rule, completeness;
  6. finite differences of the library's own eval forward at full size;
  7. nothing else moves, refusals.
"""
import ctypes as C

import pytest
import torch

from oracle import tcvn_oracle as O
import hit_gradients_reference as R
from model_utils import build_trainer, to_device

pytestmark = pytest.mark.gpu

GATE_F32 = 1e-3          # the project's fp32 gate, applied to the relative L2 error
# Case A, the plain gradient: torch's own float32 pass of the oracle is 9e-7 (event) / 1.2e-6 (prong) from float64, and the library measured
# 9.6e-7 / 1.1e-6 (post-norm 9.3e-7 / 9.9e-7, pre-norm 1.9e-6 / 2.5e-6; worst single map 3.8e-6) -- within 10x of torch's figure, so the
# gate of test 1 is tightened to 10x that figure
GATE_A = dict(event=9e-6, prong=1.2e-5, event_map=9e-6, prong_map=1.2e-5)


def case_a(**over):
    cfg = O.tutorial_config(**dict(dict(pixel_shape=(104, 72), densenet_structure=[3, 3, 2], num_encoder_layers=2, dropout=0.0,
                                        pixel_noise_std=0.0), **over))
    batch = O.synthetic_batch([1, 3], seed=7, cfg=cfg, event_hits=(150, 300), prong_hits=(10, 80))
    return cfg, O.fill_state(cfg, seed=3), batch


def case_b():
    cfg = O.tutorial_config(pixel_shape=(40, 280), densenet_structure=[3, 2], num_encoder_layers=2, dropout=0.0, pixel_noise_std=0.0)
    batch = O.synthetic_batch([2, 2], seed=11, cfg=cfg, event_hits=(150, 300), prong_hits=(10, 80))
    return cfg, O.fill_state(cfg, seed=5), batch


CLASSES_A = torch.tensor([1, 2])
_oracle = {}


def oracle_a(norm_first=False, autocast=False):
    """float64 (or autocast) gradients of case A, computed once per variant and left unchanged."""
    key = (norm_first, autocast)
    if key not in _oracle:
        cfg, sd, batch = case_a(transformer_norm_first=norm_first)
        _oracle[key] = R.oracle_hit_gradients(sd, cfg, batch[:8], CLASSES_A, "prob", torch.float32 if autocast else torch.float64,
                                              autocast=autocast)
    return _oracle[key]


def trainer_of(cfg, sd, precision="fp32"):
    """build_trainer on the maps of cfg (the synthetic dataset behind it has the tutorial's 400 x 280)."""
    model = build_trainer(cfg, sd, precision=precision)
    model.training_dataset.pixel_shape = model.network.pixel_shape = tuple(cfg.pixel_shape)
    return model


def model_of(cfg, sd, precision="fp32"):
    model = trainer_of(cfg, sd, precision)
    model.eval()
    return model


def report(tag, got_ev, got_pr, ref_ev, ref_pr, batch):
    figs = dict(event=R.rel_l2(got_ev, ref_ev), prong=R.rel_l2(got_pr, ref_pr),
                event_map=R.per_map_rel_l2(got_ev, ref_ev, batch[2]), prong_map=R.per_map_rel_l2(got_pr, ref_pr, batch[5]))
    print(f"hit_gradients[{tag}] relative L2 vs float64: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    return figs


# ---- 1. fp32 mode against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,dropout", [("fused", 0.0), ("fused", 0.1), ("post_norm", 0.0), ("pre_norm", 0.0)])
def test_fp32_gradients_match_the_float64_oracle(path, dropout):
    from transformercvn.hip._lib import lib
    cfg, sd, batch = case_a(transformer_norm_first=path == "pre_norm", dropout=dropout)
    ref_ev, ref_pr, ref_evl, ref_prl = oracle_a(path == "pre_norm")
    model = model_of(cfg, sd)
    if path == "post_norm":
        model.network.hip_runtime().ensure_bound()
        lib.tcvn_head_set_fused_encoder(model.network.hip_runtime().head.handle, 0)
    res = model.hit_gradients(*to_device(batch[:8]), target=CLASSES_A, value="prob")
    figs = report(f"A fp32 {path} dropout {dropout}", res.event_grad, res.prong_grad, ref_ev, ref_pr, batch)
    assert R.rel_l2(res.event_logits, ref_evl) < GATE_F32
    assert all(v <= GATE_A[k] for k, v in figs.items()), figs
    assert torch.equal(res.event_attr, res.event_grad * batch[3].cuda()) and torch.equal(res.prong_attr, res.prong_grad * batch[6].cuda())
    assert res.completeness_gap is None and res.value is None


def test_case_b_prong_target_and_raw_seeds():
    """280-wide maps.  target "prong" sums the predicted class of every valid prong; the raw pair is handed on as it is, and a padded
    slot seeded non-zero contributes nothing."""
    cfg, sd, batch = case_b()
    model = model_of(cfg, sd)
    dev = to_device(batch[:8])
    ref = R.oracle_hit_gradients(sd, cfg, batch[:8], "prong", "prob")
    res = model.hit_gradients(*dev, target="prong", value="prob")
    figs = report("B fp32 prong", res.event_grad, res.prong_grad, ref[0], ref[1], batch)
    assert all(v <= GATE_F32 for v in figs.values()), figs
    g = torch.Generator().manual_seed(20)
    B, P = batch[7].shape
    seeds = (torch.randn(B, cfg.num_event_classes, generator=g), torch.randn(B, P, cfg.num_prong_classes, generator=g))
    ref = R.oracle_hit_gradients(sd, cfg, batch[:8], seeds, "logit")
    res = model.hit_gradients(*dev, target=tuple(t.cuda() for t in seeds))
    figs = report("B fp32 raw seeds", res.event_grad, res.prong_grad, ref[0], ref[1], batch)
    assert all(v <= GATE_F32 for v in figs.values()), figs
    cfg2, sd2, batch2 = case_a()                               # two padded slots
    g = torch.Generator().manual_seed(21)
    B, P = batch2[7].shape
    d_ev = torch.randn(B, cfg2.num_event_classes, generator=g)
    d_pr = torch.randn(B, P, cfg2.num_prong_classes, generator=g)
    assert (~batch2[7]).any() and (d_pr[~batch2[7]] != 0).all()
    ref = R.oracle_hit_gradients(sd2, cfg2, batch2[:8], (d_ev, d_pr), "logit")
    res = model_of(cfg2, sd2).hit_gradients(*to_device(batch2[:8]), target=(d_ev.cuda(), d_pr.cuda()))
    figs = report("A fp32 raw seeds", res.event_grad, res.prong_grad, ref[0], ref[1], batch2)
    assert all(v <= GATE_F32 for v in figs.values()), figs


# ---- 2. bf16 mode ------------------------------------------------------------------------------------------------------------------------
def test_bf16_gradients_stay_within_twice_the_autocast_oracle():
    cfg, sd, batch = case_a()
    ref_ev, ref_pr, _, _ = oracle_a()
    ac_ev, ac_pr, _, _ = oracle_a(autocast=True)
    res = model_of(cfg, sd, "bf16").hit_gradients(*to_device(batch[:8]), target=CLASSES_A, value="prob")
    for name, got, ac, ref in (("event", res.event_grad, ac_ev, ref_ev), ("prong", res.prong_grad, ac_pr, ref_pr)):
        l2, l2_ac, cos, cos_ac = R.rel_l2(got, ref), R.rel_l2(ac, ref), R.cosine(got, ref), R.cosine(ac, ref)
        print(f"hit_gradients[A bf16] {name}: relative L2 {l2:.4f} (autocast oracle {l2_ac:.4f}), cosine {cos:.5f} (autocast {cos_ac:.5f})")
        assert l2 <= 2 * l2_ac, (name, l2, l2_ac)
        assert cos >= cos_ac - (1 - cos_ac), (name, cos, cos_ac)


# ---- 3. stages ------------------------------------------------------------------------------------------------------------------------
def oracle_token_path(sd, cfg, rows, event_mask, prong_mask):
    """The oracle from the combined embedding's input rows on (prong_embedding_forward's tail, encoder, decoders)."""
    ctx = O._Ctx(False, 0.0, None)
    B, P = prong_mask.shape
    comb = O.linear_block(sd, "network.prong_embedding.combined_embedding", cfg, rows, ctx)
    I1, I2 = O.pack_indices(prong_mask)
    padded = torch.zeros(B, P, comb.shape[1], dtype=comb.dtype)
    padded[I1, I2] = comb[B:]
    tokens = torch.cat((comb[:B].view(B, 1, -1), padded), dim=1)
    hidden = O.encoder_forward(sd, cfg, tokens, torch.cat((event_mask, prong_mask), dim=1), ctx)
    return O.decoders_forward(sd, cfg, hidden, ctx)


def test_token_path_alone():
    from transformercvn.network.layers.packed_data import token_rows
    cfg, sd, batch = case_a(dropout=0.1)
    model = model_of(cfg, sd)
    rt = model.network.hip_runtime()
    rt.ensure_bound()
    B, P = batch[7].shape
    nP = int(batch[7].sum())
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(B + nP, rt.head.cfg.in_dim, generator=g)
    d_ev, d_pr = torch.randn(B, cfg.num_event_classes, generator=g), torch.randn(B, P, cfg.num_prong_classes, generator=g)
    r64 = rows.double().requires_grad_(True)
    ev, pr = oracle_token_path(R.cast_state(sd, torch.float64), cfg, r64, batch[4], batch[7])
    ((d_ev.double() * ev).sum() + (d_pr.double() * pr)[batch[7]].sum()).backward()
    tok = token_rows(batch[7].cuda(), B)
    rows_d = rows.cuda()
    ev_d, pr_d = rt.head.forward_frozen(rows_d, tok, B, P, nP)
    d_rows = rt.head.input_gradient(rows_d, tok, d_ev.cuda(), (d_pr * batch[7].unsqueeze(2)).cuda().contiguous())
    err = R.rel_l2(d_rows, r64.grad)
    print(f"hit_gradients[token path alone] d_rows relative L2 {err:.3e}, logits {R.rel_l2(ev_d, ev.detach()):.3e}")
    assert err <= GATE_F32
    # the training backward is refused on a frozen forward's workspace, and the data-only backward anywhere else
    from transformercvn.hip._lib import lib
    from transformercvn.hip.native import ptr, stream_ptr
    ws, out = rt.head._ws, torch.empty_like(rows_d)
    args = (rt.head.handle, B, P, nP, ptr(rows_d), ptr(tok), ptr(d_ev.cuda()), ptr(d_pr.cuda()), ptr(out), ptr(ws), ws.numel(), stream_ptr())
    assert lib.tcvn_head_backward(*args) != 0
    rt.head.forward(rows_d, tok, B, P, nP, False)
    assert lib.tcvn_head_input_gradient(*args) != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_one_embedder_alone(precision):
    """The prong embedder of case A: d_out seeded at random, the gradient gathered at the hits."""
    cfg, sd, batch = case_a(dropout=0.1)
    model = model_of(cfg, sd, precision)
    rt = model.network.hip_runtime()
    rt.ensure_bound()
    coords, values = batch[5], batch[6]
    n = int(batch[7].sum())
    pix = O.embed_dims(cfg)[0]
    d_out = torch.randn(n, pix, generator=torch.Generator().manual_seed(9))
    prefix = "network.prong_embedding.prong_pixel_embedding"

    def oracle(dtype, autocast):
        v = values.to(dtype).clone().requires_grad_(True)
        s = R.cast_state(sd, dtype)
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out = O.densenet_forward(s, prefix, cfg, O.preprocess_pixels(cfg, coords, v, False), O._Ctx(False, 0.0, None))
        else:
            out = O.densenet_forward(s, prefix, cfg, O.preprocess_pixels(cfg, coords, v, False), O._Ctx(False, 0.0, None))
        (out.to(dtype) * d_out.to(dtype)).sum().backward()
        return v.grad.double(), out.detach()
    ref, ref_out = oracle(torch.float64, False)
    out = torch.empty(n, pix, device="cuda")
    c_d, v_d = coords.to(torch.int32).cuda().contiguous(), values.float().cuda().contiguous()
    rt.pr_engine.forward_frozen(c_d, v_d, n, out, 0)
    got = rt.pr_engine.input_gradient(d_out.cuda())
    l2, worst = R.rel_l2(got, ref), R.per_map_rel_l2(got, ref, coords)
    print(f"hit_gradients[embedder alone {precision}] relative L2 {l2:.3e}, worst map {worst:.3e}, output {R.rel_l2(out, ref_out):.3e}")
    if precision == "fp32":
        assert l2 <= GATE_F32 and worst <= GATE_F32
    else:
        ac, _ = oracle(torch.float32, True)
        l2_ac, cos, cos_ac = R.rel_l2(ac, ref), R.cosine(got, ref), R.cosine(ac, ref)
        print(f"    autocast oracle: relative L2 {l2_ac:.4f}, cosine {cos_ac:.5f}; library cosine {cos:.5f}")
        assert l2 <= 2 * l2_ac and cos >= cos_ac - (1 - cos_ac)


# ---- 4. the gather kernel alone --------------------------------------------------------------------------------------------------------
def gather_case(C=3):
    H, W, N = 20, 12, 64
    g = torch.Generator().manual_seed(4)
    hits = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (1, 0, 0), (1, H - 1, W - 1)]
    hits += [(0, 7, x) for x in range(W)]                                   # a full row
    hits += [(1, 5, 5), (1, 9, 3), (1, 5, 5), (1, 12, 8), (1, 9, 3), (1, 12, 8), (1, 2, 11), (1, 12, 8)]      # two listed twice, one three times
    hits += [(1, 13, 4), (0, 3, 6)]
    coords = torch.tensor(hits, dtype=torch.int32)
    values = torch.rand(len(hits), C, generator=g) * 200 + 1
    e0 = torch.randn(2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, N, generator=g)
    w0 = torch.randn(N, C, 7, 7, generator=g) * 0.1
    return (H, W), coords, values, e0, w0


def _gather_kernel_alone(value_mode, cpix):
    from transformercvn.hip import gradients
    from transformercvn.hip._lib import lib, check, MODE_F32, MODE_BF16
    from transformercvn.hip.native import ptr, stream_ptr
    shape, coords, values, e0_f32, w0 = gather_case(cpix)
    assert values.shape[1] == cpix and w0.shape[1] == cpix
    own = torch.tensor(R.owners(coords, 2, *shape))
    assert (~own).sum() == 4
    c, v, w = coords.cuda(), values.cuda(), w0.cuda()
    ws = torch.empty(lib.tcvn_hit_gradient_workspace_bytes(2, *shape, cpix), dtype=torch.uint8, device="cuda")
    for mode, e0 in ((MODE_F32, e0_f32), (MODE_BF16, e0_f32.to(torch.bfloat16))):
        ref = R.gather(e0, w0, coords, values, shape, value_mode)
        e = e0.cuda().contiguous()
        out = torch.full_like(v, float("nan"))
        check(lib.tcvn_hit_gradient_gather(mode, ptr(c), ptr(v), c.shape[0], 2, *shape, cpix, value_mode, ptr(e), 64, 64, ptr(w), ptr(out), ptr(ws),
                                           ws.numel(), stream_ptr()), "hit_gradient_gather")
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.equal(got, gradients.gather(e, w, c, v, shape, value_mode).cpu())      # the Python wrapper is this entry
        assert torch.isfinite(got).all()                                    # every hit written (the output starts as NaN)
        assert (got[~own] == 0).all() and (ref[own] != 0).all()
        rel = ((got.double() - ref).abs() / ref.abs())[own]
        print(f"hit_gradients[gather {'bf16' if mode == MODE_BF16 else 'fp32'} mode {value_mode} Cpix {cpix}] worst relative error per element {float(rel.max()):.3e}")
        assert float(rel.max()) <= 1e-5


@pytest.mark.parametrize("value_mode", [0, 1, 2])
def test_gather_kernel_alone(value_mode):
    """Both instances of k_hit_gradient through the C entry.  bf16: E0 is rounded to bf16 before either side sees it (the kernel reads
    2-byte elements at a row stride of N of them); the gate is the same."""
    _gather_kernel_alone(value_mode, 3)


@pytest.mark.parametrize("value_mode", [0, 1, 2])
@pytest.mark.parametrize("cpix", [1, 2, 4])
def test_gather_kernel_alone_at_other_channel_counts(cpix, value_mode):
    """The same list with 1, 2 and 4 value channels per hit (HG_MAXC = 4): the kernel indexes hit * Cpix + lane and c * 49 * N + co."""
    _gather_kernel_alone(value_mode, cpix)


def test_gather_kernel_refuses_five_channels():
    from transformercvn.hip._lib import lib, MODE_F32
    from transformercvn.hip.native import ptr, stream_ptr
    (H, W), coords, values, e0, w0 = gather_case(5)
    c, v, e, w = coords.cuda(), values.cuda(), e0.cuda(), w0.cuda()
    ws = torch.empty(lib.tcvn_hit_gradient_workspace_bytes(2, H, W, 5), dtype=torch.uint8, device="cuda")
    out = torch.full_like(v, float("nan"))
    rc = lib.tcvn_hit_gradient_gather(MODE_F32, ptr(c), ptr(v), c.shape[0], 2, H, W, 5, 0, ptr(e), 64, 64, ptr(w), ptr(out), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert rc == -2 and torch.isnan(out).all()                              # refused in front of the gather's launch: nothing written


def test_gather_kernel_writes_every_hit_and_refuses_one_hot():
    from transformercvn.hip._lib import lib, MODE_F32
    from transformercvn.hip.native import ptr, stream_ptr
    (H, W), coords, values, e0, w0 = gather_case()
    c, v, e, w = coords.cuda(), values.cuda(), e0.cuda(), w0.cuda()
    ws = torch.empty(lib.tcvn_hit_gradient_workspace_bytes(2, H, W, 3), dtype=torch.uint8, device="cuda")

    def run(mode, out):
        return lib.tcvn_hit_gradient_gather(MODE_F32, ptr(c), ptr(v), c.shape[0], 2, H, W, 3, mode, ptr(e), 64, 64, ptr(w), ptr(out), ptr(ws),
                                            ws.numel(), stream_ptr())
    a = torch.full_like(v, float("nan"))
    b = torch.full_like(v, float("nan"))
    assert run(0, a) == 0 and run(0, b) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a, b)                   # written exactly once each, the same bits twice
    poison = torch.full_like(v, float("nan"))
    assert run(3, poison) != 0                                             # one-hot pixels: refused, nothing launched
    torch.cuda.synchronize()
    assert torch.isnan(poison).all()


# ---- 5. integrated gradients -----------------------------------------------------------------------------------------------------------
def test_integrated_gradients_match_the_oracle_midpoint_rule_and_are_complete():
    cfg, sd, batch = case_a()
    model = model_of(cfg, sd)
    dev = to_device(batch[:8])

    def grads(vals):
        return R.oracle_hit_gradients(sd, cfg, batch[:8], CLASSES_A, "prob", values=vals)[:2]
    ref_ev, ref_pr = R.integrated_gradients(grads, [batch[3], batch[6]], 32)
    res = model.hit_gradients(*dev, target=CLASSES_A, value="prob", method="integrated", steps=32)
    figs = report("A fp32 integrated, 32 steps", res.event_attr, res.prong_attr, ref_ev, ref_pr, batch)
    assert all(v <= GATE_F32 for v in figs.values()), figs
    res = model.hit_gradients(*dev, target=CLASSES_A, value="prob", method="integrated", steps=64)
    moved = (res.value - res.baseline_value).abs()
    print(f"hit_gradients[A fp32 integrated, 64 steps] completeness gap / |value - baseline|: {(res.completeness_gap / moved).tolist()}")
    assert (res.completeness_gap <= 0.01 * moved).all()
    b_of_prong = batch[7].nonzero()[:, 0]
    again = R.completeness_gap(res.event_attr.cpu(), res.prong_attr.cpu(), batch[2][:, 0], b_of_prong[batch[5][:, 0].long()],
                               res.value.cpu(), res.baseline_value.cpu())
    assert torch.allclose(res.completeness_gap.cpu(), again, rtol=1e-9, atol=1e-12)
    # value / baseline_value are the ordinary eval forward's
    ev, _ = model.network(*model._network_inputs(*dev))
    assert torch.allclose(res.value.cpu(), ev.double().softmax(1).cpu().gather(1, CLASSES_A.view(-1, 1)).squeeze(1), rtol=1e-12, atol=0)


# ---- 6. finite differences at full size ----------------------------------------------------------------------------------------------
def test_finite_differences_of_the_eval_forward_at_full_size():
    """Independent of the oracle: f = the class logit from the library's ordinary eval forward(), perturbed along v * (1 + eps r), the
    direction d = r v random per value.  The central difference D(eps) has a truncation term ~ eps^2 and a rounding term ~ delta / eps, with
    delta the noise of an fp32 forward, taken as 2^-20 max(|f|, 1) (two ulp of a logit of size one; the differences observed are of that
    size).  Both are measured without the oracle: the truncation term of step eps is 4/3 |D(eps) - D(eps / 2)| (Richardson).  eps is the
    largest power of two from 2^-1 down whose truncation term is below its rounding term; the gate is 1 % of <grad, d>.
    r is uniform in [0, 1]: with r of either sign <grad, d> is a random walk over the ~10^4 values, sqrt(N) times smaller than a coherent
    sum, and the rounding term delta / eps alone is then tens of per cent of it at every step the truncation term admits (measured: <grad, d>
    = -6.3e-4, D = -6.0e-4 at eps = 2^-7, where delta / eps = 1.2e-4) -- the yardstick, not the gradient, is what such a direction tests.
    Three signed directions are run as well and held to what the yardstick can resolve there: |D - <grad, d>| at most four times the
    rounding term of the chosen step plus its truncation estimate."""
    cfg = O.tutorial_config(num_encoder_layers=2, dropout=0.0, pixel_noise_std=0.0)
    batch = O.synthetic_batch([2], seed=5, cfg=cfg)
    model = model_of(cfg, O.fill_state(cfg, seed=6))
    dev = list(to_device(batch[:8]))
    res = model.hit_gradients(*dev, target=1, value="logit")

    def f(ev_v, pr_v):
        b = list(dev)
        b[3], b[6] = ev_v, pr_v
        return float(model.network(*model._network_inputs(*b))[0][0, 1].double())
    g = torch.Generator().manual_seed(8)
    for k in range(6):
        signed = k >= 3
        lo = -1.0 if signed else 0.0
        d_ev = ((torch.rand(dev[3].shape, generator=g) * (1 - lo) + lo).cuda() * dev[3]).double()
        d_pr = ((torch.rand(dev[6].shape, generator=g) * (1 - lo) + lo).cuda() * dev[6]).double()
        want = float((res.event_grad.double() * d_ev).sum() + (res.prong_grad.double() * d_pr).sum())

        def D(eps):
            up = f((dev[3].double() + eps * d_ev).float(), (dev[6].double() + eps * d_pr).float())
            dn = f((dev[3].double() - eps * d_ev).float(), (dev[6].double() - eps * d_pr).float())
            return (up - dn) / (2 * eps), max(abs(up), abs(dn), 1.0)
        eps, (cur, mag) = 0.5, D(0.5)
        while eps > 2 ** -12:
            nxt, _ = D(eps / 2)
            trunc = 4 / 3 * abs(cur - nxt)
            if trunc < 2 ** -20 * mag / eps:
                break
            eps, cur = eps / 2, nxt
        rounding = 2 ** -20 * mag / eps
        rel = abs(cur - want) / abs(want)
        print(f"hit_gradients[finite differences {k}{' signed' if signed else ''}] eps 2^{torch.log2(torch.tensor(eps)).item():.0f}: D {cur:.6e}, <grad, d> {want:.6e}, "
              f"relative difference {rel:.3e}, rounding term {2 ** -20 * mag / eps / abs(want):.3e} of it")
        assert abs(cur - want) <= 4 * rounding + trunc if signed else rel <= 0.01


# ---- 7. nothing else moves ---------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    """State, gradients, step counter and hook around hit_gradients (both methods), and the training step that follows against the same
    step of a fresh model: the loss and every gradient bit-identical -- except where the training step itself is not reproducible.  In
    fp32 mode every convolution of the embedders ends its weight and bias gradient in float atomics between workgroups (conv_bwd.hip
    k_conv_wgrad, conv1x1_f32.hip, conv3x3_f32.hip; the hit-list conv0 gradient in LDS atomics between waves, stem.hip), so two fresh
    models differ there themselves by the arrival order: conv0, conv1, conv2 and the transition conv, weight and bias, of both
    embedders.  Nothing reads those tensors inside the step, so every other gradient is reproducible and is compared exactly (a second
    fresh model checks that).  An atomic sum of at most 512 workgroup partials moves by at most 512 roundings: those tensors are held to
    512 * 2^-24 of the largest weight gradient of their convolution (a bias gradient in front of a batch-statistics BatchNorm is exactly
    zero in exact arithmetic, pure rounding noise, so its own size is no scale)."""
    cfg, sd, batch = case_a(dropout=0.1, pixel_noise_std=0.001)
    full = to_device(batch)
    dev = full[:8]

    def train_step(model):
        model.train()
        model.network.hip_runtime().zero_grad()
        loss = model.training_step(full, 0)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: None if p.grad is None else p.grad.clone() for k, p in model.named_parameters()}
    fresh = trainer_of(cfg, sd)
    loss0, _ = train_step(fresh)                                            # step 0 of both models
    loss1_fresh, grads1_fresh = train_step(fresh)
    control = trainer_of(cfg, sd)
    train_step(control)
    loss1_control, grads1_control = train_step(control)
    assert torch.equal(loss1_control, loss1_fresh)
    conv = lambda k: k.rsplit(".", 1)[0]
    atomic = lambda k: "pixel_embedding.features." in k and conv(k).endswith((".conv0", ".conv1", ".conv2", ".conv"))
    exact = {k for k, g in grads1_fresh.items() if g is not None and not atomic(k)}
    assert all(torch.equal(grads1_fresh[k], grads1_control[k]) for k in exact), [k for k in exact if not torch.equal(grads1_fresh[k], grads1_control[k])]
    model = trainer_of(cfg, sd)
    hooked = []
    train_step(model)
    model.network.hip_runtime().grad_ready_hook = hooked.append
    model.eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    grads_before = {k: None if p.grad is None else p.grad.clone() for k, p in model.named_parameters()}
    step_before = model.network.hip_runtime().step
    a = model.hit_gradients(*dev, target="event")
    b = model.hit_gradients(*dev, target="event")
    ig_a = model.hit_gradients(*dev, target="event", method="integrated", steps=4)
    ig_b = model.hit_gradients(*dev, target="event", method="integrated", steps=4)
    for x, y in ((a, b), (ig_a, ig_b)):
        for name in ("event_grad", "prong_grad", "event_attr", "prong_attr"):
            assert torch.equal(getattr(x, name), getattr(y, name)), name
    assert torch.equal(ig_a.completeness_gap, ig_b.completeness_gap)
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), [k for k in before if not torch.equal(before[k], after[k])]
    assert all((p.grad is None) if grads_before[k] is None else torch.equal(grads_before[k], p.grad) for k, p in model.named_parameters())
    assert model.network.hip_runtime().step == step_before and hooked == []
    for p in model.parameters():
        p.grad = None
    model.hit_gradients(*dev, target="event")
    assert all(p.grad is None for p in model.parameters())
    model.network.hip_runtime().grad_ready_hook = None
    loss1, grads1 = train_step(model)                                       # step 1 behind the hit_gradients calls
    assert torch.equal(loss1, loss1_fresh)
    assert all(grads1[k] is None for k in grads1 if grads1_fresh[k] is None)
    assert all(torch.equal(grads1[k], grads1_fresh[k]) for k in exact), [k for k in exact if not torch.equal(grads1[k], grads1_fresh[k])]
    for k, g in grads1_fresh.items():
        if g is not None and k not in exact:
            scale = float(grads1_fresh[conv(k) + ".weight"].abs().max())
            assert float((grads1[k] - g).abs().max()) <= 512 * 2 ** -24 * scale, k


def test_refusals_after_a_frozen_and_after_a_train_forward():
    from transformercvn.hip._lib import lib
    from transformercvn.hip.native import ptr, stream_ptr
    cfg, sd, batch = case_a()
    model = model_of(cfg, sd)
    rt = model.network.hip_runtime()
    rt.ensure_bound()
    eng = rt.pr_engine
    n = int(batch[7].sum())
    c, v = batch[5].to(torch.int32).cuda().contiguous(), batch[6].float().cuda().contiguous()
    out = torch.empty(n, eng.out_dim, device="cuda")
    d_out, d_val = torch.ones_like(out), torch.full_like(v, float("nan"))
    eng.forward_frozen(c, v, n, out, 0)
    ws = eng._ws
    assert lib.tcvn_densenet_backward(eng.handle, n, ptr(d_out), d_out.stride(0), ptr(ws), ws.numel(), stream_ptr()) != 0
    assert lib.tcvn_densenet_forward_mc(eng.handle, n, ptr(c), ptr(v), c.shape[0], 0, ptr(out), out.stride(0), ptr(ws), ws.numel(),
                                        C.c_uint64(1), 1, stream_ptr()) != 0
    with pytest.raises(RuntimeError):
        eng.backward(d_out)
    eng.forward(c, v, n, out, True, 5)                                       # a train forward: the data-only backward is refused
    ws = eng._ws
    assert lib.tcvn_densenet_input_gradient(eng.handle, n, ptr(d_out), d_out.stride(0), ptr(d_val), ptr(ws), ws.numel(), stream_ptr()) != 0
    eng.forward(c, v, n, out, False)                                         # ... and after a plain eval forward
    ws = eng._ws
    assert lib.tcvn_densenet_input_gradient(eng.handle, n, ptr(d_out), d_out.stride(0), ptr(d_val), ptr(ws), ws.numel(), stream_ptr()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(d_val).all()                                          # refused, not run
    with pytest.raises(RuntimeError):
        eng.forward_frozen(c, v, n, out, 3)                                  # one-hot pixels
