"""Explaining a prediction on the GPU: the attention probabilities both encoder paths leave in the head workspace, the rollout
kernel and the leave-one-prong-out scan, against the CPU walk of the model's own holder modules (attention_reference.py).

Gates (absolute on probabilities, max-norm relative on logits; none is derived from what the kernels give):
  weights   |hip - walk| <= 5e-5 on every entry  -- the project's gate for eval-mode hidden-state taps (test_submodules_gpu.py)
  logits    rel_err < 1e-4                       -- the project's gate for stage-by-stage logits (test_submodules_gpu.py)
  rollout   |kernel - float64 formula on the same emitted weights| <= 5e-5  (L (S+2) 2^-24 = 3e-5 at L = 8, S = 64)
  rows of valid queries sum to 1 within 1e-5 (S 2^-24 = 4e-6 at S = 64); padded rows and columns are exactly 0.
Every compared case has an event with padding and one without, token 0 is valid everywhere, all entries are compared and every valid
prong of every event is ablated.  Each test prints its maxima."""
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case, rel_err
from model_utils import build_trainer, to_device
import attention_reference as R

pytestmark = pytest.mark.gpu

GOLDENS = ["small_b3", "tutorial_b2p4", "tutorial_ragged", "tutorial_b2p8", "tutorial_b2p12"]
W_TOL, LOGIT_TOL, ROW_TOL = 5e-5, 1e-4, 1e-5
_models = {}


def small_cfg(**over):
    """Tutorial token path (d = 128, 8 heads, 6 layers) behind a small DenseNet: the encoder is what these tests are about."""
    return O.tutorial_config(**dict(dict(densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16,
                                         pixel_embedding_dim=64, pixel_noise_std=0.0), **over))


def small_model(seed=5, **over):
    cfg = small_cfg(**over)
    model = build_trainer(cfg, O.fill_state(cfg, seed))
    model.eval()
    return cfg, model


def golden_model(name, precision="fp32", training=False, dropout=None):
    cfg, over, batch, g = load_case(name)
    if dropout is not None:
        cfg = O.tutorial_config(**dict(over, dropout=dropout, pixel_noise_std=0.0))
    model = build_trainer(cfg, O.fill_state(cfg, int(g["weight_seed"])), precision=precision)
    model.train(training)
    return cfg, model, batch


def golden_tokens(model, batch):
    """(tokens [B, S, D], mask [B, S]) of the model's own embedding stage in eval arithmetic, trimmed to the widest event as
    shared_step does; a case without padding gets the tail of event 0 padded so that it has one event of each kind."""
    f, x, ec, ev, em, pc, pv, pm, et, pt = to_device(batch)
    width = int(pm.sum(1).max())
    f, pm = f[:, :width].contiguous(), pm[:, :width].contiguous()
    shape = model.training_dataset.pixel_shape
    pe = model.network.prong_embedding
    was = pe.training
    pe.eval()
    with torch.no_grad():
        tokens, mask = pe(f, x, model.preprocess_pixels(ec, ev, shape), em, model.preprocess_pixels(pc, pv, shape), pm)
    pe.train(was)
    mask = mask.clone()
    if bool(mask.all()):
        mask[0, -max(1, width // 3):] = False
    assert bool(mask[:, 0].all()) and bool(mask.all(1).any()) and bool((~mask.all(1)).any())
    return tokens, mask


def random_tokens(cfg, B, S, seed):
    mask = R.ragged_mask(B, S, seed)
    assert bool(mask[:, 0].all()) and bool(mask.all(1).any()) and bool((~mask.all(1)).any())
    tokens = torch.randn(B, S, cfg.hidden_dim, generator=torch.Generator().manual_seed(seed))
    return tokens.cuda(), mask.cuda()


def set_fused(model, on):
    from transformercvn.hip._lib import lib
    rt = model.network.hip_runtime()
    rt.ensure_bound()
    lib.tcvn_head_set_fused_encoder(rt.head.handle, int(on))


def check_structure(weights, mask, what):
    """Padded-key columns and padded-query rows exactly 0; rows of valid queries sum to 1."""
    w, m = weights.cpu(), mask.cpu()
    L, B, H, S, _ = w.shape
    assert m.shape == (B, S)
    cols = (~m)[None, :, None, None, :].expand_as(w)
    rows = (~m)[None, :, None, :, None].expand_as(w)
    assert (w[cols] == 0).all(), what + ": padded-key column not zero"
    assert (w[rows] == 0).all(), what + ": padded-query row not zero"
    sums = w.double().sum(-1)[m[None, :, None, :].expand(L, B, H, S)]
    err = (sums - 1).abs().max().item()
    print(f"{what}: rows of valid queries sum to 1 within {err:.2e}")
    assert err <= ROW_TOL, what
    assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0


def check_weights(model, tokens, mask, weights, what, layers=None):
    cfg_layers, heads = len(model.network.encoder.encoder.layers), model.network.encoder.encoder.layers[0].self_attn.num_heads
    B, S = mask.shape
    assert weights.shape == (cfg_layers, B, heads, S, S) and weights.dtype == torch.float32
    _, ref = R.walk(model.network.encoder.encoder, tokens, mask)
    d = (weights.cpu() - ref).abs()
    per_layer = [d[l].max().item() for l in range(cfg_layers)]
    print(f"{what}: max |weights - walk| per layer " + " ".join(f"{e:.2e}" for e in per_layer))
    for l in (range(cfg_layers) if layers is None else layers):
        assert per_layer[l] <= W_TOL, (what, l, per_layer[l])
    check_structure(weights, mask, what)


def run_stage(model, tokens, mask, what, layers=None):
    enc = model.network.encoder
    hidden, weights = enc.attention(tokens, mask)
    if not enc.training:
        assert torch.equal(hidden, enc(tokens, mask)[0]), what + ": hidden differs from forward()'s"
    check_weights(model, tokens, mask, weights, what, layers)
    return weights


# ---- 1. stage level, the path the plan picks (S = 5 .. 17: one fused launch) ------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", GOLDENS)
def test_attention_maps_match_the_reference_walk(name, precision):
    cfg, model, batch = golden_model(name, precision)
    tokens, mask = golden_tokens(model, batch)
    run_stage(model, tokens, mask, f"{name} {precision} S={mask.shape[1]}")


# ---- 2. the layer-by-layer kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_attention_maps_layer_by_layer_on_the_goldens(name):
    cfg, model, batch = golden_model(name)
    tokens, mask = golden_tokens(model, batch)
    set_fused(model, 0)
    run_stage(model, tokens, mask, f"{name} unfused S={mask.shape[1]}")


@pytest.mark.parametrize("S", [23, 40, 64])
def test_attention_maps_layer_by_layer_long_sequences(S):
    cfg, model = small_model()
    tokens, mask = random_tokens(cfg, 4, S, S)
    w = run_stage(model, tokens, mask, f"random tokens S={S}")
    assert w.numel() == 6 * 4 * 8 * S * S


@pytest.mark.parametrize("over,S,fused", [(dict(transformer_norm_first=True), 9, 1), (dict(transformer_norm_first=True), 40, 1),
                                          (dict(num_attention_heads=4), 9, 1), (dict(num_attention_heads=4), 9, 0),
                                          (dict(num_attention_heads=4), 40, 1)])
def test_attention_maps_norm_first_and_four_heads(over, S, fused):
    cfg, model = small_model(**over)
    tokens, mask = random_tokens(cfg, 3, S, 100 + S)
    set_fused(model, fused)
    run_stage(model, tokens, mask, f"{over} S={S} fused={fused}")


# ---- 4. whole model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tutorial_ragged", "small_b3"])
def test_forward_with_attention_is_forward_plus_the_maps(name, precision):
    cfg, model, batch = golden_model(name, precision)
    args = to_device(batch)[:8]
    with torch.no_grad():
        ev1, pr1 = model.forward(*args)
        ev2, pr2 = model.forward(*args)
        ev, pr, weights = model.forward_with_attention(*args)
    # forward is atomic-free: two plain calls agree bit for bit, and so must the call that also exports the maps
    assert torch.equal(ev1, ev2) and torch.equal(pr1, pr2), "forward() itself is not reproducible here"
    assert torch.equal(ev, ev1) and torch.equal(pr, pr1)
    assert not weights.requires_grad and not ev.requires_grad
    net = model.network
    with torch.no_grad():
        tokens, mask = net.prong_embedding(*model._network_inputs(*args))
    assert bool(mask.all(1).any()) and bool((~mask.all(1)).any())
    check_weights(model, tokens, mask, weights, f"whole model {name} {precision}")


# ---- 5. training mode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_attention_maps_in_training_mode_are_pre_dropout(dropout, fused):
    cfg, model, batch = golden_model("tutorial_ragged", dropout=dropout)
    tokens, mask = golden_tokens(model, batch)
    set_fused(model, fused)
    model.network.encoder.train()
    # dropout 0: every layer is the walk's.  dropout 0.1: nothing random precedes layer 0's softmax, so layer 0 is the walk's, and the
    # probabilities of every layer are still probabilities (exported before the attention dropout: rows sum to 1, no 1/(1-p) scaling)
    run_stage(model, tokens, mask, f"train dropout={dropout} fused={fused}", layers=None if dropout == 0.0 else [0])


def test_forward_with_attention_in_training_mode_is_a_training_forward():
    cfg, model, batch = golden_model("tutorial_ragged", training=True, dropout=0.0)
    args = to_device(batch)[:8]
    rt = model.network.hip_runtime()
    rt.ensure_bound()
    nbt, step = rt.flat_nbt.clone(), rt.step
    ev, pr, weights = model.forward_with_attention(*args)
    assert rt.step == step + 1 and torch.equal(rt.flat_nbt, nbt + rt._nbt_inc) and not ev.requires_grad
    with torch.no_grad():
        tokens, mask = model.network.prong_embedding(*model._network_inputs(*args))      # train mode: batch statistics, as in the step
    check_weights(model, tokens, mask, weights, "whole model, train mode, dropout 0")


# ---- 6. training is left alone ---------------------------------------------------------------------------------------------------------
def test_exporting_the_maps_between_forward_and_backward_changes_nothing():
    from transformercvn.network.layers.packed_data import token_rows
    cfg, over, batch, g = load_case("tutorial_ragged")
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    dev_batch = to_device(batch)
    pm = dev_batch[7]
    width = int(pm.sum(1).max())
    res = {}
    for tag in "ABC":
        model = build_trainer(cfg, sd)
        model.train()
        rt = model.network.hip_runtime()
        rt.zero_grad()
        loss = model.training_step(dev_batch, 0)
        if tag == "C":
            weights = rt.head.attention(token_rows(pm[:, :width].contiguous(), pm.shape[0]))
            check_structure(weights, torch.cat((dev_batch[4], pm[:, :width]), 1), "maps taken inside a training step (dropout 0.1)")
        loss.backward()
        torch.cuda.synchronize()
        res[tag] = (loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if "network.encoder." in k})
    assert torch.equal(res["C"][0], res["A"][0]), (res["C"][0].item(), res["A"][0].item())
    assert len(res["A"][1]) == 6 * 12
    worst_ab = worst_ac = 0.0
    for k, a in res["A"][1].items():
        ab, ac = (res["B"][1][k] - a).abs().max().item(), (res["C"][1][k] - a).abs().max().item()
        worst_ab, worst_ac = max(worst_ab, ab), max(worst_ac, ac)
        assert ac <= ab, (k, ac, ab)           # equal where the plain step repeats itself exactly, else within its own noise
    print(f"encoder gradients: plain step vs plain step {worst_ab:.2e}, plain step vs step with the export {worst_ac:.2e}")


def test_explaining_in_eval_mode_changes_no_state():
    cfg, model, batch = golden_model("tutorial_ragged")
    args = to_device(batch)[:8]
    with torch.no_grad():
        model.forward(*args)                          # binds the arenas: state_dict tensors are arena views from here on
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in before) and any(k.endswith("running_var") for k in before)
    model.forward_with_attention(*args)
    model.leave_one_prong_out(*args)
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys())
    for k, v in before.items():
        assert torch.equal(after[k], v), k


# ---- 7. rollout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", ["mean", "max"])
@pytest.mark.parametrize("S", [5, 17, 64])
def test_rollout_kernel_matches_the_float64_formula(S, fusion):
    from transformercvn.hip import attention
    key = ("small",)
    if key not in _models:
        _models[key] = small_model()
    cfg, model = _models[key]
    tokens, mask = random_tokens(cfg, 4, S, 7 * S)
    _, weights = model.network.encoder.attention(tokens, mask)
    roll = attention.rollout(weights, mask, fusion)
    assert roll.shape == (4, S, S) and roll.dtype == torch.float32 and roll.is_cuda
    ref = R.rollout(weights, mask, fusion)
    err = (roll.cpu().double() - ref).abs().max().item()
    print(f"rollout {fusion} S={S}: max |kernel - float64 formula| {err:.2e}")
    assert err <= 5e-5
    m = mask.cpu()
    r = roll.cpu()
    assert (r[(~m)[:, :, None].expand_as(r)] == 0).all() and (r[(~m)[:, None, :].expand_as(r)] == 0).all()
    e2p = attention.event_to_prongs(roll).cpu()
    assert e2p.shape == (4, S - 1) and (e2p[~m[:, 1:]] == 0).all() and (e2p >= 0).all()
    if fusion == "mean":          # every factor is row-stochastic: the event row sums to 1
        assert ((e2p.double().sum(1) - (1 - r[:, 0, 0].double())).abs() <= 1e-5).all()
    with pytest.raises(ValueError):
        attention.rollout(weights, mask, "median")


# ---- 8. leave one prong out ------------------------------------------------------------------------------------------------------------
def check_loo(model, tokens, mask, what):
    net = model.network
    rt = net.hip_runtime()
    ev, loo = rt.leave_one_prong_out(tokens, mask)
    B, S = mask.shape
    assert ev.shape[0] == B and loo.shape == (B, S - 1, ev.shape[1]) and loo.dtype == torch.float32
    ref_ev, ref_loo, n = R.leave_one_out(net.encoder.encoder, net.event_decoder, tokens, mask)
    assert n == int(mask[:, 1:].sum())
    e_base, e_loo = rel_err(ev.cpu(), ref_ev), rel_err(loo.cpu(), ref_loo)
    with torch.no_grad():
        hidden = net.encoder(tokens, mask)[0]
        e_dec = rel_err(ev.cpu(), net.event_decoder(hidden[0]).cpu())
    spread = (ref_loo - ref_ev[:, None]).abs().max().item() / ref_ev.abs().max().item()
    print(f"{what}: {n} variants; rel err base {e_base:.2e}, loo {e_loo:.2e}, base vs event_decoder(encoder) {e_dec:.2e}; "
          f"largest effect of one prong {spread:.2e}")
    assert e_base < LOGIT_TOL and e_loo < LOGIT_TOL and e_dec < LOGIT_TOL
    pad = ~mask[:, 1:]
    assert torch.equal(loo[pad], ev[:, None, :].expand_as(loo)[pad]), what + ": padded slots are not the base logits"
    assert spread > 10 * LOGIT_TOL, "the ablations must move the logits by much more than the gate"
    return n


@pytest.mark.parametrize("name", GOLDENS)
def test_leave_one_prong_out_on_the_goldens(name):
    cfg, model, batch = golden_model(name)
    tokens, mask = golden_tokens(model, batch)
    check_loo(model, tokens, mask, f"{name} S={mask.shape[1]}")


@pytest.mark.parametrize("B,S", [(4, 23), (8, 64)])
def test_leave_one_prong_out_long_sequences_and_several_passes(B, S):
    from transformercvn.hip import _lib
    cfg, model = small_model()
    tokens, mask = random_tokens(cfg, B, S, 3 * S)
    n = check_loo(model, tokens, mask, f"random tokens B={B} S={S}")
    if S == 64:       # more sequences than one pass holds: the host loop runs more than once
        assert B + n > _lib.LOO_MAX_PASS


def test_leave_one_prong_out_whole_model():
    cfg, model, batch = golden_model("tutorial_ragged")
    args = to_device(batch)[:8]
    net = model.network
    with torch.no_grad():
        ev0, pr0 = model.forward(*args)
        ev, pr, loo = model.leave_one_prong_out(*args)
        tokens, mask = net.prong_embedding(*model._network_inputs(*args))
    B, P = args[7].shape
    assert loo.shape == (B, P, ev.shape[1]) and torch.equal(pr, pr0)
    print("whole model: scan's base logits vs forward()'s", (ev - ev0).abs().max().item())
    assert rel_err(ev.cpu(), ev0.cpu()) < LOGIT_TOL
    ref_ev, ref_loo, n = R.leave_one_out(net.encoder.encoder, net.event_decoder, tokens, mask)
    assert n == int(args[7].sum())
    e_base, e_loo = rel_err(ev.cpu(), ref_ev), rel_err(loo.cpu(), ref_loo)
    print(f"whole model tutorial_ragged: {n} variants; rel err base {e_base:.2e}, loo {e_loo:.2e}")
    assert e_base < LOGIT_TOL and e_loo < LOGIT_TOL
    pad = ~args[7]
    assert bool(pad.any()) and torch.equal(loo[pad], ev[:, None, :].expand_as(loo)[pad])
    # difference-based relevance is exactly zero at padded slots
    assert ((loo - ev[:, None, :])[pad] == 0).all()
    model.train()
    with pytest.raises(RuntimeError):
        model.leave_one_prong_out(*args)
    with pytest.raises(RuntimeError):
        model.network.leave_one_prong_out(*model._network_inputs(*args))
