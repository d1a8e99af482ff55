"""Prong Shapley values on the GPU against the CPU yardstick (shapley_reference.py: the walk of the model's own holder modules for every
listed coalition, the defining formulas in float64).

Gates (the project's own; none is derived from what the kernels give):
  coalition logits   rel_err < LOGIT_TOL = 1e-4 against the walk (max-norm relative, as every stage-by-stage logit here)
  phi, interaction   against the float64 formulas on the REFERENCE's logits: 2 W_TOL = 1e-4 absolute in "prob" mode (a Shapley value is a
                     convex combination of differences of two probabilities, each within W_TOL = 5e-5), 2 LOGIT_TOL max|ref logit| in
                     "logit" mode
  phi, stderr, interaction against the float64 formulas on the result's OWN coalition_logits (and permutations): 1e-6, the heat map's gate
  efficiency, interaction rows summing to phi: 1e-6; padded slots exactly 0; interaction NaN exactly between valid slots of sampled events.
Every case has an event with padding and one without.  Each test prints its maxima."""
import itertools

import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case, rel_err
from model_utils import build_trainer, to_device
from test_explain_gpu import golden_model, golden_tokens, random_tokens, set_fused, small_model
import shapley_reference as SR

pytestmark = pytest.mark.gpu

W_TOL, LOGIT_TOL, OWN_TOL = 5e-5, 1e-4, 1e-6
_cases, _refs = {}, {}


def golden_case(name, precision="fp32", **over):
    """(model, tokens, mask) of a golden, built once per (name, precision, overrides)."""
    key = (name, precision, tuple(sorted(over.items())))
    if key not in _cases:
        if over:
            _, base, batch, g = load_case(name)
            cfg = O.tutorial_config(**dict(base, **over))
            model = build_trainer(cfg, O.fill_state(cfg, int(g["weight_seed"])), precision=precision)
            model.eval()
        else:
            _, model, batch = golden_model(name, precision)
        _cases[key] = (model,) + tuple(golden_tokens(model, batch))
    return _cases[key]


def small_case(B, S, seed):
    key = ("small", B, S, seed)
    if key not in _cases:
        if "small_model" not in _cases:
            _cases["small_model"] = small_model()
        cfg, model = _cases["small_model"]
        _cases[key] = (model,) + tuple(random_tokens(cfg, B, S, seed))
    return _cases[key]


def widest(mask):
    return int(mask[:, 1:].sum(1).max())


def reference(key, model, tokens, mask, res, max_exact, samples):
    """The coalition list by host integer arithmetic and the walk's logits of every listed coalition, computed once per key and left
    unchanged (the permutations of a seed are part of the key's result: the same seed gives the same list)."""
    if key not in _refs:
        net = model.network
        offsets, event, masks, exact = SR.coalition_list(mask, max_exact, samples, res.permutations.cpu())
        _refs[key] = (offsets, event, masks, exact, SR.coalition_logits(net.encoder.encoder, net.event_decoder, tokens, mask, event, masks))
    return _refs[key]


def check_list(model, tokens, mask, res, ref, what):
    """Test 1: offsets / event / masks / exact, the logits of every coalition, the full coalition against the stage forward."""
    offsets, event, masks, exact, ref_lg = ref
    assert res.offsets.cpu().tolist() == offsets and res.exact.cpu().tolist() == exact, what
    assert res.event.cpu().tolist() == event and res.masks.cpu().tolist() == masks, what
    assert res.masks.dtype == torch.int64 and res.coalition_logits.shape == ref_lg.shape
    e_all = rel_err(res.coalition_logits.cpu(), ref_lg)
    net = model.network
    with torch.no_grad():
        stage = net.event_decoder(net.encoder(tokens, mask)[0][0])
    full = [offsets[b + 1] - 1 if exact[b] else offsets[b] + 1 for b in range(len(exact))]
    assert torch.equal(res.event_logits, res.coalition_logits[torch.tensor(full, device=res.event_logits.device)])
    e_full = rel_err(res.event_logits.cpu(), stage.cpu())
    spread = max((ref_lg[offsets[b]:offsets[b + 1]] - ref_lg[full[b]]).abs().max().item() for b in range(len(exact))) / ref_lg.abs().max().item()
    print(f"{what}: {len(masks)} coalitions, exact {exact}; rel err of the coalition logits {e_all:.2e}, full coalition vs "
          f"event_decoder(encoder) {e_full:.2e}; largest effect of a coalition {spread:.2e}")
    assert e_all < LOGIT_TOL and e_full < LOGIT_TOL
    assert spread > 10 * LOGIT_TOL, "the coalitions must move the logits by much more than the gate"


def nan_gap(a, b):
    """max |a - b| where both are numbers; the NaN patterns must be the same."""
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    d = (a - b).abs()
    d = d[~torch.isnan(d)]
    return d.max().item() if d.numel() else 0.0


def check_values(mask, res, ref, max_exact, samples, value, what):
    """Test 2 (and the sampled events' share of test 6)."""
    offsets, event, masks, exact, ref_lg = ref
    m = mask.cpu()
    B, P = m.shape[0], m.shape[1] - 1
    perms = res.permutations.cpu()
    phi, se, inter = res.phi.cpu().double(), res.stderr.cpu().double(), res.interaction.cpu().double()
    assert res.phi.dtype == torch.float32 and phi.shape == (B, P, ref_lg.shape[1]) and inter.shape == (B, P, P, ref_lg.shape[1])
    gate = 2 * W_TOL if value == "prob" else 2 * LOGIT_TOL * ref_lg.abs().max().item()
    r_phi, _, r_inter = SR.reduce_result(SR.values(ref_lg, value), m, max_exact, samples, perms, offsets, masks)
    o_phi, o_se, o_inter = SR.reduce_result(SR.values(res.coalition_logits, value), m, max_exact, samples, perms, offsets, masks)
    g = dict(phi_ref=(phi - r_phi).abs().max().item(), inter_ref=nan_gap(inter, r_inter), phi_own=(phi - o_phi).abs().max().item(),
             se_own=(se - o_se).abs().max().item(), inter_own=nan_gap(inter, o_inter),
             efficiency=(phi.sum(1) - (res.full - res.empty).cpu()).abs().max().item())
    ex = torch.tensor(exact)
    rows = (inter[ex].sum(2) - phi[ex]).abs().max().item() if bool(ex.any()) else 0.0
    print(f"{what} {value}: vs reference phi {g['phi_ref']:.2e} interaction {g['inter_ref']:.2e} (gate {gate:.2e}); vs float64 on own "
          f"logits phi {g['phi_own']:.2e} stderr {g['se_own']:.2e} interaction {g['inter_own']:.2e}; efficiency {g['efficiency']:.2e}; "
          f"interaction rows vs phi {rows:.2e}; largest |phi| {phi.abs().max().item():.2e}")
    assert g["phi_ref"] <= gate and g["inter_ref"] <= gate
    assert g["phi_own"] <= OWN_TOL and g["se_own"] <= OWN_TOL and g["inter_own"] <= OWN_TOL
    assert g["efficiency"] <= OWN_TOL and rows <= OWN_TOL
    clean = torch.nan_to_num(inter, nan=-7.0)
    assert torch.equal(clean, clean.transpose(1, 2)), "interaction is not symmetric"
    pad = ~m[:, 1:]
    assert (phi[pad] == 0).all() and (se[pad] == 0).all() and (se[ex] == 0).all()
    assert (inter[pad] == 0).all() and (inter.transpose(1, 2)[pad] == 0).all()
    both = m[:, 1:, None] & m[:, None, 1:]
    for b in range(B):          # NaN exactly between the valid slots of sampled events
        between = torch.isnan(inter[b][both[b]])
        assert bool(between.all()) if not exact[b] else not bool(between.any()), b


def run(model, tokens, mask, **kw):
    return model.network.hip_runtime().prong_shapley(tokens, mask, **kw)


# ---- 1, 2. coalition list and exact values on the goldens (the 16-prong event of tutorial_ragged is sampled) -------------------------
@pytest.mark.parametrize("name", ["small_b3", "tutorial_b2p4", "tutorial_ragged", "tutorial_b2p8"])
def test_coalitions_and_exact_values_on_the_goldens(name):
    model, tokens, mask = golden_case(name)
    max_exact = min(widest(mask), 10)
    res = run(model, tokens, mask, max_exact=max_exact, samples=4)
    ref = reference((name, max_exact, 4, 0), model, tokens, mask, res, max_exact, 4)
    if name == "tutorial_ragged":
        assert widest(mask) == 16 and ref[3].count(False) == 1
    else:
        assert all(ref[3])
    check_list(model, tokens, mask, res, ref, name)
    check_values(mask, res, ref, max_exact, 4, "prob", name)
    check_values(mask, run(model, tokens, mask, max_exact=max_exact, samples=4, value="logit"), ref, max_exact, 4, "logit", name)


# ---- 3. n = 12: several passes, pass boundaries inside an event ----------------------------------------------------------------------
def test_twelve_prongs_take_several_passes():
    from transformercvn.hip import _lib
    model, tokens, mask = golden_case("tutorial_b2p12")
    assert widest(mask) == 12
    res = run(model, tokens, mask, max_exact=12)
    ref = reference(("tutorial_b2p12", 12, 64, 0), model, tokens, mask, res, 12, 64)
    offsets = ref[0]
    cap = _lib.SHAP_MAX_PASS
    assert all(ref[3]) and offsets[-1] >= 4096 and offsets[-1] > cap                                  # more than one pass, whichever cap
    assert any(offsets[b] < k < offsets[b + 1] for k in range(cap, offsets[-1], cap) for b in range(2)), "no pass boundary inside an event"
    check_list(model, tokens, mask, res, ref, "tutorial_b2p12")
    check_values(mask, res, ref, 12, 64, "prob", "tutorial_b2p12")
    check_values(mask, run(model, tokens, mask, max_exact=12, value="logit"), ref, 12, 64, "logit", "tutorial_b2p12")


# ---- 4. one prong and none ---------------------------------------------------------------------------------------------------------------
def test_one_prong_equals_leave_one_out_and_no_prong_is_a_zero_row():
    model, tokens, mask = golden_case("tutorial_ragged")
    rt = model.network.hip_runtime()
    n = mask[:, 1:].sum(1)
    assert bool((n == 1).any())
    b = int((n == 1).nonzero()[0])
    p = int(mask[b, 1:].nonzero()[0])
    res = run(model, tokens, mask, max_exact=10, samples=4)
    ev, loo = rt.leave_one_prong_out(tokens, mask)
    want = (torch.softmax(ev[b].double(), -1) - torch.softmax(loo[b, p].double(), -1)).cpu()
    gap = (res.phi[b, p].cpu().double() - want).abs().max().item()
    print(f"one-prong event {b}, slot {p}: |phi - (value(base) - value(loo))| {gap:.2e}; |phi| {want.abs().max().item():.2e}")
    assert gap <= 2 * W_TOL and int(res.offsets[b + 1] - res.offsets[b]) == 2
    # a token-level call whose mask leaves event 1 without any prong
    bare = mask.clone()
    bare[1, 1:] = False
    res = run(model, tokens, bare, max_exact=10, samples=4)
    assert int(res.offsets[2] - res.offsets[1]) == 1 and int(res.masks[res.offsets[1]]) == 0 and bool(res.exact[1])
    assert (res.phi[1] == 0).all() and (res.stderr[1] == 0).all() and (res.interaction[1] == 0).all()
    assert torch.equal(res.full[1], res.empty[1])
    net = model.network
    ref = SR.coalition_logits(net.encoder.encoder, net.event_decoder, tokens, bare, [1], [0])
    assert rel_err(res.event_logits[1:2].cpu(), ref) < LOGIT_TOL


def test_events_without_prong_slots():
    """max_prongs = 0: sequences of the event token alone; one coalition per event, the prong-shaped outputs are empty."""
    model, tokens, mask = small_case(4, 6, 11)
    tokens, mask = tokens[:, :1].contiguous(), mask[:, :1].contiguous()
    res = run(model, tokens, mask)
    Ce = res.event_logits.shape[1]
    assert res.phi.shape == (4, 0, Ce) and res.stderr.shape == (4, 0, Ce) and res.interaction.shape == (4, 0, 0, Ce)
    assert res.permutations.shape == (4, 64, 0) and res.for_target().shape == (4, 0) and res.pairs().shape == (4, 0, 0)
    assert res.offsets.tolist() == [0, 1, 2, 3, 4] and res.event.tolist() == [0, 1, 2, 3] and res.masks.tolist() == [0] * 4
    assert bool(res.exact.all()) and torch.equal(res.event_logits, res.coalition_logits) and torch.equal(res.full, res.empty)
    net = model.network
    ref = SR.coalition_logits(net.encoder.encoder, net.event_decoder, tokens, mask, [0, 1, 2, 3], [0] * 4)
    e = rel_err(res.event_logits.cpu(), ref)
    print(f"no prong slots: rel err of the four event-token sequences {e:.2e}")
    assert e < LOGIT_TOL


# ---- 5. symmetry and dummy ---------------------------------------------------------------------------------------------------------------
def test_symmetry_and_dummy():
    model, tokens, mask = small_case(4, 6, 11)
    tokens = tokens.clone()
    tokens[:, 3] = tokens[:, 2]                      # prong slot p is token 1 + p: slot 2 becomes a copy of slot 1
    res = run(model, tokens, mask)
    twins = (mask[:, 2] & mask[:, 3]).cpu()
    assert bool(twins.any()) and bool(res.exact.all())
    gap = (res.phi[:, 1] - res.phi[:, 2])[twins].abs().max().item()
    print(f"symmetry: |phi_1 - phi_2| {gap:.2e} over {int(twins.sum())} events; |phi| up to {res.phi[:, 1][twins].abs().max().item():.2e}")
    assert gap <= 2 * W_TOL
    # dummy, value "logit": phi_p is a convex combination of p's marginal contributions, so it is bounded by the largest of them; a
    # prong whose removal never moves the reference logits beyond the gate has |phi| within the gate
    res = run(model, tokens, mask, value="logit")
    ref = reference(("small", 4, 6, 11, "twins"), model, tokens, mask, res, 10, 64)
    offsets, _, masks, _, ref_lg = ref
    gate = 2 * LOGIT_TOL * ref_lg.abs().max().item()
    dummies, worst = 0, 0.0
    for b, slots in enumerate(SR.valid_slots(mask)):
        row = {c: j for j, c in enumerate(masks[offsets[b]:offsets[b + 1]])}
        v = ref_lg[offsets[b]:offsets[b + 1]].double()
        for p in slots:
            effect = max((v[row[c | (1 << p)]] - v[j]).abs().max().item() for c, j in row.items() if not (c >> p) & 1)
            mine = res.phi[b, p].abs().max().item()
            worst = max(worst, mine - effect)
            assert mine <= effect + gate
            if effect <= gate:
                dummies += 1
                assert mine <= gate
    print(f"dummy: |phi| exceeds the largest marginal effect of its prong by at most {worst:.2e} (gate {gate:.2e}); {dummies} prongs "
          f"never move the logits beyond the gate")


# ---- 6. sampled mode ---------------------------------------------------------------------------------------------------------------------
def check_permutations(res, mask, samples):
    perms, m = res.permutations.cpu(), mask.cpu()
    B, P = m.shape[0], m.shape[1] - 1
    assert perms.shape == (B, samples, P) and perms.dtype == torch.int32
    for b, slots in enumerate(SR.valid_slots(m)):
        for k in range(samples):
            row = perms[b, k].tolist()
            assert sorted(row[:len(slots)]) == slots and all(x == -1 for x in row[len(slots):]), (b, k, row)


@pytest.mark.parametrize("B,S,samples", [(4, 23, 8), (2, 64, 2)])
def test_sampled_mode(B, S, samples):
    model, tokens, mask = small_case(B, S, 5 * S)
    assert int(mask[0, 1:].sum()) == S - 1
    res = run(model, tokens, mask, max_exact=3, samples=samples, seed=9)
    assert not bool(res.exact.any())
    check_permutations(res, mask, samples)
    ref = reference(("small", B, S, samples, 9), model, tokens, mask, res, 3, samples)
    if S == 64:
        assert max(ref[2]) >> 62 == 1                # bit 62 of a mask in use
    check_list(model, tokens, mask, res, ref, f"sampled B={B} S={S}")       # masks are the permutations' prefixes: coalition_list builds them so
    check_values(mask, res, ref, 3, samples, "prob", f"sampled B={B} S={S}")
    assert (res.stderr > 0).any()
    again = run(model, tokens, mask, max_exact=3, samples=samples, seed=9)
    other = run(model, tokens, mask, max_exact=3, samples=samples, seed=10)
    assert torch.equal(again.permutations, res.permutations) and torch.equal(again.phi, res.phi)
    assert not torch.equal(other.permutations, res.permutations)


def test_permutations_are_uniform():
    model, tokens, mask = small_case(2, 4, 21)
    assert int(mask[0, 1:].sum()) == 3
    res = run(model, tokens, mask, max_exact=0, samples=600, seed=1)
    check_permutations(res, mask, 600)
    seen = {}
    for row in res.permutations[0].cpu().tolist():
        seen[tuple(row)] = seen.get(tuple(row), 0) + 1
    print("orders of three prongs in 600 permutations:", sorted(seen.values()))
    assert len(seen) == 6 and all(55 <= c <= 145 for c in seen.values())      # 100 +- 5 sigma of a binomial(600, 1/6)
    one = run(model, tokens, mask, max_exact=0, samples=1, seed=1)
    assert (one.stderr == 0).all() and torch.equal(one.permutations[:, 0], res.permutations[:, 0])


# ---- 7. exact and sampled agree in expectation ------------------------------------------------------------------------------------------------
def test_all_permutations_reproduce_the_exact_values():
    model, tokens, mask = small_case(2, 5, 31)
    assert int(mask[0, 1:].sum()) == 4
    res = run(model, tokens, mask)
    v = SR.values(res.coalition_logits[: 16], "prob")
    exact = SR.exact_phi(v)
    ph, _ = SR.sampled_phi([list(p) for p in itertools.permutations(range(4))], lambda C: v[sum(1 << i for i in C)])
    gap = max((ph[i] - exact[i]).abs().max().item() for i in range(4))
    dev = (res.phi[0].cpu().double() - exact).abs().max().item()
    print(f"all 24 orders vs the subset formula on the device's logits {gap:.2e}; the device's phi vs either {dev:.2e}")
    assert gap <= 1e-9 and dev <= OWN_TOL


# ---- 8. paths and modes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_fused_and_layer_by_layer_encoder(fused):
    model, tokens, mask = golden_case("tutorial_b2p4")
    max_exact = min(widest(mask), 10)
    set_fused(model, fused)
    try:
        res = run(model, tokens, mask, max_exact=max_exact, samples=4)
    finally:
        set_fused(model, 1)
    ref = reference(("tutorial_b2p4", max_exact, 4, 0), model, tokens, mask, res, max_exact, 4)
    check_list(model, tokens, mask, res, ref, f"tutorial_b2p4 fused={fused}")
    check_values(mask, res, ref, max_exact, 4, "prob", f"tutorial_b2p4 fused={fused}")


@pytest.mark.parametrize("name,precision,over", [("small_b3", "fp32", dict(transformer_norm_first=True)), ("tutorial_ragged", "bf16", {})])
def test_norm_first_and_bf16_embedders(name, precision, over):
    model, tokens, mask = golden_case(name, precision, **over)
    max_exact = min(widest(mask), 10)
    res = run(model, tokens, mask, max_exact=max_exact, samples=4)
    ref = reference((name, precision, "over" if over else "", max_exact, 4), model, tokens, mask, res, max_exact, 4)
    check_list(model, tokens, mask, res, ref, f"{name} {precision} {over}")
    check_values(mask, res, ref, max_exact, 4, "prob", f"{name} {precision} {over}")


# ---- 9. whole model ----------------------------------------------------------------------------------------------------------------------
def test_whole_model():
    from transformercvn.hip.attention import ProngShapley
    from transformercvn.network.layers.packed_data import token_rows
    cfg, model, batch = golden_model("tutorial_ragged")
    args = to_device(batch)[:8]
    net = model.network
    with torch.no_grad():
        ev0, pr0, weights = model.forward_with_attention(*args)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    res = model.prong_shapley(*args, samples=4)
    assert isinstance(res, ProngShapley) and torch.equal(res.prong_logits, pr0)
    e = rel_err(res.event_logits.cpu(), ev0.cpu())
    print(f"whole model: the scan's full coalitions vs forward()'s event logits {e:.2e}")
    assert e < LOGIT_TOL
    rt = net.hip_runtime()
    assert torch.equal(rt.head.attention(token_rows(args[7], args[7].shape[0])), weights), "the forward's workspace was touched by the scan"
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    with torch.no_grad():
        tokens, mask = net.prong_embedding(*model._network_inputs(*args))
    ref = reference(("whole", 10, 4), model, tokens, mask, res, 10, 4)
    check_list(model, tokens, mask, res, ref, "whole model tutorial_ragged")
    check_values(mask, res, ref, 10, 4, "prob", "whole model tutorial_ragged")
    B, P = args[7].shape
    cls = res.event_logits.argmax(1)
    assert res.for_target().shape == (B, P) and res.pairs().shape == (B, P, P)
    assert torch.equal(res.for_target(), res.phi[torch.arange(B), :, cls]) and torch.equal(res.for_target(1), res.phi[:, :, 1])
    assert torch.equal(res.for_target(cls), res.for_target("event"))
    assert torch.equal(torch.nan_to_num(res.pairs(2)), torch.nan_to_num(res.interaction[..., 2]))
    with pytest.raises(ValueError):
        res.for_target(res.phi.shape[2])
    with pytest.raises(ValueError):
        res.for_target("prong")
    model.train()
    with pytest.raises(RuntimeError):
        model.prong_shapley(*args)
    with pytest.raises(RuntimeError):
        net.prong_shapley(*model._network_inputs(*args))
    with pytest.raises(RuntimeError):
        rt.forward_prong_shapley(*model._network_inputs(*args))


def test_a_scan_counts_as_one_forward_for_the_training_step_that_follows():
    """Two identically seeded bf16 models (dropout 0.1, pixel noise on): eval forward() in one, prong_shapley() in the other, then the same
    training step in both: the same seeds are drawn, so the losses are equal bit for bit."""
    cfg, over, batch, g = load_case("tutorial_b2p4")
    assert cfg.dropout > 0
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    dev_batch = to_device(batch)
    out = {}
    for tag in ("forward", "scan"):
        model = build_trainer(cfg, sd, precision="bf16")
        model.eval()
        rt = model.network.hip_runtime()
        with torch.no_grad():
            if tag == "forward":
                model.forward(*dev_batch[:8])
            else:
                model.prong_shapley(*dev_batch[:8])
        assert rt.step == 1
        model.train()
        rt.zero_grad()
        loss = model.training_step(dev_batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        out[tag] = loss.detach().clone()
    print(f"training step after forward() {out['forward'].item():.6f}, after prong_shapley() {out['scan'].item():.6f}")
    assert torch.equal(out["forward"], out["scan"])


# ---- 10. no atomics: two runs agree bit for bit ------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    model, tokens, mask = golden_case("tutorial_ragged")
    a, b = (run(model, tokens, mask, max_exact=8, samples=16, seed=3) for _ in range(2))
    assert not bool(a.exact.all()) and bool(a.exact.any())
    for k in ("event_logits", "phi", "stderr", "exact", "offsets", "masks", "event", "coalition_logits", "permutations"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(torch.isnan(a.interaction), torch.isnan(b.interaction))
    assert torch.equal(torch.nan_to_num(a.interaction), torch.nan_to_num(b.interaction))
