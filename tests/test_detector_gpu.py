"""Detector-effect scans on the GPU.

Engine level, no model: tcvn_detector_variants / _build_pass on synthetic lists whose maps hold 0, 1, 255, 256 and 700 hits (the chunk
boundaries of the build kernel; duplicate pixels included) against detector_reference (Philox restated with numpy integers, the effect
in torch float32): header, pass bounds, vimg, index, out_coords and out_values are torch.equal -- the scale is one float32 multiplication
on both sides.

Model level: every variant of both scopes against the brute force (the plain forward() of the same model on event b alone with the
perturbed lists, the draws taken with the event's original (b, s)), none sampled; identity and empty maps; the response against the
float64 formula on the result's own logits, and -- no fixture flips an arg-max -- on hand-made random logits whose reference holds
both values of `flipped`; and what the call must leave alone.  Each test prints its maxima.

Gates (max-norm relative on logits, as in test_occlusion_gpu.py; none is derived from what the scan gives):
  fp32 vs brute force / base    rel_err < 1e-4   the project's gate for stage-by-stage logits
  bf16 vs brute force           M = the largest rel_err between forward(batch)[b] and forward(event b alone) over the events of small_b3
                                and tutorial_ragged, measured in the test on plain forward(); M == 0: the fp32 gate, otherwise max(2 M, 1e-4)
  response                      |kernel - float64 formula| <= 1e-6 (fp32 values of a probability and of a difference of two)
  surviving, index, flipped, the NaN pattern     exact

Measured on an MI355X: see DESIGN.md section 5g."""
import ctypes as C

import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case, rel_err
from model_utils import build_trainer, to_device
import occlusion_reference as R
import detector_reference as DR

pytestmark = pytest.mark.gpu

LOGIT_TOL, RESPONSE_TOL = 1e-4, 1e-6
GUARD = 4                       # rows behind a pass's hit list that the build must leave alone
_cache = {}


def E(**kw):
    from transformercvn.hip.detector import DetectorEffect
    return DetectorEffect(**kw)


# ---- 1. engine level: synthetic lists ---------------------------------------------------------------------------------------------------------
SHAPE, CHANNELS, COUNTS = (40, 28), 3, (0, 1, 255, 256, 700)
MAPS5 = torch.tensor([[0, 0], [0, 1], [0, 2], [1, 0], [1, 1]], dtype=torch.int32)


def list_effects():
    return [E(), E(scale=0.5), E(threshold=128.0), E(dead_rows=(0, 40)), E(dead_cols=(10, 14)), E(drop=0.0, seed=3), E(drop=1.0, seed=3),
            E(drop=0.3, seed=3), E(shift=(-5, 0)), E(shift=(5, 0)), E(shift=(0, -5)), E(shift=(0, 5)),
            E(scale=0.5, threshold=40.0, dead_rows=(3, 6), dead_cols=(10, 14), drop=0.3, shift=(2, -3), seed=7)]


def synthetic_list(channels=CHANNELS):
    """Five maps of 40 x 28 with 0, 1, 255, 256 and 700 hits, sorted by map, uint8-like values; hit 40 of the 255-hit map repeats the
    pixel of hit 7, and 700 hits on 1 120 pixels collide on their own.  (The same hits at every channel count.)"""
    key = "list" if channels == CHANNELS else f"list {channels}"
    if key not in _cache:
        g = torch.Generator().manual_seed(21)
        rows = []
        for img, n in enumerate(COUNTS):
            c = torch.stack((torch.full((n,), img), torch.randint(0, SHAPE[0], (n,), generator=g),
                             torch.randint(0, SHAPE[1], (n,), generator=g)), 1)
            if n == 255:
                c[40, 1:] = c[7, 1:]
            rows.append(c)
        coords = torch.cat(rows).int()
        values = torch.randint(0, 256, (coords.shape[0], channels), generator=g).float()
        big = coords[coords[:, 0] == 4]
        assert len({(y, x) for _, y, x in big.tolist()}) < 700 and coords.shape[0] == sum(COUNTS)
        _cache[key] = (coords, values)
    return _cache[key]


def device_variants(coords, values, effects, max_pass, n_img=5, img_bs=MAPS5):
    """One tcvn_detector_variants call -> (host words, vimg, index, workspace, the list on the device), the outputs pre-filled with -7."""
    from transformercvn.hip import detector
    from transformercvn.hip._lib import lib
    from transformercvn.hip.native import ptr, stream_ptr
    dev, K = torch.device("cuda"), len(effects)
    d_coords, d_values, d_bs = coords.to(dev).contiguous(), values.to(dev).contiguous(), img_bs.to(dev).contiguous()
    rows = n_img * K
    need = lib.tcvn_detector_workspace_bytes(n_img, K, max_pass)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    vimg = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    index = torch.full((rows, 4), -7, dtype=torch.int32, device=dev)
    words = 4 + -(-rows // max_pass) + 1
    host = (C.c_int64 * words)(*([-7] * words))
    table = detector.effect_table(effects)
    rc = lib.tcvn_detector_variants(ptr(d_coords), coords.shape[0], n_img, *SHAPE, values.shape[1], ptr(d_values), ptr(d_bs), table, K, max_pass,
                                    ptr(vimg), ptr(index), ptr(ws), ws.numel(), host, words, stream_ptr())
    for k in range(K):                       # the caller's array is not read after the call: overwrite it before any build pass
        table[k].scale, table[k].drop, table[k].shift_x = 123.0, 1.0, 9
    assert rc == 0
    return list(host), vimg, index, ws, (d_coords, d_values, d_bs)


def check_passes(ref, vimg, index, ws, on_device, K, max_pass, n_img=5):
    from transformercvn.hip._lib import lib
    from transformercvn.hip.native import ptr, stream_ptr
    d_coords, d_values, d_bs = on_device
    channels = d_values.shape[1]
    V, bounds = ref["header"][0], ref["bounds"]
    for k in range(-(-V // max_pass)):
        first, count, n = k * max_pass, min(max_pass, V - k * max_pass), bounds[k + 1] - bounds[k]
        if n == 0:
            continue
        out_coords = torch.full((n + GUARD, 3), -7, dtype=torch.int32, device=d_coords.device)
        out_values = torch.full((n + GUARD, channels), -7.0, device=d_coords.device)
        assert lib.tcvn_detector_build_pass(ptr(d_coords), ptr(d_values), d_coords.shape[0], channels, n_img, *SHAPE, ptr(d_bs), K, max_pass,
                                            ptr(vimg), ptr(ws), ws.numel(), first, count, ptr(out_coords), ptr(out_values), n + GUARD,
                                            stream_ptr()) == 0
        want_coords, want_values = DR.pass_reference(ref, first, count, channels)
        assert want_coords.shape[0] == n
        assert torch.equal(out_coords[:n].cpu(), want_coords), f"pass {k}: coords"
        assert torch.equal(out_values[:n].cpu(), want_values), f"pass {k}: values"
        assert bool((out_coords[n:] == -7).all()) and bool((out_values[n:] == -7.0).all()), f"pass {k}: rows behind the list"


def test_the_reference_exercises_every_branch():
    """What the exact comparison below rests on, asserted on the host reference: the threshold leaves hits with one, two and three
    channels and removes some; drop = 0.3 keeps and removes hits in every map of at least 255 hits; every shift pushes hits off its edge."""
    coords, values = synthetic_list()
    effects = list_effects()
    at, _, v = DR.apply_effect(coords, values, MAPS5, effects[2], SHAPE)
    assert {int(n) for n in (v != 0).sum(1).tolist()} == {1, 2, 3} and 0 < at.numel() < coords.shape[0]
    at, _, _ = DR.apply_effect(coords, values, MAPS5, effects[7], SHAPE)
    kept = torch.bincount(coords[at, 0].long(), minlength=5).tolist()
    assert all(0 < kept[i] < COUNTS[i] for i in (2, 3, 4)), kept
    assert DR.apply_effect(coords, values, MAPS5, effects[3], SHAPE)[0].numel() == 0
    assert DR.apply_effect(coords, values, MAPS5, effects[6], SHAPE)[0].numel() == 0
    assert DR.apply_effect(coords, values, MAPS5, effects[5], SHAPE)[0].numel() == coords.shape[0]
    for e in effects[8:12]:
        assert 0 < DR.apply_effect(coords, values, MAPS5, e, SHAPE)[0].numel() < coords.shape[0]
    at, _, v = DR.apply_effect(coords, values, MAPS5, effects[12], SHAPE)
    assert 0 < at.numel() < coords.shape[0] and bool((v == 0).any())


@pytest.mark.parametrize("max_pass", [1, 3, 256])
def test_variant_list_and_hit_lists_are_exact(max_pass):
    coords, values = synthetic_list()
    effects = list_effects()
    K = len(effects)
    ref = DR.list_reference(coords, values, 5, SHAPE, MAPS5, effects, max_pass)
    host, vimg, index, ws, on_device = device_variants(coords, values, effects, max_pass)
    V = ref["header"][0]
    print(f"V {host[0]} unsorted {host[1]} bad {host[2]} nh {host[3]} passes {-(-V // max_pass)} (reference {ref['header']})")
    assert V == 4 * K, "the map without hits has no variant, every other map one per effect"
    assert host[:4] == ref["header"] and host[4:] == ref["bounds"]
    assert torch.equal(vimg[:V].cpu(), ref["vimg"]) and bool((vimg[V:] == -7).all())
    assert torch.equal(index[:V].cpu(), ref["index"]) and bool((index[V:] == -7).all())
    assert ref["index"][ref["index"][:, 2] == 3][:, 3].tolist() == [0, 0, 0, 0], "dead rows over the whole map: empty variants"
    check_passes(ref, vimg, index, ws, on_device, K, max_pass)


@pytest.mark.parametrize("channels", [1, 4])
def test_variant_list_and_hit_lists_are_exact_at_other_channel_counts(channels):
    """The same lists with one and four value channels per hit: the threshold's "any channel left" rule and the build pass's value rows
    (hit * channels + c) against the reference, exactly as at three."""
    coords, values = synthetic_list(channels)
    assert values.shape[1] == channels and torch.equal(coords, synthetic_list()[0])
    effects, max_pass = list_effects(), 3
    K = len(effects)
    ref = DR.list_reference(coords, values, 5, SHAPE, MAPS5, effects, max_pass)
    at, _, v = DR.apply_effect(coords, values, MAPS5, effects[2], SHAPE)
    assert {int(n) for n in (v != 0).sum(1).tolist()} == set(range(1, channels + 1)) and 0 < at.numel() < coords.shape[0]
    host, vimg, index, ws, on_device = device_variants(coords, values, effects, max_pass)
    V = ref["header"][0]
    assert V == 4 * K and host[:4] == ref["header"] and host[4:] == ref["bounds"]
    assert torch.equal(vimg[:V].cpu(), ref["vimg"]) and bool((vimg[V:] == -7).all())
    assert torch.equal(index[:V].cpu(), ref["index"]) and bool((index[V:] == -7).all())
    check_passes(ref, vimg, index, ws, on_device, K, max_pass)


def test_flags_and_the_cleaning_retry():
    """A shuffled list raises the first flag, a hit outside the map the second; plan_variants' clean-and-sort retry then gives the
    variants of the clean list (the same counts: which hits survive does not depend on their order)."""
    from dataclasses import replace
    from transformercvn.hip import detector, occlusion
    from transformercvn.hip.engine import _EmbedderEngine
    coords, values = synthetic_list()
    effects = list_effects()
    K, max_pass = len(effects), 3
    clean = DR.list_reference(coords, values, 5, SHAPE, MAPS5, effects, max_pass)
    engine = _EmbedderEngine()                       # the list calls need no plan
    dev = torch.device("cuda")
    perm = torch.randperm(coords.shape[0], generator=torch.Generator().manual_seed(2))
    assert coords[300, 0] == 3 and coords[600, 0] == 4            # y = H in map 3, x = -1 in map 4 and a hit of map n_img, in map order
    outside = torch.cat((coords[:300], torch.tensor([[3, 40, 3]], dtype=torch.int32), coords[300:600],
                         torch.tensor([[4, 5, -1]], dtype=torch.int32), coords[600:], torch.tensor([[5, 1, 1]], dtype=torch.int32)))
    extra = torch.full((1, 3), 200.0)
    outside_values = torch.cat((values[:300], extra, values[300:600], extra, values[600:], extra))
    for what, c, v, flags in (("shuffled", coords[perm], values[perm], (True, False)), ("outside", outside, outside_values, (False, True))):
        lst = occlusion.HitList(engine, c.contiguous().to(dev), v.contiguous().to(dev), 0, 5, MAPS5.to(dev), 0, 0)
        table = detector.effect_table(effects)
        _, unsorted, bad = engine.detector_variants(lst.coords, lst.values, 5, SHAPE, lst.img_bs, max_pass, table)
        assert (unsorted, bad) == flags, what
        cleaned, plan = occlusion.plan_variants(lst, SHAPE, None, max_pass, detector=(table,))
        assert cleaned is not lst and cleaned.coords.shape[0] == coords.shape[0]
        assert torch.equal(plan.index.cpu(), clean["index"]) and torch.equal(plan.vimg.cpu(), clean["vimg"]) and plan.V == 4 * K
        assert plan.bounds == clean["bounds"][:len(plan.bounds)]
        ref = DR.list_reference(cleaned.coords.cpu(), cleaned.values.cpu(), 5, SHAPE, MAPS5, effects, max_pass)
        if what == "outside":
            assert torch.equal(cleaned.coords.cpu(), coords) and torch.equal(cleaned.values.cpu(), values)
        check_passes(ref, plan.vimg, plan.index, plan.ws, (cleaned.coords, cleaned.values, cleaned.img_bs), K, max_pass)


# ---- 2. model level -------------------------------------------------------------------------------------------------------------------------
def golden_model(name, precision="fp32", **over_cfg):
    cfg, over, batch, g = load_case(name)
    if over_cfg:
        cfg = O.tutorial_config(**dict(over, **over_cfg))
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    model = build_trainer(cfg, sd, precision=precision)
    model.eval()
    return cfg, model, batch, sd


def light(name):
    """The case's inputs behind a small DenseNet: for tests of what does not depend on the weights."""
    if "light " + name not in _cache:
        _cache["light " + name] = golden_model(name, densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16,
                                               pixel_embedding_dim=64, num_encoder_layers=2)
    return _cache["light " + name]


def model_effects():
    """Identity, the five effects of the documentation's example, every row dead (empty maps), and all five at once."""
    return [E(), E(scale=0.95), E(threshold=20.0), E(dead_cols=(120, 136)), E(drop=0.05, seed=1), E(shift=(0, 4)), E(dead_rows=(0, 400)),
            E(scale=0.9, threshold=30.0, dead_rows=(100, 110), dead_cols=(120, 136), drop=0.3, shift=(-3, 2), seed=5)]


IDENTITY, EMPTY = 0, 6


def scan(model, batch, effects, scope, **kw):
    res = model.detector_scan(*to_device(batch)[:8], effects=effects, scope=scope, **kw)
    B, P = batch[7].shape
    K, Ce, Cp = len(effects), res.event_logits.shape[1], res.prong_logits.shape[2]
    tensors = [res.event_logits, res.prong_logits, res.varied_event_logits, res.varied_prong_logits, res.valid]
    if scope == "event":
        assert res.index is None and res.surviving.dtype == torch.int32 and res.surviving.shape == (K, B, 1 + P)
        assert res.varied_event_logits.shape == (K, B, Ce) and res.varied_prong_logits.shape == (K, B, P, Cp)
        tensors.append(res.surviving)
    else:
        V = res.index.shape[0]
        assert res.surviving is None and res.index.dtype == torch.int32 and res.index.shape == (V, 4) and res.num_variants == V
        assert res.varied_event_logits.shape == (V, Ce) and res.varied_prong_logits.shape == (V, P, Cp)
        tensors.append(res.index)
    for t in tensors:
        assert not t.requires_grad and t.is_cuda
    assert res.scope == scope and res.effects == tuple(effects)
    assert torch.equal(res.valid.cpu()[:, 1:] >= 0, batch[7].cpu()) and bool((res.valid[:, 0] >= 0).all())
    return res


def expected_maps(batch, maps="all"):
    """(b, s) of every scanned map, ascending (every map of the fixtures holds a hit)."""
    return [(b, s) for b in range(batch[7].shape[0]) for s in DR.scanned_slots(batch, b, maps)]


def check_map_scope(model, batch, cfg, what, key, gate=LOGIT_TOL, **kw):
    effects = model_effects()
    res = scan(model, batch, effects, "map", **kw)
    index = res.index.cpu()
    want = [(b, s, k) for b, s in expected_maps(batch) for k in range(len(effects))]
    assert [tuple(r[:3]) for r in index.tolist()] == want, what + ": variant list"
    if key not in _cache:
        _cache[key] = DR.brute_force(model, batch, [(b, effects[k], [s]) for b, s, k in want], cfg.pixel_shape)
    ref_ev, ref_pr, left = _cache[key]
    assert index[:, 3].tolist() == [left[i][s] for i, (b, s, k) in enumerate(want)], what + ": surviving hits"
    e_ev = rel_err(res.varied_event_logits.cpu(), ref_ev)
    e_pr = rel_err(R.valid_rows(res.varied_prong_logits.cpu(), index, batch[7]), R.valid_rows(ref_pr, index, batch[7]))
    base = res.event_logits.cpu()
    effect = (ref_ev - base[index[:, 0].long()]).abs().max().item() / base.abs().max().item()
    same = index[:, 2] == IDENTITY
    e_id = rel_err(res.varied_event_logits.cpu()[same], base[index[same][:, 0].long()])
    p_id = rel_err(R.valid_rows(res.varied_prong_logits.cpu()[same], index[same], batch[7]),
                   R.valid_rows(res.prong_logits.cpu()[index[same][:, 0].long()], index[same], batch[7]))
    print(f"{what}: {index.shape[0]} variants, rel err event logits {e_ev:.2e}, prong logits {e_pr:.2e}; identity vs base event {e_id:.2e} "
          f"prong {p_id:.2e} (gate {gate:.1e}); largest move of the logits {effect:.2e}")
    assert max(e_ev, e_pr, e_id, p_id) < gate, (what, e_ev, e_pr, e_id, p_id)
    assert effect > gate, "the variants must move the logits by more than the gate"
    return res


def check_event_scope(model, batch, cfg, what, key, gate=LOGIT_TOL, **kw):
    effects = model_effects()
    res = scan(model, batch, effects, "event", **kw)
    B, P = batch[7].shape
    K = len(effects)
    cases = [(k, b) for k in range(K) for b in range(B)]
    if key not in _cache:
        _cache[key] = DR.brute_force(model, batch, [(b, effects[k], DR.scanned_slots(batch, b)) for k, b in cases], cfg.pixel_shape)
    ref_ev, ref_pr, left = _cache[key]
    want = torch.full((K, B, 1 + P), -1, dtype=torch.int32)
    for i, (k, b) in enumerate(cases):
        for s, n in left[i].items():
            want[k, b, s] = n
    assert torch.equal(res.surviving.cpu(), want), what + ": surviving hits"
    assert torch.equal(want < 0, (res.valid.cpu() < 0).expand(K, B, 1 + P)) and bool((want[EMPTY][want[EMPTY] >= 0] == 0).all())
    rows = torch.tensor([[b] for k, b in cases])                 # valid_rows reads the event of every row
    ev, pr = res.varied_event_logits.cpu().reshape(K * B, -1), res.varied_prong_logits.cpu().reshape(K * B, P, -1)
    e_ev = rel_err(ev, ref_ev)
    e_pr = rel_err(R.valid_rows(pr, rows, batch[7]), R.valid_rows(ref_pr, rows, batch[7]))
    base = res.event_logits.cpu()
    effect = (ref_ev - base[rows[:, 0]]).abs().max().item() / base.abs().max().item()
    e_id = rel_err(res.varied_event_logits.cpu()[IDENTITY], base)
    p_id = rel_err(res.varied_prong_logits.cpu()[IDENTITY][batch[7]], res.prong_logits.cpu()[batch[7]])
    print(f"{what}: {K} settings x {B} events, rel err event logits {e_ev:.2e}, prong logits {e_pr:.2e}; identity vs base event {e_id:.2e} "
          f"prong {p_id:.2e} (gate {gate:.1e}); largest move of the logits {effect:.2e}")
    assert max(e_ev, e_pr, e_id, p_id) < gate, (what, e_ev, e_pr, e_id, p_id)
    assert effect > gate, "the settings must move the logits by more than the gate"
    return res


def shared_small_b3():
    """The full fp32 small_b3 model, built once."""
    if "model" not in _cache:
        _cache["model"] = golden_model("small_b3")
    return _cache["model"]


@pytest.mark.parametrize("max_pass", [8, 256])
def test_every_map_variant_equals_the_brute_force(max_pass):
    """9 maps x 8 effects = 72 variants: passes of at most 8 maps, or one pass per hit list."""
    cfg, model, batch, _ = shared_small_b3()
    res = check_map_scope(model, batch, cfg, f"small_b3 scope map max_maps_per_pass={max_pass}", "bf map", max_maps_per_pass=max_pass)
    assert res.index.shape[0] == 72
    _cache["map result"] = res


def test_every_event_setting_equals_the_brute_force():
    cfg, model, batch, _ = shared_small_b3()
    for max_pass in (8, 256):
        check_event_scope(model, batch, cfg, f"small_b3 scope event max_maps_per_pass={max_pass}", "bf event", max_maps_per_pass=max_pass)


def test_empty_maps_equal_the_whole_map_brute_force():
    """Scope map under "every row is dead": the variant is the empty map, which the occlusion scan's whole-map brute force removes too."""
    cfg, model, batch, _ = shared_small_b3()
    res = _cache.get("map result") or scan(model, batch, model_effects(), "map")
    index = res.index.cpu()
    empty = index[:, 2] == EMPTY
    assert int(empty.sum()) == 9 and bool((index[empty][:, 3] == 0).all())
    ref_ev, ref_pr = R.brute_force(model, batch, index[empty], (1, 1), whole_map=True)
    e_ev = rel_err(res.varied_event_logits.cpu()[empty], ref_ev)
    e_pr = rel_err(R.valid_rows(res.varied_prong_logits.cpu()[empty], index[empty], batch[7]), R.valid_rows(ref_pr, index[empty], batch[7]))
    effect = (ref_ev - res.event_logits.cpu()[index[empty][:, 0].long()]).abs().max().item() / res.event_logits.abs().max().item()
    print(f"empty maps vs the whole-map brute force: event {e_ev:.2e} prong {e_pr:.2e} (gate {LOGIT_TOL:.1e}); effect of an empty map {effect:.2e}")
    assert max(e_ev, e_pr) < LOGIT_TOL and effect > LOGIT_TOL


def batch_composition_spread(model, batch):
    """M of one case: forward(batch)[b] against forward(event b alone), both plain forward()."""
    worst = 0.0
    with torch.no_grad():
        ev, pr = model.forward(*to_device(batch)[:8])
        for b in range(batch[7].shape[0]):
            ev1, pr1 = model.forward(*to_device(R.single_event(batch, b)))
            m = batch[7][b]
            worst = max(worst, rel_err(ev1[0].cpu(), ev[b].cpu()), rel_err(pr1[0].cpu()[m], pr[b].cpu()[m]))
    return worst


@pytest.mark.parametrize("scope", ["map", "event"])
def test_every_variant_equals_the_brute_force_bf16(scope):
    """The gate is measured on forward() alone first (see the module docstring)."""
    if "bf16" not in _cache:
        cases = {name: golden_model(name, "bf16") for name in ("small_b3", "tutorial_ragged")}
        _cache["bf16"] = (cases["small_b3"], max(batch_composition_spread(model, batch) for cfg, model, batch, _ in cases.values()))
    (cfg, model, batch, _), M = _cache["bf16"]
    gate = LOGIT_TOL if M == 0 else max(2 * M, LOGIT_TOL)
    print(f"bf16: batch-composition spread of forward() M = {M:.3e} -> gate {gate:.3e}")
    check = check_map_scope if scope == "map" else check_event_scope
    for max_pass in (8, 256):
        check(model, batch, cfg, f"small_b3 bf16 scope {scope} max_maps_per_pass={max_pass}", "bf16 bf " + scope, gate=gate,
              max_maps_per_pass=max_pass)


def test_the_ragged_batch_with_padded_slots():
    """tutorial_ragged behind the light model: 3 events of 16 prong slots, 22 of them valid, so 26 slots are padded.  Every variant of
    both scopes against the brute force, none sampled: 25 maps x 8 effects = 200 variants (scope map), 8 settings x 3 events (scope
    event)."""
    cfg, model, batch, _ = light("tutorial_ragged")
    effects = model_effects()
    B, P = batch[7].shape
    assert int(batch[7].sum()) == 22 and not bool(batch[7].all())
    by_all = check_map_scope(model, batch, cfg, "tutorial_ragged (light) scope map", "ragged bf map")
    assert by_all.index.shape[0] == 25 * len(effects)
    res = check_event_scope(model, batch, cfg, "tutorial_ragged (light) scope event", "ragged bf event")
    assert bool((res.surviving.cpu()[:, :, 1:][:, ~batch[7]] == -1).all()) and bool((res.surviving.cpu()[:, :, 1:][:, batch[7]] >= 0).all())
    only = scan(model, batch, effects, "event", maps="prongs")
    assert bool((only.surviving[:, :, 0] == -1).all()) and torch.equal(only.surviving[:, :, 1:], res.surviving[:, :, 1:])
    by_map = scan(model, batch, effects[:3], "map", maps="event")
    assert by_map.index.cpu()[:, :3].tolist() == [[b, 0, k] for b in range(B) for k in range(3)]


def test_both_scopes_equal_the_brute_force_sdxl():
    """The SDXL embedder serves the scan through the same engine calls: test_sdxl_gpu.py's small model, 3 events with 2, 3 and 1 prongs."""
    cfg = O.tutorial_config(embedder="sdxl", initial_pixel_dim=8, pixel_embedding_dim=64, hidden_dim=64, num_encoder_layers=2,
                            num_prong_decoder_layers=3, dropout=0.0, pixel_noise_std=0.0)
    model = build_trainer(cfg, O.fill_state(cfg, 7))
    batch = O.synthetic_batch([2, 3, 1], 9, cfg)
    assert type(model).__name__ == "NeutrinoFullSDXLTrainer"
    model.eval()
    res = check_map_scope(model, batch, cfg, "sdxl small model scope map", "sdxl bf map")
    assert res.index.shape[0] == 9 * len(model_effects())
    check_event_scope(model, batch, cfg, "sdxl small model scope event", "sdxl bf event")


# ---- 3. response ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maps", ["all", "event"])
@pytest.mark.parametrize("scope", ["event", "map"])
def test_response_and_summary(scope, maps):
    cfg, model, batch, _ = light("small_b3")
    B, P = batch[7].shape
    effects = model_effects()
    K = len(effects)
    res = scan(model, batch, effects, scope, maps=maps)
    classes = torch.tensor([(int(res.event_logits[b].argmax()) + 1 + b) % res.event_logits.shape[1] for b in range(B)])
    for target in ("event", "prong", 1, classes, classes.cuda()):
        prong = isinstance(target, str) and target == "prong"
        r = res.response(target)
        ref_p, ref_d, ref_f = DR.response_reference(res, target.cpu() if torch.is_tensor(target) else target)
        shape = (K, B, 1 + P) if scope == "map" else (K, B, P) if prong else (K, B)
        assert r.prob.shape == r.delta.shape == r.flipped.shape == shape and r.prob.dtype == r.delta.dtype == torch.float32
        assert r.flipped.dtype == torch.uint8 and r.prob.is_cuda
        there = ~torch.isnan(ref_p)
        assert torch.equal(~torch.isnan(r.prob.cpu()), there) and torch.equal(~torch.isnan(r.delta.cpu()), there), "the NaN pattern"
        assert torch.equal(r.flipped.cpu().bool(), ref_f), "flipped"
        if scope == "map":                   # a variant per scanned map (every map of the fixture holds a hit); "prong" leaves s = 0 out
            scanned = torch.zeros(B, 1 + P, dtype=torch.bool)
            scanned[:, 0] = not prong
            if maps == "all":
                scanned[:, 1:] = batch[7]
            assert torch.equal(there, scanned.expand(K, B, 1 + P))
        elif prong:
            assert torch.equal(there, batch[7].expand(K, B, P))
        else:
            assert bool(there.all())
        if not there.any():
            continue
        e_p = (r.prob.cpu().double() - ref_p)[there].abs().max().item()
        e_d = (r.delta.cpu().double() - ref_d)[there].abs().max().item()
        moved = ref_d[there].abs().max().item()
        s = res.summary(target)
        want_mean = torch.nanmean(ref_d.abs().reshape(K, -1), 1)
        want_flip = torch.stack([ref_f[k][there[k]].double().mean() for k in range(K)])
        e_s = max((s.mean_abs_delta.cpu().double() - want_mean).abs().max().item(), (s.flip_rate.cpu().double() - want_flip).abs().max().item())
        print(f"response scope={scope} maps={maps} target={target if not torch.is_tensor(target) else 'tensor'}: max |kernel - float64| prob "
              f"{e_p:.2e} delta {e_d:.2e} summary {e_s:.2e}; largest |delta| {moved:.2e}; flipped {int(ref_f.sum())} of {int(there.sum())}")
        assert e_p <= RESPONSE_TOL and e_d <= RESPONSE_TOL and e_s <= RESPONSE_TOL
        assert s.mean_abs_delta.shape == s.flip_rate.shape == (K,)
        if not (scope == "map" and maps == "event" and prong):
            assert moved > RESPONSE_TOL          # a response that never moves would not tell prob from the base probability


@pytest.mark.parametrize("scope", ["event", "map"])
def test_response_of_hand_made_logits_with_flips(scope):
    """The fixtures' predictions never flip, so `flipped` and `flip_rate` are checked here on seeded random logits (no model): 5 events
    with 1 to 4 valid prong slots of 4, 6 settings, half of the varied rows close to the base row and half unrelated to it.  The
    reference holds both values of `flipped` for every target, which the test asserts, and the kernel must put each at its entry."""
    res = DR.random_result(scope, device="cuda")
    host = DR.random_result(scope)
    B, P, K = 5, 4, 6
    assert bool((host.valid[:, 1:] < 0).any()) and bool((host.valid[:, 1:] >= 0).any())
    classes = torch.tensor([(b + 1) % 4 for b in range(B)])
    for target in ("event", "prong", 1, classes):
        prong = isinstance(target, str) and target == "prong"
        r, s = res.response(target), res.summary(target)
        ref_p, ref_d, ref_f = DR.response_reference(host, target)
        there = ~torch.isnan(ref_p)
        assert r.prob.shape == ref_p.shape == ((K, B, 1 + P) if scope == "map" else (K, B, P) if prong else (K, B))
        assert torch.equal(~torch.isnan(r.prob.cpu()), there) and torch.equal(~torch.isnan(r.delta.cpu()), there), "the NaN pattern"
        assert bool(there.any()) and (scope == "event" and not prong or not bool(there.all()))
        flips = ref_f[there]
        assert bool(flips.any()) and not bool(flips.all()), "the reference must hold both values of flipped"
        assert torch.equal(r.flipped.cpu().bool(), ref_f), "flipped"
        e_p = (r.prob.cpu().double() - ref_p)[there].abs().max().item()
        e_d = (r.delta.cpu().double() - ref_d)[there].abs().max().item()
        want_mean = torch.nanmean(ref_d.abs().reshape(K, -1), 1)
        want_flip = torch.stack([ref_f[k][there[k]].double().mean() for k in range(K)])
        e_m = (s.mean_abs_delta.cpu().double() - want_mean).abs().max().item()
        e_f = (s.flip_rate.cpu().double() - want_flip).abs().max().item()
        print(f"hand-made scope={scope} target={target if not torch.is_tensor(target) else 'tensor'}: max |kernel - float64| prob {e_p:.2e} "
              f"delta {e_d:.2e} mean_abs_delta {e_m:.2e} flip_rate {e_f:.2e}; flipped {int(flips.sum())} of {int(there.sum())}, "
              f"flip rates {[round(float(x), 3) for x in want_flip]}")
        assert max(e_p, e_d, e_m, e_f) <= RESPONSE_TOL
        assert bool(((want_flip > 0) & (want_flip < 1)).any()), "a flip rate strictly between 0 and 1"


# ---- 4. what the call leaves alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["event", "map"])
def test_attention_state_and_the_next_forward_survive_the_scan(scope):
    from transformercvn.network.layers.packed_data import token_rows
    cfg, model, batch, _ = light("tutorial_ragged")
    args = to_device(batch)[:8]
    effects = model_effects()[:4]
    rt = model.network.hip_runtime()
    ev, pr, weights = model.forward_with_attention(*args)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    step = rt.step
    res = model.detector_scan(*args, effects=effects, scope=scope)
    assert rt.step == step + 1, "the scan counts as one forward()"
    again = rt.head.attention(token_rows(args[7], args[7].shape[0]))
    assert torch.equal(again, weights), "the head's forward workspace was touched by the scan"
    assert torch.equal(res.event_logits, ev) and torch.equal(res.prong_logits, pr)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    with torch.no_grad():
        ev2, pr2 = model.forward(*args)
    assert torch.equal(ev2, ev) and torch.equal(pr2, pr)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            model.detector_scan(*args, effects=effects, scope=scope)
    finally:
        model.eval()


@pytest.mark.parametrize("scope", ["event", "map"])
def test_two_calls_agree_and_the_pass_size_does_not_matter(scope):
    cfg, model, batch, _ = light("small_b3")
    effects = model_effects()
    a, b, one = scan(model, batch, effects, scope), scan(model, batch, effects, scope), scan(model, batch, effects, scope, max_maps_per_pass=1)
    hits = "surviving" if scope == "event" else "index"
    for k in ("event_logits", "prong_logits", "varied_event_logits", "varied_prong_logits", "valid", hits):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for target in ("event", "prong"):            # bit patterns: NaN entries compare equal too
        for x, y in zip(a.response(target), b.response(target)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), target
    assert torch.equal(getattr(one, hits), getattr(a, hits)), "the hit lists do not depend on max_maps_per_pass"
    e_ev = rel_err(one.varied_event_logits.cpu(), a.varied_event_logits.cpu())
    valid = (a.valid.cpu()[:, 1:] >= 0)
    rows = (lambda t: t.cpu()[:, valid]) if scope == "event" else (lambda t: R.valid_rows(t.cpu(), a.index.cpu(), batch[7]))
    e_pr = rel_err(rows(one.varied_prong_logits), rows(a.varied_prong_logits))
    print(f"scope {scope}: max_maps_per_pass 1 vs 256, rel err event {e_ev:.2e} prong {e_pr:.2e} (gate {LOGIT_TOL:.1e})")
    assert max(e_ev, e_pr) < LOGIT_TOL
