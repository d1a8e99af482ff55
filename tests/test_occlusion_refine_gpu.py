"""Coarse-to-fine occlusion maps on the GPU.  With keep = 0 every level is the flat scan at its tile; with keep > 0 every level's variant
list is the stated rule applied on the host (numpy float32, integer arithmetic on the COO lists) to the previous level's own device heat
values -- exact, because the rule reads the kernel's float32 values --; every evaluated variant is compared with the flat scan's row of
the same (b, s, ty, tx), those of the last level also with the brute force (forward() on that event alone with the tile's hits
removed); the final map is the host painting of the levels' own heat arrays, exactly; and the call leaves alone what a flat scan leaves
alone.  Every variant of a case is compared, none sampled; each test prints its figures.

Gates (max-norm relative on logits, as in test_occlusion_gpu.py; none is derived from what the refinement gives):
  fp32   rel_err < 1e-4   the project's gate for stage-by-stage logits
  bf16   M = the largest rel_err between forward(batch)[b] and forward(event b alone), measured in the test on plain forward();
         M == 0: the fp32 gate, otherwise max(2 M, 1e-4)
  index, selection, final map: exact

KEEP = 0.25 -- chosen from {0.1, 0.25, 0.5} so that on the full fp32 small_b3 model, tile (64, 64), levels 3, every refined level both
selects and rejects variants for target "event" and "prong" (the test asserts it).  Measured on an MI355X, variants per level
(selected by the rule at that level); all three values would do, 0.25 is the call's default:
  target "event"  keep 0.1: 301 (191) / 685 (564) / 1761 (1165);  keep 0.25: 301 (125) / 471 (299) / 1033 (452);
                  keep 0.5: 301 (79) / 306 (107) / 405 (69)
  target "prong"  keep 0.1: 301 (170) / 531 (417) / 1032 (718);   keep 0.25: 301 (127) / 436 (236) / 638 (298);
                  keep 0.5: 301 (75) / 273 (80) / 237 (63)
"""
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case, rel_err
from model_utils import build_trainer, to_device
import occlusion_reference as R
import occlusion_refine_reference as RR

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
KEEP = 0.25
_cache = {}


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
    return golden_model(name, densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64,
                        num_encoder_layers=2)


def shared_small_b3():
    """The full fp32 small_b3 model and its refinements, built once."""
    if "model" not in _cache:
        _cache["model"] = golden_model("small_b3")
    return _cache["model"]


def shared_refinement(target):
    cfg, model, batch, _ = shared_small_b3()
    if ("refine", target) not in _cache:
        _cache[("refine", target)] = refine(model, batch, tile=(64, 64), levels=3, keep=KEEP, target=target)
    return _cache[("refine", target)]


def shared_flat(tile):
    cfg, model, batch, _ = shared_small_b3()
    if ("flat", tile) not in _cache:
        _cache[("flat", tile)] = model.occlusion_maps(*to_device(batch)[:8], tile=tile)
    return _cache[("flat", tile)]


def refine(model, batch, **kw):
    res = model.occlusion_refine(*to_device(batch)[:8], **kw)
    B, P = batch[7].shape
    assert res.keep == kw.get("keep", 0.25) and len(res.levels) == len(res.heats) == len(res.evaluated)
    for lv, level in enumerate(res.levels):
        assert level.event_logits is res.event_logits and level.prong_logits is res.prong_logits, "one forward(): the same objects"
        assert level.tile == RR.level_tile(tuple(kw["tile"]), lv)
        V = level.index.shape[0]
        assert level.index.dtype == torch.int32 and level.index.is_cuda and not level.occluded_event_logits.requires_grad
        assert level.occluded_event_logits.shape == (V, res.event_logits.shape[1])
        assert level.occluded_prong_logits.shape == (V, P, res.prong_logits.shape[2])
    return res


def rows_of(flat, index):
    """Positions in the flat scan of the rows (b, s, ty, tx) of `index`."""
    where = {tuple(r): v for v, r in enumerate(flat.index.cpu().tolist())}
    return torch.tensor([where[tuple(r)] for r in index.cpu().tolist()], dtype=torch.long)


def against_flat(level, flat, prong_mask, what, gate):
    """Every variant of a refinement level against the flat scan's row of the same (b, s, ty, tx) -> (errors, torch.equal)."""
    assert level.grid == flat.grid and level.tile == flat.tile
    index = level.index.cpu()
    pos = rows_of(flat, index)
    ev, fev = level.occluded_event_logits.cpu(), flat.occluded_event_logits.cpu()[pos]
    pr, fpr = level.occluded_prong_logits.cpu(), flat.occluded_prong_logits.cpu()[pos]
    e_ev = rel_err(ev, fev) if len(pos) else 0.0
    e_pr = rel_err(R.valid_rows(pr, index, prong_mask), R.valid_rows(fpr, index, prong_mask)) if len(pos) else 0.0
    same = torch.equal(ev, fev) and torch.equal(R.valid_rows(pr, index, prong_mask), R.valid_rows(fpr, index, prong_mask))
    print(f"{what}: {index.shape[0]} of {flat.index.shape[0]} variants, rel err vs the flat scan event logits {e_ev:.2e}, "
          f"prong logits {e_pr:.2e} (gate {gate:.1e}); torch.equal: {same}")
    assert e_ev < gate and e_pr < gate, (what, e_ev, e_pr)
    return same


def check_rule(res, batch, shape, target, what, maps="all", need_both=True):
    """Level 0 is the flat list; every later level's index is the host rule on the previous level's own device heat values."""
    counts = []
    for lv, level in enumerate(res.levels):
        tile = level.tile
        if lv == 0:
            want = R.expected_index(batch, tile, shape, maps)
        else:
            prev = res.levels[lv - 1]
            chosen = RR.selected_rows(prev.heatmap(target).cpu(), prev.index.cpu(), res.keep, target)
            counts.append((prev.index.shape[0], int(chosen.sum())))
            want = RR.child_index(batch, prev.index.cpu(), chosen, tile, shape, maps)
        assert level.grid == R.grid_of(shape, tile)
        assert level.index.shape[0] == want.shape[0], (what, lv, level.index.shape[0], want.shape[0])
        assert torch.equal(level.index.cpu(), want), (what, lv)
    last = res.levels[-1]
    chosen = RR.selected_rows(last.heatmap(target).cpu(), last.index.cpu(), res.keep, target)
    print(f"{what}: variants per level (selected by the rule) "
          + " / ".join(f"{v} ({k})" for v, k in counts + [(last.index.shape[0], int(chosen.sum()))]))
    if need_both:                     # if everything is refined, or nothing is, the comparison above shows nothing
        for lv, (v, k) in enumerate(counts):
            assert 0 < k < v, f"{what}: level {lv} selects {k} of {v} variants"
    return counts


def check_refine(model, batch, cfg, what, tile, gate=LOGIT_TOL, target="event", **kw):
    """One other configuration: the rule at every level, and every evaluated variant against the flat scan at that level's tile."""
    res = refine(model, batch, tile=tile, levels=3, keep=KEEP, target=target, **kw)
    assert len(res.levels) == 3 and res.stopped_at is None
    check_rule(res, batch, cfg.pixel_shape, target, what, need_both=False)
    args = to_device(batch)[:8]
    effect = 0.0
    for level in res.levels:
        flat = model.occlusion_maps(*args, tile=level.tile)
        against_flat(level, flat, batch[7], f"{what} tile {level.tile}", gate)
        base = res.event_logits.cpu()
        if level.index.shape[0]:
            effect = max(effect, (level.occluded_event_logits.cpu() - base[level.index.cpu()[:, 0].long()]).abs().max().item()
                         / base.abs().max().item())
    assert effect > gate, "the occlusions must move the logits by more than the gate"
    assert sum(l.index.shape[0] for l in res.levels[1:]) > 0, "nothing was refined"
    return res


# ---- 1. keep = 0 is the flat scan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, counts", [("small_b3", (301, 927, 2439, 4411)), ("tutorial_ragged", (839, 2552, 6172, 9922))])
def test_keep_0_is_the_flat_scan(name, counts):
    cfg, model, batch, _ = light(name)
    res = refine(model, batch, tile=(64, 64), levels=4, keep=0)
    assert len(res.levels) == 4 and res.stopped_at is None and res.num_variants == sum(counts)
    args = to_device(batch)[:8]
    for lv, level in enumerate(res.levels):
        tile = (64 >> lv, 64 >> lv)
        assert level.tile == tile and level.grid == R.grid_of(cfg.pixel_shape, tile)
        assert level.index.shape[0] == counts[lv]
        assert torch.equal(level.index.cpu(), R.expected_index(batch, tile, cfg.pixel_shape)), (name, tile)
        flat = model.occlusion_maps(*args, tile=tile)
        assert torch.equal(level.index, flat.index)
        against_flat(level, flat, batch[7], f"{name} keep=0 tile {tile}", LOGIT_TOL)
    for maps, want in (("event", 0), ("prongs", 1)):
        part = refine(model, batch, tile=(64, 64), levels=2, keep=0, maps=maps)
        for lv, level in enumerate(part.levels):
            assert torch.equal(level.index.cpu(), R.expected_index(batch, (64 >> lv, 64 >> lv), cfg.pixel_shape, maps))
            assert bool(((level.index[:, 1] > 0).long() == want).all())


# ---- 2. selection is the stated rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["event", "prong"])
def test_selection_is_the_stated_rule(target):
    cfg, model, batch, _ = shared_small_b3()
    res = shared_refinement(target)
    assert len(res.levels) == 3 and res.stopped_at is None and res.target == target and res.keep == KEEP
    flat = shared_flat((64, 64))
    assert torch.equal(res.levels[0].index, flat.index)
    assert against_flat(res.levels[0], flat, batch[7], f"small_b3 target={target} level 0", LOGIT_TOL)
    check_rule(res, batch, cfg.pixel_shape, target, f"small_b3 fp32 64x64 levels=3 keep={KEEP} target={target}")


def test_selection_with_explicit_classes_is_the_stated_rule():
    """An int and a [B] tensor of classes: the event groups, the heat values of those classes."""
    cfg, model, batch, _ = light("small_b3")
    B = batch[7].shape[0]
    with torch.no_grad():
        ev, _ = model.forward(*to_device(batch)[:8])
    classes = torch.tensor([(int(ev[b].argmax()) + 1 + b) % ev.shape[1] for b in range(B)])
    for target in (1, classes, classes.cuda()):
        res = refine(model, batch, tile=(64, 64), levels=3, keep=KEEP, target=target)
        host = target.cpu() if torch.is_tensor(target) else target
        check_rule(res, batch, cfg.pixel_shape, host, f"light small_b3 explicit classes {host}", need_both=False)
        assert res.levels[1].index.shape[0] > 0


# ---- 3. every evaluated variant is right ------------------------------------------------------------------------------------------------
def test_every_evaluated_variant_is_right():
    cfg, model, batch, _ = shared_small_b3()
    for target in ("event", "prong"):
        res = shared_refinement(target)
        for level in res.levels:
            against_flat(level, shared_flat(level.tile), batch[7], f"small_b3 target={target} tile {level.tile}", LOGIT_TOL)
    res = shared_refinement("event")
    last = res.levels[-1]
    index = last.index.cpu()
    assert index.shape[0] > 0
    ref_ev, ref_pr = R.brute_force(model, batch, index, last.tile)
    e_ev = rel_err(last.occluded_event_logits.cpu(), ref_ev)
    e_pr = rel_err(R.valid_rows(last.occluded_prong_logits.cpu(), index, batch[7]), R.valid_rows(ref_pr, index, batch[7]))
    effect = (ref_ev - res.event_logits.cpu()[index[:, 0].long()]).abs().max().item() / res.event_logits.abs().max().item()
    print(f"last level {last.tile} vs the brute force: {index.shape[0]} variants, rel err event logits {e_ev:.2e}, prong logits "
          f"{e_pr:.2e} (gate {LOGIT_TOL:.1e}); largest effect of one tile {effect:.2e}")
    assert e_ev < LOGIT_TOL and e_pr < LOGIT_TOL
    assert effect > LOGIT_TOL, "the occlusions must move the logits by more than the gate"


# ---- 4. other configurations ------------------------------------------------------------------------------------------------------------
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


def test_refine_bf16():
    cfg, model, batch, _ = golden_model("small_b3", "bf16")
    M = batch_composition_spread(model, batch)
    gate = LOGIT_TOL if M == 0 else max(2 * M, LOGIT_TOL)
    print(f"bf16: batch-composition spread of forward() M = {M:.3e} -> gate {gate:.3e}")
    check_refine(model, batch, cfg, "small_b3 bf16", (64, 64), gate=gate)


def test_refine_norm_first():
    cfg, model, batch, _ = golden_model("small_b3", transformer_norm_first=True)
    check_refine(model, batch, cfg, "small_b3 transformer_norm_first", (64, 64))


def test_refine_tutorial_ragged_layer_by_layer():
    from transformercvn.hip._lib import lib
    cfg, model, batch, _ = golden_model("tutorial_ragged")
    rt = model.network.hip_runtime()
    rt.ensure_bound()
    lib.tcvn_head_set_fused_encoder(rt.head.handle, 0)
    check_refine(model, batch, cfg, "tutorial_ragged layer by layer", (64, 64), target="prong")
    assert batch[7].shape[1] + 1 == 17


def test_refine_sdxl():
    cfg = O.tutorial_config(embedder="sdxl", initial_pixel_dim=8, pixel_embedding_dim=64, hidden_dim=64, num_encoder_layers=2,
                            num_prong_decoder_layers=3, dropout=0.0, pixel_noise_std=0.0)          # test_sdxl_gpu.py's small model
    sd = O.fill_state(cfg, 7)
    batch = O.synthetic_batch([2, 3, 1], 9, cfg)
    model = build_trainer(cfg, sd)
    assert type(model).__name__ == "NeutrinoFullSDXLTrainer"
    model.eval()
    res = check_refine(model, batch, cfg, "sdxl small model", (200, 140))
    assert [l.grid for l in res.levels] == [(2, 2), (4, 4), (8, 8)]


def test_refine_of_a_shuffled_hit_list():
    """An unsorted list gives the same index at every level, and (the order inside an image kept by a stable sort) the same logits."""
    cfg, model, batch, _ = light("small_b3")
    res = refine(model, batch, tile=(64, 64), levels=3, keep=KEEP)
    g = torch.Generator().manual_seed(11)
    shuffled = list(batch)
    for c, v in ((2, 3), (5, 6)):
        perm = torch.randperm(batch[c].shape[0], generator=g)
        shuffled[c], shuffled[v] = batch[c][perm].contiguous(), batch[v][perm].contiguous()
    assert not bool((shuffled[5][1:, 0] >= shuffled[5][:-1, 0]).all())
    res2 = refine(model, tuple(shuffled), tile=(64, 64), levels=3, keep=KEEP)
    assert len(res2.levels) == 3 and res.levels[1].index.shape[0] > 0
    for a, b in zip(res.levels, res2.levels):
        assert torch.equal(a.index, b.index) and a.grid == b.grid
        # the fixtures have unique coordinates per image, so the order of the hits does not change any image: same logits
        e = rel_err(b.occluded_event_logits.cpu(), a.occluded_event_logits.cpu()) if a.index.shape[0] else 0.0
        print(f"shuffled hit list, tile {a.tile}: {a.index.shape[0]} variants, rel err vs the sorted list {e:.2e}")
        assert e < LOGIT_TOL
    assert torch.equal(res.heatmap(), res2.heatmap())


# ---- 5. the final heat map --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["event", "prong"])
def test_final_heat_map_is_the_host_painting(target):
    from transformercvn.hip import occlusion
    cfg, model, batch, _ = shared_small_b3()
    res = shared_refinement(target)
    B, P = batch[7].shape
    heat = res.heatmap()
    last = res.levels[-1]
    assert heat.shape == (B, 1 + P, *last.grid) and heat.dtype == torch.float32 and heat.is_cuda
    assert torch.equal(heat, occlusion.refined_heatmap(res))
    own = [level.heatmap(target).cpu() for level in res.levels]
    occupied = RR.occupied_cells(batch, last.tile, cfg.pixel_shape)
    want = RR.paint(own, [level.index.cpu() for level in res.levels], occupied)
    h = heat.cpu()
    assert torch.equal(h, want), f"{int((h != want).sum())} cells differ from the host painting"
    assert (h[~occupied] == 0).all(), "cells without a hit must be exactly 0"
    assert (h[:, 1:][~batch[7]] == 0).all()
    # the map holds values of every level: cells painted from a coarser level exist beside cells of the last one
    deepest = torch.zeros_like(occupied)
    i = last.index.cpu().long()
    deepest[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = True
    assert bool(deepest.any()) and bool((occupied & ~deepest & (h != 0)).any())
    print(f"final map target={target}: grid {last.grid}, {int(occupied.sum())} cells with hits, {int(deepest.sum())} from the last "
          f"level, largest entry {h.abs().max().item():.3e}")
    assert h.abs().max().item() > 1e-6            # a map of zeros would pass the comparisons above for the wrong reason


# ---- 6. the variant budget --------------------------------------------------------------------------------------------------------------
def test_max_variants_stops_before_the_level_that_would_pass_it():
    cfg, model, batch, _ = light("small_b3")
    full = refine(model, batch, tile=(64, 64), levels=4, keep=0)
    assert [l.index.shape[0] for l in full.levels] == [301, 927, 2439, 4411]
    for budget, stop in ((300, 0), (301, 1), (301 + 927 + 2438, 2), (301 + 927 + 2439, 3), (301 + 927 + 2439 + 4411, None)):
        res = refine(model, batch, tile=(64, 64), levels=4, keep=0, max_variants=budget)
        assert res.stopped_at == stop, (budget, res.stopped_at)
        assert len(res.levels) == (4 if stop is None else stop) and res.num_variants <= budget
        for a, b in zip(res.levels, full.levels):
            assert torch.equal(a.index, b.index) and torch.equal(a.occluded_event_logits, b.occluded_event_logits)
            assert torch.equal(a.occluded_prong_logits, b.occluded_prong_logits)
        if res.levels:
            assert res.heatmap().shape[2:] == res.levels[-1].grid
        else:
            with pytest.raises(ValueError):
                res.heatmap()


# ---- 7. what it leaves alone ------------------------------------------------------------------------------------------------------------
def test_attention_of_the_explained_forward_survives_the_refinement():
    from transformercvn.network.layers.packed_data import token_rows
    cfg, model, batch, _ = light("tutorial_ragged")
    args = to_device(batch)[:8]
    ev, pr, weights = model.forward_with_attention(*args)
    res = model.occlusion_refine(*args, tile=(64, 64), levels=3, keep=KEEP)
    rt = model.network.hip_runtime()
    again = rt.head.attention(token_rows(args[7], args[7].shape[0]))
    assert torch.equal(again, weights), "the head's forward workspace was touched by the refinement"
    assert torch.equal(res.event_logits, ev) and torch.equal(res.prong_logits, pr)
    assert res.levels[1].index.shape[0] > 0


def test_a_refinement_counts_as_one_forward_for_the_training_step_that_follows():
    """Two identically seeded bf16 models (dropout 0.1, pixel noise on): eval forward() in one, occlusion_refine() in the other, then the
    same training step in both: the same seeds are drawn, so the losses and the dense layers' convolution weight gradients (the set
    test_determinism_gpu.py shows to be bit-reproducible) are equal bit for bit."""
    cfg, over, batch, g = load_case("tutorial_b2p4")
    assert cfg.dropout > 0
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    dev_batch = to_device(batch)
    out = {}
    for tag in ("forward", "refine"):
        model = build_trainer(cfg, sd, precision="bf16")
        model.eval()
        rt = model.network.hip_runtime()
        with torch.no_grad():
            if tag == "forward":
                model.forward(*dev_batch[:8])
            else:
                res = model.occlusion_refine(*dev_batch[:8], tile=(200, 140), levels=3, keep=KEEP)
                assert len(res.levels) == 3 and res.levels[2].index.shape[0] > 0
        assert rt.step == 1
        model.train()
        rt.zero_grad()
        loss = model.training_step(dev_batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if ".dense" in k and k.endswith(("conv1.weight", "conv2.weight"))}
        out[tag] = (loss.detach().clone(), grads)
    assert torch.equal(out["forward"][0], out["refine"][0]), (out["forward"][0].item(), out["refine"][0].item())
    assert len(out["forward"][1]) == 2 * 2 * sum(cfg.densenet_structure)
    diff = [k for k, v in out["forward"][1].items() if not torch.equal(v, out["refine"][1][k])]
    print(f"training step after forward() vs after occlusion_refine(): loss {out['refine'][0].item():.6f}, "
          f"{len(diff)} of {len(out['forward'][1])} dense-layer weight gradients differ")
    assert not diff, diff[:3]


def test_refinement_changes_no_state_and_train_mode_raises():
    cfg, model, batch, _ = light("small_b3")
    args = to_device(batch)[:8]
    with torch.no_grad():
        model.forward(*args)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    a = model.occlusion_refine(*args, tile=(64, 64), levels=2, keep=KEEP)
    b = model.occlusion_refine(*args, tile=(64, 64), levels=2, keep=KEEP)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    for x, y in zip(a.levels, b.levels):              # deterministic: two calls return identical tensors
        assert torch.equal(x.index, y.index) and torch.equal(x.occluded_event_logits, y.occluded_event_logits)
    assert torch.equal(a.heatmap(), b.heatmap())
    model.train()
    with pytest.raises(RuntimeError):
        model.occlusion_refine(*args)
