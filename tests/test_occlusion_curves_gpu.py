"""Deletion / insertion curves on the GPU.  The ranking and the variant list (b, s, k, m_k) against a Python sort by (-relevance, tile
index) on the host, exactly; every variant against the brute force (the plain forward() of the same model on event b alone with the hits
of the m_k top-ranked tiles removed / kept -- forward() is pinned to the reference goldens by test_full_model_gpu.py); the end points
against the base prediction and the whole-map brute force; step 1 of a 4-tile map against the flat scan's variant of its top tile; curve
and area against the float64 formula on the result's own logits; and what the call must leave alone.  Every variant of a case is
compared, none sampled; each test prints its maxima.

Gates (max-norm relative on logits, as in test_occlusion_gpu.py; none is derived from what the curves give):
  fp32 vs brute force / base / flat scan   rel_err < 1e-4   the project's gate for stage-by-stage logits
  bf16 vs brute force    M = the largest rel_err between forward(batch)[b] and forward(event b alone) over the events of small_b3 and
                         tutorial_ragged, measured in the test on plain forward(); M == 0: the fp32 gate, otherwise max(2 M, 1e-4)
  curve, area            |kernel - float64 formula| <= 1e-6 (fp32 values of a probability; the area is an average of at most 65 of them)
  rank, index            exact

Measured on an MI355X: see DESIGN.md section 5d."""
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case, rel_err
from model_utils import build_trainer, to_device
import occlusion_reference as R
import occlusion_curves_reference as CR

pytestmark = pytest.mark.gpu

LOGIT_TOL, CURVE_TOL = 1e-4, 1e-6
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
    if "light " + name not in _cache:
        _cache["light " + name] = golden_model(name, densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16,
                                               pixel_embedding_dim=64, num_encoder_layers=2)
    return _cache["light " + name]


def shared_small_b3():
    """The full fp32 small_b3 model, built once: its curves and brute-force results are shared between tests."""
    if "model" not in _cache:
        _cache["model"] = golden_model("small_b3")
    return _cache["model"]


def tied_relevance(batch, tile, shape, seed=3):
    """Quarters in [0, 1) from a seeded generator, so that every map has ties; in the event map of event 0 the two occupied tiles with
    the lowest indices carry -0.0 and 0.0 in that order: -0.0 counts as +0.0, so the lower index still comes first."""
    B, P = batch[7].shape
    Ht, Wt = R.grid_of(shape, tile)
    rel = torch.randint(0, 4, (B, 1 + P, Ht, Wt), generator=torch.Generator().manual_seed(seed)).float() / 4
    tiles = sorted(ty * Wt + tx for ty, tx in CR.occupied_tiles(batch, tile, "event")[(0, 0)])
    rel[0, 0].view(-1)[tiles[0]] = -0.0
    rel[0, 0].view(-1)[tiles[1]] = 0.0
    assert torch.signbit(rel[0, 0].view(-1)[tiles[0]]) and not torch.signbit(rel[0, 0].view(-1)[tiles[1]])
    return rel


def curves(model, batch, relevance, **kw):
    res = model.occlusion_curves(*to_device(batch)[:8], relevance, **kw)
    for t in (res.event_logits, res.prong_logits, res.step_event_logits, res.step_prong_logits, res.index, res.rank):
        assert not t.requires_grad and t.is_cuda
    V = res.index.shape[0]
    B, P = batch[7].shape
    assert res.index.dtype == torch.int32 and res.index.shape == (V, 4) and res.num_variants == V
    assert res.rank.dtype == torch.int32 and res.rank.shape == (B, 1 + P, *res.grid)
    assert res.step_event_logits.shape == (V, res.event_logits.shape[1])
    assert res.step_prong_logits.shape == (V, P, res.prong_logits.shape[2])
    return res


# ---- 1. ranking and variant list ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [(64, 64), (16, 16)])
@pytest.mark.parametrize("name", ["small_b3", "tutorial_ragged"])
def test_ranking_and_variant_list_are_exact(name, tile):
    cfg, model, batch, _ = light(name)
    shape = cfg.pixel_shape
    rel = tied_relevance(batch, tile, shape)
    n_maps = {"event": batch[7].shape[0], "prongs": int(batch[7].sum())}
    n_maps["all"] = n_maps["event"] + n_maps["prongs"]
    assert n_maps["all"] == {"small_b3": 9, "tutorial_ragged": 25}[name]
    occupied = []
    for maps in ("all", "event", "prongs"):
        for steps in (1, 4, 7):
            res = curves(model, batch, rel, tile=tile, steps=steps, maps=maps, mode="deletion" if steps != 4 else "insertion")
            rank, index = CR.expected_rank_and_index(batch, rel, tile, shape, steps, maps)
            assert res.grid == R.grid_of(shape, tile) and res.tile == tile and res.steps == steps
            assert res.index.shape[0] == (steps + 1) * n_maps[maps], (maps, steps, res.index.shape[0])
            assert torch.equal(res.rank.cpu(), rank), (maps, steps)
            assert torch.equal(res.index.cpu(), index), (maps, steps)
        if maps == "all":
            occupied = [int((rank[b, s] >= 0).sum()) for b, s in sorted(CR.occupied_tiles(batch, tile).keys())]
            ties = min(int(rank[b, s].max()) + 1 - len(set(rel[b, s][rank[b, s] >= 0].tolist()))
                       for b, s in CR.occupied_tiles(batch, tile).keys())
            assert ties > 0, "every map must hold tiles of equal relevance"
    print(f"{name} {tile}: occupied tiles per map {min(occupied)}..{max(occupied)}, {n_maps['all']} maps, rank and index exact")
    table = {("small_b3", (64, 64)): (27, 35), ("small_b3", (16, 16)): (66, 446), ("tutorial_ragged", (64, 64)): (18, 35),
             ("tutorial_ragged", (16, 16)): (38, 450)}
    assert (min(occupied), max(occupied)) == table[(name, tile)]          # the figures counted from the fixtures on the host


def test_a_shuffled_hit_list_gives_the_same_ranking_and_variants():
    cfg, model, batch, _ = light("small_b3")
    tile = (64, 64)
    rel = tied_relevance(batch, tile, cfg.pixel_shape)
    res = curves(model, batch, rel, tile=tile, steps=4)
    g = torch.Generator().manual_seed(11)
    shuffled = list(batch)
    for c, v in ((2, 3), (5, 6)):
        perm = torch.randperm(batch[c].shape[0], generator=g)
        shuffled[c], shuffled[v] = batch[c][perm].contiguous(), batch[v][perm].contiguous()
    assert not bool((shuffled[5][1:, 0] >= shuffled[5][:-1, 0]).all())
    res2 = curves(model, tuple(shuffled), rel, tile=tile, steps=4)
    assert torch.equal(res2.rank, res.rank) and torch.equal(res2.index, res.index)
    # the fixtures have unique coordinates per image, so the order of the hits does not change any image: same logits
    e = rel_err(res2.step_event_logits.cpu(), res.step_event_logits.cpu())
    print(f"shuffled hit list: {res.index.shape[0]} variants, rel err vs the sorted list {e:.2e}")
    assert e < LOGIT_TOL


# ---- 2. every variant equals the brute force ------------------------------------------------------------------------------------------------
TILE, STEPS = (100, 70), 4


def check_curves(model, batch, cfg, what, mode, key=None, gate=LOGIT_TOL, **kw):
    """Every variant against forward() on event b alone with the hits of the m_k first tiles removed / kept."""
    rel = tied_relevance(batch, TILE, cfg.pixel_shape, seed=7)
    res = curves(model, batch, rel, tile=TILE, steps=STEPS, mode=mode, **kw)
    rank, index = CR.expected_rank_and_index(batch, rel, TILE, cfg.pixel_shape, STEPS)
    assert torch.equal(res.rank.cpu(), rank) and torch.equal(res.index.cpu(), index), what + ": ranking / variant list"
    if key is None or key not in _cache:
        ref = CR.brute_force(model, batch, index, rank, TILE, mode)
        if key is not None:
            _cache[key] = ref
    else:
        ref = _cache[key]
    ref_ev, ref_pr = ref
    e_ev = rel_err(res.step_event_logits.cpu(), ref_ev)
    e_pr = rel_err(R.valid_rows(res.step_prong_logits.cpu(), index, batch[7]), R.valid_rows(ref_pr, index, batch[7]))
    effect = (ref_ev - res.event_logits.cpu()[index[:, 0].long()]).abs().max().item() / res.event_logits.abs().max().item()
    print(f"{what}: {index.shape[0]} variants, rel err event logits {e_ev:.2e}, prong logits {e_pr:.2e} (gate {gate:.1e}); "
          f"largest move of the logits {effect:.2e}")
    assert e_ev < gate and e_pr < gate, (what, e_ev, e_pr)
    # the comparison says something only if a result that returned the unoccluded logits for every variant would fail it
    assert effect > gate, "the variants must move the logits by more than the gate"
    return res


@pytest.mark.parametrize("max_pass", [8, 256])
@pytest.mark.parametrize("mode", ["deletion", "insertion"])
def test_every_variant_equals_the_brute_force(mode, max_pass):
    """9 maps x 5 steps = 45 variants per mode: 6 passes (3 event + 3 prong) of at most 8 maps, or one pass per hit list."""
    cfg, model, batch, _ = shared_small_b3()
    res = check_curves(model, batch, cfg, f"small_b3 100x70 {mode} max_maps_per_pass={max_pass}", mode, key="bf " + mode,
                       max_maps_per_pass=max_pass)
    assert res.index.shape[0] == 45 and res.grid == (4, 4) and res.mode == mode
    _cache["curves " + mode] = res


# ---- 3. end points --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["deletion", "insertion"])
def test_end_points(mode):
    cfg, model, batch, _ = shared_small_b3()
    res = _cache.get("curves " + mode) or curves(model, batch, tied_relevance(batch, TILE, cfg.pixel_shape, seed=7), tile=TILE,
                                                 steps=STEPS, mode=mode)
    index = res.index.cpu()
    k_full, k_empty = (0, STEPS) if mode == "deletion" else (STEPS, 0)
    full, empty = index[:, 2] == k_full, index[:, 2] == k_empty
    assert int(full.sum()) == int(empty.sum()) == 9
    n = torch.tensor([int((res.rank[b, s] >= 0).sum()) for b, s in index[full][:, :2].tolist()], dtype=torch.int32)
    assert (index[index[:, 2] == 0][:, 3] == 0).all() and torch.equal(index[index[:, 2] == STEPS][:, 3], n), "m_0 = 0 and m_K = n"
    ev, pr = res.step_event_logits.cpu(), res.step_prong_logits.cpu()
    # the unoccluded map: the base prediction of its event
    b = index[full][:, 0].long()
    e_ev = rel_err(ev[full], res.event_logits.cpu()[b])
    e_pr = rel_err(R.valid_rows(pr[full], index[full], batch[7]), R.valid_rows(res.prong_logits.cpu()[b], index[full], batch[7]))
    # the empty map: the whole-map brute force
    if "bf whole" not in _cache:
        _cache["bf whole"] = R.brute_force(model, batch, index[empty], TILE, whole_map=True)
    ref_ev, ref_pr = _cache["bf whole"]
    w_ev = rel_err(ev[empty], ref_ev)
    w_pr = rel_err(R.valid_rows(pr[empty], index[empty], batch[7]), R.valid_rows(ref_pr, index[empty], batch[7]))
    effect = (ref_ev - res.event_logits.cpu()[index[empty][:, 0].long()]).abs().max().item() / res.event_logits.abs().max().item()
    print(f"end points {mode}: unoccluded vs base event {e_ev:.2e} prong {e_pr:.2e}; empty vs whole-map brute force event {w_ev:.2e} "
          f"prong {w_pr:.2e} (gate {LOGIT_TOL:.1e}); effect of an empty map {effect:.2e}")
    assert max(e_ev, e_pr, w_ev, w_pr) < LOGIT_TOL
    assert effect > LOGIT_TOL


# ---- 4. agreement with the flat scan --------------------------------------------------------------------------------------------------------
def test_step_one_of_four_tiles_is_the_flat_scan_variant_of_the_top_tile():
    cfg, model, batch, _ = shared_small_b3()
    tile = (200, 140)
    rel = tied_relevance(batch, tile, cfg.pixel_shape, seed=9)
    res = curves(model, batch, rel, tile=tile, steps=4)
    scan = model.occlusion_maps(*to_device(batch)[:8], tile=tile)
    index, rank = res.index.cpu(), res.rank.cpu()
    rows = {tuple(r): v for v, r in enumerate(scan.index.cpu().tolist())}
    step1 = (index[:, 2] == 1).nonzero().flatten().tolist()
    assert len(step1) == 9 and (index[step1][:, 3] == 1).all(), "every map has 4 occupied tiles, so m_1 = 1"
    pick = []
    for v in step1:
        b, s = index[v, 0].item(), index[v, 1].item()
        assert int((rank[b, s] >= 0).sum()) == 4
        ty, tx = (rank[b, s] == 0).nonzero()[0].tolist()
        pick.append(rows[(b, s, ty, tx)])
    e_ev = rel_err(res.step_event_logits.cpu()[step1], scan.occluded_event_logits.cpu()[pick])
    e_pr = rel_err(R.valid_rows(res.step_prong_logits.cpu()[step1], index[step1], batch[7]),
                   R.valid_rows(scan.occluded_prong_logits.cpu()[pick], index[step1], batch[7]))
    effect = (scan.occluded_event_logits.cpu()[pick] - scan.event_logits.cpu()[index[step1][:, 0].long()]).abs().max().item() \
        / scan.event_logits.abs().max().item()
    print(f"deletion step 1 vs the flat scan's top tile (200x140): event {e_ev:.2e}, prong {e_pr:.2e}; effect {effect:.2e}")
    assert e_ev < LOGIT_TOL and e_pr < LOGIT_TOL
    assert effect > LOGIT_TOL


# ---- 5. curve and area ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maps", ["all", "event"])
def test_curve_and_area(maps):
    cfg, model, batch, _ = light("small_b3")
    B, P = batch[7].shape
    rel = tied_relevance(batch, TILE, cfg.pixel_shape)
    res = curves(model, batch, rel, tile=TILE, steps=5, maps=maps, mode="insertion")
    scanned = torch.zeros(B, 1 + P, dtype=torch.bool)
    scanned[:, 0] = True
    if maps == "all":
        scanned[:, 1:] = batch[7]
    assert not scanned.all()
    classes = torch.tensor([(int(res.event_logits[b].argmax()) + 1 + b) % res.event_logits.shape[1] for b in range(B)])
    for target in ("event", "prong", 1, classes, classes.cuda()):
        curve, auc = res.curve(target), res.auc(target)
        assert curve.shape == (B, 1 + P, 6) and auc.shape == (B, 1 + P) and curve.dtype == auc.dtype == torch.float32 and curve.is_cuda
        ref_curve, ref_auc = CR.curve_reference(res, target.cpu() if torch.is_tensor(target) else target)
        want = scanned.clone()
        if isinstance(target, str) and target == "prong":
            want[:, 0] = False
        assert torch.equal(~torch.isnan(curve.cpu()), want[..., None].expand(-1, -1, 6)), "NaN exactly at the rows without variants"
        assert torch.equal(~torch.isnan(auc.cpu()), want) and torch.equal(torch.isnan(ref_auc), torch.isnan(auc.cpu()))
        if not want.any():
            continue
        e_c = (curve.cpu().double() - ref_curve)[want].abs().max().item()
        e_a = (auc.cpu().double() - ref_auc)[want].abs().max().item()
        spread = (ref_curve[want].max(-1).values - ref_curve[want].min(-1).values).max().item()
        print(f"curve maps={maps} target={target if not torch.is_tensor(target) else 'tensor'}: max |kernel - float64| curve {e_c:.2e}, "
              f"area {e_a:.2e}; largest rise of a curve {spread:.2e}")
        assert e_c <= CURVE_TOL and e_a <= CURVE_TOL
        assert spread > CURVE_TOL          # flat curves would not tell the steps apart


# ---- 6. accepted inputs ---------------------------------------------------------------------------------------------------------------------
def test_results_are_accepted_as_relevance():
    from transformercvn.hip import occlusion
    cfg, model, batch, _ = light("small_b3")
    args = to_device(batch)[:8]
    scan = model.occlusion_maps(*args, tile=TILE)
    refined = model.occlusion_refine(*args, tile=(200, 140), levels=2, keep=0.25)
    assert refined.levels[-1].tile == TILE
    for result, heat in ((scan, occlusion.heatmap(scan, "event")), (refined, occlusion.refined_heatmap(refined))):
        direct = curves(model, batch, result, steps=3)
        named = curves(model, batch, result, tile=TILE, steps=3)
        by_map = curves(model, batch, heat, tile=TILE, steps=3)
        assert direct.tile == TILE and direct.grid == (4, 4)
        assert int((direct.rank >= 0).sum()) > 0
        for other in (named, by_map):
            assert torch.equal(direct.rank, other.rank) and torch.equal(direct.index, other.index)
            assert torch.equal(direct.step_event_logits, other.step_event_logits)


# ---- 7. bf16 --------------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("mode", ["deletion", "insertion"])
def test_every_variant_equals_the_brute_force_bf16(mode):
    """The gate is measured on forward() alone first (see the module docstring)."""
    if "bf16" not in _cache:
        cases = {name: golden_model(name, "bf16") for name in ("small_b3", "tutorial_ragged")}
        _cache["bf16"] = (cases["small_b3"], max(batch_composition_spread(model, batch) for cfg, model, batch, _ in cases.values()))
    (cfg, model, batch, _), M = _cache["bf16"]
    gate = LOGIT_TOL if M == 0 else max(2 * M, LOGIT_TOL)
    print(f"bf16: batch-composition spread of forward() M = {M:.3e} -> gate {gate:.3e}")
    for max_pass in (8, 256):
        check_curves(model, batch, cfg, f"small_b3 100x70 bf16 {mode} max_maps_per_pass={max_pass}", mode, key="bf16 bf " + mode, gate=gate,
                     max_maps_per_pass=max_pass)


# ---- 8. what the call leaves alone ----------------------------------------------------------------------------------------------------------
def test_attention_state_and_the_next_forward_survive_the_curves():
    from transformercvn.network.layers.packed_data import token_rows
    cfg, model, batch, _ = light("tutorial_ragged")
    args = to_device(batch)[:8]
    rel = tied_relevance(batch, TILE, cfg.pixel_shape)
    ev, pr, weights = model.forward_with_attention(*args)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    res = model.occlusion_curves(*args, rel, tile=TILE, steps=3)
    rt = model.network.hip_runtime()
    again = rt.head.attention(token_rows(args[7], args[7].shape[0]))
    assert torch.equal(again, weights), "the head's forward workspace was touched by the curves"
    assert torch.equal(res.event_logits, ev) and torch.equal(res.prong_logits, pr)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    with torch.no_grad():
        ev2, pr2 = model.forward(*args)
    assert torch.equal(ev2, ev) and torch.equal(pr2, pr)
    model.train()
    try:
        with pytest.raises(RuntimeError):
            model.occlusion_curves(*args, rel, tile=TILE)
    finally:
        model.eval()


def test_two_calls_return_identical_tensors():
    cfg, model, batch, _ = light("small_b3")
    rel = tied_relevance(batch, (64, 64), cfg.pixel_shape)
    a, b = (curves(model, batch, rel, tile=(64, 64), steps=4, mode="insertion") for _ in range(2))
    for k in ("event_logits", "prong_logits", "index", "rank", "step_event_logits", "step_prong_logits"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for target in ("event", "prong"):          # bit patterns: NaN rows compare equal too
        assert torch.equal(a.curve(target).view(torch.int32), b.curve(target).view(torch.int32)), target
        assert torch.equal(a.auc(target).view(torch.int32), b.auc(target).view(torch.int32)), target
