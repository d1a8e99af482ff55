"""Tile Shapley values on the GPU.  The variant list (b, s, m, k), the modes, the tile counts and the permutations against integer
arithmetic, the Python Philox and a Python sort on the host, exactly; every variant against the brute force (the plain forward() of the
same model on event b alone with only the coalition's hits kept -- forward() is pinned to the reference goldens by
test_full_model_gpu.py); phi, stderr, full and empty against the float64 formulas on the result's own logits and permutations; the
sampled estimate of a 2-tile map against the closed-form mixture of the exact marginals; and what the call must leave alone.  Every
variant of a case is compared, none sampled; each test prints its maxima.

Gates (none is derived from what the scan gives):
  fp32 vs brute force    rel_err < 1e-4 (max-norm relative on logits)   the project's gate for stage-by-stage logits
  bf16 vs brute force    M = the largest rel_err between forward(batch)[b] and forward(event b alone) over the events of small_b3 and
                         tutorial_ragged, measured in the test on plain forward(); M == 0: the fp32 gate, otherwise max(2 M, 1e-4)
  phi, stderr, full, empty   |kernel - float64 formula| <= 1e-6 for "prob" (fp32 values of differences of probabilities; both sides
                         start from the same fp32 logits and only the final rounding differs), <= 2^-22 max|logit| for "logit"
  efficiency             |sum phi - (full - empty)| <= (n + 2) 2^-24 max(|phi|, |full|, |empty|): n roundings of phi to fp32
  index, exact, n_tiles, permutations, V    exact

Measured on an MI355X: see DESIGN.md section 5i."""
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import rel_err
from model_utils import build_trainer, to_device
import occlusion_reference as R
import occlusion_shapley_reference as SR
import test_occlusion_curves_gpu as CG

pytestmark = pytest.mark.gpu

LOGIT_TOL, PROB_TOL = CG.LOGIT_TOL, CG.CURVE_TOL
assert (LOGIT_TOL, PROB_TOL) == (1e-4, 1e-6)
COARSE, FINE = (200, 140), (100, 70)
_cache = {}


def shapley(model, batch, **kw):
    res = model.occlusion_shapley(*to_device(batch)[:8], **kw)
    for t in (res.event_logits, res.prong_logits, res.coalition_event_logits, res.coalition_prong_logits, res.index, res.permutations,
              res.exact, res.n_tiles):
        assert not t.requires_grad and t.is_cuda
    V = res.index.shape[0]
    B, P = batch[7].shape
    Ht, Wt = res.grid
    assert res.index.dtype == torch.int32 and res.index.shape == (V, 4) and res.num_variants == V
    assert res.permutations.dtype == torch.int32 and res.permutations.shape == (B, 1 + P, res.samples, Ht * Wt)
    assert res.exact.dtype == torch.bool and res.exact.shape == (B, 1 + P)
    assert res.n_tiles.dtype == torch.int32 and res.n_tiles.shape == (B, 1 + P)
    assert res.coalition_event_logits.shape == (V, res.event_logits.shape[1])
    assert res.coalition_prong_logits.shape == (V, P, res.prong_logits.shape[2])
    return res


def check_lists(res, batch, shape, what, maps="all"):
    index, exact, n_tiles, perms = SR.expected_lists(batch, res.tile, shape, res.max_exact, res.samples, res.seed, maps)
    assert res.index.shape[0] == index.shape[0], (what, res.index.shape[0], index.shape[0])
    assert torch.equal(res.n_tiles.cpu(), n_tiles), what + ": n_tiles"
    assert torch.equal(res.exact.cpu(), exact), what + ": exact"
    assert torch.equal(res.index.cpu(), index), what + ": index"
    assert torch.equal(res.permutations.cpu(), perms), what + ": permutations"
    return index, exact, n_tiles, perms


# ---- 1. the lists ---------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"coarse exact": dict(tile=COARSE, max_exact=4, samples=3), "coarse sampled": dict(tile=COARSE, max_exact=3, samples=3),
           "fine sampled": dict(tile=FINE, samples=2)}
EXPECTED_V = {("tutorial_ragged", "coarse exact"): 375, ("tutorial_ragged", "coarse sampled"): 250,
              ("small_b3", "coarse exact"): 135, ("small_b3", "coarse sampled"): 90}
OCCUPIED = {("small_b3", COARSE): (4, 4), ("tutorial_ragged", COARSE): (4, 4), ("small_b3", FINE): (15, 16),
            ("tutorial_ragged", FINE): (13, 16)}


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["small_b3", "tutorial_ragged"])
def test_lists_are_exact(name, config):
    cfg, model, batch, _ = CG.light(name)
    kw = CONFIGS[config]
    res = shapley(model, batch, seed=5, **kw)
    assert res.tile == kw["tile"] and res.grid == R.grid_of(cfg.pixel_shape, kw["tile"]) and res.seed == 5
    index, exact, n_tiles, perms = check_lists(res, batch, cfg.pixel_shape, f"{name} {config}")
    n = n_tiles[n_tiles >= 0]
    n_maps = {"small_b3": 9, "tutorial_ragged": 25}[name]
    assert n.numel() == n_maps and (int(n.min()), int(n.max())) == OCCUPIED[(name, kw["tile"])]
    want = int(sum((2 ** k - 1) if 1 <= k <= res.max_exact else 1 + res.samples * (k - 1) for k in n.tolist()))
    assert res.num_variants == want == EXPECTED_V.get((name, config), want)
    assert bool(exact[n_tiles >= 0].all()) == (config == "coarse exact") and bool(exact.any()) == (config == "coarse exact")
    print(f"{name} {config}: {n_maps} maps, occupied tiles per map {int(n.min())}..{int(n.max())}, V = {want}; index, exact, n_tiles "
          f"and permutations equal the host's")
    for maps in ("event", "prongs"):
        part = shapley(model, batch, seed=5, maps=maps, **kw)
        check_lists(part, batch, cfg.pixel_shape, f"{name} {config} maps={maps}", maps)
        assert 0 < part.num_variants < want


def test_same_seed_same_bits_another_seed_another_table_and_a_shuffled_hit_list_the_same_lists():
    cfg, model, batch, _ = CG.light("small_b3")
    a, b = (shapley(model, batch, tile=FINE, samples=2, seed=3) for _ in range(2))
    for k in ("event_logits", "prong_logits", "index", "permutations", "exact", "n_tiles", "coalition_event_logits",
              "coalition_prong_logits"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for target in ("event", "prong"):            # bit patterns: NaN entries compare equal too
        for value in ("prob", "logit"):
            for x, y in zip(a.values(target, value), b.values(target, value)):
                assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (target, value)
    other = shapley(model, batch, tile=FINE, samples=2, seed=4)
    assert torch.equal(other.n_tiles, a.n_tiles) and torch.equal(other.index, a.index)
    assert not torch.equal(other.permutations, a.permutations)
    check_lists(other, batch, cfg.pixel_shape, "seed 4")
    wide = shapley(model, batch, tile=FINE, samples=2, seed=3 + (1 << 32))
    assert not torch.equal(wide.permutations, a.permutations), "the high word of the seed is part of the key"
    check_lists(wide, batch, cfg.pixel_shape, "seed 3 + 2^32")
    g = torch.Generator().manual_seed(11)
    shuffled = list(batch)
    for c, v in ((2, 3), (5, 6)):
        perm = torch.randperm(batch[c].shape[0], generator=g)
        shuffled[c], shuffled[v] = batch[c][perm].contiguous(), batch[v][perm].contiguous()
    assert not bool((shuffled[5][1:, 0] >= shuffled[5][:-1, 0]).all())
    res2 = shapley(model, tuple(shuffled), tile=FINE, samples=2, seed=3)
    for k in ("index", "permutations", "exact", "n_tiles"):
        assert torch.equal(getattr(res2, k), getattr(a, k)), k
    # the fixtures have unique coordinates per image, so the order of the hits does not change any image: same logits
    e = rel_err(res2.coalition_event_logits.cpu(), a.coalition_event_logits.cpu())
    print(f"shuffled hit list: {a.num_variants} variants, rel err vs the sorted list {e:.2e}")
    assert e < LOGIT_TOL


def test_max_variants_is_checked_before_any_variant_runs():
    cfg, model, batch, _ = CG.light("small_b3")
    args = to_device(batch)[:8]
    head = model.network.hip_runtime().head
    passes = []
    original = head.occlusion_pass
    head.occlusion_pass = lambda *a, **k: (passes.append(1), original(*a, **k))[1]
    try:
        with pytest.raises(ValueError, match="135"):
            model.occlusion_shapley(*args, tile=COARSE, max_exact=4, max_variants=134)
        assert passes == [], "no variant may run once the lists are known to hold too many"
        res = model.occlusion_shapley(*args, tile=COARSE, max_exact=4, max_variants=135)
        assert res.num_variants == 135 and len(passes) == 2
    finally:
        del head.occlusion_pass


# ---- 2. exact, sampled and empty maps in one call -------------------------------------------------------------------------------------------
def cut_event_maps(batch, tile, shape, counts, empty_prong=None):
    """The batch with the event map of event b cut to its first counts[b] occupied tiles (ascending tile index), and every hit of prong
    image `empty_prong` removed."""
    Wt = R.grid_of(shape, tile)[1]
    occ = SR.occupied(batch, tile, shape)
    out = [t.clone() for t in batch[:8]]
    ec, pc = out[2].long(), out[5].long()
    cell = (ec[:, 1] // tile[0]) * Wt + ec[:, 2] // tile[1]
    keep = torch.ones(ec.shape[0], dtype=torch.bool)
    for b, count in counts.items():
        assert len(occ[(b, 0)]) >= count
        inside = torch.zeros_like(keep)
        for t in occ[(b, 0)][:count]:
            inside |= cell == t
        keep &= (ec[:, 0] != b) | inside
    out[2], out[3] = out[2][keep].contiguous(), out[3][keep].contiguous()
    if empty_prong is not None:
        keep = pc[:, 0] != empty_prong
        out[5], out[6] = out[5][keep].contiguous(), out[6][keep].contiguous()
    return tuple(out)


def mixed_batch(batch, tile, shape):
    """small_b3 with the event map of event 0 cut to its first occupied tile (n = 1), the event map of event 1 to its first two (n = 2)
    and the first prong map to no hit at all (n = 0); the other six maps keep their four tiles."""
    return cut_event_maps(batch, tile, shape, {0: 1, 1: 2}, empty_prong=0)


def mixed():
    if "mixed" not in _cache:
        cfg, model, batch, _ = CG.light("small_b3")
        _cache["mixed"] = (cfg, model, mixed_batch(batch, COARSE, cfg.pixel_shape))
    return _cache["mixed"]


def test_exact_sampled_and_empty_maps_in_one_call():
    cfg, model, batch = mixed()
    B, P = batch[7].shape
    pb, pp = R.prong_slots(batch[7])
    first_prong = (pb[0], 1 + pp[0])
    res = shapley(model, batch, tile=COARSE, max_exact=2, samples=3, seed=1)
    index, exact, n_tiles, perms = check_lists(res, batch, cfg.pixel_shape, "mixed batch")
    assert int(n_tiles[0, 0]) == 1 and int(n_tiles[1, 0]) == 2 and int(n_tiles[first_prong]) == 0
    assert sorted(n_tiles[n_tiles >= 0].tolist()) == [0, 1, 2] + [4] * 6
    assert bool(exact[0, 0]) and bool(exact[1, 0]) and not bool(exact[first_prong]) and int(exact.sum()) == 2
    assert res.num_variants == 1 + 3 + 6 * (1 + 3 * 3)
    rows = index[:, :2].tolist()
    assert rows.count([0, 0]) == 1 and rows.count([1, 0]) == 3 and rows.count(list(first_prong)) == 0
    padded = torch.ones(B, 1 + P, dtype=torch.bool)
    padded[:, 0] = False
    padded[:, 1:] = ~batch[7].cpu()
    assert bool(padded.any()) and torch.equal(n_tiles < 0, padded)
    for value in ("prob", "logit"):
        phi, se, full, empty = (t.cpu() for t in res.values("event", value))
        assert phi.dtype == se.dtype == torch.float32 and full.dtype == empty.dtype == torch.float64
        assert phi.shape == se.shape == (B, 1 + P, 2, 2) and full.shape == empty.shape == (B, 1 + P)
        for t in (phi, se):
            assert torch.equal(torch.isnan(t), padded[..., None, None].expand(-1, -1, 2, 2)), "NaN exactly at the padded slots"
        assert torch.equal(torch.isnan(full), padded) and torch.equal(torch.isnan(empty), padded)
        # n = 1: one variant, phi = full - empty at the one occupied tile, stderr = 0
        t0 = SR.occupied(batch, COARSE, cfg.pixel_shape)[(0, 0)][0]
        one = phi[0, 0].flatten()
        assert one[t0].item() == (full[0, 0] - empty[0, 0]).float().item() and one[t0].item() != 0.0
        assert int((one != 0).sum()) == 1 and bool((se[0, 0] == 0).all()) and bool((se[1, 0] == 0).all())
        # n = 0: no variant, phi all 0, and the map without hits is the map as it is
        assert bool((phi[first_prong] == 0).all()) and bool((se[first_prong] == 0).all())
        assert full[first_prong].item() == empty[first_prong].item()
        # sampled maps: a standard error somewhere, 0 at the tiles without hits of every map
        assert bool((se[2, 0] > 0).any()) and int((phi[1, 0] != 0).sum()) == 2
    heat = res.heatmap("event")
    assert heat.shape == (B, 1 + P, 2, 2) and bool(torch.isfinite(heat).all()), "the shape and values occlusion_curves(relevance=) takes"
    assert torch.equal(heat.cpu()[~padded], res.values("event")[0].cpu()[~padded]) and bool((heat.cpu()[padded] == 0).all())
    curves = model.occlusion_curves(*to_device(batch)[:8], heat, tile=COARSE, steps=2)
    assert curves.num_variants == 3 * 8


# ---- 3. every variant equals the brute force ------------------------------------------------------------------------------------------------
def check_variants(model, batch, cfg, what, key=None, gate=LOGIT_TOL, **kw):
    res = shapley(model, batch, tile=COARSE, **kw)
    index, exact, n_tiles, perms = check_lists(res, batch, cfg.pixel_shape, what)
    if key is None or key not in _cache:
        ref = SR.brute_force(model, batch, index, exact, perms, COARSE, cfg.pixel_shape)
        if key is not None:
            _cache[key] = ref
    else:
        ref = _cache[key]
    ref_ev, ref_pr = ref
    e_ev = rel_err(res.coalition_event_logits.cpu(), ref_ev)
    e_pr = rel_err(R.valid_rows(res.coalition_prong_logits.cpu(), index, batch[7]), R.valid_rows(ref_pr, index, batch[7]))
    effect = (ref_ev - res.event_logits.cpu()[index[:, 0].long()]).abs().max().item() / res.event_logits.abs().max().item()
    print(f"{what}: {index.shape[0]} variants, rel err event logits {e_ev:.2e}, prong logits {e_pr:.2e} (gate {gate:.1e}); "
          f"largest move of the logits {effect:.2e}")
    assert e_ev < gate and e_pr < gate, (what, e_ev, e_pr)
    # the comparison says something only if a result that returned the unoccluded logits for every variant would fail it
    assert effect > gate, "the variants must move the logits by more than the gate"
    return res


MODES = {"exact": dict(max_exact=4, samples=3), "sampled": dict(max_exact=3, samples=3)}


@pytest.mark.parametrize("max_pass", [8, 256])
@pytest.mark.parametrize("mode", ["exact", "sampled"])
def test_every_variant_equals_the_brute_force(mode, max_pass):
    """9 maps of 4 occupied tiles: 9 x 15 = 135 coalitions, or 9 x (1 + 3 x 3) = 90 prefixes; in passes of at most 8 maps or one pass per
    hit list."""
    cfg, model, batch, _ = CG.shared_small_b3()
    res = check_variants(model, batch, cfg, f"small_b3 200x140 {mode} max_maps_per_pass={max_pass}", key="bf " + mode, seed=2,
                         max_maps_per_pass=max_pass, **MODES[mode])
    assert res.num_variants == {"exact": 135, "sampled": 90}[mode] and res.grid == (2, 2)
    # efficiency on real values: the scores of a map add up to what its hits are worth
    for value in ("prob", "logit"):
        phi, se, full, empty = (t.cpu().double() for t in res.values("event", value))
        scanned = res.n_tiles.cpu() >= 0
        gap = (phi.sum((2, 3)) - (full - empty))[scanned].abs()
        size = torch.maximum(phi.abs().amax((2, 3)), torch.maximum(full.abs(), empty.abs()))[scanned]
        bound = (res.n_tiles.cpu()[scanned] + 2).double() * 2.0 ** -24 * size
        print(f"  efficiency {value}: largest |sum phi - (full - empty)| {gap.max().item():.2e}, its bound {bound[gap.argmax()].item():.2e}")
        assert bool((gap <= bound).all())


def test_every_variant_equals_the_brute_force_bf16():
    """The gate is measured on forward() alone first (see the module docstring)."""
    if "bf16" not in CG._cache:
        cases = {name: CG.golden_model(name, "bf16") for name in ("small_b3", "tutorial_ragged")}
        CG._cache["bf16"] = (cases["small_b3"], max(CG.batch_composition_spread(model, batch) for cfg, model, batch, _ in cases.values()))
    (cfg, model, batch, _), M = CG._cache["bf16"]
    gate = LOGIT_TOL if M == 0 else max(2 * M, LOGIT_TOL)
    print(f"bf16: batch-composition spread of forward() M = {M:.3e} -> gate {gate:.3e}")
    check_variants(model, batch, cfg, "small_b3 200x140 bf16 sampled", gate=gate, seed=2, **MODES["sampled"])


def test_every_variant_equals_the_brute_force_sdxl():
    import test_sdxl_gpu
    cfg = test_sdxl_gpu._cfg()                                         # test_sdxl_gpu.py's small model
    model = build_trainer(cfg, O.fill_state(cfg, 7))
    batch = O.synthetic_batch([2, 3, 1], 9, cfg)
    assert type(model).__name__ == "NeutrinoFullSDXLTrainer"
    model.eval()
    res = check_variants(model, batch, cfg, "sdxl small model 200x140", seed=2, max_exact=3, samples=2)
    n = res.n_tiles.cpu()
    assert bool(res.exact.any()) or bool((n > 3).any())
    print(f"  sdxl: occupied tiles per map {sorted(n[n >= 0].tolist())}, exact maps {int(res.exact.sum())}")


# ---- 4. phi, stderr, full and empty against the float64 formulas ------------------------------------------------------------------------------
def check_values(res, batch, what):
    B = batch[7].shape[0]
    scanned = res.n_tiles.cpu() >= 0
    classes = torch.tensor([(int(res.event_logits[b].argmax()) + 1 + b) % res.event_logits.shape[1] for b in range(B)])
    top = max(res.event_logits.abs().max().item(), res.coalition_event_logits.abs().max().item(),
              res.prong_logits.cpu()[batch[7].cpu()].abs().max().item(),
              R.valid_rows(res.coalition_prong_logits.cpu(), res.index.cpu(), batch[7]).abs().max().item())
    for value, tol in (("prob", PROB_TOL), ("logit", 2.0 ** -22 * top)):
        for target in ("event", "prong", 1, classes, classes.cuda()):
            got = [t.cpu().double() for t in res.values(target, value)]
            ref = SR.values_reference(res, target.cpu() if torch.is_tensor(target) else target, value)
            want = scanned.clone()
            if isinstance(target, str) and target == "prong":
                want[:, 0] = False
            names = ("phi", "stderr", "full", "empty")
            errs = []
            for name, g, r in zip(names, got, ref):
                assert torch.equal(torch.isnan(g), torch.isnan(r)), (what, name, target, value)
                shown = want if g.dim() == 2 else want[..., None, None].expand_as(g)
                assert torch.equal(~torch.isnan(g), shown), (what, name, target, value)
                errs.append((g - r)[shown].abs().max().item() if bool(shown.any()) else 0.0)
            if not want.any():
                continue
            phi, se, full, empty = got
            n = res.n_tiles.cpu()[want]
            gap = (phi.sum((2, 3)) - (full - empty))[want].abs()
            size = torch.maximum(phi.abs().amax((2, 3)), torch.maximum(full.abs(), empty.abs()))[want]
            bound = (n + 2).double() * 2.0 ** -24 * size
            label = target if not torch.is_tensor(target) else "tensor"
            print(f"{what} value={value} target={label}: max |kernel - float64| phi {errs[0]:.2e} stderr {errs[1]:.2e} full {errs[2]:.2e} "
                  f"empty {errs[3]:.2e} (gate {tol:.2e}); efficiency gap {gap.max().item():.2e} (bound {bound[gap.argmax()].item():.2e}); "
                  f"largest |phi| {phi[want].abs().max().item():.2e}, largest stderr {se[want].max().item():.2e}")
            assert max(errs) <= tol, (what, target, value, errs)
            assert bool((gap <= bound).all()), (what, target, value)
            assert phi[want].abs().max().item() > tol, "scores below the gate would not tell the tiles apart"
            # tiles without hits are exactly 0
            Ht, Wt = res.grid
            occupied = torch.zeros(*res.n_tiles.shape, Ht * Wt, dtype=torch.bool)
            for (b, s), tiles in SR.occupied(batch, res.tile, (Ht * res.tile[0], Wt * res.tile[1])).items():
                occupied[b, s, tiles] = True
            free = want[..., None] & ~occupied
            assert bool((phi.reshape(*free.shape)[free] == 0).all()) and bool((se.reshape(*free.shape)[free] == 0).all())


def test_values_equal_the_float64_formulas_exact_and_sampled():
    cfg, model, batch = mixed()
    res = shapley(model, batch, tile=COARSE, max_exact=2, samples=5, seed=1)
    assert bool(res.exact.any()) and bool((~res.exact.cpu() & (res.n_tiles.cpu() > 0)).any())
    check_values(res, batch, "mixed batch 200x140 max_exact=2 samples=5")
    res = shapley(model, batch, tile=COARSE, max_exact=4, samples=1, seed=1)
    assert int(res.exact.sum()) == 8
    check_values(res, batch, "mixed batch 200x140 max_exact=4")


@pytest.mark.parametrize("maps", ["all", "event"])
def test_values_equal_the_float64_formulas_fine_tiles(maps):
    """15..16 players per map, 7 permutations of each."""
    cfg, model, batch, _ = CG.light("small_b3")
    B, P = batch[7].shape
    res = shapley(model, batch, tile=FINE, samples=7, seed=8, maps=maps)
    scanned = torch.zeros(B, 1 + P, dtype=torch.bool)
    scanned[:, 0] = True
    if maps == "all":
        scanned[:, 1:] = batch[7]
    assert not scanned.all() and torch.equal(res.n_tiles.cpu() >= 0, scanned)
    check_values(res, batch, f"small_b3 100x70 samples=7 maps={maps}")


def test_values_equal_the_float64_formulas_nine_players():
    """Exact maps wide enough that a player's 2^(n-1) coalitions are spread over all lanes of its wave: event maps cut to 9, 9 and 7
    occupied tiles at 100x70, 511 + 511 + 127 coalitions."""
    cfg, model, batch, _ = CG.light("small_b3")
    cut = cut_event_maps(batch, FINE, cfg.pixel_shape, {0: 9, 1: 9, 2: 7})
    res = shapley(model, cut, tile=FINE, max_exact=9, samples=1, maps="event")
    check_lists(res, cut, cfg.pixel_shape, "nine players", "event")
    assert res.num_variants == 511 + 511 + 127 and int(res.exact.sum()) == 3
    check_values(res, cut, "small_b3 100x70 event maps cut to 9, 9, 7 tiles, exact")


def test_values_of_a_single_permutation_have_no_standard_error():
    cfg, model, batch, _ = CG.light("small_b3")
    res = shapley(model, batch, tile=FINE, samples=1, seed=8, maps="event")
    phi, se, full, empty = res.values("event")
    scanned = res.n_tiles >= 0
    assert bool((se[scanned] == 0).all()) and bool((phi[scanned] != 0).any())


# ---- 5. exact against sampled, with no statistics ---------------------------------------------------------------------------------------------
def test_the_sampled_estimate_of_a_two_tile_map_is_the_mixture_of_the_exact_marginals():
    """Two players have two orders: with a share f of the permutations putting tile a first, phi_a = f (v{a} - v{}) + (1 - f)
    (v{a, b} - v{b}) and phi_b likewise, from the exact run's own coalitions."""
    cfg, model, batch = mixed()
    M = 8
    exact = shapley(model, batch, tile=COARSE, max_exact=2, samples=M, seed=6)
    sampled = shapley(model, batch, tile=COARSE, max_exact=1, samples=M, seed=6)
    assert bool(exact.exact[1, 0]) and not bool(sampled.exact[1, 0]) and int(sampled.n_tiles[1, 0]) == 2
    assert torch.equal(exact.permutations, sampled.permutations), "the permutations do not depend on the mode"
    a, b = SR.occupied(batch, COARSE, cfg.pixel_shape)[(1, 0)]
    order = sampled.permutations[1, 0, :, :2].cpu().tolist()
    assert all(sorted(o) == [a, b] for o in order)
    f = sum(o[0] == a for o in order) / M
    assert 0 < f < 1, "both orders must occur among the permutations"
    rows = (exact.index.cpu()[:, :2] == torch.tensor([1, 0])).all(1).nonzero().flatten().tolist()
    assert len(rows) == 3 and exact.index.cpu()[rows, 3].tolist() == [0, 1, 2]
    c = int(exact.event_logits[1].argmax())
    top = max(exact.event_logits.abs().max().item(), exact.coalition_event_logits.abs().max().item())
    for value, tol in (("prob", PROB_TOL), ("logit", 2.0 ** -22 * top)):
        def worth(row):
            row = row.cpu().double()
            return float(torch.softmax(row, 0)[c]) if value == "prob" else float(row[c])
        v0, va, vb = (worth(exact.coalition_event_logits[r]) for r in rows)
        vab = worth(exact.event_logits[1])
        want = {a: f * (va - v0) + (1 - f) * (vab - vb), b: f * (vab - va) + (1 - f) * (vb - v0)}
        phi_s, se_s = (t.cpu().double()[1, 0].flatten() for t in sampled.values("event", value)[:2])
        phi_e = exact.values("event", value)[0].cpu().double()[1, 0].flatten()
        err = max(abs(phi_s[t].item() - want[t]) for t in (a, b))
        half = max(abs(phi_e[t].item() - (0.5 * (w1 + w2))) for t, w1, w2 in ((a, va - v0, vab - vb), (b, vab - va, vb - v0)))
        print(f"two-tile map value={value}: f = {f}, sampled phi vs the mixture of the exact marginals {err:.2e}, exact phi vs the even "
              f"mixture {half:.2e} (gate {tol:.2e}); phi {want[a]:.3e} {want[b]:.3e}, stderr {se_s[a].item():.2e}")
        assert err <= tol and half <= tol
        assert se_s[a].item() > 0 and abs(se_s[a].item() - se_s[b].item()) <= tol, "two players: the marginals differ by the same amount"


# ---- 6. what the call leaves alone ------------------------------------------------------------------------------------------------------------
def test_state_gradients_step_counter_and_the_next_forward_survive_the_scan():
    from transformercvn.network.layers.packed_data import token_rows
    cfg, model, batch, _ = CG.light("tutorial_ragged")
    args = to_device(batch)[:8]
    rt = model.network.hip_runtime()
    ev, pr, weights = model.forward_with_attention(*args)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
    step = rt.step
    res = model.occlusion_shapley(*args, tile=COARSE, max_exact=4)
    assert rt.step == step + 1, "the scan counts as one forward(), as the other scans do"
    again = rt.head.attention(token_rows(args[7], args[7].shape[0]))
    assert torch.equal(again, weights), "the head's forward workspace was touched by the scan"
    assert torch.equal(res.event_logits, ev) and torch.equal(res.prong_logits, pr)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    for k, p in model.named_parameters():
        assert (p.grad is None) == (grads[k] is None) and (p.grad is None or torch.equal(p.grad, grads[k])), k
    res.values("event")
    res.values("prong", "logit")
    assert rt.step == step + 1
    with torch.no_grad():
        ev2, pr2 = model.forward(*args)
    assert torch.equal(ev2, ev) and torch.equal(pr2, pr)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            model.occlusion_shapley(*args, tile=COARSE)
    finally:
        model.eval()
