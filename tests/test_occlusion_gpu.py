"""Occlusion maps on the GPU: the variant list against host integer arithmetic, the scan against the brute force (the plain forward() of
the same model on event b alone with that tile's hits removed -- forward() is pinned to the reference goldens at 5e-5 by
test_full_model_gpu.py and is the yardstick here), three variants against the CPU oracle, the heat map against float64 softmax
differences, and what the scan must leave alone.  Every variant of a case is compared, none sampled; each test prints its maxima.

Gates (max-norm relative on logits; none is derived from what the scan gives):
  fp32 scan vs brute force   rel_err < 1e-4   the project's gate for stage-by-stage logits (test_submodules_gpu.py, test_explain_gpu.py)
  fp32 scan vs CPU oracle    rel_err < 5e-5   what test_full_model_gpu.py asserts for fp32 eval logits
  heat map                   |kernel - float64 formula on the result's own logits| <= 1e-6 (fp32 softmax of at most 8 classes)
  bf16 scan vs brute force   measured on forward() alone: M = the largest rel_err between forward(batch)[b] and forward(event b alone)
                             over the events of small_b3 and tutorial_ragged.  M == 0 (each map's arithmetic does not depend on its
                             neighbours in the launch): the fp32 gate.  Otherwise 2 M (the scan and the brute force may each sit one
                             batch composition away from the other), and not below 1e-4.  The test measures M again on every run.
                             Measured on an MI355X: M = 0.0 (event and prong logits, both cases), so the gate is 1e-4.
In bf16 eval the stem path is chosen per call (sparse stem while nnz <= 8192 * n_img); the fixtures stay far below that line (at most
3 493 hits per map), so no pass here falls on the other side of it from the base call."""
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case, rel_err
from model_utils import build_trainer, to_device
import occlusion_reference as R

pytestmark = pytest.mark.gpu

LOGIT_TOL, ORACLE_TOL, HEAT_TOL = 1e-4, 5e-5, 1e-6
_cache = {}


def golden_model(name, precision="fp32", **over_cfg):
    cfg, over, batch, g = load_case(name)
    if over_cfg:
        cfg = O.tutorial_config(**dict(over, **over_cfg))
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    model = build_trainer(cfg, sd, precision=precision)
    model.eval()
    return cfg, model, batch, sd


def shared_small_b3():
    """The full fp32 small_b3 model, built once: its brute-force results are shared between tests."""
    if "model small_b3" not in _cache:
        _cache["model small_b3"] = golden_model("small_b3")
    return _cache["model small_b3"]


def light(name):
    """The case's inputs behind a small DenseNet: for tests of what does not depend on the weights."""
    return golden_model(name, densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64,
                        num_encoder_layers=2)


def set_fused(model, on):
    from transformercvn.hip._lib import lib
    rt = model.network.hip_runtime()
    rt.ensure_bound()
    lib.tcvn_head_set_fused_encoder(rt.head.handle, int(on))


def scan(model, batch, **kw):
    res = model.occlusion_maps(*to_device(batch)[:8], **kw)
    for t in (res.event_logits, res.prong_logits, res.occluded_event_logits, res.occluded_prong_logits, res.index):
        assert not t.requires_grad and t.is_cuda
    V = res.index.shape[0]
    B, P = batch[7].shape
    assert res.index.dtype == torch.int32 and res.index.shape == (V, 4)
    assert res.occluded_event_logits.shape == (V, res.event_logits.shape[1])
    assert res.occluded_prong_logits.shape == (V, P, res.prong_logits.shape[2])
    return res


def check_scan(model, batch, cfg, what, tile, key=None, gate=LOGIT_TOL, whole_map=False, **kw):
    """Every variant of the scan against forward() on event b alone with the tile's hits removed."""
    res = scan(model, batch, tile=tile, **kw)
    index = res.index.cpu()
    assert torch.equal(index, R.expected_index(batch, tile, cfg.pixel_shape, kw.get("maps", "all"))), what + ": variant list"
    if key is None or key not in _cache:
        ref = R.brute_force(model, batch, index, tile, whole_map)
        if key is not None:
            _cache[key] = ref
    else:
        ref = _cache[key]
    ref_ev, ref_pr = ref
    e_ev = rel_err(res.occluded_event_logits.cpu(), ref_ev)
    e_pr = rel_err(R.valid_rows(res.occluded_prong_logits.cpu(), index, batch[7]), R.valid_rows(ref_pr, index, batch[7]))
    effect = (ref_ev - res.event_logits.cpu()[index[:, 0].long()]).abs().max().item() / res.event_logits.abs().max().item()
    print(f"{what}: {index.shape[0]} variants, rel err event logits {e_ev:.2e}, prong logits {e_pr:.2e} (gate {gate:.1e}); "
          f"largest effect of one tile {effect:.2e}")
    assert e_ev < gate and e_pr < gate, (what, e_ev, e_pr)
    # the comparison says something only if a scan that returned the unoccluded logits for every variant would fail it
    assert effect > gate, "the occlusions must move the logits by more than the gate"
    return res


# ---- 1. the variant list ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_b3", "tutorial_ragged"])
def test_variant_list_is_exact(name):
    cfg, model, batch, _ = light(name)
    shape = cfg.pixel_shape
    counted = {}
    for tile in [(100, 70), (64, 64), (16, 16)]:
        for maps in ("all", "event", "prongs"):
            res = scan(model, batch, tile=tile, maps=maps)
            want = R.expected_index(batch, tile, shape, maps)
            assert res.grid == R.grid_of(shape, tile) and res.tile == tile
            assert res.index.shape[0] == want.shape[0], (tile, maps, res.index.shape[0], want.shape[0])
            assert torch.equal(res.index.cpu(), want), (tile, maps)
            counted[(tile, maps)] = want.shape[0]
    print(name, "variants:", counted)
    # the figures counted from the fixtures on the host
    table = {"small_b3": {(100, 70): (48, 95), (64, 64): (105, 196)}, "tutorial_ragged": {(100, 70): (48, 349), (64, 64): (105, 734)}}
    for tile, (n_ev, n_pr) in table[name].items():
        assert (counted[(tile, "event")], counted[(tile, "prongs")], counted[(tile, "all")]) == (n_ev, n_pr, n_ev + n_pr)


def test_variant_list_of_a_shuffled_hit_list():
    """An unsorted list gives the same index, and (the order inside an image kept by a stable sort) the same logits."""
    cfg, model, batch, _ = light("small_b3")
    tile = (64, 64)
    res = scan(model, batch, tile=tile)
    g = torch.Generator().manual_seed(11)
    shuffled = list(batch)
    for c, v in ((2, 3), (5, 6)):
        perm = torch.randperm(batch[c].shape[0], generator=g)
        shuffled[c], shuffled[v] = batch[c][perm].contiguous(), batch[v][perm].contiguous()
    assert not bool((shuffled[5][1:, 0] >= shuffled[5][:-1, 0]).all())
    res2 = scan(model, tuple(shuffled), tile=tile)
    assert torch.equal(res2.index, res.index) and res2.grid == res.grid
    # the fixtures have unique coordinates per image, so the order of the hits does not change any image: same logits
    e = rel_err(res2.occluded_event_logits.cpu(), res.occluded_event_logits.cpu())
    print(f"shuffled hit list: {res.index.shape[0]} variants, rel err vs the sorted list {e:.2e}")
    assert e < LOGIT_TOL


# ---- 2. the scan equals the brute force -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_pass", [8, 256])
def test_scan_equals_brute_force_small_b3(max_pass):
    """64x64: 105 event-map variants (13 passes of 8 + 1 map) and 196 prong-map variants (24 passes of 8 + 4 maps)."""
    cfg, model, batch, _ = shared_small_b3()
    res = check_scan(model, batch, cfg, f"small_b3 64x64 max_maps_per_pass={max_pass}", (64, 64), key="bf small_b3 64",
                     max_maps_per_pass=max_pass)
    assert res.index.shape[0] == 105 + 196 and res.grid == (7, 5)


@pytest.mark.parametrize("fused", [1, 0])
def test_scan_equals_brute_force_tutorial_ragged(fused):
    """S = 17: the fused encoder path, and once the layer-by-layer kernels (the brute force then runs on them too)."""
    cfg, model, batch, _ = golden_model("tutorial_ragged")
    set_fused(model, fused)
    res = check_scan(model, batch, cfg, f"tutorial_ragged 100x70 fused={fused}", (100, 70))
    assert res.index.shape[0] == 48 + 349 and batch[7].shape[1] + 1 == 17


def test_scan_equals_brute_force_norm_first():
    cfg, model, batch, _ = golden_model("small_b3", transformer_norm_first=True)
    check_scan(model, batch, cfg, "small_b3 100x70 transformer_norm_first", (100, 70))


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


def test_scan_equals_brute_force_bf16():
    """The gate is measured on forward() alone first (see the module docstring): measured M = 0.0 on an MI355X -> gate 1e-4."""
    cases = {name: golden_model(name, "bf16") for name in ("small_b3", "tutorial_ragged")}
    M = max(batch_composition_spread(model, batch) for cfg, model, batch, _ in cases.values())
    gate = LOGIT_TOL if M == 0 else max(2 * M, LOGIT_TOL)
    print(f"bf16: batch-composition spread of forward() M = {M:.3e} -> gate {gate:.3e}")
    for name, (cfg, model, batch, _) in cases.items():
        check_scan(model, batch, cfg, f"{name} 100x70 bf16", (100, 70), gate=gate)


# ---- 3. anchor outside the project's kernels ---------------------------------------------------------------------------------------------
def test_three_variants_against_the_cpu_oracle():
    cfg, model, batch, sd = shared_small_b3()
    tile = (100, 70)
    res = scan(model, batch, tile=tile)
    index = res.index.cpu().tolist()
    counts = batch[7].sum(1).tolist()
    P = batch[7].shape[1]
    padded = [b for b, n in enumerate(counts) if n < P][0]
    full = [b for b, n in enumerate(counts) if n == P][0]
    picks = [next(v for v, r in enumerate(index) if r[1] == 0 and r[0] == full),
             next(v for v, r in enumerate(index) if r[1] >= 1 and r[0] == padded),
             [v for v, r in enumerate(index) if r[1] >= 1 and r[0] == full][-1]]
    for v in picks:
        b, s, ty, tx = index[v]
        ev, pr, _ = O.forward(sd, cfg, R.filtered_batch(batch, b, (s, ty, tx), tile), training=False)
        m = batch[7][b]
        e_ev, e_pr = rel_err(res.occluded_event_logits[v].cpu(), ev[b]), rel_err(res.occluded_prong_logits[v].cpu()[m], pr[b][m])
        print(f"variant {index[v]} vs the CPU oracle: event logits {e_ev:.2e}, prong logits {e_pr:.2e}")
        assert e_ev < ORACLE_TOL and e_pr < ORACLE_TOL, (index[v], e_ev, e_pr)


# ---- 4. base rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_base_rows_are_forwards(precision):
    cfg, model, batch, _ = golden_model("tutorial_b2p4", precision)
    with torch.no_grad():
        ev, pr = model.forward(*to_device(batch)[:8])
    res = scan(model, batch, tile=(100, 70))
    assert torch.equal(res.event_logits, ev) and torch.equal(res.prong_logits, pr)
    assert res.index.shape[0] == 32 + 128


# ---- 5. heat map -------------------------------------------------------------------------------------------------------------------------
def test_heat_map():
    from transformercvn.hip import occlusion
    cfg, model, batch, _ = light("small_b3")
    tile = (100, 70)
    res = scan(model, batch, tile=tile)
    B, P = batch[7].shape
    occupied = torch.zeros(B, 1 + P, *res.grid, dtype=torch.bool)
    i = res.index.cpu().long()
    occupied[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = True
    assert int((~occupied[:, 1:][batch[7]]).sum()) == 1, "the fixture has one empty tile among its 96 prong-map tiles"
    classes = torch.tensor([(int(res.event_logits[b].argmax()) + 1 + b) % res.event_logits.shape[1] for b in range(B)])
    for target in ("event", "prong", 1, classes, classes.cuda()):
        heat = occlusion.heatmap(res, target)
        assert heat.shape == (B, 1 + P, *res.grid) and heat.dtype == torch.float32 and heat.is_cuda
        ref = R.heat_reference(res, target.cpu() if torch.is_tensor(target) else target)
        err = (heat.cpu().double() - ref).abs().max().item()
        print(f"heat map target={target if not torch.is_tensor(target) else 'tensor'}: max |kernel - float64| {err:.2e}, "
              f"largest entry {ref.abs().max().item():.2e}")
        assert err <= HEAT_TOL
        h = heat.cpu()
        assert (h[~occupied] == 0).all(), "tiles without hits and padded slots must be exactly 0"
        assert (h[:, 1:][~batch[7]] == 0).all()
        if isinstance(target, str) and target == "prong":
            assert (h[:, 0] == 0).all()
        assert ref.abs().max().item() > HEAT_TOL          # a map of zeros would fail the gate
    assert torch.equal(res.heatmap(), occlusion.heatmap(res, "event"))


# ---- 6. a tile as large as the map -----------------------------------------------------------------------------------------------------
def test_tile_larger_than_the_map():
    """One variant per non-empty map; its map goes to the embedder as an image without hits (the token stays in the sequence)."""
    cfg, model, batch, _ = shared_small_b3()
    res = check_scan(model, batch, cfg, "small_b3 tile 400x280", (400, 280), whole_map=True)
    B = batch[7].shape[0]
    assert res.grid == (1, 1) and res.index.shape[0] == B + int(batch[7].sum())
    ev_only = check_scan(model, batch, cfg, "small_b3 tile 400x280 event maps", (400, 280), whole_map=True, maps="event")
    assert ev_only.index.shape[0] == B          # a pass whose hit list is empty altogether when max_maps_per_pass = 1
    one = scan(model, batch, tile=(400, 280), maps="event", max_maps_per_pass=1)
    assert torch.equal(one.index, ev_only.index)
    assert rel_err(one.occluded_event_logits.cpu(), ev_only.occluded_event_logits.cpu()) < LOGIT_TOL


# ---- 7. the scan leaves the rest alone ----------------------------------------------------------------------------------------------------
def test_attention_of_the_explained_forward_survives_the_scan():
    from transformercvn.network.layers.packed_data import token_rows
    cfg, model, batch, _ = light("tutorial_ragged")
    args = to_device(batch)[:8]
    ev, pr, weights = model.forward_with_attention(*args)
    res = model.occlusion_maps(*args, tile=(100, 70))
    rt = model.network.hip_runtime()
    again = rt.head.attention(token_rows(args[7], args[7].shape[0]))
    assert torch.equal(again, weights), "the head's forward workspace was touched by the scan"
    assert torch.equal(res.event_logits, ev) and torch.equal(res.prong_logits, pr)


def test_two_scans_return_identical_tensors():
    cfg, model, batch, _ = light("small_b3")
    a, b = scan(model, batch, tile=(64, 64)), scan(model, batch, tile=(64, 64))
    for k in ("event_logits", "prong_logits", "index", "occluded_event_logits", "occluded_prong_logits"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_a_scan_counts_as_one_forward_for_the_training_step_that_follows():
    """Two identically seeded bf16 models (dropout 0.1, pixel noise on): eval forward() in one, occlusion_maps() in the other, then the
    same training step in both: the same seeds are drawn, so the losses and the dense layers' convolution weight gradients (the set
    test_determinism_gpu.py shows to be bit-reproducible) are equal bit for bit."""
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
                model.occlusion_maps(*dev_batch[:8], tile=(100, 70))
        assert rt.step == 1
        model.train()
        rt.zero_grad()
        loss = model.training_step(dev_batch, 0)
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if ".dense" in k and k.endswith(("conv1.weight", "conv2.weight"))}
        out[tag] = (loss.detach().clone(), grads)
    assert torch.equal(out["forward"][0], out["scan"][0]), (out["forward"][0].item(), out["scan"][0].item())
    assert len(out["forward"][1]) == 2 * 2 * sum(cfg.densenet_structure)
    diff = [k for k, v in out["forward"][1].items() if not torch.equal(v, out["scan"][1][k])]
    print(f"training step after forward() vs after occlusion_maps(): loss {out['scan'][0].item():.6f}, "
          f"{len(diff)} of {len(out['forward'][1])} dense-layer weight gradients differ")
    assert not diff, diff[:3]


def test_scan_changes_no_state():
    cfg, model, batch, _ = light("small_b3")
    args = to_device(batch)[:8]
    with torch.no_grad():
        model.forward(*args)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.occlusion_maps(*args, tile=(100, 70))
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    model.train()
    with pytest.raises(RuntimeError):
        model.occlusion_maps(*args)


# ---- 8. the SDXL embedder ---------------------------------------------------------------------------------------------------------------
def test_scan_equals_brute_force_sdxl():
    cfg = O.tutorial_config(embedder="sdxl", initial_pixel_dim=8, pixel_embedding_dim=64, hidden_dim=64, num_encoder_layers=2,
                            num_prong_decoder_layers=3, dropout=0.0, pixel_noise_std=0.0)          # test_sdxl_gpu.py's small model
    sd = O.fill_state(cfg, 7)
    batch = O.synthetic_batch([2, 3, 1], 9, cfg)
    model = build_trainer(cfg, sd)
    assert type(model).__name__ == "NeutrinoFullSDXLTrainer"
    model.eval()
    res = check_scan(model, batch, cfg, "sdxl small model 200x140", (200, 140))
    assert res.grid == (2, 2)
