"""Monte-Carlo dropout through the whole model (model.mc_dropout: eval statistics, dropout drawn) on the GPU.

  1. every sample is the oracle's eval-statistics forward under the kernels' own masks (fp32, the 1e-3 mask-replay gate);
  2. the masks are really drawn in eval arithmetic: the zeros of a 3x3 output slice are tcvn_dropout_keep's, in fp32 and bf16;
  3. nothing is left behind: state dict, step counter, the head's forward workspace, the training step that follows;
  4. same seed, same bits; another seed, other samples; reuse_stem changes no bit; resume is refused where it would be wrong;
  5. dropout = 0, one sample, padded prong slots;
  6. the statistics kernel against the float64 reference, on the result's own logits and fed directly;
  7. bf16 embedders against fp32 ones under the same masks.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case, rel_err
from head_utils import keep
from mc_dropout_reference import oracle_sample, stats
from model_utils import build_trainer, to_device
from test_dropout_noise_gpu import _provider, _replay_case

pytestmark = pytest.mark.gpu

T = 3
MLP_SITE = "network.prong_embedding.feature_embedding.embedding."
STAT_KEYS = ("mean_prob", "std_prob", "entropy", "expected_entropy", "mutual_info", "votes")


def trimmed(batch):
    """The eight network inputs cut to the widest event, as shared_step hands them on."""
    mp = int(batch[7].sum(1).max())
    b = list(batch[:8])
    b[0], b[7] = b[0][:, :mp].contiguous(), b[7][:, :mp].contiguous()
    return tuple(b)


def provider(cfg, seeds_row, B, P):
    """test_dropout_noise_gpu._provider with the seeds of one sample (McDropout.seeds[t] = event, prong, head, mlp), plus the
    smart-feature MLP's sites (stream ids 0x4800 + i)."""
    ev, pr, head, mlp = (int(v) for v in seeds_row)
    base = _provider(cfg, SimpleNamespace(last_seeds={"event": ev, "prong": pr, "head": head}), B, P)

    def fn(site, shape):
        if site.startswith(MLP_SITE):
            return keep(0, cfg.dropout, mlp, 0x4800 + int(site[len(MLP_SITE):]), shape[0], shape[1]).cpu()
        return base(site, shape)
    return fn


def same(a, b):
    """torch.equal that lets NaN equal NaN (padded prong slots)."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def same_result(a, b):
    return (torch.equal(a.sample_event_logits, b.sample_event_logits) and torch.equal(a.sample_prong_logits, b.sample_prong_logits) and
            torch.equal(a.seeds, b.seeds) and all(same(getattr(a.event, k), getattr(b.event, k)) for k in STAT_KEYS) and
            all(same(getattr(a.prong, k), getattr(b.prong, k)) for k in STAT_KEYS))


def golden_model(name, precision="fp32", **over_more):
    cfg, over, batch, g = load_case(name)
    if over_more:
        cfg = O.tutorial_config(**dict(over, **over_more))
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    model = build_trainer(cfg, sd, precision=precision)
    model.eval()
    return cfg, sd, batch, model


# ---- 1. every sample is the oracle's eval-statistics forward under the kernels' own masks ---------------------------------------------
@pytest.mark.parametrize("which", ["small_b3", "hidden128_p8", "norm_first", "small_b3_smart"])
def test_every_sample_is_the_oracle_eval_statistics_forward_under_the_kernels_masks(which):
    if which == "small_b3_smart":                               # the smart-feature MLP's dropout sites (0x4800 + i) under seeds[t, 3]
        _, over, batch, gold = load_case("small_b3")
        cfg, wseed = O.tutorial_config(**dict(over, disable_smart_features=False)), int(gold["weight_seed"])
        g = torch.Generator().manual_seed(5)
        batch = (torch.randn(batch[0].shape, generator=g), torch.randn(batch[1].shape, generator=g)) + tuple(batch[2:])
    else:
        cfg, batch, wseed = _replay_case(which)
    assert cfg.dropout == 0.1 and cfg.pixel_noise_std > 0
    sd = O.fill_state(cfg, wseed)
    model = build_trainer(cfg, sd)
    model.eval()
    b8 = trimmed(batch)
    res = model.mc_dropout(*to_device(b8), samples=T, seed=11)
    torch.cuda.synchronize()
    B, P = b8[7].shape
    assert res.sample_event_logits.shape[:2] == (T, B) and res.sample_prong_logits.shape[:3] == (T, B, P) and res.seeds.shape == (T, 4)
    ev0, pr0, _ = O.forward(sd, cfg, b8, training=False)
    assert rel_err(res.event_logits.cpu(), ev0) < 1e-3 and rel_err(res.prong_logits.cpu(), pr0) < 1e-3
    worst = 0.0
    for t in range(T):
        sites = []
        fn = provider(cfg, res.seeds[t].tolist(), B, P)
        ev, pr, _ = oracle_sample(sd, cfg, b8, lambda site, shape: (sites.append(site), fn(site, shape))[1])
        e1, e2 = rel_err(res.sample_event_logits[t].cpu(), ev), rel_err(res.sample_prong_logits[t].cpu(), pr)
        worst = max(worst, e1, e2)
        print(f"mc_dropout {which} sample {t}: logits vs oracle replay event {e1:.2e} prong {e2:.2e}")
        assert e1 < 1e-3 and e2 < 1e-3
        assert rel_err(ev, ev0) > 1e-3, "the masks moved the logits by less than the gate: the eval forward would pass too"
        assert any(s.startswith(MLP_SITE) for s in sites) == (which == "small_b3_smart")
    print(f"mc_dropout {which}: worst sample logit error vs oracle replay {worst:.2e}")


# ---- 2. the masks are really drawn, in eval arithmetic ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_masks_are_drawn_in_eval_arithmetic(precision):
    cfg, sd, batch, model = golden_model("tutorial_b2p4", precision)
    rt = model.network.hip_runtime()
    dbatch = to_device(batch)
    p, gr, c0 = cfg.dropout, cfg.densenet_growth_rate, cfg.initial_pixel_dim
    masks = []
    for n_samples in (1, 2):                                    # the workspaces hold the last sample: t = 0, then t = 1
        res = model.mc_dropout(*dbatch[:8], samples=n_samples, seed=5)
        torch.cuda.synchronize()
        t = n_samples - 1
        for col, eng in ((0, rt.ev_engine), (1, rt.pr_engine)):
            D = eng.tap("dense1")
            n, H, W, _ = D.shape
            sl = D[..., c0:c0 + gr].float().reshape(n * H * W, gr)
            m = keep(1, p, int(res.seeds[t, col]), 1, n * H * W, gr)
            assert torch.equal(sl != 0, m != 0), (precision, t, col)      # an un-dropped conv output is never exactly 0
            rate = (m != 0).float().mean().item()
            assert abs(rate - (1 - p)) < 4 * (p * (1 - p) / m.numel()) ** 0.5
            masks.append(m != 0)
    assert not torch.equal(masks[0], masks[2]) and not torch.equal(masks[1], masks[3])      # sample 0 against sample 1
    for m in rt.network.modules():                              # eval arithmetic: no module was switched to training
        assert not m.training


# ---- 3. nothing is left behind ------------------------------------------------------------------------------------------------------------
def test_state_step_counter_attention_and_the_training_step_that_follows():
    """Two identically seeded bf16 models: eval forward() in one, mc_dropout() in the other.  State dict untouched, one step counted, the
    head's forward workspace as forward() left it, and the same training step afterwards gives the same loss bit for bit."""
    from transformercvn.network.layers.packed_data import token_rows
    cfg, over, batch, g = load_case("tutorial_b2p4")
    assert cfg.dropout > 0
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    dbatch = to_device(batch)
    tok = token_rows(dbatch[7], dbatch[7].shape[0])
    out = {}
    for tag in ("forward", "mc"):
        model = build_trainer(cfg, sd, precision="bf16")
        model.eval()
        rt = model.network.hip_runtime()
        with torch.no_grad():
            if tag == "forward":
                ev, pr = model(*dbatch[:8])
            else:
                rt.ensure_bound()
                before = {k: v.clone() for k, v in model.state_dict().items()}
                res = model.mc_dropout(*dbatch[:8], samples=T, seed=2)
                ev, pr = res.event_logits, res.prong_logits
                for k, v in model.state_dict().items():
                    assert torch.equal(v, before[k]), k          # running statistics and num_batches_tracked included
        assert rt.step == 1
        weights = rt.head.attention(tok)
        model.train()
        rt.zero_grad()
        loss = model.training_step(dbatch, 0)
        loss.backward()
        torch.cuda.synchronize()
        out[tag] = (ev.clone(), pr.clone(), weights, loss.detach().clone())
    for a, b in zip(out["forward"], out["mc"]):
        assert torch.equal(a, b)
    print(f"training step after forward() {out['forward'][3].item():.6f}, after mc_dropout() {out['mc'][3].item():.6f}")


# ---- 4. determinism, reuse of the stem, refused resumes -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("small_b3", "fp32"), ("tutorial_b2p4", "bf16")])
def test_same_seed_same_bits_and_reuse_stem_changes_nothing(name, precision):
    cfg, sd, batch, model = golden_model(name, precision)
    dbatch = to_device(batch)
    a = model.mc_dropout(*dbatch[:8], samples=T, seed=3)
    b = model.mc_dropout(*dbatch[:8], samples=T, seed=3)
    c = model.mc_dropout(*dbatch[:8], samples=T, seed=4)
    d = model.mc_dropout(*dbatch[:8], samples=T, seed=3, reuse_stem=False)
    torch.cuda.synchronize()
    assert same_result(a, b)
    assert not torch.equal(a.sample_event_logits, c.sample_event_logits) and not torch.equal(a.seeds, c.seeds)
    assert not torch.equal(a.sample_prong_logits, c.sample_prong_logits)
    assert same_result(a, d), "reuse_stem must not change a bit"
    assert torch.equal(a.event_logits, c.event_logits) and torch.equal(a.prong_logits, d.prong_logits)
    assert not torch.equal(a.sample_event_logits[0], a.sample_event_logits[1])
    expect = [[s ^ k for k in (0x1111, 0x2222, 0x3333, 0x4444)] for s in ((3 * 1000003 + t) & 0x7FFFFFFFFFFFFFFF for t in range(T))]
    assert a.seeds.dtype == torch.int64 and a.seeds.tolist() == expect


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resume_is_refused_after_other_inputs_or_a_train_mode_forward(precision):
    cfg, sd, batch, model = golden_model("small_b3", precision)
    rt = model.network.hip_runtime()
    rt.ensure_bound()
    eng = rt.pr_engine
    n_img = int(batch[7].sum())
    coords, values = batch[5].cuda(), batch[6].cuda()
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(coords, values, n_img, out, train=True, seed=1)                 # (first: the workspace it sizes serves every later call)
    with pytest.raises(RuntimeError, match="densenet_forward_mc"):
        eng.forward_mc(coords, values, n_img, out, seed=9, resume=True)         # after a train-mode forward
    eng.forward(coords, values, n_img, out, train=False)
    whole = torch.empty_like(out)
    eng.forward_mc(coords, values, n_img, whole, seed=9, resume=False)
    eng.forward_mc(coords, values, n_img, out, seed=9, resume=True)             # after an eval-kind forward of these inputs: fine
    torch.cuda.synchronize()
    assert torch.equal(out, whole)
    other = coords.clone()
    with pytest.raises(RuntimeError, match="densenet_forward_mc"):
        eng.forward_mc(other, values, n_img, out, seed=9, resume=True)          # another hit list
    with pytest.raises(RuntimeError, match="densenet_forward_mc"):
        eng.forward_mc(coords, values, n_img - 1, out[:n_img - 1], seed=9, resume=True)
    eng.forward_mc(other, values, n_img, out, seed=9, resume=False)
    with pytest.raises(RuntimeError, match="densenet_forward_mc"):
        eng.forward_mc(coords, values, n_img, out, seed=9, resume=True)         # the workspace now holds `other`'s forward
    torch.cuda.synchronize()


# ---- 5. degenerate cases ----------------------------------------------------------------------------------------------------------------------
def test_without_dropout_every_sample_is_the_prediction():
    cfg, sd, batch, model = golden_model("small_b3", dropout=0.0)
    assert cfg.dropout == 0.0
    dbatch = to_device(trimmed(batch))
    res = model.mc_dropout(*dbatch, samples=T, seed=1)
    torch.cuda.synchronize()
    for t in range(T):
        assert torch.equal(res.sample_event_logits[t], res.event_logits) and torch.equal(res.sample_prong_logits[t], res.prong_logits)
    mask = dbatch[7]
    assert bool((res.event.std_prob == 0).all()) and bool((res.prong.std_prob[mask] == 0).all())
    assert res.event.mutual_info.max().item() <= 1e-12 and res.prong.mutual_info[mask].max().item() <= 1e-12
    assert bool((res.event.votes.sum(1) == 1).all())


def test_one_sample_has_no_spread():
    cfg, sd, batch, model = golden_model("small_b3")
    dbatch = to_device(trimmed(batch))
    res = model.mc_dropout(*dbatch, samples=1, seed=1)
    torch.cuda.synchronize()
    assert res.samples == 1
    assert bool((res.event.std_prob == 0).all()) and bool((res.prong.std_prob[dbatch[7]] == 0).all())
    assert not torch.equal(res.sample_event_logits[0], res.event_logits)


def test_padded_prong_slots_are_nan_and_only_they():
    cfg, sd, batch, model = golden_model("tutorial_ragged", "bf16")
    mask = batch[7]
    assert sorted(mask.sum(1).tolist()) == [1, 5, 16]
    res = model.mc_dropout(*to_device(batch)[:8], samples=T, seed=6)
    torch.cuda.synchronize()
    B, P = mask.shape
    for k in STAT_KEYS:
        ev, pr = getattr(res.event, k).cpu(), getattr(res.prong, k).cpu()
        assert ev.shape[0] == B and pr.shape[:2] == (B, P)
        assert bool(torch.isfinite(ev).all()), k
        nan = torch.isnan(pr).reshape(B, P, -1)
        assert torch.equal(nan.all(2), ~mask) and torch.equal(nan.any(2), ~mask), k
    assert torch.isfinite(torch.nanmean(res.prong.mutual_info)).item()
    assert res.prong.mutual_info[mask.cuda()].min().item() >= 0


# ---- 6. the statistics kernel -----------------------------------------------------------------------------------------------------------------
def _close(got, ref, what):
    """Every output within 1e-6 of the float64 reference, NaN exactly where it is NaN -> the worst difference."""
    worst = 0.0
    for k in STAT_KEYS:
        a, b = got[k].double().cpu().numpy(), ref[k]
        assert a.shape == b.shape, (what, k)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, k)
        err = float(np.nanmax(np.abs(a - b))) if np.isfinite(b).any() else 0.0
        assert err <= 1e-6, (what, k, err)
        worst = max(worst, err)
    return worst


def test_statistics_of_a_result_match_float64_on_its_own_logits():
    cfg, sd, batch, model = golden_model("small_b3")
    b8 = trimmed(batch)
    res = model.mc_dropout(*to_device(b8), samples=T, seed=8)
    torch.cuda.synchronize()
    B, P = b8[7].shape
    ref = stats(res.sample_event_logits.cpu().numpy())
    e_ev = _close({k: getattr(res.event, k) for k in STAT_KEYS}, ref, "event")
    valid = np.where(b8[7].numpy().reshape(-1), 0, -1)
    ref = stats(res.sample_prong_logits.cpu().numpy().reshape(T, B * P, -1), valid)
    ref = {k: v.reshape(B, P, *v.shape[1:]) for k, v in ref.items()}
    e_pr = _close({k: getattr(res.prong, k) for k in STAT_KEYS}, ref, "prong")
    print(f"mc_dropout statistics vs float64 on own logits: event {e_ev:.2e} prong {e_pr:.2e}")
    assert res.event.std_prob.max().item() > 0 and res.event.mutual_info.max().item() > 0


@pytest.mark.parametrize("n_samples", [1, 2, 63, 64, 65, 200])
def test_statistics_kernel_fed_directly(n_samples):
    from transformercvn.hip.engine import mc_stats
    rng = np.random.default_rng(100 + n_samples)
    R = 7                                                       # two workgroups of four rows, the second one ragged
    worst = 0.0
    for Cn in (1, 4, 8, 9, 17):
        x = (rng.normal(size=(n_samples, R, Cn)) * rng.choice([0.1, 1.0, 8.0], size=(1, R, 1))).astype(np.float32)
        valid = np.array([0, 3, -1, 5, -1, 1, 2], dtype=np.int32)
        got = mc_stats(torch.from_numpy(x).cuda(), torch.from_numpy(valid).cuda())
        worst = max(worst, _close(got, stats(x, valid), (n_samples, Cn)))
        got = mc_stats(torch.from_numpy(x).cuda())                              # valid = NULL: every row counts
        worst = max(worst, _close(got, stats(x), (n_samples, Cn, "all rows")))
        assert got["mutual_info"].min().item() >= 0
    print(f"tcvn_mc_dropout_stats T = {n_samples}: worst output error vs float64 {worst:.2e}")


def test_statistics_kernel_ties_vote_for_the_lowest_class():
    from transformercvn.hip.engine import mc_stats
    x = torch.zeros(5, 3, 9)
    x[:, 0, 2] = x[:, 0, 6] = 1.5                               # classes 2 and 6 tie: 2 wins every sample
    x[:, 1, :] = -0.75                                          # all nine tie: class 0
    x[:3, 2, 8] = 2.0                                           # class 8 in three of five samples; the two all-zero samples vote 0
    got = mc_stats(x.cuda())
    votes = got["votes"].cpu()
    assert votes[0].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert votes[1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert votes[2, 8].item() == pytest.approx(0.6) and votes[2, 0].item() == pytest.approx(0.4)
    assert _close(got, stats(x.numpy()), "ties") <= 1e-6


def test_statistics_kernel_argument_errors():
    from transformercvn.hip._lib import lib
    dev = "cuda"
    x = torch.zeros(2, 3, 4, device=dev)
    o2 = [torch.empty(3, 4, device=dev) for _ in range(3)]      # mean, std, votes
    o1 = [torch.empty(3, device=dev) for _ in range(3)]         # entropy, expected entropy, mutual information
    p = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(logits=x, n=2, rows=3, classes=4, null=None):
        outs = [o2[0], o2[1], o1[0], o1[1], o1[2], o2[2]]
        if null is not None:
            outs[null] = None
        return lib.tcvn_mc_dropout_stats(p(logits), p(None), n, rows, classes, *(p(t) for t in outs), st)
    assert call() == 0
    assert call(logits=None) != 0
    for i in range(6):
        assert call(null=i) != 0, i
    assert call(n=0) != 0 and call(n=-1) != 0
    assert call(classes=0) != 0 and call(classes=257) != 0
    big = torch.zeros(1, 1, 256, device=dev)
    outs = [torch.empty(1, 256, device=dev), torch.empty(1, 256, device=dev), torch.empty(1, device=dev), torch.empty(1, device=dev),
            torch.empty(1, device=dev), torch.empty(1, 256, device=dev)]
    assert lib.tcvn_mc_dropout_stats(p(big), p(None), 1, 1, 256, *(p(t) for t in outs), st) == 0       # the widest row is accepted
    torch.cuda.synchronize()
    assert outs[2].item() == pytest.approx(np.log(256), abs=1e-6)


# ---- 7. bf16 embedders under the same masks ---------------------------------------------------------------------------------------------------
def test_bf16_samples_stay_as_close_to_fp32_as_the_plain_prediction_does():
    """tutorial_b2p4 (fused encoder).  The masks are identical by construction (test 2), so a bf16 sample differs from the fp32 sample of
    the same seeds by bf16 rounding alone.  The yardstick is the same distance for the plain eval logits -- the quantity
    test_full_model_gpu.py bands with autocast_bf16_band.npz --, the gate twice that: dropout scales single-rounded bf16 values by
    1/(1-p) and zeroes others, which moves roundings about but adds none."""
    cfg, over, batch, g = load_case("tutorial_b2p4")
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    dbatch = to_device(batch)
    res = {}
    for precision in ("fp32", "bf16"):
        model = build_trainer(cfg, sd, precision=precision)
        model.eval()
        res[precision] = model.mc_dropout(*dbatch[:8], samples=T, seed=21)
        torch.cuda.synchronize()
    f, b = res["fp32"], res["bf16"]
    assert torch.equal(f.seeds, b.seeds)
    plain = max(rel_err(b.event_logits.cpu(), f.event_logits.cpu()), rel_err(b.prong_logits.cpu(), f.prong_logits.cpu()))
    sampled = max(max(rel_err(b.sample_event_logits[t].cpu(), f.sample_event_logits[t].cpu()),
                      rel_err(b.sample_prong_logits[t].cpu(), f.sample_prong_logits[t].cpu())) for t in range(T))
    print(f"mc_dropout bf16 vs fp32, same seeds: plain eval logits {plain:.3e}, worst of {T} samples {sampled:.3e}")
    assert plain > 0
    assert sampled <= 2 * plain
