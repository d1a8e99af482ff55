"""Noise-averaged hit gradients (model.smooth_hit_gradients) on the GPU.

  1. the four kernels alone through their C entries against the float64 restatement (tests/smooth_gradients_reference.py);
  2. fp32 mode, case A: the perturbed values, every per-sample gradient against the float64 oracle at those very values, the reported
     statistics against the float64 statistics of the device's own samples, the three kinds, the heat map;
  3. samples batched into one frozen pass against one pass per sample;
  4. noise = 0 is hit_gradients(method="gradient");
  5. bf16 mode against the oracle under torch.autocast;
  6. target "prong" (case B) and raw seeds with a padded slot;
  7. nothing else moves.
"""
import numpy as np
import pytest
import torch

from oracle import tcvn_oracle as O
import hit_gradients_reference as R
import smooth_gradients_reference as S
from model_utils import build_trainer, to_device

pytestmark = pytest.mark.gpu

GATE_F32 = 1e-3          # the project's fp32 gate, applied to the relative L2 error
# Case A, per-sample gradients at the perturbed values.  The plain gradient of the same case measures 9.6e-7 (event) / 1.1e-6 (prong)
# against float64 (tests/test_hit_gradients_gpu.py).  Measured here over the four samples: event 9.7e-7 .. 1.14e-6 (worst map 1.58e-6),
# prong 9.1e-7 .. 1.17e-6 (worst map 1.39e-6) -- within 10x of the plain figures, so the gate is tightened to 10x the measured worst, as 5h
# did -- with ONE exception: in sample 0 the float64 oracle finds a PReLU input of prong image 1 at 1.4e-8 of its layer's largest, which
# fp32 cannot tell from zero (kink_maps); the library lands on the other side of that kink, torch's own float32 pass happens not to, and
# that map's gradient moves by the unit's whole contribution: 1.92e-3 in the map, 7.6e-4 in the prong tensor.  hit_gradients on the same
# values gives the same bits, so this is the frozen pass of 5h at an input near a kink, not the batching.  A tensor or map that such a
# kink touches is therefore held to the project's gate on the whole tensor (what the feature's specification sets), every other one to
# the tightened gate.
GATE_SAMPLE = dict(event=1.6e-5, prong=1.4e-5)
SAMPLES, NOISE, SEED = 4, 0.1, 5
CLASSES_A = torch.tensor([1, 2])


def case_a(**over):
    cfg = O.tutorial_config(**dict(dict(pixel_shape=(104, 72), densenet_structure=[3, 3, 2], num_encoder_layers=2, dropout=0.0,
                                        pixel_noise_std=0.0), **over))
    batch = O.synthetic_batch([1, 3], seed=7, cfg=cfg, event_hits=(150, 300), prong_hits=(10, 80))
    return cfg, O.fill_state(cfg, seed=3), batch


def case_b():
    cfg = O.tutorial_config(pixel_shape=(40, 280), densenet_structure=[3, 2], num_encoder_layers=2, dropout=0.0, pixel_noise_std=0.0)
    batch = O.synthetic_batch([2, 2], seed=11, cfg=cfg, event_hits=(150, 300), prong_hits=(10, 80))
    return cfg, O.fill_state(cfg, seed=5), batch


def trainer_of(cfg, sd, precision="fp32"):
    model = build_trainer(cfg, sd, precision=precision)
    model.training_dataset.pixel_shape = model.network.pixel_shape = tuple(cfg.pixel_shape)
    return model


def model_of(cfg, sd, precision="fp32"):
    model = trainer_of(cfg, sd, precision)
    model.eval()
    return model


def tables(prong_mask):
    """img_bs of the event list and of the prong list of a batch."""
    B = prong_mask.shape[0]
    b, p = prong_mask.nonzero(as_tuple=True)
    return (np.stack((np.arange(B), np.zeros(B, dtype=np.int64)), 1).astype(np.int32), np.stack((b.numpy(), p.numpy() + 1), 1).astype(np.int32))


def reference_samples(cfg, batch, noise, seed, t0, reps):
    """sigma [B, 1 + P] and the perturbed values ([reps, nnzE, C], [reps, nnzP, C]) of a batch by the restatement."""
    mask = batch[7]
    B, P = mask.shape
    ev_bs, pr_bs = tables(mask)
    shape = tuple(cfg.pixel_shape)
    sig = S.sigma(batch[2].numpy(), batch[3].numpy(), B, shape, ev_bs, B, P, noise)
    sig = S.sigma(batch[5].numpy(), batch[6].numpy(), len(pr_bs), shape, pr_bs, B, P, noise, sig)
    ev = S.replicate(batch[2].numpy(), batch[3].numpy(), B, shape, ev_bs, P, sig, seed, t0, reps)[1]
    pr = S.replicate(batch[5].numpy(), batch[6].numpy(), len(pr_bs), shape, pr_bs, P, sig, seed, t0, reps)[1]
    return sig, ev.reshape(reps, *batch[3].shape), pr.reshape(reps, *batch[6].shape)


def one_ulp(got, ref):
    """got (device fp32) within one fp32 unit in the last place of the restatement's value."""
    got, ref = got.cpu().numpy().astype(np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) <= S.ulp32(ref)


_oracle = {}


def oracle_a_at(t, ev_values, pr_values, autocast=False):
    """float64 (or autocast) gradients of case A, classes CLASSES_A, at the hit values of sample t: computed once per sample and left
    unchanged (the values of a sample are the same in every test: same seed, same noise; checked)."""
    key = (t, autocast)
    ev_values, pr_values = ev_values.cpu(), pr_values.cpu()
    if key not in _oracle or not (torch.equal(_oracle[key][0], ev_values) and torch.equal(_oracle[key][1], pr_values)):
        cfg, sd, batch = case_a()
        g = R.oracle_hit_gradients(sd, cfg, batch[:8], CLASSES_A, "prob", torch.float32 if autocast else torch.float64,
                                   values=(ev_values, pr_values), autocast=autocast)
        _oracle[key] = (ev_values, pr_values, g[0], g[1])
    return _oracle[key][2:]


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------------
def hand_list(C):
    """3 maps of 20 x 12, B = 2, P = 2: image 0 = (0, 0) varied (corners, a full row, one pixel twice, one three times, a few negative
    values), image 1 = (0, 2) without hits, image 2 = (1, 1) all values 7.5; one entry outside the maps at the end of image 0."""
    H, W = 20, 12
    rng = np.random.default_rng(40 + C)
    px = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [(7, x) for x in range(W)] + [(3, 4), (12, 5), (3, 4), (15, 9), (12, 5), (12, 5)]
    c0 = [(0, y, x) for y, x in px] + [(0, H, 3)]
    c2 = [(2, 1, 1), (2, 10, 6), (2, 19, 11), (2, 5, 0)]
    coords = np.array(c0 + c2, dtype=np.int32)
    values = (rng.random((len(coords), C)) * 90 + 10).astype(np.float32)
    values[5, 0] = -3.25
    values[9, C - 1] = -12.5
    values[len(c0):] = 7.5
    img_bs = np.array([[0, 0], [0, 2], [1, 1]], dtype=np.int32)
    return (H, W), coords, values, img_bs


@pytest.mark.parametrize("C", [1, 3, 4])
def test_sigma_and_replicate_kernels_against_the_restatement(C):
    from transformercvn.hip import gradients
    shape, coords, values, img_bs = hand_list(C)
    nnz, n_img, B, P, noise, seed = len(coords), 3, 2, 2, 0.15, (1 << 62) + 12345
    c, v, bs = torch.from_numpy(coords).cuda(), torch.from_numpy(values).cuda(), torch.from_numpy(img_bs).cuda()
    sigma = torch.full((B, 1 + P), float("nan"), device="cuda")
    gradients.noise_sigma(c, v, n_img, shape, bs, noise, sigma)
    ref_sigma = S.sigma(coords, values, n_img, shape, img_bs, B, P, noise)
    assert np.array_equal(sigma.cpu().numpy(), ref_sigma, equal_nan=True)                  # exact: max and min are exact
    assert ref_sigma[0, 2] == 0 and ref_sigma[1, 1] == np.float32(noise * 7.5) and ref_sigma[0, 0] == np.float32(noise * (float(values[:-5].max()) + 12.5))
    assert np.isnan(ref_sigma[[0, 1, 1], [1, 0, 2]]).all()
    out_c, out_v = gradients.noise_replicate(c, v, n_img, shape, bs, sigma, seed, 0, 5)
    ref_c, ref_v, _ = S.replicate(coords, values, n_img, shape, img_bs, P, ref_sigma, seed, 0, 5)
    assert np.array_equal(out_c.cpu().numpy(), ref_c)                                       # coordinates replicated exactly
    ok = one_ulp(out_v, ref_v)
    print(f"noise_replicate[C {C}]: {int((out_v.cpu().numpy() != ref_v).sum())} of {ref_v.size} values differ from the restatement, "
          f"{int((~ok).sum())} by more than one fp32 ulp")
    assert ok.all()
    got = out_v.view(5, nnz, C)
    assert (got >= 0).all()                                                               # the negative values sit inside map 0: clamped or lifted
    # duplicates get equal draws: (3, 4) is entries 16 and 18, (12, 5) entries 17, 20 and 21; their values differ, v' - v does not, up to
    # the fp32 rounding of the two v' (values below 256: half an ulp is at most 7.6e-6 each), where the clamp did not act
    d = got.double() - v.double()
    for i, j in ((16, 18), (17, 20), (17, 21)):
        assert np.array_equal(coords[i], coords[j])
        free = (got[:, i] > 0) & (got[:, j] > 0)
        assert free.any() and torch.allclose(d[:, i][free], d[:, j][free], rtol=0, atol=1.6e-5), (i, j)
    assert torch.equal(got[:, nnz - 5], v[nnz - 5].expand(5, C))                            # the entry outside the maps: unperturbed
    assert not torch.equal(got[0, :16], v[:16]) and not torch.equal(got[0], got[1])
    # a split gives the same bits
    a_c, a_v = gradients.noise_replicate(c, v, n_img, shape, bs, sigma, seed, 0, 2)
    b_c, b_v = gradients.noise_replicate(c, v, n_img, shape, bs, sigma, seed, 2, 3)
    assert torch.equal(torch.cat((a_v, b_v)), out_v) and torch.equal(a_c, out_c[:2 * nnz])
    assert torch.equal(b_c[:, 1:], out_c[:3 * nnz, 1:]) and torch.equal(b_c[:, 0], out_c[:3 * nnz, 0])       # image indices restart at t0
    # noise 0 copies the values bit for bit, negative ones included
    zero = torch.full((B, 1 + P), float("nan"), device="cuda")
    gradients.noise_sigma(c, v, n_img, shape, bs, 0.0, zero)
    assert np.array_equal(zero.cpu().numpy(), S.sigma(coords, values, n_img, shape, img_bs, B, P, 0.0), equal_nan=True)
    _, z_v = gradients.noise_replicate(c, v, n_img, shape, bs, zero, seed, 0, 2)
    assert torch.equal(z_v.view(torch.int32), v.repeat(2, 1).view(torch.int32))


@pytest.mark.parametrize("C", [1, 3, 4])
def test_accumulate_and_finish_kernels_within_the_stated_bound(C):
    from transformercvn.hip import gradients
    rng = np.random.default_rng(70 + C)
    T, nnz = 5, 333
    g = (rng.standard_normal((T, nnz, C)) * 2.0 ** rng.integers(-20, 21, (T, nnz, C))).astype(np.float32)
    g[:, :7] = 0                                                              # entries that own nothing
    v = (rng.random((T, nnz, C)) * 100).astype(np.float32)
    gd, vd = torch.from_numpy(g).cuda(), torch.from_numpy(v).cuda()
    acc = torch.full((4, nnz, C), float("nan"), dtype=torch.float64, device="cuda")      # t0 = 0 starts from zero whatever acc holds
    gradients.noise_accumulate(acc, gd, vd, 0)
    split = torch.zeros_like(acc)
    gradients.noise_accumulate(split, gd[:2].contiguous(), vd[:2].contiguous(), 0)
    gradients.noise_accumulate(split, gd[2:].contiguous(), vd[2:].contiguous(), 2)
    assert torch.equal(acc.view(torch.int64), split.view(torch.int64))
    one = torch.zeros_like(acc)
    for t in range(T):
        gradients.noise_accumulate(one, gd[t:t + 1].contiguous(), vd[t:t + 1].contiguous(), t)
    assert torch.equal(acc.view(torch.int64), one.view(torch.int64))
    for x, st in zip((g.astype(np.float64), g.astype(np.float64) * v.astype(np.float64)), gradients.noise_finish(acc, T)):
        for name, got, ref, bound in zip(("mean", "var", "mean_sq"), (st.mean, st.var, st.mean_sq), S.stats(x), S.stat_bounds(x)):
            ok = S.within(got.cpu().numpy(), ref, bound)
            assert ok.all(), (name, int((~ok).sum()))
        assert (st.var >= 0).all() and (st.var[:7] == 0).all() and (st.mean[:7] == 0).all()
    first = gradients.noise_finish(one[:, :, :].contiguous(), 1)[0]
    assert torch.isnan(first.var).all()


# ---- 2. end to end, fp32, case A ----------------------------------------------------------------------------------------------------------
KINK = 2.0 ** -22


def kink_maps(sd, cfg, batch8, ev_values, pr_values):
    """The images of (event list, prong list) in which the float64 oracle finds a PReLU input of an embedder closer to zero than fp32 can
    tell: |x| < 2^-22 of the largest input of that activation in that image.  Such an x is the difference of a convolution output times
    the BatchNorm scale and the BatchNorm shift, each carried with a relative error of a few 2^-24 in fp32, so four roundings of the
    layer's scale is the distance inside which fp32 arithmetic -- any, torch's as well -- may land on the other side of the kink.  The
    gradient then changes by that unit's whole contribution, a step that has nothing to do with the accuracy of the kernels."""
    found = {"event": set(), "prong": set()}
    state = {"which": None}
    dense, prelu = O.densenet_forward, O._prelu

    def spy_dense(sd_, prefix, *a):
        state["which"] = "event" if prefix.endswith("event_pixel_embedding") else "prong"
        try:
            return dense(sd_, prefix, *a)
        finally:
            state["which"] = None

    def spy_prelu(x, slope):
        if state["which"] is not None and x.dim() == 4:
            a = x.detach().abs().flatten(1)
            found[state["which"]].update(torch.nonzero(a.min(1).values < KINK * a.max(1).values).flatten().tolist())
        return prelu(x, slope)
    b = list(batch8)
    b[3], b[6] = ev_values.cpu().double(), pr_values.cpu().double()
    O.densenet_forward, O._prelu = spy_dense, spy_prelu
    try:
        with torch.no_grad():
            O.forward(R.cast_state(sd, torch.float64), cfg, tuple(b), training=False)
    finally:
        O.densenet_forward, O._prelu = dense, prelu
    return found


def map_figures(got, ref, coords):
    """image -> relative L2 of that map's gradient (R.per_map_rel_l2 on one map at a time)."""
    got, img = got.cpu(), coords[:, 0]
    return {n: R.per_map_rel_l2(got[img == n], ref[img == n], coords[img == n]) for n in img.unique().tolist()}


def sample_figures(tag, res, sd, cfg, batch, oracle_of, samples):
    """Prints every sample's figures -> (the worst relative L2 of a tensor or map that no kink touches, of one that a kink touches)."""
    clear, touched = dict(event=0.0, prong=0.0), dict(event=0.0, prong=0.0)
    for t in range(samples):
        ref = oracle_of(t, res.sample_event_values[t], res.sample_prong_values[t])
        kinks = kink_maps(sd, cfg, batch[:8], res.sample_event_values[t], res.sample_prong_values[t])
        for name, got, r, coords in (("event", res.sample_event_grad[t], ref[0], batch[2]), ("prong", res.sample_prong_grad[t], ref[1], batch[5])):
            whole, maps = R.rel_l2(got, r), map_figures(got, r, coords)
            print(f"smooth_hit_gradients[{tag}] sample {t} {name}: relative L2 vs float64 {whole:.3e}, per map "
                  + " ".join(f"{v:.3e}" for v in maps.values()) + f", maps with a PReLU input inside fp32's reach of its kink: {sorted(kinks[name])}")
            for n, v in maps.items():
                side = touched if n in kinks[name] else clear
                side[name] = max(side[name], v)
            side = touched if kinks[name] else clear
            side[name] = max(side[name], whole)
    return clear, touched


def test_fp32_samples_statistics_kinds_and_heatmap():
    cfg, sd, batch = case_a()
    model = model_of(cfg, sd)
    dev = to_device(batch[:8])
    res = model.smooth_hit_gradients(*dev, target=CLASSES_A, value="prob", samples=SAMPLES, noise=NOISE, seed=SEED, keep_samples=True)
    plain = model.hit_gradients(*dev, target=CLASSES_A, value="prob")
    assert torch.equal(res.event_logits, plain.event_logits) and torch.equal(res.prong_logits, plain.prong_logits)
    assert (res.samples, res.noise, res.seed, res.kind, res.method) == (SAMPLES, NOISE, SEED, "smoothgrad", "gradient")
    # (a) the perturbed values
    sig, ev_v, pr_v = reference_samples(cfg, batch, NOISE, SEED, 0, SAMPLES)
    assert np.array_equal(res.sigma.cpu().numpy(), sig, equal_nan=True) and np.isnan(sig).sum() == int((~batch[7]).sum())
    assert res.sample_event_values.shape == (SAMPLES, *batch[3].shape) and res.sample_prong_grad.shape == (SAMPLES, *batch[6].shape)
    assert one_ulp(res.sample_event_values, ev_v).all() and one_ulp(res.sample_prong_values, pr_v).all()
    assert not torch.equal(res.sample_event_values[0], dev[3]) and (res.sample_event_values >= 0).all()
    # (b) every per-sample gradient against float64 at those very values
    clear, touched = sample_figures("A fp32", res, sd, cfg, batch, oracle_a_at, SAMPLES)
    assert all(clear[k] <= GATE_SAMPLE[k] for k in clear), clear
    for t in range(SAMPLES):                   # the specification's gate: every per-sample gradient, whole tensor, kink or not
        ref = oracle_a_at(t, res.sample_event_values[t], res.sample_prong_values[t])
        assert R.rel_l2(res.sample_event_grad[t], ref[0]) <= GATE_F32 and R.rel_l2(res.sample_prong_grad[t], ref[1]) <= GATE_F32, t
    print(f"smooth_hit_gradients[A fp32] worst relative L2 clear of every kink {clear}, touched by one {touched}")
    # (c) the reported statistics are the float64 statistics of the device's own samples
    for grads, vals, fields in ((res.sample_event_grad, res.sample_event_values, ("event_grad", "event_attr")),
                                (res.sample_prong_grad, res.sample_prong_values, ("prong_grad", "prong_attr"))):
        g = grads.cpu().numpy().astype(np.float64)
        for x, field in zip((g, g * vals.cpu().numpy().astype(np.float64)), fields):
            (mean, var, _), (b_mean, b_var, _) = S.stats(x), S.stat_bounds(x)
            assert S.within(getattr(res, field + "_mean").cpu().numpy(), mean, b_mean).all(), field
            assert S.within(getattr(res, field + "_var").cpu().numpy(), var, b_var).all(), field
    se_ev, se_pr = res.stderr()
    assert torch.equal(se_ev, (res.event_grad_var / SAMPLES).sqrt()) and se_pr.shape == res.prong_grad.shape and (se_ev > 0).any()
    # (d) event_grad is the field `kind` names
    assert torch.equal(res.event_grad, res.event_grad_mean) and torch.equal(res.prong_attr, res.prong_attr_mean)
    var = model.smooth_hit_gradients(*dev, target=CLASSES_A, samples=SAMPLES, noise=NOISE, seed=SEED, kind="vargrad")
    assert var.sample_event_grad is None and var.sample_prong_values is None and var.kind == "vargrad"
    assert torch.equal(var.event_grad, res.event_grad_var) and torch.equal(var.prong_grad, res.prong_grad_var)
    assert torch.equal(var.event_attr, res.event_attr_var) and torch.equal(var.event_grad_mean, res.event_grad_mean)
    sq = model.smooth_hit_gradients(*dev, target=CLASSES_A, samples=SAMPLES, noise=NOISE, seed=SEED, kind="smoothgrad_sq")
    for got, grads, vals in ((sq.event_grad, res.sample_event_grad, None), (sq.prong_grad, res.sample_prong_grad, None),
                             (sq.event_attr, res.sample_event_grad, res.sample_event_values),
                             (sq.prong_attr, res.sample_prong_grad, res.sample_prong_values)):
        x = grads.cpu().numpy().astype(np.float64) * (1.0 if vals is None else vals.cpu().numpy().astype(np.float64))
        assert S.within(got.cpu().numpy(), S.stats(x)[2], S.stat_bounds(x)[2]).all()
    assert torch.equal(sq.event_grad_var, res.event_grad_var)
    # (e) the heat map
    hm, hm_plain = res.heatmap((8, 8)), plain.heatmap((8, 8))
    assert hm.shape == hm_plain.shape == (2, 4, 13, 9) and torch.equal(torch.isnan(hm), torch.isnan(hm_plain))
    assert torch.isnan(hm[:, 1:][~batch[7]]).all() and (hm[:, 0] != 0).any()
    assert (torch.nan_to_num(hm)[torch.nan_to_num(hm_plain) == 0] == 0).all()                  # a tile without hits stays 0


# ---- 3. batched equals looped ---------------------------------------------------------------------------------------------------------
def test_samples_in_one_pass_match_one_pass_per_sample():
    cfg, sd, batch = case_a()
    model = model_of(cfg, sd)
    dev = to_device(batch[:8])
    kw = dict(target=CLASSES_A, samples=SAMPLES, noise=NOISE, seed=SEED, keep_samples=True)
    one = model.smooth_hit_gradients(*dev, **kw)                                # 6 maps per sample: all four in one pass
    loop = model.smooth_hit_gradients(*dev, max_maps_per_pass=1, **kw)           # one sample per pass
    two = model.smooth_hit_gradients(*dev, max_maps_per_pass=12, **kw)           # two passes of two
    for other in (loop, two):
        assert torch.equal(one.sample_event_values, other.sample_event_values) and torch.equal(one.sample_prong_values, other.sample_prong_values)
        assert torch.equal(one.sigma.view(torch.int32), other.sigma.view(torch.int32))
    figs = dict(event=R.rel_l2(one.sample_event_grad, loop.sample_event_grad.cpu()), prong=R.rel_l2(one.sample_prong_grad, loop.sample_prong_grad.cpu()),
                event_two=R.rel_l2(two.sample_event_grad, loop.sample_event_grad.cpu()), prong_two=R.rel_l2(two.sample_prong_grad, loop.sample_prong_grad.cpu()))
    same = torch.equal(one.sample_event_grad, loop.sample_event_grad) and torch.equal(one.sample_prong_grad, loop.sample_prong_grad)
    print(f"smooth_hit_gradients[A fp32] batched against looped: bit-identical {same}; relative L2 " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert figs["event"] <= GATE_SAMPLE["event"] and figs["event_two"] <= GATE_SAMPLE["event"]
    assert figs["prong"] <= GATE_SAMPLE["prong"] and figs["prong_two"] <= GATE_SAMPLE["prong"]
    assert R.rel_l2(one.event_grad, loop.event_grad.cpu()) <= GATE_SAMPLE["event"]


# ---- 4. noise = 0 -----------------------------------------------------------------------------------------------------------------------
def test_noise_zero_is_the_plain_gradient():
    cfg, sd, batch = case_a()
    model = model_of(cfg, sd)
    dev = to_device(batch[:8])
    plain = model.hit_gradients(*dev, target=CLASSES_A, value="prob")
    res = model.smooth_hit_gradients(*dev, target=CLASSES_A, samples=3, noise=0.0, seed=SEED, keep_samples=True)
    mask = batch[7]
    assert (res.sigma.cpu()[:, 0] == 0).all() and (res.sigma.cpu()[:, 1:][mask] == 0).all() and torch.isnan(res.sigma.cpu()[:, 1:][~mask]).all()
    for t in range(3):
        assert torch.equal(res.sample_event_values[t], dev[3]) and torch.equal(res.sample_prong_values[t], dev[6])
        figs = (R.rel_l2(res.sample_event_grad[t], plain.event_grad.cpu()), R.rel_l2(res.sample_prong_grad[t], plain.prong_grad.cpu()))
        print(f"smooth_hit_gradients[A fp32 noise 0] sample {t} (three in one pass) against hit_gradients: relative L2 event {figs[0]:.3e}, "
              f"prong {figs[1]:.3e}, bit-identical {torch.equal(res.sample_event_grad[t], plain.event_grad) and torch.equal(res.sample_prong_grad[t], plain.prong_grad)}")
        assert figs[0] <= GATE_SAMPLE["event"] and figs[1] <= GATE_SAMPLE["prong"]
        # test 3 measured bit identity between a map's gradient in a pass of many samples and in a pass of its own: the three
        # copies of one pass then agree bit for bit
        assert torch.equal(res.sample_event_grad[t], res.sample_event_grad[0]) and torch.equal(res.sample_prong_grad[t], res.sample_prong_grad[0])
    # one sample per pass: the same pass on the same batch shape, three times
    loop = model.smooth_hit_gradients(*dev, target=CLASSES_A, samples=3, noise=0.0, seed=SEED, max_maps_per_pass=1, kind="vargrad")
    assert torch.equal(loop.event_grad_mean, plain.event_grad) and torch.equal(loop.prong_grad_mean, plain.prong_grad)
    assert torch.equal(loop.event_attr_mean, plain.event_attr) and torch.equal(loop.prong_attr_mean, plain.prong_attr)
    for v in (loop.event_grad_var, loop.prong_grad_var, loop.event_attr_var, loop.prong_attr_var, loop.event_grad, loop.prong_attr):
        assert (v == 0).all()


# ---- 5. bf16 mode -------------------------------------------------------------------------------------------------------------------------
def test_bf16_samples_stay_within_twice_the_autocast_oracle():
    cfg, sd, batch = case_a()
    res = model_of(cfg, sd, "bf16").smooth_hit_gradients(*to_device(batch[:8]), target=CLASSES_A, value="prob", samples=2, noise=NOISE,
                                                         seed=SEED, keep_samples=True)
    for t in range(2):
        ref = oracle_a_at(t, res.sample_event_values[t], res.sample_prong_values[t])
        ac = oracle_a_at(t, res.sample_event_values[t], res.sample_prong_values[t], autocast=True)
        for name, got, a, r in (("event", res.sample_event_grad[t], ac[0], ref[0]), ("prong", res.sample_prong_grad[t], ac[1], ref[1])):
            l2, l2_ac, cos, cos_ac = R.rel_l2(got, r), R.rel_l2(a, r), R.cosine(got, r), R.cosine(a, r)
            print(f"smooth_hit_gradients[A bf16] sample {t} {name}: relative L2 {l2:.4f} (autocast oracle {l2_ac:.4f}), cosine {cos:.5f} "
                  f"(autocast {cos_ac:.5f})")
            assert l2 <= 2 * l2_ac, (t, name, l2, l2_ac)
            assert cos >= cos_ac - (1 - cos_ac), (t, name, cos, cos_ac)


# ---- 6. target and seeds ------------------------------------------------------------------------------------------------------------------
def test_case_b_prong_target_and_raw_seeds_with_a_padded_slot():
    cfg, sd, batch = case_b()
    model = model_of(cfg, sd)
    dev = to_device(batch[:8])
    res = model.smooth_hit_gradients(*dev, target="prong", value="prob", samples=2, noise=NOISE, seed=SEED, keep_samples=True)
    _, ev_v, pr_v = reference_samples(cfg, batch, NOISE, SEED, 0, 2)
    assert one_ulp(res.sample_event_values, ev_v).all() and one_ulp(res.sample_prong_values, pr_v).all()
    classes = res.prong_logits.argmax(2).cpu()
    for t in range(2):
        ref = R.oracle_hit_gradients(sd, cfg, batch[:8], "prong", "prob", values=(res.sample_event_values[t].cpu(), res.sample_prong_values[t].cpu()))
        # the oracle takes the classes its own prediction at the perturbed values names; the library those of the unperturbed one
        assert torch.equal(ref[3].argmax(2)[batch[7]], classes[batch[7]])
        figs = dict(event=R.rel_l2(res.sample_event_grad[t], ref[0]), prong=R.rel_l2(res.sample_prong_grad[t], ref[1]),
                    event_map=R.per_map_rel_l2(res.sample_event_grad[t], ref[0], batch[2]),
                    prong_map=R.per_map_rel_l2(res.sample_prong_grad[t], ref[1], batch[5]))
        print(f"smooth_hit_gradients[B fp32 prong] sample {t} relative L2 vs float64: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
        assert all(v <= GATE_F32 for v in figs.values()), figs
    # raw seeds, case A (two padded slots seeded non-zero): the padded slots contribute nothing
    cfg, sd, batch = case_a()
    model = model_of(cfg, sd)
    dev = to_device(batch[:8])
    g = torch.Generator().manual_seed(21)
    B, P = batch[7].shape
    d_ev = torch.randn(B, cfg.num_event_classes, generator=g)
    d_pr = torch.randn(B, P, cfg.num_prong_classes, generator=g)
    assert (~batch[7]).any() and (d_pr[~batch[7]] != 0).all()
    kw = dict(samples=2, noise=NOISE, seed=SEED, keep_samples=True)
    res = model.smooth_hit_gradients(*dev, target=(d_ev.cuda(), d_pr.cuda()), **kw)
    clean = model.smooth_hit_gradients(*dev, target=(d_ev.cuda(), (d_pr * batch[7].unsqueeze(2)).cuda()), **kw)
    for name in ("sample_event_grad", "sample_prong_grad", "event_grad", "prong_grad", "event_attr_var", "prong_attr_var"):
        assert torch.equal(getattr(res, name), getattr(clean, name)), name
    ref = R.oracle_hit_gradients(sd, cfg, batch[:8], (d_ev, d_pr), "logit", values=(res.sample_event_values[1].cpu(), res.sample_prong_values[1].cpu()))
    figs = dict(event=R.rel_l2(res.sample_event_grad[1], ref[0]), prong=R.rel_l2(res.sample_prong_grad[1], ref[1]))
    print(f"smooth_hit_gradients[A fp32 raw seeds] sample 1 relative L2 vs float64: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert all(v <= GATE_F32 for v in figs.values()), figs


# ---- 7. nothing else moves ----------------------------------------------------------------------------------------------------------------
FIELDS = ("event_logits", "prong_logits", "event_grad", "prong_grad", "event_attr", "prong_attr", "event_grad_mean", "event_grad_var",
          "event_attr_mean", "event_attr_var", "prong_grad_mean", "prong_grad_var", "prong_attr_mean", "prong_attr_var", "sigma",
          "sample_event_values", "sample_event_grad", "sample_prong_values", "sample_prong_grad")


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_nothing_else_moves():
    """State, gradients, step counter, last_seeds and hook around smooth_hit_gradients, and the training step that follows against the
    same step of a fresh model: the loss and every gradient bit-identical -- except where the training step itself is not reproducible.
    In fp32 mode every convolution of the embedders ends its weight and bias gradient in float atomics between workgroups, so two fresh
    models differ there themselves by the arrival order (tests/test_hit_gradients_gpu.py::test_nothing_else_moves documents which
    tensors and why): those are held to 512 * 2^-24 of the largest weight gradient of their convolution, every other gradient exactly."""
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
    train_step(fresh)                                                       # step 0 of both models
    loss1_fresh, grads1_fresh = train_step(fresh)
    conv = lambda k: k.rsplit(".", 1)[0]
    atomic = lambda k: "pixel_embedding.features." in k and conv(k).endswith((".conv0", ".conv1", ".conv2", ".conv"))
    exact = {k for k, g in grads1_fresh.items() if g is not None and not atomic(k)}
    model = trainer_of(cfg, sd)
    hooked = []
    train_step(model)
    rt = model.network.hip_runtime()
    rt.grad_ready_hook = hooked.append
    model.eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    grads_before = {k: None if p.grad is None else p.grad.clone() for k, p in model.named_parameters()}
    step_before, seeds_before = rt.step, dict(rt.last_seeds)
    plain_before = model.hit_gradients(*dev, target="event")
    kw = dict(target="event", samples=3, noise=NOISE, keep_samples=True)
    a = model.smooth_hit_gradients(*dev, seed=1, **kw)
    b = model.smooth_hit_gradients(*dev, seed=1, **kw)
    other = model.smooth_hit_gradients(*dev, seed=2, **kw)
    for name in FIELDS:
        assert same_bits(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(a.sample_event_values, other.sample_event_values) and not torch.equal(a.event_grad, other.event_grad)
    assert same_bits(a.sigma, other.sigma) and torch.equal(a.event_logits, other.event_logits)
    plain_after = model.hit_gradients(*dev, target="event")
    for name in ("event_logits", "prong_logits", "event_grad", "prong_grad", "event_attr", "prong_attr"):
        assert torch.equal(getattr(plain_before, name), getattr(plain_after, name)), name
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), [k for k in before if not torch.equal(before[k], after[k])]
    assert all((p.grad is None) if grads_before[k] is None else torch.equal(grads_before[k], p.grad) for k, p in model.named_parameters())
    assert rt.step == step_before and rt.last_seeds == seeds_before and hooked == []
    for p in model.parameters():
        p.grad = None
    model.smooth_hit_gradients(*dev, target="event", samples=2)
    assert all(p.grad is None for p in model.parameters())
    rt.grad_ready_hook = None
    loss1, grads1 = train_step(model)                                       # step 1 behind the smooth_hit_gradients calls
    assert torch.equal(loss1, loss1_fresh)
    assert all(grads1[k] is None for k in grads1 if grads1_fresh[k] is None)
    assert all(torch.equal(grads1[k], grads1_fresh[k]) for k in exact), [k for k in exact if not torch.equal(grads1[k], grads1_fresh[k])]
    for k, g in grads1_fresh.items():
        if g is not None and k not in exact:
            scale = float(grads1_fresh[conv(k) + ".weight"].abs().max())
            assert float((grads1[k] - g).abs().max()) <= 512 * 2 ** -24 * scale, k
