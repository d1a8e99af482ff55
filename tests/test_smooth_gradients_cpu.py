"""Noise-averaged hit gradients without a GPU: the argument checks and refusals of smooth_hit_gradients, the float64 restatement
(tests/smooth_gradients_reference.py) against itself -- moments of the draws, independence of list order and chunking, the statistics
against numpy -- and the header's declarations."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import tcvn_oracle as O
import smooth_gradients_reference as S

SMALL = dict(densenet_structure=[2, 2], densenet_growth_rate=8, initial_pixel_dim=16, num_encoder_layers=2, pixel_embedding_dim=64,
             hidden_dim=64, num_prong_decoder_layers=3)
SYMBOLS = ("tcvn_noise_workspace_bytes", "tcvn_noise_sigma", "tcvn_noise_replicate", "tcvn_noise_accumulate", "tcvn_noise_finish")


def _model(**cfg_kw):
    from model_utils import build_trainer
    cfg = O.tutorial_config(**cfg_kw)
    return build_trainer(cfg, None, device=None), O.synthetic_batch([2, 1], 3, cfg)


BAD = (dict(kind="vargrad", samples=1), dict(samples=0), dict(samples=True), dict(samples=2.5), dict(samples=4097), dict(noise=-0.1),
       dict(noise=float("nan")), dict(noise=float("inf")), dict(noise="0.1"), dict(seed=-1), dict(seed=1 << 63), dict(seed=1.0),
       dict(max_maps_per_pass=0), dict(max_maps_per_pass=257), dict(kind="smooth"), dict(value="odds"), dict(target="track"),
       dict(target=-1))


def test_argument_checks_come_before_any_device_work():
    model, batch = _model(**SMALL)
    model.eval()
    for bad in BAD:
        with pytest.raises(ValueError, match="hit_gradients"):
            model.smooth_hit_gradients(*batch[:8], **bad)
        with pytest.raises(ValueError, match="hit_gradients"):
            model.network.smooth_hit_gradients(*model._network_inputs(*batch[:8]), None, **bad)


def test_check_smooth_args_returns_plain_numbers():
    from transformercvn.hip import gradients
    out = gradients.check_smooth_args("event", "logit", "vargrad", 2, 0, (1 << 63) - 1, 256)
    assert out == ("event", 1, "vargrad", 2, 0.0, (1 << 63) - 1, 256) and isinstance(out[4], float)
    assert gradients.check_smooth_args(3, "prob", "smoothgrad_sq", 4096, 0.15, 0, 1)[1:] == (0, "smoothgrad_sq", 4096, 0.15, 0, 1)
    assert gradients.KINDS == ("smoothgrad", "smoothgrad_sq", "vargrad")


def test_training_mode_is_refused():
    model, batch = _model(**SMALL)
    model.train()
    with pytest.raises(RuntimeError, match=r"smooth_hit_gradients .* call \.eval\(\) first"):
        model.smooth_hit_gradients(*batch[:8])
    with pytest.raises(RuntimeError, match=r"smooth_hit_gradients .* call \.eval\(\) first"):
        model.network.smooth_hit_gradients(*model._network_inputs(*batch[:8]))


def test_one_hot_pixels_are_refused():
    from transformercvn.hip import gradients
    from transformercvn.hip.pixels import SparsePixels, VALUE_ONE_HOT
    with pytest.raises(ValueError, match="one-hot"):
        gradients.check_smooth_args("event", "prob", "smoothgrad", 16, 0.15, 0, 256, one_hot=True)
    model, batch = _model(**SMALL)
    model.eval()
    f, x, ev_px, em, pr_px, pm = model._network_inputs(*batch[:8])
    hot = SparsePixels(ev_px.coords, ev_px.values, ev_px.shape, VALUE_ONE_HOT)
    with pytest.raises(ValueError, match="one-hot"):
        model.network.smooth_hit_gradients(f, x, hot, em, pr_px, pm)


def test_sdxl_network_has_no_smooth_hit_gradients():
    model, batch = _model(embedder="sdxl", initial_pixel_dim=8, pixel_embedding_dim=64, hidden_dim=64, num_encoder_layers=2)
    model.eval()
    with pytest.raises(NotImplementedError, match="SDXL"):
        model.smooth_hit_gradients(*batch[:8])
    with pytest.raises(ValueError):                       # the keywords are still looked at first
        model.smooth_hit_gradients(*batch[:8], samples=0)


def test_result_selects_the_statistic_of_kind_and_keeps_the_heatmap():
    from transformercvn.hip import gradients
    g = torch.Generator().manual_seed(4)
    mask = torch.tensor([[True, False], [True, True]])
    ev_c = torch.tensor([[0, 0, 0], [1, 3, 2]], dtype=torch.int32)
    pr_c = torch.tensor([[0, 1, 1], [1, 2, 2], [2, 0, 3]], dtype=torch.int32)

    def stats(n):
        return tuple(gradients.NoiseStats(*(torch.rand(n, 3, generator=g) for _ in range(3))) for _ in range(2))
    ev, pr = stats(2), stats(3)
    for kind, field in (("smoothgrad", "mean"), ("smoothgrad_sq", "mean_sq"), ("vargrad", "var")):
        res = gradients.SmoothHitGradients(None, None, ev, pr, ev_c, pr_c, mask, (4, 4), torch.zeros(2, 3), 4, 0.1, 7, kind)
        assert isinstance(res, gradients.HitGradients) and res.method == "gradient"
        assert res.value is None and res.baseline_value is None and res.completeness_gap is None
        assert res.event_grad is getattr(ev[0], field) and res.event_attr is getattr(ev[1], field)
        assert res.prong_grad is getattr(pr[0], field) and res.prong_attr is getattr(pr[1], field)
        assert res.event_grad_mean is ev[0].mean and res.event_grad_var is ev[0].var and res.prong_attr_var is pr[1].var
        assert res.sample_event_values is None and res.sample_prong_grad is None
        assert (res.samples, res.noise, res.seed, res.kind) == (4, 0.1, 7, kind)
        se_ev, se_pr = res.stderr()
        assert torch.equal(se_ev, (ev[0].var / 4).sqrt()) and torch.equal(se_pr, (pr[0].var / 4).sqrt())
        hm = res.heatmap((2, 2))
        assert hm.shape == (2, 3, 2, 2) and torch.isnan(hm[0, 2]).all() and not torch.isnan(hm[:, 0]).any()
        assert torch.equal(torch.nan_to_num(hm), torch.nan_to_num(gradients.heatmap(res.event_attr, res.prong_attr, ev_c, pr_c, mask, (4, 4),
                                                                                    (2, 2), "sum")))


# ---- the reference against itself -------------------------------------------------------------------------------------------------------
def test_philox_restatement_matches_the_published_vectors():
    """Random123's known-answer tests for philox4x32-10."""
    got = S.philox4(0, 0, 0, 0, 0, 0)
    assert [int(w) for w in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = S.philox4(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(w) for w in got] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    got = S.philox4(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(w) for w in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_draws_have_the_moments_of_a_standard_normal():
    """2^17 draws of one seed: mean and variance within 5 standard errors of 0 and 1, the cos and sin branches uncorrelated to the same
    standard.  The draws are deterministic, so this passes or fails for good."""
    n = 1 << 15
    q = np.arange(n)
    z = S.draw(0x1234567, 3, q[:, None], 5, np.arange(4)[None, :])            # [n, 4]: channels 0 / 2 are cosines, 1 / 3 sines
    assert z.size == 1 << 17 and np.isfinite(z).all()
    N = z.size
    assert abs(z.mean()) < 5 / np.sqrt(N)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / N)                                  # var of the sample variance of a normal: 2 / N
    assert abs((z ** 4).mean() - 3) < 5 * np.sqrt(96 / N)                         # var of z^4: 105 - 9
    for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (0, 3)):                         # same call (cos, sin) and across the word pairs
        assert abs((z[:, a] * z[:, b]).mean()) < 5 / np.sqrt(n)
    # other samples, maps, seeds and channel groups are other draws
    base = S.draw(9, 0, q, 0, 0)
    for other in (S.draw(9, 1, q, 0, 0), S.draw(9, 0, q, 1, 0), S.draw(10, 0, q, 0, 0), S.draw(9 + (1 << 32), 0, q, 0, 0),
                  S.draw(9, 0, q, 0, 4)):
        assert abs((base * other).mean()) < 5 / np.sqrt(n) and not np.array_equal(base, other)


def _list(C=3, seed=0):
    rng = np.random.default_rng(seed)
    H, W, n_img = 20, 12, 3
    flat = rng.permutation(2 * H * W)[:50]
    coords = np.stack((flat // (H * W), (flat % (H * W)) // W, flat % W), 1).astype(np.int32)
    coords = coords[np.argsort(coords[:, 0], kind="stable")]
    coords = np.concatenate((coords, coords[[4, 4, 9]], [[0, H, 0]], [[3, 0, 0]], [[-1, 2, 2]])).astype(np.int32)   # duplicates, outside entries
    values = (rng.random((coords.shape[0], C)) * 100 + 1).astype(np.float32)
    img_bs = np.array([[0, 0], [1, 0], [1, 2]], dtype=np.int32)                 # map 2 (1, 2) holds no hit
    return (H, W), n_img, coords, values, img_bs


def test_sigma_and_perturbed_values_follow_the_definitions():
    shape, n_img, coords, values, img_bs = _list()
    sig = S.sigma(coords, values, n_img, shape, img_bs, 2, 2, 0.1)
    ok = S.inside(coords, n_img, *shape)
    assert np.isnan(sig[0, 1:]).all() and np.isnan(sig[1, 1]) and sig[1, 2] == 0
    for img, (b, s) in enumerate(img_bs[:2]):
        assert sig[b, s] == np.float32(0.1 * float(values[ok & (coords[:, 0] == img)].max()))
    c, v, v64 = S.replicate(coords, values, n_img, shape, img_bs, 2, sig, 5, 2, 3)
    nnz = coords.shape[0]
    assert c.shape == (3 * nnz, 3) and v.shape == (3 * nnz, 3) and v.dtype == np.float32 and (v >= 0).all()
    for r in range(3):
        blk = c[r * nnz:(r + 1) * nnz]
        assert np.array_equal(blk[:, 1:], coords[:, 1:])
        assert np.array_equal(blk[:-2, 0], coords[:-2, 0] + r * n_img) and (blk[-2:, 0] == -1).all()
        assert np.array_equal(v[r * nnz:(r + 1) * nnz][~ok], values[~ok])          # outside entries: unperturbed
        i = int(np.flatnonzero(ok)[7])
        b, s = img_bs[coords[i, 0]]
        z = S.draw(5, 2 + r, int(coords[i, 1]) * shape[1] + int(coords[i, 2]), int(b) * 3 + int(s), np.arange(3))
        want = np.maximum(values[i].astype(np.float64) + float(sig[b, s]) * z, 0).astype(np.float32)
        assert np.array_equal(v[r * nnz + i], want)
    # two entries of one pixel get one draw
    a, b = 4, nnz - 6
    assert np.array_equal(coords[a], coords[b])
    assert np.allclose((v64[a] - values[a]), (v64[b] - values[b]), rtol=0, atol=1e-9) and not np.array_equal(v64[a], values[a].astype(np.float64))
    # noise 0: a bit copy
    zero = S.sigma(coords, values, n_img, shape, img_bs, 2, 2, 0.0)
    assert np.array_equal(S.replicate(coords, values, n_img, shape, img_bs, 2, zero, 5, 0, 2)[1], np.tile(values, (2, 1)))


def test_draws_do_not_depend_on_list_order_or_on_the_split_into_chunks():
    shape, n_img, coords, values, img_bs = _list(C=4, seed=3)
    sig = S.sigma(coords, values, n_img, shape, img_bs, 2, 2, 0.2)
    nnz = coords.shape[0]
    _, whole, _ = S.replicate(coords, values, n_img, shape, img_bs, 2, sig, 11, 0, 5)
    _, first, _ = S.replicate(coords, values, n_img, shape, img_bs, 2, sig, 11, 0, 2)
    _, rest, _ = S.replicate(coords, values, n_img, shape, img_bs, 2, sig, 11, 2, 3)
    assert np.array_equal(whole, np.concatenate((first, rest)))
    perm = np.random.default_rng(1).permutation(nnz)
    _, shuffled, _ = S.replicate(coords[perm], values[perm], n_img, shape, img_bs, 2, sig, 11, 0, 5)
    assert np.array_equal(shuffled.reshape(5, nnz, 4), whole.reshape(5, nnz, 4)[:, perm])
    # a batch that holds only the second event: same (b, s), other image index, same draws
    keep = coords[:, 0] == 1
    alone = coords[keep].copy()
    alone[:, 0] = 0
    _, sub, _ = S.replicate(alone, values[keep], 1, shape, img_bs[1:2], 2, sig, 11, 0, 5)
    assert np.array_equal(sub.reshape(5, -1, 4), whole.reshape(5, nnz, 4)[:, keep])


@pytest.mark.parametrize("T", [1, 2, 5, 64])
def test_statistics_match_numpy_within_the_stated_bound(T):
    rng = np.random.default_rng(T)
    x = (rng.standard_normal((T, 300, 3)) * 2.0 ** rng.integers(-20, 21, (T, 300, 3))).astype(np.float32).astype(np.float64)
    x[:, :20] = x[0, :20] + 1e-3 * np.abs(x[0, :20]) * rng.standard_normal((T, 20, 3))       # a large mean under a small spread
    mean, var, msq = S.stats(x)
    b_mean, b_var, b_msq = S.stat_bounds(x)
    assert (np.abs(mean - x.mean(0)) <= b_mean).all()
    assert (np.abs(msq - (x * x).mean(0)) <= b_msq).all()
    if T == 1:
        assert np.isnan(var).all() and np.array_equal(mean, x[0])
    else:
        assert (np.abs(var - x.var(0, ddof=1)) <= b_var).all() and (var >= 0).all()
    # a split carries (mean, M2) over in double: the same bits
    m_a, m2_a = S.welford(x)
    assert np.array_equal(m_a, mean)
    assert S.within(mean.astype(np.float32), mean, 0).all()


def test_header_declares_the_noise_entries_and_the_loader_lists_them():
    from transformercvn.hip import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tcvn_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert getattr(_lib.lib, name).argtypes is not None
    assert header.index("Hit gradients") < header.index("tcvn_noise_sigma")
