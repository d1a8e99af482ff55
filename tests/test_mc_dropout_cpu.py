"""Monte-Carlo dropout without a GPU: the float64 statistics reference on cases with known answers, the oracle's eval-statistics sample
against its own eval forward, and the argument / mode checks that must fire before any device work."""
import math

import numpy as np
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case
from mc_dropout_reference import oracle_sample, stats


def test_library_exports_the_mc_entry_points():
    from transformercvn.hip import _lib
    for name in ("tcvn_densenet_forward_mc", "tcvn_head_forward_mc", "tcvn_rows_bn_prelu_forward_mc", "tcvn_mc_dropout_stats"):
        assert name in _lib.EXPORTS, name
        assert hasattr(_lib.lib, name), name


def test_stats_of_identical_samples_have_no_spread():
    row = np.random.default_rng(0).normal(size=(1, 5, 4))
    s = stats(np.repeat(row, 7, axis=0))
    assert np.all(s["std_prob"] == 0) and np.all(s["mutual_info"] <= 1e-15)
    assert np.allclose(s["entropy"], s["expected_entropy"], rtol=0, atol=1e-15)
    assert np.allclose(s["votes"].sum(1), 1.0)


def test_stats_of_two_one_hot_samples_on_different_classes():
    big = 1000.0                                                # softmax of (1000, 0, 0) is one-hot in float64
    x = np.zeros((2, 1, 3))
    x[0, 0, 0] = big
    x[1, 0, 2] = big
    s = stats(x)
    assert s["entropy"][0] == pytest.approx(math.log(2), abs=1e-15)
    assert s["expected_entropy"][0] == 0.0
    assert s["mutual_info"][0] == pytest.approx(math.log(2), abs=1e-15)
    assert s["votes"][0].tolist() == [0.5, 0.0, 0.5]
    assert s["mean_prob"][0].tolist() == [0.5, 0.0, 0.5]
    assert s["std_prob"][0] == pytest.approx([math.sqrt(0.5), 0.0, math.sqrt(0.5)])


def test_stats_padded_rows_are_nan_and_ties_vote_for_the_lowest_class():
    x = np.random.default_rng(1).normal(size=(3, 4, 5))
    x[:, 2, :] = 0.25                                           # all classes equal: the arg max is class 0
    s = stats(x, valid=np.array([0, -1, 7, -1]))
    for k, v in s.items():
        assert np.isnan(v[[1, 3]]).all() and np.isfinite(v[[0, 2]]).all(), k
    assert s["votes"][2].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert s["entropy"][2] == pytest.approx(math.log(5))
    s1 = stats(x[:1])
    assert np.all(s1["std_prob"] == 0)                          # one sample: no spread by definition


def test_stats_mutual_information_is_never_negative():
    rng = np.random.default_rng(2)
    for T, C, scale in ((1, 3, 1.0), (2, 4, 5.0), (17, 9, 0.01), (64, 2, 30.0)):
        s = stats(rng.normal(size=(T, 50, C)) * scale)
        assert np.all(s["mutual_info"] >= 0)
        assert np.all(s["entropy"] - s["expected_entropy"] > -1e-12)      # Jensen: the clamp only removes rounding
        assert np.allclose(s["mean_prob"].sum(1), 1.0) and np.allclose(s["votes"].sum(1), 1.0)


def test_oracle_sample_with_all_ones_masks_is_the_eval_forward():
    """Validates the swapped BatchNorm: with every mask 1 the eval-statistics sample is O.forward(training=False), in float64."""
    cfg, over, batch, g = load_case("small_b3")
    assert cfg.dropout > 0 and cfg.pixel_noise_std > 0
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = tuple(t.double() if t.is_floating_point() else t for t in batch[:8])
    sites = []

    def ones(site, shape):
        sites.append(site)
        return torch.ones(shape, dtype=torch.float64)
    ev, pr, ctx = oracle_sample(sd64, cfg, b64, ones)
    with torch.no_grad():
        ev0, pr0, _ = O.forward(sd64, cfg, b64, training=False)
    assert sites, "no dropout site fired: the sample would be the eval forward by construction"
    assert any(":dense" in s for s in sites) and any("combined_embedding" in s for s in sites)
    assert (ev - ev0).abs().max().item() < 1e-12 and (pr - pr0).abs().max().item() < 1e-12
    assert O._batch_norm.__module__ == O.__name__               # the oracle's own function is back


def test_check_args_rejections():
    from transformercvn.hip.uncertainty import check_args, sample_seeds
    assert check_args(1, 0) == (1, 0) and check_args(32, 2 ** 63 - 1) == (32, 2 ** 63 - 1)
    for samples in (0, -3, 2.0, "8", True, None):
        with pytest.raises(ValueError):
            check_args(samples, 0)
    for seed in (-1, 2 ** 63, 1.5, "0", False, None):
        with pytest.raises(ValueError):
            check_args(4, seed)
    s = (5 * 1000003 + 2) & 0x7FFFFFFFFFFFFFFF                  # the derivation of HipRuntime._next_seeds with t in the step's place
    assert sample_seeds(5, 2) == (s ^ 0x1111, s ^ 0x2222, s ^ 0x3333, s ^ 0x4444)


def test_mc_dropout_refuses_train_mode_and_bad_keywords_before_device_work():
    from model_utils import build_trainer
    cfg, over, batch, g = load_case("small_b3")
    model = build_trainer(cfg, None, device=None)               # CPU-built: any device work would raise something else
    model.train()
    with pytest.raises(RuntimeError, match=r"mc_dropout .* call \.eval\(\) first"):
        model.mc_dropout(*batch[:8])
    with pytest.raises(RuntimeError, match=r"mc_dropout .* call \.eval\(\) first"):
        model.network.mc_dropout(*model._network_inputs(*batch[:8]))
    model.eval()
    with pytest.raises(ValueError):
        model.mc_dropout(*batch[:8], samples=0)
    with pytest.raises(ValueError):
        model.mc_dropout(*batch[:8], seed=-1)


def test_sdxl_network_has_no_monte_carlo_dropout():
    """The SDXL embedder has no dropout site: mc_dropout says so (NotImplementedError) before any device work."""
    from model_utils import build_trainer
    cfg = O.tutorial_config(embedder="sdxl", initial_pixel_dim=8, pixel_embedding_dim=64, hidden_dim=64, num_encoder_layers=2)
    batch = O.synthetic_batch([2, 1], 3, cfg)
    model = build_trainer(cfg, None, device=None)
    model.eval()
    with pytest.raises(NotImplementedError, match="SDXL"):
        model.mc_dropout(*batch[:8], samples=2)
