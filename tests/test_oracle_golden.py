"""The CPU oracle (oracle/tcvn_oracle.py) against golden vectors produced by the real reference."""
import numpy as np
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case, train_cfg, rel_err, tap_sample

def is_noise_grad(key):
    """Every DenseNet conv bias feeds (only) train-mode BatchNorms, so its exact gradient is 0 and what the
    reference reports is fp32 rounding noise (~1e-4) -- compare those by magnitude only."""
    return "pixel_embedding.features" in key and key.endswith(("conv0.bias", "conv1.bias", "conv2.bias", "conv.bias"))


def grad_close(key, mine, ref, rtol=6e-3):
    # fp32 backward through 65 conv layers: the reference's own gradients sit 1-2e-3 (max-norm) from an fp64
    # evaluation of the same graph (measured), so fp32-vs-fp32 comparisons get a 6e-3 band.
    floor = 5e-3 if is_noise_grad(key) else 1e-6         # exact-zero gradients show up as rounding noise
    if np.abs(mine).max() < floor and np.abs(ref).max() < floor:
        return True
    return rel_err(mine, ref) < rtol


CASES = ["small_b3", "tutorial_b2p4", "tutorial_ragged", "tutorial_b2p8", "tutorial_b2p12", "tutorial_b32p8"]


def test_state_layout_matches_reference_counts():
    lay = O.state_layout(O.tutorial_config())
    assert len(lay) == 1208
    assert sum(int(np.prod(s)) if len(s) else 1 for s in lay.values()) == 5779136


def test_synthetic_batch_at_three_channels_is_the_golden_batch_bit_for_bit():
    """synthetic_batch draws cfg.pixel_dim value channels per hit; at the default 3 its Philox stream -- and with it every golden and every
    seeded case of the suite -- is unchanged: the committed small_b3 batch comes back bit for bit."""
    cfg, over, batch, g = load_case("small_b3")
    assert cfg.pixel_dim == 3
    again = O.synthetic_batch([int(n) for n in g["prongs"]], int(g["batch_seed"]), cfg)
    assert len(again) == len(batch) == 10
    for i, (a, b) in enumerate(zip(again, batch)):
        assert a.dtype == b.dtype and torch.equal(a, b), i


@pytest.mark.parametrize("pixel_dim", [1, 2, 4])
def test_synthetic_batch_draws_the_configured_channel_count(pixel_dim):
    cfg = O.tutorial_config(pixel_dim=pixel_dim, pixel_shape=(45, 37))
    batch = O.synthetic_batch([2, 1], 9, cfg, event_hits=(20, 40), prong_hits=(5, 20))
    for coords, values in ((batch[2], batch[3]), (batch[5], batch[6])):
        assert values.shape == (coords.shape[0], pixel_dim) and values.dtype == torch.float32
        assert float(values.min()) >= 1 and float(values.max()) <= 255 and bool((values == values.round()).all())
    if pixel_dim > 1:                                          # the channels are drawn independently
        assert not torch.equal(batch[6][:, 0], batch[6][:, 1])


@pytest.mark.parametrize("name", CASES)
def test_eval_logits(name):
    cfg, over, batch, g = load_case(name)
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    with torch.no_grad():
        et, pt, ev, pr, ctx = O.shared_step(sd, cfg, batch, training=False)
    assert rel_err(ev, g["eval_event_logits"]) < 2e-5
    assert rel_err(pr, g["eval_prong_logits"]) < 2e-5
    # events must not be degenerate copies of each other (SURVEY.md 7 'Degenerate goldens')
    assert np.abs(g["eval_event_logits"][0] - g["eval_event_logits"][1]).max() > 1e-3
    for k, t in ctx.taps.items():
        if "evaltap_stat:" + k in g:
            s, smp = tap_sample(t)
            assert rel_err(smp, g["evaltap_samp:" + k]) < 5e-5, k


@pytest.mark.parametrize("name", CASES)
def test_train_step(name):
    cfg, over, batch, g = load_case(name)
    cfgt = train_cfg(over)
    sd = O.fill_state(cfgt, int(g["weight_seed"]))
    (total, el, pl), (ev, pr), grads, ctx = O.train_step(sd, cfgt, batch)
    assert abs(total.item() - float(g["train_total_loss"])) < 2e-5 * abs(float(g["train_total_loss"]))
    assert abs(el.item() - float(g["train_event_loss"])) < 5e-5
    assert abs(pl.item() - float(g["train_prong_loss"])) < 5e-5
    # train mode on 2-3 events: BatchNorm1d over that few rows amplifies fp32 summation-order noise (measured up to 5.9e-5 on b2p8)
    assert rel_err(ev, g["train_event_logits"]) < 1e-4
    assert rel_err(pr, g["train_prong_logits"]) < 1e-4
    for k in [k for k in g if k.startswith("grad:")]:
        assert grad_close(k[5:], grads[k[5:]].numpy(), g[k]), k
    gn = dict(zip([str(k) for k in g["grad_keys"]], g["grad_norms"]))
    for k, v in grads.items():
        ref = gn[k]
        if is_noise_grad(k):
            continue
        # (+1e-5: Linear biases in front of a train-mode BatchNorm1d have an exactly-zero gradient; both sides report ~1e-6 of noise)
        assert abs(v.double().norm().item() - ref) <= 6e-3 * max(ref, 1e-6) + 1e-5, k
    for k in [k for k in g if k.startswith("newstat:")]:
        name_ = k[8:]
        if name_.endswith("num_batches_tracked"):
            continue
        assert rel_err(ctx.new_running[name_], g[k]) < 1e-5, k


def test_fp64_oracle_bounds_reference_noise():
    """fp64 evaluation of the oracle vs the reference's fp32 golden: logits to 2e-5, gradients to 3e-3."""
    cfg, over, batch, g = load_case("small_b3")
    cfgt = train_cfg(over)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in O.fill_state(cfgt, int(g["weight_seed"])).items()}
    b64 = tuple(t.double() if t.is_floating_point() else t for t in batch)
    (total, el, pl), (ev, pr), grads, ctx = O.train_step(sd, cfgt, b64)
    assert rel_err(g["train_event_logits"], ev) < 2e-5
    assert rel_err(g["train_prong_logits"], pr) < 2e-5
    for k in [k for k in g if k.startswith("grad:")]:
        assert grad_close(k[5:], g[k], grads[k[5:]].numpy(), rtol=3e-3), k


def test_oracle_norm_first_layer_matches_torch_module():
    """Pins the oracle's transformer_norm_first branch (no golden covers it: both option files use post-norm) to
    torch.nn.TransformerEncoderLayer(norm_first=True), the module the reference instantiates (prong_custom_bert_encoder.py:45-52)."""
    import torch
    from torch import nn
    cfg = O.tutorial_config(transformer_norm_first=True, hidden_dim=64, num_attention_heads=8)
    layer = nn.TransformerEncoderLayer(64, 8, 64, 0.0, "gelu", norm_first=True).eval()
    p = "network.encoder.encoder.layers.0"
    sd = {f"{p}.{k}": v.detach() for k, v in layer.state_dict().items()}
    x = torch.randn(5, 3, 64)
    pad = torch.tensor([[False, False, True, True, True], [False] * 5, [False, False, False, True, True]])
    with torch.no_grad():
        ref = layer(x, src_key_padding_mask=pad)
        mine = O.encoder_layer_forward(sd, p, cfg, x, pad, O._Ctx(False, 0.0))
    valid = (~pad).t().unsqueeze(-1)
    assert torch.allclose(mine * valid, ref * valid, atol=2e-6)
