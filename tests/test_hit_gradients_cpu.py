"""Hit gradients without a GPU: the float64 references the GPU tests rest on (tests/hit_gradients_reference.py) against torch autograd
and against each other, the host arithmetic of transformercvn.hip.gradients, and the argument checks."""
import math

import pytest
import torch

from oracle import tcvn_oracle as O
import hit_gradients_reference as R


def _case(dups=False):
    H, W, N, Cpix = 20, 12, 8, 3
    g = torch.Generator().manual_seed(2)
    flat = torch.randperm(2 * H * W, generator=g)[:60]
    coords = torch.stack((flat // (H * W), (flat % (H * W)) // W, flat % W), 1).to(torch.int32)
    coords = torch.cat((coords, torch.tensor([[0, 0, 0], [0, H - 1, W - 1], [1, 0, W - 1], [1, H - 1, 0]], dtype=torch.int32)))
    coords = torch.unique(coords, dim=0)
    if dups:
        coords = torch.cat((coords, coords[[3, 10, 3]]))
    values = torch.rand(coords.shape[0], Cpix, generator=g) * 100 + 1
    e0 = torch.randn(2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, N, generator=g)
    w0 = torch.randn(N, Cpix, 7, 7, generator=g)
    return (H, W), coords, values, e0, w0


@pytest.mark.parametrize("value_mode", [0, 1, 2])
def test_reference_gather_is_the_autograd_of_conv2d_on_a_scattered_map(value_mode):
    shape, coords, values, e0, w0 = _case()
    ref = R.gather(e0, w0, coords, values, shape, value_mode)
    auto = R.gather_autograd(e0, w0, coords, values, shape, value_mode)
    assert torch.allclose(ref, auto, rtol=1e-11, atol=1e-13)
    assert (ref != 0).all()


def test_reference_gather_gives_a_duplicated_pixel_to_its_highest_entry():
    shape, coords, values, e0, w0 = _case(dups=True)
    n = coords.shape[0] - 3
    own = torch.tensor(R.owners(coords, 2, *shape))
    assert own.tolist() == [i not in (3, 10, n) for i in range(n + 3)]          # entry n repeats 3 and loses to n + 2
    ref = R.gather(e0, w0, coords, values, shape, 1)
    assert (ref[~own] == 0).all() and (ref[own] != 0).all()
    auto = R.gather_autograd(e0, w0, coords[own], values[own], shape, 1)
    assert torch.allclose(ref[own], auto, rtol=1e-11, atol=1e-13)
    with pytest.raises(ValueError):
        R.gather(e0, w0, coords, values, shape, 3)


def test_midpoint_weights_and_completeness_arithmetic():
    from transformercvn.hip import gradients
    for steps in (1, 4, 32):
        aw = gradients.ig_alphas(steps)
        assert aw == R.ig_weights(steps) and len(aw) == steps
        assert math.isclose(sum(w for _, w in aw), 1.0, rel_tol=1e-15)
        assert aw[0][0] == 0.5 / steps and aw[-1][0] == (steps - 0.5) / steps
    # F(x) = sum x^2: the gradient is linear along the path, so the midpoint rule is exact and attribution_i = x_i^2
    x = [torch.tensor([[1.0, -2.0, 3.0]], dtype=torch.float64), torch.tensor([[0.5, 4.0, 0.0], [2.0, 2.0, 2.0]], dtype=torch.float64)]
    attr = R.integrated_gradients(lambda vs: [2 * v for v in vs], x, 3)
    assert all(torch.allclose(a, v.double() ** 2, rtol=1e-14) for a, v in zip(attr, x))
    ev_attr = torch.tensor([[1.0, 2.0, 3.0], [0.5, 0.5, 0.0], [1.0, 0.0, 0.0]])
    pr_attr = torch.tensor([[0.25, 0.0, 0.0], [0.0, 1.0, 1.0]])
    ev_img, pr_event = torch.tensor([0, 1, 1], dtype=torch.int32), torch.tensor([1, 0])
    value, base = torch.tensor([8.5, 2.0], dtype=torch.float64), torch.tensor([0.25, 0.5], dtype=torch.float64)
    gap = gradients.completeness_gap(ev_attr, pr_attr, ev_img, pr_event, value, base)
    assert torch.allclose(gap, torch.tensor([abs(8.0 - 8.25), abs(2.25 - 1.5)], dtype=torch.float64))
    assert torch.allclose(gap, R.completeness_gap(ev_attr, pr_attr, ev_img, pr_event, value, base))


@pytest.mark.parametrize("tile,reduce", [((1, 1), "sum"), ((4, 3), "sum"), ((4, 3), "abs"), ((16, 16), "abs")])
def test_heatmap_painting_and_nan_slots(tile, reduce):
    from transformercvn.hip import gradients
    g = torch.Generator().manual_seed(6)
    shape = (10, 7)
    mask = torch.tensor([[True, False, True], [False, False, True]])
    ev_c = torch.tensor([[0, 0, 0], [0, 9, 6], [1, 4, 4], [1, 4, 5], [1, 5, 4]], dtype=torch.int32)
    pr_c = torch.tensor([[0, 1, 1], [0, 2, 2], [1, 9, 0], [2, 0, 6], [2, 3, 3], [2, 3, 4]], dtype=torch.int32)
    ev_a, pr_a = torch.randn(5, 3, generator=g), torch.randn(6, 3, generator=g)
    got = gradients.heatmap(ev_a, pr_a, ev_c, pr_c, mask, shape, tile, reduce)
    ref = R.heatmap(ev_a, pr_a, ev_c, pr_c, mask, shape, tile, reduce)
    assert got.shape == ref.shape == (2, 4, -(-10 // tile[0]), -(-7 // tile[1]))
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.isnan(got[0, 2]).all() and torch.isnan(got[1, 1:3]).all()
    assert torch.allclose(torch.nan_to_num(got).double(), torch.nan_to_num(ref), rtol=1e-6, atol=1e-7)
    res = gradients.HitGradients(None, None, ev_a, pr_a, ev_a, pr_a, ev_c, pr_c, mask, shape, "gradient")
    assert torch.equal(torch.nan_to_num(res.heatmap(tile, reduce)), torch.nan_to_num(got))
    with pytest.raises(ValueError):
        res.heatmap((0, 1))
    with pytest.raises(ValueError):
        res.heatmap((1, 1), "max")


def test_argument_checks_come_before_any_device_work():
    from model_utils import build_trainer
    cfg = O.tutorial_config(densenet_structure=[2, 2], densenet_growth_rate=8, initial_pixel_dim=16, num_encoder_layers=2,
                            pixel_embedding_dim=64, hidden_dim=64, num_prong_decoder_layers=3)
    batch = O.synthetic_batch([2, 1], 3, cfg)
    model = build_trainer(cfg, None, device=None)
    model.train()
    with pytest.raises(RuntimeError, match=r"hit_gradients .* call \.eval\(\) first"):
        model.hit_gradients(*batch[:8])
    with pytest.raises(RuntimeError, match=r"hit_gradients .* call \.eval\(\) first"):
        model.network.hit_gradients(*model._network_inputs(*batch[:8]))
    model.eval()
    for bad in (dict(steps=0), dict(steps=2.5), dict(steps=True), dict(method="smooth"), dict(value="odds"), dict(target="track"),
                dict(target=-1), dict(target=1.5), dict(target=(torch.zeros(2, 4),)), dict(target=torch.zeros(2))):
        with pytest.raises(ValueError):
            model.hit_gradients(*batch[:8], **bad)
        with pytest.raises(ValueError):
            model.network.hit_gradients(*model._network_inputs(*batch[:8]), None, **bad)


def test_one_hot_pixels_have_no_gradient():
    from transformercvn.hip import gradients
    from transformercvn.hip.pixels import SparsePixels, VALUE_ONE_HOT
    with pytest.raises(ValueError, match="one-hot"):
        gradients.check_args("event", "prob", "gradient", 32, one_hot=True)
    from model_utils import build_trainer
    cfg = O.tutorial_config(densenet_structure=[2, 2], densenet_growth_rate=8, initial_pixel_dim=16, num_encoder_layers=2,
                            pixel_embedding_dim=64, hidden_dim=64, num_prong_decoder_layers=3)
    batch = O.synthetic_batch([2, 1], 3, cfg)
    model = build_trainer(cfg, None, device=None)
    model.eval()
    f, x, ev_px, em, pr_px, pm = model._network_inputs(*batch[:8])
    hot = SparsePixels(ev_px.coords, ev_px.values, ev_px.shape, VALUE_ONE_HOT)
    with pytest.raises(ValueError, match="one-hot"):
        model.network.hit_gradients(f, x, hot, em, pr_px, pm)


def test_sdxl_network_has_no_hit_gradients():
    """The SDXL embedder has neither a frozen forward nor a data-only backward: hit_gradients says so before any device work."""
    from model_utils import build_trainer
    cfg = O.tutorial_config(embedder="sdxl", initial_pixel_dim=8, pixel_embedding_dim=64, hidden_dim=64, num_encoder_layers=2)
    batch = O.synthetic_batch([2, 1], 3, cfg)
    model = build_trainer(cfg, None, device=None)
    model.eval()
    with pytest.raises(NotImplementedError, match="SDXL"):
        model.hit_gradients(*batch[:8])
