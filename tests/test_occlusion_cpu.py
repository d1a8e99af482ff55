"""Occlusion maps, host side: argument and mode errors are raised before any device work, the heat map of a hand-made result on the
host reports that it runs on the GPU only, and the C ABI of the scan is declared and exported."""
import ctypes
import os
import re

import pytest
import torch

from oracle import tcvn_oracle as O
from model_utils import build_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tcvn_occlusion_workspace_bytes", "tcvn_occlusion_variants", "tcvn_occlusion_build_pass",
           "tcvn_head_occlusion_workspace_bytes", "tcvn_head_occlusion", "tcvn_occlusion_heatmap"]


def small():
    cfg = O.tutorial_config(densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64,
                            num_encoder_layers=1, pixel_noise_std=0.0)
    return cfg, build_trainer(cfg, None, device=None), O.synthetic_batch([2, 1], 3, cfg, event_hits=(5, 9), prong_hits=(2, 4))[:8]


def test_train_mode_raises_before_any_device_work():
    cfg, model, batch = small()
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.occlusion_maps(*batch)
    net = model.network
    with pytest.raises(RuntimeError, match="eval"):
        net.occlusion_maps(*model._network_inputs(*batch))
    assert net._runtime is None, "the runtime (native plans) must not have been created"


@pytest.mark.parametrize("kw", [dict(tile=(0, 16)), dict(tile=(16, -1)), dict(tile=16), dict(tile=(16, 16, 16)), dict(tile=(16.0, 16)),
                                dict(tile=(True, 16)), dict(maps="prong"), dict(maps=None), dict(max_maps_per_pass=0),
                                dict(max_maps_per_pass=257), dict(max_maps_per_pass=8.0)])
def test_bad_arguments_raise_value_error_before_any_device_work(kw):
    cfg, model, batch = small()
    model.eval()
    with pytest.raises(ValueError):
        model.occlusion_maps(*batch, **kw)
    with pytest.raises(ValueError):
        model.network.occlusion_maps(*model._network_inputs(*batch), None, **kw)
    assert model.network._runtime is None
    model.train()                       # a bad argument is reported as such in either mode
    with pytest.raises(ValueError):
        model.occlusion_maps(*batch, **kw)


def test_check_args_accepts_the_documented_forms():
    from transformercvn.hip import occlusion
    assert occlusion.check_args((16, 16), "all", 256) == ((16, 16), "all", 256)
    assert occlusion.check_args([400, 280], "event", 1) == ((400, 280), "event", 1)
    assert occlusion.check_args((1, 7), "prongs", 8) == ((1, 7), "prongs", 8)
    assert occlusion.MAX_MAPS_PER_PASS == 256


def hand_made():
    from transformercvn.hip.occlusion import OcclusionResult
    g = torch.Generator().manual_seed(1)
    ev, pr = torch.randn(2, 4, generator=g), torch.randn(2, 3, 5, generator=g)
    index = torch.tensor([[0, 0, 0, 1], [0, 2, 1, 0], [1, 0, 1, 1]], dtype=torch.int32)
    return OcclusionResult(ev, pr, index, torch.randn(3, 4, generator=g), torch.randn(3, 3, 5, generator=g), (2, 2), (200, 140))


def test_heatmap_on_the_host_is_gpu_only_and_validates_its_target():
    from transformercvn.hip import occlusion
    res = hand_made()
    assert res.num_variants == 3 and res.grid == (2, 2) and res.tile == (200, 140)
    for target in ("event", "prong", 2, torch.tensor([1, 3])):
        with pytest.raises(RuntimeError, match="GPU only"):
            occlusion.heatmap(res, target)
    with pytest.raises(RuntimeError, match="GPU only"):
        res.heatmap()
    for target in ("events", 4, -1, 1.5, torch.tensor([1, 2, 3]), torch.tensor([0, 4]), torch.tensor([[0, 1]])):
        with pytest.raises(ValueError):
            occlusion.heatmap(res, target)


def test_occlusion_symbols_are_declared_and_exported():
    from transformercvn.hip import _lib
    header = open(os.path.join(ROOT, "include", "tcvn_hip.h")).read()
    declared = set(re.findall(r"\b(tcvn_[a-z0-9_]+)\s*\(", header))
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(dll, name), name
        assert name in _lib.EXPORTS, name
    assert re.search(r"#define\s+TCVN_OCC_MAX_PASS\s+256\b", header) and _lib.OCC_MAX_PASS == 256


def test_native_calls_reject_bad_arguments_before_any_device_call(capfd):
    """NULL pointers, tile < 1, max_pass outside 1..256: non-zero and one 'tcvn:' line, on a machine without a GPU too."""
    from transformercvn.hip._lib import lib
    assert lib.tcvn_occlusion_workspace_bytes(3, 400, 280, 0, 16, 256) == -1
    assert lib.tcvn_occlusion_workspace_bytes(3, 400, 280, 16, 16, 257) == -1
    assert lib.tcvn_occlusion_workspace_bytes(0, 400, 280, 16, 16, 256) == -1
    assert lib.tcvn_occlusion_workspace_bytes(3, 400, 280, 16, 16, 256) > 3 * 25 * 18 * 4
    host = (ctypes.c_int64 * 16)()
    assert lib.tcvn_occlusion_variants(None, 5, 1, 400, 280, 16, 16, None, 256, None, None, None, 0, host, 16, None) != 0
    assert lib.tcvn_occlusion_build_pass(None, None, 0, 3, 1, 400, 280, 16, 16, 256, None, None, 0, 0, 1, None, None, 0, None) != 0
    assert lib.tcvn_head_occlusion(None, 1, 1, 1, None, None, None, 1, None, None, 0, None, 0, 0, 1, None, None, None, 0, None) != 0
    assert lib.tcvn_head_occlusion_workspace_bytes(None, 4) == -1
    assert lib.tcvn_occlusion_heatmap(None, None, None, None, None, 1, 1, 0, 4, 4, 2, 2, 7, None, None, None) != 0
    err = capfd.readouterr().err
    assert err.count("tcvn:") == 4, err
