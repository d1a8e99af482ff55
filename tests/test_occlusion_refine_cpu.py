"""Coarse-to-fine occlusion maps, host side: the C ABI is declared and exported by both libraries and rejects bad arguments before any
device call, argument and mode errors of the public calls are raised before any device work, and the host reference (selection rule,
child list, painting) is itself checked: with keep = 0 it must reproduce the flat variant lists counted from the fixtures."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import load_case
from model_utils import build_trainer
import occlusion_reference as R
import occlusion_refine_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tcvn_occlusion_select", "tcvn_occlusion_refine_variants", "tcvn_occlusion_mark", "tcvn_occlusion_occupancy",
           "tcvn_occlusion_paint"]


def small():
    cfg = O.tutorial_config(densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64,
                            num_encoder_layers=1, pixel_noise_std=0.0)
    return cfg, build_trainer(cfg, None, device=None), O.synthetic_batch([2, 1], 3, cfg, event_hits=(5, 9), prong_hits=(2, 4))[:8]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_refine_symbols_are_declared_and_exported_by_both_libraries():
    from transformercvn.hip import _lib
    header = open(os.path.join(ROOT, "include", "tcvn_hip.h")).read()
    declared = set(re.findall(r"\b(tcvn_[a-z0-9_]+)\s*\(", header))
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    for so in ("libtcvn_hip.so", "libtcvn_hip_dbg.so"):
        dll = ctypes.CDLL(os.path.join(lib_dir, so))
        for name in SYMBOLS:
            assert hasattr(dll, name), (so, name)
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
    assert re.search(r"#define\s+TCVN_OCC_MAX_LEVELS\s+16\b", header) and _lib.OCC_MAX_LEVELS == 16
    assert re.search(r"#define\s+TCVN_OCC_GROUP_EVENT\s+0\b", header) and _lib.OCC_GROUP_EVENT == 0
    assert re.search(r"#define\s+TCVN_OCC_GROUP_MAP\s+1\b", header) and _lib.OCC_GROUP_MAP == 1


def test_native_refine_calls_reject_bad_arguments_before_any_device_call(capfd):
    """Every pointer below is NULL or a host array: a call that got as far as the device would fail differently, or crash."""
    from transformercvn.hip._lib import lib
    host = (ctypes.c_int64 * 16)()
    one = ctypes.c_void_p(1)              # a non-NULL pointer that is never dereferenced: the argument check comes first
    assert lib.tcvn_occlusion_select(None, None, 1, 1, 0, 2, 2, 0, 0.25, None, None, None) != 0
    assert lib.tcvn_occlusion_select(one, one, 1, 1, 0, 2, 2, 0, 1.5, one, one, None) != 0                     # keep > 1
    assert lib.tcvn_occlusion_select(one, one, 1, 1, 0, 2, 2, 0, float("nan"), one, one, None) != 0            # keep NaN
    assert lib.tcvn_occlusion_select(one, one, 1, 1, 0, 2, 2, 2, 0.25, one, one, None) != 0                    # unknown group
    # no keep_map; then a parent grid that is not the grid of 32x32 tiles on a 400x280 map (13 x 9)
    assert lib.tcvn_occlusion_refine_variants(one, 5, 1, 400, 280, 16, 16, one, None, 1, 0, 13, 9, 256, one, one, one, 1 << 20, host, 16,
                                              None) != 0
    assert lib.tcvn_occlusion_refine_variants(one, 5, 1, 400, 280, 16, 16, one, one, 1, 0, 25, 18, 256, one, one, one, 1 << 20, host, 16,
                                              None) != 0
    # the checks it shares with tcvn_occlusion_variants: max_pass outside 1..256
    assert lib.tcvn_occlusion_refine_variants(one, 5, 1, 400, 280, 16, 16, one, one, 1, 0, 13, 9, 257, one, one, one, 1 << 20, host, 16,
                                              None) != 0
    assert lib.tcvn_occlusion_mark(None, 1, 1, 0, 2, 2, None, None) != 0
    assert lib.tcvn_occlusion_occupancy(None, 5, 1, 400, 280, 16, 16, None, 1, 0, None, None) != 0
    heat = (ctypes.c_void_p * 2)(1, 1)
    gh, gw = (ctypes.c_int * 2)(7, 13), (ctypes.c_int * 2)(5, 9)
    assert lib.tcvn_occlusion_paint(0, heat, heat, gh, gw, one, 1, 0, one, None) != 0                           # levels < 1
    assert lib.tcvn_occlusion_paint(17, heat, heat, gh, gw, one, 1, 0, one, None) != 0                          # levels > 16
    assert lib.tcvn_occlusion_paint(2, heat, heat, gh, gw, None, 1, 0, one, None) != 0                          # no occupancy
    bad = (ctypes.c_int * 2)(6, 13)                                                                             # ceil(13 / 2) is 7
    assert lib.tcvn_occlusion_paint(2, heat, heat, bad, gw, one, 1, 0, one, None) != 0
    err = capfd.readouterr().err
    assert err.count("tcvn:") == 13, err


# ---- the public calls ----------------------------------------------------------------------------------------------------------------------
BAD = [dict(levels=0), dict(levels=-1), dict(levels=2.0), dict(levels=True), dict(levels=17), dict(tile=(64, 64), levels=8),
       dict(tile=(64, 60), levels=4), dict(tile=(6, 64), levels=3), dict(keep=-0.1), dict(keep=1.5), dict(keep=float("nan")),
       dict(keep="0.25"), dict(keep=None), dict(keep=True), dict(target="events"), dict(target=1.5), dict(target=-1), dict(target=None),
       dict(target=torch.tensor([0.5, 1.0])), dict(target=torch.tensor([[0, 1]])), dict(max_variants=0), dict(max_variants=-5),
       dict(max_variants=10.0), dict(max_variants=True),
       # explicit classes the model does not have, or not one per event (two events)
       dict(target=99), dict(target=torch.tensor([0, 99])), dict(target=torch.tensor([0, 1, 2])),
       # everything check_args rejects
       dict(tile=(0, 16)), dict(tile=16), dict(tile=(16.0, 16)), dict(maps="prong"), dict(maps=None), dict(max_maps_per_pass=0),
       dict(max_maps_per_pass=257)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(k) for k in BAD])
def test_bad_arguments_raise_value_error_before_any_device_work(kw):
    cfg, model, batch = small()
    model.eval()
    with pytest.raises(ValueError):
        model.occlusion_refine(*batch, **kw)
    with pytest.raises(ValueError):
        model.network.occlusion_refine(*model._network_inputs(*batch), None, **kw)
    assert model.network._runtime is None, "the runtime (native plans) must not have been created"
    model.train()                       # a bad argument is reported as such in either mode
    with pytest.raises(ValueError):
        model.occlusion_refine(*batch, **kw)


def test_train_mode_raises_before_any_device_work():
    cfg, model, batch = small()
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.occlusion_refine(*batch)
    with pytest.raises(RuntimeError, match="eval"):
        model.network.occlusion_refine(*model._network_inputs(*batch))
    assert model.network._runtime is None


def test_check_refine_args_accepts_the_documented_forms():
    from transformercvn.hip import occlusion
    assert occlusion.check_refine_args((64, 64), 3, 0.25, "event", "all", 256, None) == ((64, 64), 3, 0.25, "all", 256, None)
    assert occlusion.check_refine_args([64, 32], 4, 0, "prong", "event", 8, 1000) == ((64, 32), 4, 0.0, "event", 8, 1000)
    assert occlusion.check_refine_args((7, 5), 1, 1, 2, "prongs", 1, 1) == ((7, 5), 1, 1.0, "prongs", 1, 1)
    assert occlusion.check_refine_args((64, 64), 7, 0.5, torch.tensor([1, 0, 2]), "all", 256, None)[1] == 7
    assert occlusion.MAX_LEVELS == 16


def test_parse_target_checks_explicit_classes_against_the_model():
    from transformercvn.hip import occlusion
    for target in (4, torch.tensor([0, 4]), torch.tensor([1, 2, 3])):
        with pytest.raises(ValueError):
            occlusion.parse_target(target, 2, 4)
    assert occlusion.parse_target(3, 2, 4)[1].tolist() == [3, 3]
    assert occlusion.parse_target("prong", 2, 4)[1] is None


def test_refined_heatmap_on_the_host_is_gpu_only():
    from transformercvn.hip.occlusion import OcclusionResult, RefinedOcclusion, refined_heatmap
    ev, pr = torch.zeros(1, 4), torch.zeros(1, 1, 5)
    index = torch.tensor([[0, 0, 0, 0]], dtype=torch.int32)
    level = OcclusionResult(ev, pr, index, torch.zeros(1, 4), torch.zeros(1, 1, 5), (1, 1), (400, 280))
    res = RefinedOcclusion(ev, pr, [level], [torch.zeros(1, 2, 1, 1)], [torch.ones(1, 2, 1, 1, dtype=torch.uint8)],
                           torch.ones(1, 2, 1, 1, dtype=torch.uint8), "event", 0.25, None)
    assert res.num_variants == 1 and res.stopped_at is None and res.keep == 0.25 and res.target == "event"
    with pytest.raises(RuntimeError, match="GPU only"):
        res.heatmap()
    empty = RefinedOcclusion(ev, pr, [], [], [], None, "event", 0.25, 0)
    with pytest.raises(ValueError):
        refined_heatmap(empty)


# ---- the host reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, counts", [("small_b3", (301, 927, 2439, 4411)), ("tutorial_ragged", (839, 2552, 6172, 9922))])
def test_reference_with_keep_0_is_the_flat_list_at_every_level(name, counts):
    """Tiles (64, 64) -> (8, 8); the figures were counted from the fixtures on the host."""
    cfg, over, batch, g = load_case(name)
    shape = cfg.pixel_shape
    levels = RR.keep0_levels(batch, (64, 64), 4, shape)
    for lv, index in enumerate(levels):
        tile = RR.level_tile((64, 64), lv)
        assert tile == (64 >> lv, 64 >> lv)
        assert torch.equal(index, R.expected_index(batch, tile, shape)), (name, tile)
    assert tuple(i.shape[0] for i in levels) == counts


def test_reference_selection_rule():
    """Two events, two maps each, a 1 x 4 grid.  Event target: the maps of an event compete; prong target: every map on its own."""
    heat = np.zeros((2, 2, 1, 4), dtype=np.float32)
    heat[0, 0, 0] = [0.8, -0.4, 0.1, 0.0]
    heat[0, 1, 0] = [0.2, 0.19, 0.0, 0.0]
    heat[1, 0, 0] = [0.0, 0.0, 0.0, 0.0]
    index = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3], [0, 1, 0, 0], [0, 1, 0, 1], [1, 0, 0, 0], [1, 0, 0, 2]],
                         dtype=torch.int32)
    # keep 0.25, event groups: bound 0.2 for event 0 -> 0.8, 0.4 and the 0.2 of map 1 (0.2 >= float32(0.25) * float32(0.8) exactly: both
    # sides are the float32 nearest to 0.2); event 1 is all zeros: nothing (score > 0 is required when keep > 0)
    assert RR.selected_rows(heat, index, 0.25, "event").tolist() == [True, True, False, False, True, False, False, False]
    # map groups: map (0, 1) has its own maximum 0.2 -> bound 0.05: both of its variants
    assert RR.selected_rows(heat, index, 0.25, "prong").tolist() == [True, True, False, False, True, True, False, False]
    # keep 0: everything, zeros included; keep 1: the maxima alone
    assert RR.selected_rows(heat, index, 0.0, "event").all()
    assert RR.selected_rows(heat, index, 1.0, "event").tolist() == [True] + [False] * 7


def test_reference_child_list_and_painting_on_a_hand_made_example():
    """One event, one prong, an 8 x 8 map, tiles 4 -> 2 -> 1.  Event map hits: (0,0) (1,3) (5,5) (7,0); prong map hit: (2,2)."""
    shape = (8, 8)
    ec = torch.tensor([[0, 0, 0], [0, 1, 3], [0, 5, 5], [0, 7, 0]], dtype=torch.int32)
    pc = torch.tensor([[0, 2, 2]], dtype=torch.int32)
    batch = (None, None, ec, None, None, pc, None, torch.ones(1, 1, dtype=torch.bool))
    i0 = R.expected_index(batch, (4, 4), shape)
    assert i0.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1], [0, 1, 0, 0]]
    # level 0: refine (0,0,0,0) and the prong tile, not the two others of the event map
    i1 = RR.child_index(batch, i0, [True, False, False, True], (2, 2), shape)
    assert i1.tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1]]          # children with hits: (0,0)->(0,0); (1,3)->(0,1); prong (2,2)->(1,1)
    # level 1: refine only (0,0,0,1)
    i2 = RR.child_index(batch, i1, [False, True, False], (1, 1), shape)
    assert i2.tolist() == [[0, 0, 1, 3]]
    heats = [torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 8, 8)]
    heats[0][0, 0] = torch.tensor([[0.5, 9.0], [0.25, -0.125]])               # 9.0 sits on a tile without hits: never evaluated
    heats[0][0, 1, 0, 0] = 0.75
    heats[1][0, 0, 0, 0], heats[1][0, 0, 0, 1], heats[1][0, 1, 1, 1] = 0.3, 0.2, -0.6
    heats[2][0, 0, 1, 3] = 0.1
    heats[2][0, 0, 0, 0] = 7.0                                                # stored, but not an evaluated variant of level 2
    occ = RR.occupied_cells(batch, (1, 1), shape)
    assert occ.sum() == 5
    out = RR.paint(heats, [i0, i1, i2], occ)
    want = torch.zeros(1, 2, 8, 8)
    want[0, 0, 0, 0] = 0.3            # deepest evaluated tile that holds (0,0): level 1 (0,0)
    want[0, 0, 1, 3] = 0.1            # level 2
    want[0, 0, 5, 5] = -0.125         # never refined: level 0 tile (1,1)
    want[0, 0, 7, 0] = 0.25           # level 0 tile (1,0)
    want[0, 1, 2, 2] = -0.6           # level 1 (1,1) of the prong map
    assert torch.equal(out, want)
    # painting on a coarser last level: cells are the 2x2 tiles
    out1 = RR.paint(heats[:2], [i0, i1], RR.occupied_cells(batch, (2, 2), shape))
    want1 = torch.zeros(1, 2, 4, 4)
    want1[0, 0, 0, 0], want1[0, 0, 0, 1], want1[0, 0, 2, 2], want1[0, 0, 3, 0], want1[0, 1, 1, 1] = 0.3, 0.2, -0.125, 0.25, -0.6
    assert torch.equal(out1, want1)
