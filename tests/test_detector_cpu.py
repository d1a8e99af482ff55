"""Detector-effect scans, host side: argument and mode errors are raised before any device work, the response of a hand-made result on
the host reports that it runs on the GPU only, the C ABI is declared, exported and rejects bad arguments, and the host reference of one
effect (detector_reference.apply_effect) does what the documented order says on a hand-written list."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import tcvn_oracle as O
from model_utils import build_trainer
import detector_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tcvn_detector_workspace_bytes", "tcvn_detector_variants", "tcvn_detector_build_pass", "tcvn_detector_response"]
SMALL = dict(densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64, num_encoder_layers=1,
             pixel_noise_std=0.0)


def small(**over):
    cfg = O.tutorial_config(**dict(SMALL, **over))
    assert tuple(cfg.pixel_shape) == (400, 280)
    return cfg, build_trainer(cfg, None, device=None), O.synthetic_batch([2, 1], 3, cfg, event_hits=(5, 9), prong_hits=(2, 4))[:8]


def E(**kw):
    from transformercvn.hip.detector import DetectorEffect
    return DetectorEffect(**kw)


def test_effect_defaults_are_the_identity_and_frozen():
    import dataclasses
    e = E()
    assert dataclasses.asdict(e) == dict(scale=1.0, threshold=0.0, dead_rows=None, dead_cols=None, drop=0.0, shift=(0, 0), seed=0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        e.scale = 2.0


def bad_calls():
    ok = [E()]
    return {
        "no effects": dict(effects=[]), "65 effects": dict(effects=[E()] * 65), "effects None": dict(effects=None),
        "not an effect": dict(effects=[dict(scale=1.0)]), "one effect, not a list": dict(effects=E()),
        "scale negative": dict(effects=[E(scale=-0.5)]), "scale inf": dict(effects=[E(scale=float("inf"))]),
        "scale NaN": dict(effects=[E(scale=float("nan"))]), "scale beyond float32": dict(effects=[E(scale=1e39)]),
        "scale str": dict(effects=[E(scale="1")]), "scale beyond any float": dict(effects=[E(scale=10 ** 400)]),
        "threshold beyond any float": dict(effects=[E(threshold=10 ** 400)]),
        "threshold negative": dict(effects=[E(threshold=-1.0)]), "threshold inf": dict(effects=[E(threshold=float("inf"))]),
        "drop negative": dict(effects=[E(drop=-0.1)]), "drop above 1": dict(effects=[E(drop=1.5)]), "drop NaN": dict(effects=[E(drop=float("nan"))]),
        "dead_rows reversed": dict(effects=[E(dead_rows=(10, 5))]), "dead_rows beyond the map": dict(effects=[E(dead_rows=(0, 401))]),
        "dead_rows negative": dict(effects=[E(dead_rows=(-1, 5))]), "dead_rows not a pair": dict(effects=[E(dead_rows=(1, 2, 3))]),
        "dead_cols beyond the map": dict(effects=[E(dead_cols=(0, 281))]), "dead_cols float": dict(effects=[E(dead_cols=(0.0, 4.0))]),
        "shift too far": dict(effects=[E(shift=(0, 32768))]), "shift float": dict(effects=[E(shift=(0.5, 0))]),
        "shift not a pair": dict(effects=[E(shift=4)]),
        "seed negative": dict(effects=[E(seed=-1)]), "seed 2^63": dict(effects=[E(seed=2 ** 63)]), "seed float": dict(effects=[E(seed=1.0)]),
        "scope": dict(effects=ok, scope="prong"), "scope None": dict(effects=ok, scope=None),
        "maps": dict(effects=ok, maps="prong"), "max_maps_per_pass 0": dict(effects=ok, max_maps_per_pass=0),
        "max_maps_per_pass 257": dict(effects=ok, max_maps_per_pass=257),
        "a later effect": dict(effects=[E(), E(scale=0.9), E(drop=2.0)]),
    }


@pytest.mark.parametrize("case", sorted(bad_calls()))
def test_bad_arguments_raise_value_error_before_any_device_work(case):
    cfg, model, batch = small()
    kw = bad_calls()[case]
    model.eval()
    with pytest.raises(ValueError):
        model.detector_scan(*batch, **kw)
    with pytest.raises(ValueError):
        model.network.detector_scan(*model._network_inputs(*batch), None, **kw)
    assert model.network._runtime is None, "the runtime (native plans) must not have been created"
    model.train()                       # a bad argument is reported as such in either mode
    with pytest.raises(ValueError):
        model.detector_scan(*batch, **kw)


@pytest.mark.parametrize("effect", [dict(scale=0.95), dict(threshold=20.0), dict(scale=1.0 + 1e-6, drop=0.1)])
def test_one_hot_pixels_refuse_scale_and_threshold(effect):
    from transformercvn.hip import detector
    cfg, model, batch = small(one_hot_pixels=True)
    model.eval()
    with pytest.raises(ValueError, match="one-hot"):
        model.detector_scan(*batch, effects=[E(), E(**effect)])
    with pytest.raises(ValueError, match="one-hot"):
        model.network.detector_scan(*model._network_inputs(*batch), None, [E(**effect)])
    assert model.network._runtime is None
    # the geometric effects and drop stay available
    geometric = [E(dead_cols=(120, 136)), E(drop=0.05, seed=1), E(shift=(0, 4)), E(dead_rows=(0, 400)), E(scale=1.0, threshold=0.0)]
    assert detector.check_args(geometric, "event", "all", 256, (400, 280), one_hot=True)[0] == tuple(geometric)


def test_check_args_accepts_the_documented_forms():
    from transformercvn.hip import detector
    effects = [E(scale=0.95), E(threshold=20.0), E(dead_cols=(120, 136)), E(drop=0.05, seed=1), E(shift=(0, 4)), E(), E(scale=0, drop=1),
               E(dead_rows=(0, 400), dead_cols=(280, 280), shift=(-32767, 32767), seed=2 ** 63 - 1), E(scale=2, threshold=3)]
    assert detector.check_args(effects, "event", "all", 256, (400, 280)) == (tuple(effects), "event", "all", 256)
    assert detector.check_args(tuple(effects[:1]) * 64, "map", "prongs", 1, (400, 280))[1:] == ("map", "prongs", 1)
    assert (detector.MAX_EFFECTS, detector.SCOPES) == (64, ("event", "map"))
    table = detector.effect_table(effects)
    assert len(table) == len(effects) and ctypes.sizeof(table) == 48 * len(effects)
    assert (table[2].dead_x0, table[2].dead_x1, table[2].dead_y0, table[2].dead_y1) == (120, 136, 0, 0)
    assert table[0].scale == np.float32(0.95) and table[3].seed == 1 and (table[4].shift_y, table[4].shift_x) == (0, 4)
    assert table[7].seed == 2 ** 63 - 1 and (table[7].shift_y, table[7].shift_x) == (-32767, 32767)


def test_train_mode_raises_before_any_device_work_and_value_error_comes_before_the_gpu_guard():
    cfg, model, batch = small()
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.detector_scan(*batch, effects=[E(scale=0.95)])
    with pytest.raises(RuntimeError, match="eval"):
        model.network.detector_scan(*model._network_inputs(*batch), None, [E(scale=0.95)])
    assert model.network._runtime is None, "the runtime (native plans) must not have been created"
    with pytest.raises(ValueError):                  # on CPU tensors: the argument error, not the GPU-only guard
        model.detector_scan(*batch, effects=[E(drop=7)])


def hand_made(scope):
    from transformercvn.hip.detector import DetectorScan
    g = torch.Generator().manual_seed(1)
    ev, pr = torch.randn(2, 4, generator=g), torch.randn(2, 3, 5, generator=g)
    valid = torch.tensor([[0, 0, 0, -1], [0, 0, -1, -1]], dtype=torch.int32)
    effects = (E(scale=0.9), E(drop=0.5))
    if scope == "event":
        return DetectorScan(ev, pr, effects, scope, valid, torch.randn(2, 2, 4, generator=g), torch.randn(2, 2, 3, 5, generator=g),
                            surviving=torch.zeros(2, 2, 4, dtype=torch.int32))
    index = torch.tensor([[0, 0, 0, 3], [0, 0, 1, 1], [1, 1, 0, 2], [1, 1, 1, 0]], dtype=torch.int32)
    return DetectorScan(ev, pr, effects, scope, valid, torch.randn(4, 4, generator=g), torch.randn(4, 3, 5, generator=g), index=index)


@pytest.mark.parametrize("scope", ["event", "map"])
def test_response_on_the_host_is_gpu_only_and_validates_its_target(scope):
    res = hand_made(scope)
    assert res.num_variants == 4 and res.scope == scope and len(res.effects) == 2
    for target in ("event", "prong", 2, torch.tensor([1, 3])):
        with pytest.raises(RuntimeError, match="GPU only"):
            res.response(target)
        with pytest.raises(RuntimeError, match="GPU only"):
            res.summary(target)
    for target in ("events", 4, -1, 1.5, torch.tensor([1, 2, 3]), torch.tensor([0, 4]), torch.tensor([[0, 1]])):
        with pytest.raises(ValueError):
            res.response(target)
    # the float64 formula on the same hand-made result: shapes and the NaN pattern
    prob, delta, flipped = DR.response_reference(res, "prong")
    if scope == "event":
        assert prob.shape == (2, 2, 3) and torch.equal(~torch.isnan(prob), (res.valid[:, 1:] >= 0).expand(2, 2, 3))
    else:
        assert prob.shape == (2, 2, 4) and int((~torch.isnan(prob)).sum()) == 2 and not bool(torch.isnan(prob[:, 1, 1]).any())
    assert not bool(flipped[torch.isnan(delta)].any())


@pytest.mark.parametrize("scope", ["event", "map"])
def test_response_reference_on_planted_rows(scope):
    """The float64 formula itself, by hand: a varied row equal to the base row gives delta 0 and no flip; the negated base row moves
    the arg-max to the base row's arg-min, so it flips, and prob is softmax(-base) at the base's predicted class."""
    res = hand_made(scope)
    ev, pr = res.event_logits, res.prong_logits
    if scope == "event":                     # setting 0 of event 0 unchanged, setting 1 of event 1 negated; its prong slot 0 likewise
        res.varied_event_logits[0, 0], res.varied_event_logits[1, 1] = ev[0], -ev[1]
        res.varied_prong_logits[0, 1, 0], res.varied_prong_logits[1, 1, 0] = pr[1, 0], -pr[1, 0]
        same, negated, p_same, p_negated = (0, 0), (1, 1), (0, 1, 0), (1, 1, 0)
    else:                                    # variants 0 = (b 0, s 0, k 0) and 3 = (b 1, s 1, k 1); prong rows of variants 2 and 3
        res.varied_event_logits[0], res.varied_event_logits[3] = ev[0], -ev[1]
        res.varied_prong_logits[2, 0], res.varied_prong_logits[3, 0] = pr[1, 0], -pr[1, 0]
        same, negated, p_same, p_negated = (0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 1, 1)
    prob, delta, flipped = DR.response_reference(res, "event")
    c = int(ev[1].argmax())
    assert delta[same] == 0 and not flipped[same] and flipped[negated] and delta[negated] < 0
    assert abs(float(prob[negated]) - float(torch.softmax(-ev[1].double(), 0)[c])) < 1e-15
    assert abs(float(prob[same]) - float(torch.softmax(ev[0].double(), 0)[int(ev[0].argmax())])) < 1e-15
    prob, delta, flipped = DR.response_reference(res, 2)                       # an explicit class: the flip is still the arg-max's
    assert delta[same] == 0 and not flipped[same] and flipped[negated]
    assert abs(float(prob[negated]) - float(torch.softmax(-ev[1].double(), 0)[2])) < 1e-15
    prob, delta, flipped = DR.response_reference(res, "prong")
    cp = int(pr[1, 0].argmax())
    assert delta[p_same] == 0 and not flipped[p_same] and flipped[p_negated] and delta[p_negated] < 0
    assert abs(float(prob[p_negated]) - float(torch.softmax(-pr[1, 0].double(), 0)[cp])) < 1e-15
    # the seeded random result of the GPU test holds both values of flipped, in both scopes and for both kinds of target
    rnd = DR.random_result(scope)
    for target in ("event", "prong"):
        p, d, f = DR.response_reference(rnd, target)
        there = ~torch.isnan(p)
        assert bool(f[there].any()) and not bool(f[there].all()) and not bool(f[~there].any()) and bool((~there).any()) == (scope == "map" or target == "prong")


def test_detector_symbols_are_declared_and_exported():
    from transformercvn.hip import _lib
    header = open(os.path.join(ROOT, "include", "tcvn_hip.h")).read()
    declared = set(re.findall(r"\b(tcvn_[a-z0-9_]+)\s*\(", header))
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(dll, name), name
        assert name in _lib.EXPORTS, name
    assert re.search(r"#define\s+TCVN_DET_MAX_EFFECTS\s+64\b", header) and _lib.DET_MAX_EFFECTS == 64
    assert re.search(r"#define\s+TCVN_DET_SCOPE_EVENT\s+0\b", header) and re.search(r"#define\s+TCVN_DET_SCOPE_MAP\s+1\b", header)
    assert (_lib.DET_SCOPE_EVENT, _lib.DET_SCOPE_MAP) == (0, 1)
    assert re.search(r"struct\s+tcvn_detector_effect\s*\{\s*float scale, threshold, drop;\s*int32_t dead_y0, dead_y1, dead_x0, dead_x1, "
                     r"shift_y, shift_x;\s*uint64_t seed;\s*\}", header)
    assert [f[0] for f in _lib.DetectorEffectC._fields_] == ["scale", "threshold", "drop", "dead_y0", "dead_y1", "dead_x0", "dead_x1",
                                                             "shift_y", "shift_x", "seed"]
    assert ctypes.sizeof(_lib.DetectorEffectC) == 48


def test_native_calls_reject_bad_arguments_before_any_device_call(capfd):
    """K outside 1..64, max_pass outside 1..256, NULL pointers, an effect out of range, an unknown scope or target: non-zero and one
    'tcvn:' line, on a machine without a GPU too."""
    from transformercvn.hip import _lib
    lib = _lib.lib
    wsb = lib.tcvn_detector_workspace_bytes
    assert wsb(5, 0, 256) < 0 and wsb(5, 65, 256) < 0 and wsb(5, 8, 0) < 0 and wsb(5, 8, 257) < 0 and wsb(0, 8, 256) < 0
    assert wsb(5, 64, 256) > 5 * 64 * 4 + 64 * 48 and wsb(1, 1, 1) > 0
    assert capfd.readouterr().err.count("tcvn:") == 0           # the workspace query answers silently, as the scans' do
    host = (ctypes.c_int64 * 16)()
    one = (ctypes.c_int32 * 16)()
    f = (ctypes.c_float * 16)()
    u8 = (ctypes.c_uint8 * 16)()
    good = (_lib.DetectorEffectC * 1)()
    good[0].scale = 1.0
    calls = 0
    # NULL pointers
    assert lib.tcvn_detector_variants(None, 5, 1, 40, 28, 3, None, None, good, 1, 256, None, None, None, 0, host, 16, None) != 0
    calls += 1
    # K = 0 and K = 65, then max_pass = 257, with every pointer set
    for K, max_pass in ((0, 256), (65, 256), (1, 257)):
        assert lib.tcvn_detector_variants(one, 1, 1, 40, 28, 3, f, one, good, K, max_pass, one, one, one, 64, host, 16, None) != 0
        calls += 1
    # one effect out of range each
    for field, value in (("scale", -1.0), ("scale", float("nan")), ("threshold", float("inf")), ("drop", 1.5), ("dead_y1", 41),
                         ("dead_x0", -1), ("shift_x", 40000)):
        bad = (_lib.DetectorEffectC * 1)()
        bad[0].scale = 1.0
        setattr(bad[0], field, value)
        assert lib.tcvn_detector_variants(one, 1, 1, 40, 28, 3, f, one, bad, 1, 256, one, one, one, 64, host, 16, None) != 0, field
        calls += 1
    bad = (_lib.DetectorEffectC * 1)()
    bad[0].scale, bad[0].dead_x0, bad[0].dead_x1 = 1.0, 9, 4
    assert lib.tcvn_detector_variants(one, 1, 1, 40, 28, 3, f, one, bad, 1, 256, one, one, one, 64, host, 16, None) != 0
    calls += 1
    # a workspace that is too small
    assert lib.tcvn_detector_variants(one, 1, 1, 40, 28, 3, f, one, good, 1, 256, one, one, one, 64, host, 16, None) != 0
    calls += 1
    assert lib.tcvn_detector_build_pass(None, None, 0, 3, 1, 40, 28, None, 1, 256, None, None, 0, 0, 1, None, None, 0, None) != 0
    assert lib.tcvn_detector_build_pass(one, f, 1, 1, 1, 40, 28, one, 4, 256, one, one, 64, 0, 5, one, f, 1, None) != 0      # beyond n_img * K
    assert lib.tcvn_detector_build_pass(one, f, 1, 1, 1, 40, 28, one, 65, 256, one, one, 64, 0, 1, one, f, 1, None) != 0
    calls += 3
    assert lib.tcvn_detector_response(None, None, None, None, None, 1, None, 1, 0, 4, 4, 1, 1, 0, None, None, None, None, None) != 0
    assert lib.tcvn_detector_response(f, f, f, f, one, 1, one, 1, 0, 4, 4, 1, 2, 0, None, f, f, u8, None) != 0           # unknown scope
    assert lib.tcvn_detector_response(f, f, f, f, one, 1, one, 1, 0, 4, 4, 1, 1, 7, None, f, f, u8, None) != 0           # unknown target
    assert lib.tcvn_detector_response(f, f, f, f, one, 1, one, 1, 0, 4, 4, 65, 1, 0, None, f, f, u8, None) != 0          # 65 effects
    assert lib.tcvn_detector_response(f, f, f, f, one, 1, one, 1, 1, 4, 4, 1, 1, 1, one, f, f, u8, None) != 0            # classes with "prong"
    assert lib.tcvn_detector_response(f, f, f, f, None, 3, one, 2, 0, 4, 4, 1, 0, 0, None, f, f, u8, None) != 0          # rows != K * B
    calls += 6
    err = capfd.readouterr().err
    assert err.count("tcvn:") == calls, err


# ---- the host reference of one effect ---------------------------------------------------------------------------------------------------
SHAPE = (8, 6)
HITS = torch.tensor([[0, 0, 0], [0, 2, 5], [0, 7, 1], [1, 3, 3], [1, 3, 3], [1, 5, 2]], dtype=torch.int32)        # (image, y, x)
VALUES = torch.tensor([[10., 200., 30.], [100., 100., 100.], [255., 0., 1.], [40., 50., 60.], [7., 8., 9.], [130., 20., 250.]])
BS = torch.tensor([[0, 0], [1, 2]], dtype=torch.int32)


def applied(**kw):
    at, c, v = DR.apply_effect(HITS, VALUES, BS, E(**kw), SHAPE)
    return at.tolist(), c.tolist(), v.tolist()


def test_apply_effect_on_six_hits():
    every = list(range(6))
    assert applied() == (every, HITS.tolist(), VALUES.tolist())
    # scale: one float32 multiplication, nothing removed
    at, c, v = applied(scale=0.5)
    assert at == every and c == HITS.tolist() and v == (VALUES * 0.5).tolist()
    # threshold 100: channels below it become 0; hit 3 and hit 4 lose every channel
    at, c, v = applied(threshold=100.0)
    assert at == [0, 1, 2, 5] and c == HITS[[0, 1, 2, 5]].tolist()
    assert v == [[0., 200., 0.], [100., 100., 100.], [255., 0., 0.], [130., 0., 250.]]
    # scale acts before the threshold: 0.5 * 200 = 100 survives, 0.5 * 100 = 50 does not
    at, c, v = applied(scale=0.5, threshold=100.0)
    assert at == [0, 2, 5] and v == [[0., 100., 0.], [127.5, 0., 0.], [0., 0., 125.]]
    # dead rows / columns are half-open ranges on the original coordinates; an empty range removes nothing
    assert applied(dead_rows=(2, 4))[0] == [0, 2, 5] and applied(dead_cols=(1, 3))[0] == [0, 1, 3, 4]
    assert applied(dead_rows=(3, 3), dead_cols=(0, 0))[0] == every and applied(dead_rows=(0, 8))[0] == []
    # shift: the window moves after the detector acted; hits that leave the 8 x 6 map are removed
    at, c, v = applied(shift=(1, -1))
    assert at == [1, 3, 4, 5] and c == [[0, 3, 4], [1, 4, 2], [1, 4, 2], [1, 6, 1]] and v == VALUES[[1, 3, 4, 5]].tolist()
    at, c, v = applied(dead_rows=(3, 4), shift=(-1, 0))            # row 3 is dead although it would have moved to row 2
    assert at == [1, 2, 5] and c == [[0, 1, 5], [0, 6, 1], [1, 4, 2]]
    # drop: 0 keeps and 1 removes every hit
    assert applied(drop=0.0, seed=5)[0] == every and applied(drop=1.0, seed=5)[0] == []


def test_the_synthetic_lists_of_the_gpu_tests_exercise_every_branch():
    """The exact comparisons of test_detector_gpu.py say something only if its seeded lists reach every branch of an effect: asserted
    on the host reference, here where no GPU is needed (the GPU file asserts it again in front of its kernels)."""
    import test_detector_gpu as G
    G.test_the_reference_exercises_every_branch()
    coords, values = G.synthetic_list()
    assert torch.bincount(coords[:, 0].long(), minlength=5).tolist() == list(G.COUNTS) and values.max() <= 255 and values.min() >= 0
    assert bool((coords[1:, 0] >= coords[:-1, 0]).all()) and torch.equal(values, values.round())


def test_drop_draws_belong_to_the_pixel_the_event_and_the_slot():
    y, x = HITS[:, 1].numpy(), HITS[:, 2].numpy()
    b, s = BS[HITS[:, 0].long(), 0].numpy(), BS[HITS[:, 0].long(), 1].numpy()
    u = DR.drop_draws(y, x, b, s, SHAPE[1], 9)
    assert u.dtype == np.float32 and bool(((u >= 0) & (u < 1)).all())
    assert u[3] == u[4], "two hits on one pixel share the draw"
    assert len(set(u.tolist())) == 5
    assert not np.array_equal(u, DR.drop_draws(y, x, b, s, SHAPE[1], 10)), "the seed enters"
    assert not np.array_equal(u, DR.drop_draws(y, x, b + 1, s, SHAPE[1], 9)) and not np.array_equal(u, DR.drop_draws(y, x, b, s + 1, SHAPE[1], 9))
    assert DR.drop_draws(y, x, b, s, SHAPE[1], 9 + (3 << 32))[0] != u[0], "both halves of the seed enter"
    for p in (0.25, 0.5, 0.75):                      # the hits removed under drop = p are those whose draw lies below float32(p)
        assert applied(drop=p, seed=9)[0] == [i for i in range(6) if not u[i] < np.float32(p)]
    # Philox-4x32-10 with a zero counter and key: the first word of the published known-answer vector
    assert int(DR.philox4(0, 0, 0, 0, 0, 0)[0]) == 0x6627E8D5
