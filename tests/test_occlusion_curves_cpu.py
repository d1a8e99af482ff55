"""Deletion / insertion curves, host side: argument and mode errors are raised before any device work, the curve of a hand-made result
on the host reports that it runs on the GPU only, and the C ABI of the curves is declared, exported and rejects bad arguments."""
import ctypes
import os
import re

import pytest
import torch

from oracle import tcvn_oracle as O
from model_utils import build_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tcvn_occlusion_curve_workspace_bytes", "tcvn_occlusion_curve_variants", "tcvn_occlusion_curve_build_pass",
           "tcvn_occlusion_curve"]
TILE, GRID = (100, 70), (4, 4)          # on the 400 x 280 maps of the tutorial configuration


def small():
    cfg = O.tutorial_config(densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64,
                            num_encoder_layers=1, pixel_noise_std=0.0)
    assert tuple(cfg.pixel_shape) == (400, 280)
    return cfg, build_trainer(cfg, None, device=None), O.synthetic_batch([2, 1], 3, cfg, event_hits=(5, 9), prong_hits=(2, 4))[:8]


def relevance(batch, grid=GRID):
    B, P = batch[7].shape
    return torch.rand(B, 1 + P, *grid, generator=torch.Generator().manual_seed(5))


def hand_made_scan(batch, tile):
    """An OcclusionResult as a scan at `tile` would return it for `batch` (no variants: only its shape and tile are looked at)."""
    from transformercvn.hip.occlusion import OcclusionResult
    B, P = batch[7].shape
    grid = (-(-400 // tile[0]), -(-280 // tile[1]))
    return OcclusionResult(torch.zeros(B, 4), torch.zeros(B, P, 3), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0, 4),
                           torch.zeros(0, P, 3), grid, tile)


def test_train_mode_raises_before_any_device_work():
    cfg, model, batch = small()
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.occlusion_curves(*batch, relevance(batch), tile=TILE)
    net = model.network
    with pytest.raises(RuntimeError, match="eval"):
        net.occlusion_curves(*model._network_inputs(*batch), None, relevance(batch), TILE)
    assert net._runtime is None, "the runtime (native plans) must not have been created"


def bad_calls(batch):
    rel = relevance(batch)
    nan, inf = rel.clone(), rel.clone()
    nan[0, 0, 1, 1], inf[1, 1, 0, 0] = float("nan"), float("-inf")
    from transformercvn.hip.occlusion import RefinedOcclusion
    refined = RefinedOcclusion(
        torch.zeros(2, 4), torch.zeros(2, batch[7].shape[1], 3), [hand_made_scan(batch, (200, 140)), hand_made_scan(batch, TILE)], [], [],
        None, "event", 0.25, None)
    return {
        "steps 0": (rel, dict(tile=TILE, steps=0)), "steps 65": (rel, dict(tile=TILE, steps=65)),
        "steps float": (rel, dict(tile=TILE, steps=4.0)), "steps bool": (rel, dict(tile=TILE, steps=True)),
        "mode": (rel, dict(tile=TILE, mode="removal")), "mode None": (rel, dict(tile=TILE, mode=None)),
        "maps": (rel, dict(tile=TILE, maps="prong")), "max_maps_per_pass": (rel, dict(tile=TILE, max_maps_per_pass=257)),
        "relevance shape": (rel[:, :, :3], dict(tile=TILE)), "relevance batch": (rel[:1], dict(tile=TILE)),
        "relevance dims": (rel[0], dict(tile=TILE)), "relevance float64": (rel.double(), dict(tile=TILE)),
        "relevance int": (rel.long(), dict(tile=TILE)), "relevance list": (rel.tolist(), dict(tile=TILE)),
        "relevance None": (None, dict(tile=TILE)),
        "relevance NaN": (nan, dict(tile=TILE)), "relevance inf": (inf, dict(tile=TILE)),
        "tile of another grid": (rel, dict(tile=(64, 64))), "tile malformed": (rel, dict(tile=(0, 70))),
        "tile missing": (rel, dict()), "tile None": (rel, dict(tile=None)),
        "tile against the result": (hand_made_scan(batch, TILE), dict(tile=(64, 64))),
        "tile against the refined result": (refined, dict(tile=(200, 140))),
        "result of another batch": (hand_made_scan((None,) * 7 + (torch.ones(5, 2, dtype=torch.bool),), TILE), dict()),
        "more than 4096 tiles": (torch.zeros(2, 1 + batch[7].shape[1], 100, 70), dict(tile=(4, 4))),
    }


@pytest.mark.parametrize("case", ["steps 0", "steps 65", "steps float", "steps bool", "mode", "mode None", "maps", "max_maps_per_pass",
                                  "relevance shape", "relevance batch", "relevance dims", "relevance float64", "relevance int",
                                  "relevance list", "relevance None", "relevance NaN", "relevance inf", "tile of another grid",
                                  "tile malformed", "tile missing", "tile None", "tile against the result",
                                  "tile against the refined result", "result of another batch", "more than 4096 tiles"])
def test_bad_arguments_raise_value_error_before_any_device_work(case):
    cfg, model, batch = small()
    rel, kw = bad_calls(batch)[case]
    model.eval()
    with pytest.raises(ValueError):
        model.occlusion_curves(*batch, rel, **kw)
    with pytest.raises(ValueError):
        model.network.occlusion_curves(*model._network_inputs(*batch), None, rel, **kw)
    assert model.network._runtime is None
    model.train()                       # a bad argument is reported as such in either mode
    with pytest.raises(ValueError):
        model.occlusion_curves(*batch, rel, **kw)


def test_check_curve_args_accepts_the_documented_forms():
    from transformercvn.hip import occlusion
    cfg, model, batch = small()
    B, P = batch[7].shape
    rel = relevance(batch)
    rel[0, 0, 0, 0] = -0.0
    shape = (400, 280)
    assert occlusion.check_curve_args(rel, TILE, 10, "deletion", "all", 256, B, P, shape) == (TILE, 10, "deletion", "all", 256)
    assert occlusion.check_curve_args(rel, list(TILE), 1, "insertion", "event", 1, B, P, shape) == (TILE, 1, "insertion", "event", 1)
    assert occlusion.check_curve_args(rel, TILE, 64, "deletion", "prongs", 8, B, P, shape)[1] == 64
    # a result brings its own tile; naming it again is allowed
    res = hand_made_scan(batch, TILE)
    assert occlusion.check_curve_args(res, None, 10, "deletion", "all", 256, B, P, shape)[0] == TILE
    assert occlusion.check_curve_args(res, TILE, 10, "deletion", "all", 256, B, P, shape)[0] == TILE
    refined = occlusion.RefinedOcclusion(res.event_logits, res.prong_logits, [hand_made_scan(batch, (200, 140)), res], [], [], None,
                                         "event", 0.25, None)
    assert occlusion.check_curve_args(refined, None, 10, "deletion", "all", 256, B, P, shape)[0] == TILE
    # 8 x 8 tiles on 400 x 280 are 50 x 35 = 1750 tiles per map: admitted
    assert occlusion.check_curve_args(torch.zeros(B, 1 + P, 50, 35), (8, 8), 10, "deletion", "all", 256, B, P, shape)[0] == (8, 8)
    assert (occlusion.MAX_STEPS, occlusion.MAX_TILES, occlusion.MODES) == (64, 4096, ("deletion", "insertion"))


def hand_made():
    from transformercvn.hip.occlusion import OcclusionCurves
    g = torch.Generator().manual_seed(1)
    ev, pr = torch.randn(2, 4, generator=g), torch.randn(2, 3, 5, generator=g)
    index = torch.tensor([[0, 0, 0, 0], [0, 0, 1, 2], [0, 0, 2, 3], [1, 2, 0, 0], [1, 2, 1, 1], [1, 2, 2, 1]], dtype=torch.int32)
    return OcclusionCurves(ev, pr, index, torch.randn(6, 4, generator=g), torch.randn(6, 3, 5, generator=g),
                           torch.full((2, 4, 2, 2), -1, dtype=torch.int32), 2, "deletion", (200, 140), (2, 2))


def test_curve_on_the_host_is_gpu_only_and_validates_its_target():
    res = hand_made()
    assert res.num_variants == 6 and res.steps == 2 and res.mode == "deletion" and res.grid == (2, 2) and res.tile == (200, 140)
    for target in ("event", "prong", 2, torch.tensor([1, 3])):
        with pytest.raises(RuntimeError, match="GPU only"):
            res.curve(target)
        with pytest.raises(RuntimeError, match="GPU only"):
            res.auc(target)
    for target in ("events", 4, -1, 1.5, torch.tensor([1, 2, 3]), torch.tensor([0, 4]), torch.tensor([[0, 1]])):
        with pytest.raises(ValueError):
            res.curve(target)
        with pytest.raises(ValueError):
            res.auc(target)


def test_curve_symbols_are_declared_and_exported():
    from transformercvn.hip import _lib
    header = open(os.path.join(ROOT, "include", "tcvn_hip.h")).read()
    declared = set(re.findall(r"\b(tcvn_[a-z0-9_]+)\s*\(", header))
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(dll, name), name
        assert name in _lib.EXPORTS, name
    assert re.search(r"#define\s+TCVN_CURVE_MAX_STEPS\s+64\b", header) and _lib.CURVE_MAX_STEPS == 64
    assert re.search(r"#define\s+TCVN_CURVE_MAX_TILES\s+4096\b", header) and _lib.CURVE_MAX_TILES == 4096
    assert re.search(r"#define\s+TCVN_CURVE_DELETION\s+0\b", header) and re.search(r"#define\s+TCVN_CURVE_INSERTION\s+1\b", header)
    assert (_lib.CURVE_DELETION, _lib.CURVE_INSERTION) == (0, 1)


def test_native_calls_reject_bad_arguments_before_any_device_call(capfd):
    """NULL pointers, tile < 1, steps outside 1..64, more than 4096 tiles per map, an unknown mode or target: non-zero and one 'tcvn:'
    line, on a machine without a GPU too."""
    from transformercvn.hip._lib import lib
    wsb = lib.tcvn_occlusion_curve_workspace_bytes
    assert wsb(3, 400, 280, 0, 16, 10, 256) == -1
    assert wsb(3, 400, 280, 16, 16, 0, 256) == -1
    assert wsb(3, 400, 280, 16, 16, 65, 256) == -1
    assert wsb(3, 400, 280, 16, 16, 10, 257) == -1
    assert wsb(0, 400, 280, 16, 16, 10, 256) == -1
    assert wsb(3, 400, 280, 4, 4, 10, 256) == -1                # 100 x 70 tiles per map
    assert wsb(3, 400, 280, 8, 8, 10, 256) > 3 * 50 * 35 * 4    # 1750 tiles per map
    assert wsb(3, 256, 256, 4, 4, 64, 1) > 0                    # exactly 4096 tiles per map
    host = (ctypes.c_int64 * 16)()
    one = (ctypes.c_int32 * 16)()
    f = (ctypes.c_float * 16)()
    assert capfd.readouterr().err.count("tcvn:") == 0           # the workspace query answers -1 silently, as the scan's does
    # NULL pointers
    assert lib.tcvn_occlusion_curve_variants(None, 5, 1, 400, 280, 100, 70, None, None, 1, 0, 4, 0, None, 256, None, None, None, 0, host,
                                             16, None) != 0
    # steps out of range, then an unknown mode, then too many tiles, with every pointer set
    for steps, mode, tile in ((65, 0, 100), (4, 2, 100), (4, 0, 4)):
        assert lib.tcvn_occlusion_curve_variants(one, 1, 1, 400, 280, tile, 70 if tile == 100 else 4, one, f, 1, 0, steps, mode, one, 256,
                                                 one, one, one, 64, host, 16, None) != 0
    assert lib.tcvn_occlusion_curve_build_pass(None, None, 0, 3, 1, 400, 280, 100, 70, 4, 0, 256, None, None, 0, 0, 1, None, None, 0,
                                               None) != 0
    assert lib.tcvn_occlusion_curve_build_pass(one, f, 1, 1, 1, 400, 280, 100, 70, 4, 0, 256, one, one, 64, 0, 6, one, f, 1, None) != 0
    assert lib.tcvn_occlusion_curve(None, None, None, None, None, 1, 1, 0, 4, 4, 4, 7, None, None, None, None) != 0
    assert lib.tcvn_occlusion_curve(f, f, f, f, one, 1, 1, 0, 4, 4, 65, 0, None, f, f, None) != 0
    err = capfd.readouterr().err
    assert err.count("tcvn:") == 8, err


# ---- the driver (Scan.curves) on the host, with the stand-in engines of test_occlusion_scan_cpu.py ---------------------------------------
def test_scan_curves_merges_the_lists_by_b_s_k_and_uses_the_curve_calls():
    import test_occlusion_scan_cpu as S
    from transformercvn.hip.occlusion import Scan, VariantPlan
    from transformercvn.hip.runtime import LastForward

    class CurveEmbedder(S.Embedder):
        """The curve variant list on the host: per map the occupied tiles sorted by (-relevance, tile index)."""

        def occlusion_curve_variants(self, coords, n_img, shape, tile, img_bs, max_pass, relevance, steps, mode, rank):
            self.variant_calls += 1
            Wt = -(-shape[1] // tile[1])
            rows, surviving = [], []
            for i in range(n_img):
                b, s = img_bs[i].tolist()
                hits = [(int(y) // tile[0], int(x) // tile[1]) for img, y, x in coords.tolist() if img == i]
                order = sorted(set(hits), key=lambda t: (-float(relevance[b, s, t[0], t[1]]), t[0] * Wt + t[1]))
                for r, (ty, tx) in enumerate(order):
                    rank[b, s, ty, tx] = r
                for k in range(steps + 1 if order else 0):
                    m = (k * len(order) + steps - 1) // steps
                    top = sum(1 for h in hits if h in order[:m])
                    rows.append((i, b, s, k, m))
                    surviving.append(top if mode == 1 else len(hits) - top)
            V = len(rows)
            bounds = [sum(surviving[:min(k * max_pass, V)]) for k in range(-(-V // max_pass) + 1)]
            vimg = torch.tensor([r[0] for r in rows], dtype=torch.int32)
            index = torch.tensor([r[1:] for r in rows], dtype=torch.int32).reshape(V, 4)
            return VariantPlan(V, bounds, vimg, index, torch.empty(0), (n_img, *shape, *tile, steps, mode, max_pass)), False, False

        def occlusion_curve_build(self, plan, coords, values, first, count, out_coords, out_values):
            self.builds.append(("curve", first, count))

    ev_engine, pr_engine, head = CurveEmbedder(12), CurveEmbedder(8), S.Head()
    last = LastForward(torch.zeros(S.B + S.N_PRONGS, 16), torch.zeros(S.B, 1 + S.P, dtype=torch.int32), S.B, S.P, S.N_PRONGS)
    scan = Scan(ev_engine, pr_engine, head, S.SHAPE, last, torch.zeros(S.B, 4), torch.zeros(S.B, S.P, 3), S.pixels(S.EVENT_HITS),
                S.pixels(S.PRONG_HITS), S.MASK, "all")
    rel = torch.arange(S.B * (1 + S.P) * 4, dtype=torch.float32).reshape(S.B, 1 + S.P, 2, 2)       # the last occupied tile ranks first
    res = scan.curves(rel, S.TILE, 2, "deletion", 4)
    # maps (b, s) and their occupied tiles: (0,0) 3, (0,1) 2, (0,2) 1, (1,0) 1, (1,1) 2; slot (1,2) is padded
    n = {(0, 0): 3, (0, 1): 2, (0, 2): 1, (1, 0): 1, (1, 1): 2}
    want = [[b, s, k, (k * t + 1) // 2] for (b, s), t in sorted(n.items()) for k in range(3)]
    assert res.index.tolist() == want and res.num_variants == 3 * 5
    assert (res.steps, res.mode, res.tile, res.grid) == (2, "deletion", S.TILE, (2, 2))
    assert res.rank[0, 0].tolist() == [[2, 1], [0, -1]] and res.rank[1, 0].tolist() == [[-1, -1], [-1, 0]]
    assert (res.rank[1, 2] == -1).all() and int((res.rank >= 0).sum()) == sum(n.values())
    assert torch.equal(res.step_event_logits, res.index.float()), "the rows travel with their index"
    # 6 event-map variants and 9 prong-map variants in passes of 4; the k = 2 variants are empty maps, so the last event pass has no hit
    assert [p[0] for p in head.passes] == [4, 2, 4, 4, 1]
    assert all(b[0] == "curve" for b in ev_engine.builds + pr_engine.builds)
    assert ev_engine.variant_calls == pr_engine.variant_calls == 1
    ins = scan.curves(rel, S.TILE, 2, "insertion", 256)
    assert ins.index.tolist() == want and ins.mode == "insertion" and torch.equal(ins.rank, res.rank)
