"""Tile Shapley values, host side: argument and mode errors are raised before any device work, the values of a hand-made result on the
host report that they run on the GPU only, the C ABI is declared, exported and rejects bad arguments, and the reference formulas of
occlusion_shapley_reference.py hold the Shapley axioms on a toy value function."""
import ctypes
import itertools
import math
import os
import re

import pytest
import torch

from oracle import tcvn_oracle as O
from model_utils import build_trainer
import occlusion_shapley_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tcvn_occlusion_shapley_workspace_bytes", "tcvn_occlusion_shapley_variants", "tcvn_occlusion_shapley_build",
           "tcvn_occlusion_shapley_values"]


def small():
    cfg = O.tutorial_config(densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64,
                            num_encoder_layers=1, pixel_noise_std=0.0)
    assert tuple(cfg.pixel_shape) == (400, 280)
    return cfg, build_trainer(cfg, None, device=None), O.synthetic_batch([2, 1], 3, cfg, event_hits=(5, 9), prong_hits=(2, 4))[:8]


def test_train_mode_raises_before_any_device_work():
    cfg, model, batch = small()
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.occlusion_shapley(*batch)
    net = model.network
    with pytest.raises(RuntimeError, match="eval"):
        net.occlusion_shapley(*model._network_inputs(*batch))
    assert net._runtime is None, "the runtime (native plans) must not have been created"


BAD = {
    "tile malformed": dict(tile=(0, 32)), "tile not a pair": dict(tile=32), "tile float": dict(tile=(32.0, 32)),
    "more than 1024 tiles": dict(tile=(8, 8)),                       # 50 x 35 = 1750 tiles per map
    "max_exact -1": dict(max_exact=-1), "max_exact 11": dict(max_exact=11), "max_exact float": dict(max_exact=4.0),
    "max_exact bool": dict(max_exact=True), "max_exact None": dict(max_exact=None),
    "samples 0": dict(samples=0), "samples 257": dict(samples=257), "samples float": dict(samples=8.0), "samples bool": dict(samples=True),
    "seed negative": dict(seed=-1), "seed 2**64": dict(seed=1 << 64), "seed float": dict(seed=1.5), "seed None": dict(seed=None),
    "maps": dict(maps="prong"), "max_maps_per_pass 0": dict(max_maps_per_pass=0), "max_maps_per_pass 257": dict(max_maps_per_pass=257),
    "max_variants 0": dict(max_variants=0), "max_variants float": dict(max_variants=10.0), "max_variants bool": dict(max_variants=True),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_raise_value_error_before_any_device_work(case):
    cfg, model, batch = small()
    kw = BAD[case]
    model.eval()
    with pytest.raises(ValueError):
        model.occlusion_shapley(*batch, **kw)
    with pytest.raises(ValueError):
        model.network.occlusion_shapley(*model._network_inputs(*batch), None, **kw)
    assert model.network._runtime is None
    model.train()                       # a bad argument is reported as such in either mode
    with pytest.raises(ValueError):
        model.occlusion_shapley(*batch, **kw)


def test_check_shapley_args_accepts_the_documented_forms():
    from transformercvn.hip import occlusion
    shape = (400, 280)
    assert occlusion.check_shapley_args((32, 32), 6, 16, 0, "all", 256, None, shape) == ((32, 32), 6, 16, 0, "all", 256, None)
    assert occlusion.check_shapley_args([100, 70], 0, 1, (1 << 64) - 1, "event", 1, 1, shape) == \
        ((100, 70), 0, 1, (1 << 64) - 1, "event", 1, 1)
    assert occlusion.check_shapley_args((16, 16), 10, 256, 7, "prongs", 8, 10 ** 6, shape)[:3] == ((16, 16), 10, 256)   # 25 x 18 = 450
    assert occlusion.check_shapley_args((13, 9), 10, 256, 7, "all", 8, None, shape)[0] == (13, 9)          # 31 x 32 = 992 tiles


def hand_made():
    from transformercvn.hip.occlusion import TileShapley
    g = torch.Generator().manual_seed(1)
    ev, pr = torch.randn(2, 4, generator=g), torch.randn(2, 3, 5, generator=g)
    index = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [1, 2, 0, 0]], dtype=torch.int32)
    perms = torch.full((2, 4, 2, 4), -1, dtype=torch.int32)
    perms[0, 0, :, :2] = torch.tensor([[1, 2], [2, 1]])
    perms[1, 2, :, :1] = 3
    n = torch.full((2, 4), -1, dtype=torch.int32)
    n[0, 0], n[1, 2], n[1, 0] = 2, 1, 0
    return TileShapley(ev, pr, index, torch.randn(4, 4, generator=g), torch.randn(4, 3, 5, generator=g), perms, n > 0, n, (200, 140),
                       (2, 2), 2, 4, 9)


def test_values_on_the_host_are_gpu_only_and_validate_target_and_value():
    res = hand_made()
    assert res.num_variants == 4 and (res.tile, res.grid, res.samples, res.max_exact, res.seed) == ((200, 140), (2, 2), 2, 4, 9)
    for target in ("event", "prong", 2, torch.tensor([1, 3])):
        with pytest.raises(RuntimeError, match="GPU only"):
            res.values(target)
        with pytest.raises(RuntimeError, match="GPU only"):
            res.heatmap(target)
    for target in ("events", 4, -1, 1.5, torch.tensor([1, 2, 3]), torch.tensor([0, 4]), torch.tensor([[0, 1]])):
        with pytest.raises(ValueError):
            res.values(target)
    for value in ("probability", None, 0):
        with pytest.raises(ValueError):
            res.values("event", value)
    # the reference reads the same object on the host: 2 tiles exact, 1 tile, no tile, the rest not scanned
    phi, se, full, empty = SR.values_reference(res, "event", "logit")
    c = int(res.event_logits[0].argmax())
    v = [float(res.coalition_event_logits[k, c]) for k in range(3)] + [float(res.event_logits[0, c])]
    assert phi[0, 0].flatten().tolist() == pytest.approx([0.0, 0.5 * (v[1] - v[0]) + 0.5 * (v[3] - v[2]),
                                                           0.5 * (v[2] - v[0]) + 0.5 * (v[3] - v[1]), 0.0], abs=1e-12)
    assert float(phi[1, 2].sum()) == pytest.approx(float(full[1, 2] - empty[1, 2]), abs=1e-12) and float(phi[1, 2, 1, 1]) != 0.0
    assert (phi[1, 0] == 0).all() and float(full[1, 0]) == float(empty[1, 0])
    assert torch.isnan(phi[0, 1]).all() and torch.isnan(full[0, 1]) and (se[0, 0] == 0).all()


def test_shapley_symbols_are_declared_and_exported():
    from transformercvn.hip import _lib
    header = open(os.path.join(ROOT, "include", "tcvn_hip.h")).read()
    declared = set(re.findall(r"\b(tcvn_[a-z0-9_]+)\s*\(", header))
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(dll, name), name
        assert name in _lib.EXPORTS, name
    assert re.search(r"#define\s+TCVN_TSHAP_MAX_TILES\s+1024\b", header) and _lib.TSHAP_MAX_TILES == 1024
    assert re.search(r"#define\s+TCVN_TSHAP_MAX_SAMPLES\s+256\b", header) and _lib.TSHAP_MAX_SAMPLES == 256
    assert re.search(r"#define\s+TCVN_TSHAP_MAX_EXACT\s+10\b", header) and _lib.TSHAP_MAX_EXACT == 10
    # the stream constant of the permutation keys is no other draw's
    used = set()
    for name in ("tcvn_common.h", "shapley.hip", "detector.hip", "mc_dropout.hip"):
        src = open(os.path.join(ROOT, "dune-transformercvn_amd", "csrc", name)).read()
        used |= {int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]{8})u\b", src)}
    own = open(os.path.join(ROOT, "dune-transformercvn_amd", "csrc", "occlude_shapley.hip")).read()
    assert f"0x{SR.STREAM:08x}u" in own and SR.STREAM not in used


def test_native_calls_reject_bad_arguments_before_any_device_call(capfd):
    """NULL pointers, tile < 1, samples outside 1..256, max_exact outside 0..10, more than 1024 tiles per map, an unknown target or
    value, a short workspace: non-zero and one 'tcvn:' line, on a machine without a GPU too."""
    from transformercvn.hip._lib import lib
    wsb = lib.tcvn_occlusion_shapley_workspace_bytes
    assert wsb(3, 400, 280, 0, 32, 16, 6, 256) == -1
    assert wsb(3, 400, 280, 32, 32, 0, 6, 256) == -1
    assert wsb(3, 400, 280, 32, 32, 257, 6, 256) == -1
    assert wsb(3, 400, 280, 32, 32, 16, -1, 256) == -1
    assert wsb(3, 400, 280, 32, 32, 16, 11, 256) == -1
    assert wsb(3, 400, 280, 32, 32, 16, 6, 257) == -1
    assert wsb(0, 400, 280, 32, 32, 16, 6, 256) == -1
    assert wsb(3, 400, 280, 8, 8, 16, 6, 256) == -1                  # 50 x 35 = 1750 tiles per map
    assert wsb(3, 256, 256, 8, 8, 1, 0, 1) > 0                       # exactly 1024 tiles per map
    T = 13 * 9
    assert wsb(3, 400, 280, 32, 32, 16, 6, 256) > 3 * 16 * T * 2     # the rank table: maps x samples x tiles 16-bit words
    host = (ctypes.c_int64 * 64)()
    one = (ctypes.c_int32 * 64)()
    f = (ctypes.c_float * 64)()
    d = (ctypes.c_double * 64)()
    assert capfd.readouterr().err.count("tcvn:") == 0                # the workspace query answers -1 silently, as the scan's does
    variants, build, values = lib.tcvn_occlusion_shapley_variants, lib.tcvn_occlusion_shapley_build, lib.tcvn_occlusion_shapley_values
    # NULL pointers
    assert variants(None, 5, 1, 400, 280, 200, 140, None, 1, 0, 2, 4, 0, None, None, None, 256, None, None, None, 0, host, 64, None) != 0
    # samples, max_exact and the tiles per map out of range, then a short workspace, with every pointer set
    for samples, max_exact, tile in ((257, 4, 200), (2, 11, 200), (2, 4, 8)):
        assert variants(one, 1, 1, 400, 280, tile, 140 if tile == 200 else 8, one, 1, 0, samples, max_exact, 0, one, one, one, 256, one,
                        one, one, 256, host, 64, None) != 0
    assert variants(one, 1, 1, 400, 280, 200, 140, one, 1, 0, 2, 4, 0, one, one, one, 256, one, one, one, 64, host, 64, None) != 0
    assert build(None, None, 0, 3, 1, 400, 280, 200, 140, 2, 4, 256, None, None, 0, 0, 1, None, None, 0, None) != 0
    assert build(one, f, 1, 1, 1, 400, 280, 200, 140, 2, 4, 256, one, one, 64, 0, 16, one, f, 1, None) != 0     # 15 rows per map
    assert build(one, f, 1, 1, 1, 400, 280, 200, 140, 2, 4, 256, one, one, 64, 0, 1, one, f, 1, None) != 0      # a short workspace
    assert values(None, None, None, None, None, 1, None, None, None, 1, 0, 4, 4, 2, 2, 2, 0, None, 0, None, None, None, None, None, 0,
                  None) != 0
    for target, value, grid, scratch in ((7, 0, 2, 64), (0, 2, 2, 64), (0, 0, 33, 64), (0, 0, 2, 8)):
        assert values(f, f, f, f, one, 1, one, one, one, 1, 0, 4, 4, grid, grid, 2, target, None, value, f, f, d, d, d, scratch,
                      None) != 0
    err = capfd.readouterr().err
    assert err.count("tcvn:") == 13, err


# ---- the driver (Scan.shapley) on the host, with the stand-in engines of test_occlusion_scan_cpu.py ---------------------------------------
def test_scan_shapley_merges_the_lists_by_b_s_m_k_checks_max_variants_and_uses_the_shapley_calls():
    import test_occlusion_scan_cpu as S
    from transformercvn.hip.occlusion import Scan, VariantPlan
    from transformercvn.hip.runtime import LastForward

    class ShapleyEmbedder(S.Embedder):
        """The coalition list on the host: per map the occupied tiles, all their coalitions or the prefixes of the permutations."""

        def occlusion_shapley_variants(self, coords, n_img, shape, tile, img_bs, max_pass, samples, max_exact, seed, permutations,
                                       n_tiles, exact):
            self.variant_calls += 1
            Wt = -(-shape[1] // tile[1])
            rows, surviving = [], []
            for i in range(n_img):
                b, s = img_bs[i].tolist()
                hits = [(int(y) // tile[0]) * Wt + int(x) // tile[1] for img, y, x in coords.tolist() if img == i]
                tiles = sorted(set(hits))
                n = len(tiles)
                n_tiles[b, s], exact[b, s] = n, int(1 <= n <= max_exact)
                orders = [SR.permutation(tiles, m, b * (1 + S.P) + s, seed) for m in range(samples)]
                for m, order in enumerate(orders):
                    permutations[b, s, m, :n] = torch.tensor(order, dtype=torch.int32)
                if 1 <= n <= max_exact:
                    for k in range(2 ** n - 1):
                        members = {t for j, t in enumerate(tiles) if (k >> j) & 1}
                        rows.append((i, b, s, 0, k))
                        surviving.append(sum(h in members for h in hits))
                elif n:
                    rows.append((i, b, s, 0, 0))
                    surviving.append(0)
                    for m, order in enumerate(orders):
                        for k in range(1, n):
                            rows.append((i, b, s, m, k))
                            surviving.append(sum(h in order[:k] for h in hits))
            V = len(rows)
            bounds = [sum(surviving[:min(k * max_pass, V)]) for k in range(-(-V // max_pass) + 1)]
            vimg = torch.tensor([r[0] for r in rows], dtype=torch.int32)
            index = torch.tensor([r[1:] for r in rows], dtype=torch.int32).reshape(V, 4)
            return VariantPlan(V, bounds, vimg, index, torch.empty(0), (n_img, *shape, *tile, samples, max_exact, max_pass)), False, False

        def occlusion_shapley_build(self, plan, coords, values, first, count, out_coords, out_values):
            self.builds.append(("shapley", first, count))

    def make():
        ev_engine, pr_engine, head = ShapleyEmbedder(12), ShapleyEmbedder(8), S.Head()
        last = LastForward(torch.zeros(S.B + S.N_PRONGS, 16), torch.zeros(S.B, 1 + S.P, dtype=torch.int32), S.B, S.P, S.N_PRONGS)
        scan = Scan(ev_engine, pr_engine, head, S.SHAPE, last, torch.zeros(S.B, 4), torch.zeros(S.B, S.P, 3), S.pixels(S.EVENT_HITS),
                    S.pixels(S.PRONG_HITS), S.MASK, "all")
        return scan, ev_engine, pr_engine, head

    scan, ev_engine, pr_engine, head = make()
    res = scan.shapley(S.TILE, 2, 2, 5, 4, None)
    # maps (b, s) and their occupied tiles: (0,0) 3 (sampled: 1 + 2 x 2), (0,1) 2, (0,2) 1, (1,0) 1, (1,1) 2 (exact); slot (1,2) is padded
    want = [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 1, 1], [0, 0, 1, 2], [0, 1, 0, 0], [0, 1, 0, 1], [0, 1, 0, 2], [0, 2, 0, 0],
            [1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 1], [1, 1, 0, 2]]
    assert res.index.tolist() == want and res.num_variants == 13
    assert (res.tile, res.grid, res.samples, res.max_exact, res.seed) == (S.TILE, (2, 2), 2, 2, 5)
    assert res.n_tiles.tolist() == [[3, 2, 1], [1, 2, -1]] and res.exact.tolist() == [[False, True, True], [True, True, False]]
    assert res.exact.dtype == torch.bool and res.permutations.shape == (S.B, 1 + S.P, 2, 4)
    assert sorted(res.permutations[0, 0, 1].tolist()) == [-1, 0, 1, 2] and (res.permutations[1, 2] == -1).all()
    assert torch.equal(res.coalition_event_logits, res.index.float()), "the rows travel with their index"
    # 6 event-map variants and 7 prong-map variants in passes of 4
    assert [p[0] for p in head.passes] == [4, 2, 4, 3]
    assert all(b[0] == "shapley" for b in ev_engine.builds + pr_engine.builds)
    assert ev_engine.variant_calls == pr_engine.variant_calls == 1
    # the budget is checked when both lists are known and before any pass
    scan, ev_engine, pr_engine, head = make()
    with pytest.raises(ValueError, match="V = 13"):
        scan.shapley(S.TILE, 2, 2, 5, 4, 12)
    assert head.passes == [] and ev_engine.forwards == [] and ev_engine.variant_calls == pr_engine.variant_calls == 1
    assert scan.shapley(S.TILE, 2, 2, 5, 4, 13).num_variants == 13


# ---- the helper's own formulas on a toy value function ---------------------------------------------------------------------------------------
def toy(n=4):
    """Players 0 and 1 are interchangeable, player 2 has an effect of its own and one with player 0, player 3 changes nothing."""
    def value_of(c):
        c = frozenset(c)
        return 0.25 + 1.5 * len(c & {0, 1}) ** 2 + (0.75 if 2 in c else 0.0) + (0.5 if {0, 1} <= c and 2 in c else 0.0)
    table = [value_of({i for i in range(n) if (k >> i) & 1}) for k in range(2 ** n)]
    return value_of, table


def test_the_reference_formulas_hold_the_shapley_axioms_on_a_toy_value_function():
    value_of, table = toy()
    n = 4
    phi = SR.exact_shapley(table, n)
    brute = SR.permutation_shapley(value_of, n)
    assert phi == pytest.approx(brute, abs=1e-12), "the weighted sum over coalitions is the mean over all n! orders"
    assert sum(phi) == pytest.approx(table[-1] - table[0], abs=1e-12), "efficiency"
    assert phi[0] == pytest.approx(phi[1], abs=1e-12) and phi[0] != pytest.approx(phi[2], abs=1e-3), "symmetry"
    assert phi[3] == pytest.approx(0.0, abs=1e-12) and min(abs(p) for p in phi[:3]) > 0.1, "a null player gets 0"
    # sampling ALL orders once gives the exact values, telescopes per permutation, and a null player has no spread
    orders = [list(o) for o in itertools.permutations(range(n))]
    prefix = [[value_of(o[:k]) for k in range(n + 1)] for o in orders]
    mean, se = SR.sampled_shapley(prefix, orders)
    assert mean == pytest.approx(phi, abs=1e-12) and se[3] == 0.0 and se[0] == pytest.approx(se[1], abs=1e-12) and se[0] > 0
    two, _ = SR.sampled_shapley(prefix[:2], orders[:2])
    assert sum(two) == pytest.approx(table[-1] - table[0], abs=1e-12), "efficiency holds for any sample of permutations"
    one, err = SR.sampled_shapley(prefix[5:6], orders[5:6])
    assert err == [0.0] * n and sum(one) == pytest.approx(table[-1] - table[0], abs=1e-12)


def test_the_reference_permutations_are_orders_of_the_tiles_and_depend_on_every_counter_word():
    tiles = [0, 3, 5, 6, 9, 14]
    base = SR.permutation(tiles, 0, 0, 0)
    assert sorted(base) == tiles and SR.permutation([], 0, 0, 0) == []
    others = [SR.permutation(tiles, 1, 0, 0), SR.permutation(tiles, 0, 1, 0), SR.permutation(tiles, 0, 0, 1),
              SR.permutation(tiles, 0, 0, 1 << 32)]
    assert all(sorted(o) == tiles for o in others)
    assert sum(o != base for o in others) >= 3, "720 orders: at most one of four draws may repeat the first by chance"
    assert math.factorial(len(tiles)) == 720
