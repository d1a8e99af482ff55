"""The case `trips3` of the fused 1x1 backward's staged schedule (bwd1x1_fused.hip), with the reference alone.  No GPU.

k_bwd1x1_fused_bf16 requests the next tile's operands in two stages during a trip and waits for them by count.  The first trip of a
workgroup starts from the prologue's requests, the second from requests issued during the first; only a THIRD trip starts from a tile
that was itself requested during a trip that began from a prefetched tile -- the schedule's steady state.  The float64 cases of
test_densenet_layers_float64_gpu.py stop at two trips.  trips3: one block of two layers, cin = 520 and 552 (both cin % 8 == 0, five
128-column slices: cap max(64, 512 // 5) = 102 workgroups per slice), 31 prong maps of 25 x 17 pixels: M = 13 175 = 205 full 64-pixel
tiles + 55 rows = 206 tiles, so workgroups 0 and 1 take three tiles (workgroup 1's third is the partial one) and all others two.
This file pins the case's figures and shows that its PReLU kink sets stay under KINK_CAP.

The engine cannot run trips3 as written: its pool0 kernel takes a stem of at most 256 channels (the forward returns -2, "pool0 supports
up to 256 channels").  test_bwd1x1_pipeline_gpu.py therefore runs `trips3-deep`: the SAME 31 maps, one block of eleven layers on a
232-channel stem, whose layers 9 and 10 are the two launches of trips3 -- cin = 520 and 552, M = 13 175, grid (102, 5, 206) -- and
whose other layers add two to four slices at two trips.  Both cases are pinned and kept under the kink cap here."""
import pytest
import torch

import densenet_layer_reference as R
from oracle import tcvn_oracle as O
from test_densenet_layer_reference_cpu import _conv0, _params, fused_grid

N_IMG, M, WIDTHS = 31, 13175, (520, 552)


def trips3_case():
    """-> cfg, coords, values, n_img (prong maps only)"""
    cfg = O.tutorial_config(initial_pixel_dim=520, densenet_structure=[2], pixel_shape=(104, 72), pixel_noise_std=0.0,
                            num_encoder_layers=2, dropout=0.0)
    b = O.synthetic_batch([16, 15], 47, cfg, prong_hits=(60, 400))
    return cfg, b[5], b[6], int(b[7].sum())


DEEP_INIT, DEEP_LAYERS = 232, 11              # trips3-deep: layers 9 and 10 have trips3's widths


def trips3_deep_case():
    """-> cfg, coords, values, n_img: trips3's maps under a stem the engine's pool0 accepts"""
    cfg = O.tutorial_config(initial_pixel_dim=DEEP_INIT, densenet_structure=[DEEP_LAYERS], pixel_shape=(104, 72), pixel_noise_std=0.0,
                            num_encoder_layers=2, dropout=0.0)
    b = O.synthetic_batch([16, 15], 47, cfg, prong_hits=(60, 400))
    return cfg, b[5], b[6], int(b[7].sum())


def test_trips3_deep_holds_trips3():
    (cfg, coords, values, n_img), (dcfg, dcoords, dvalues, dn_img) = trips3_case(), trips3_deep_case()
    assert dn_img == n_img and torch.equal(dcoords, coords) and torch.equal(dvalues, values) and dcfg.pixel_shape == cfg.pixel_shape
    widths = [DEEP_INIT + l * dcfg.densenet_growth_rate for l in range(DEEP_LAYERS)]
    assert DEEP_INIT <= 256 and tuple(widths[-2:]) == WIDTHS and all(w % 8 == 0 for w in widths)
    assert [fused_grid(M, w)[:2] for w in widths] == [(206, 2)] + [(170, 3)] * 4 + [(128, 4)] * 4 + [(102, 5)] * 2


@pytest.mark.parametrize("deep", [False, True])
def test_trips3_takes_two_workgroups_through_three_trips(deep):
    cfg, coords, values, n_img = trips3_deep_case() if deep else trips3_case()
    assert n_img == N_IMG
    g = cfg.densenet_growth_rate
    assert tuple(cfg.initial_pixel_dim + l * g for l in range(cfg.densenet_structure[0]))[-2:] == WIDTHS
    H, W = ((s - 1) // 2 + 1 for s in cfg.pixel_shape)
    H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    assert (H, W) == (25, 17) and n_img * H * W == M == 205 * 64 + 55
    for cin in WIDTHS:
        assert cin % 8 == 0
        nblk, slices, tiles = fused_grid(M, cin)
        assert (nblk, slices, tiles) == (102, 5, 206)
        trips = [len(range(wg, tiles, nblk)) for wg in range(nblk)]
        assert trips[:2] == [3, 3] and set(trips[2:]) == {2}
        assert list(range(1, tiles, nblk))[-1] == tiles - 1 and M % 64 != 0      # workgroup 1's third tile is the partial one


@pytest.mark.parametrize("deep", [False, True])
def test_trips3_stays_under_the_kink_cap(deep):
    """As test_new_layer_cases_stay_under_the_kink_cap (test_densenet_layer_reference_cpu.py) computes it: the kink sets of norm1 and
    norm2 of every layer and of final_norm hold at most KINK_CAP of their tensor."""
    cfg, coords, values, n_img = trips3_deep_case() if deep else trips3_case()
    _, P = _params(cfg)
    _, maps = R.run_forward(cfg, P, True, True, _conv0(cfg, P, coords, values, True))
    x, g = maps["dense1"], cfg.densenet_growth_rate
    assert x.shape[0] * x.shape[1] * x.shape[2] == M

    def share(t, norm):
        sc, sh = (R.f32(v) for v in R.bn_table(t, P[norm + ".weight"], P[norm + ".bias"]))
        kink = (t * sc + sh).abs() <= R.R(2) * ((t * sc).abs() + sh.abs())
        return int(kink.sum()) / kink.numel()
    worst = share(x, "features.final_norm")
    for l in range(cfg.densenet_structure[0]):
        p = f"features.dense1.layers.{l}"
        cin = cfg.initial_pixel_dim + l * g
        worst = max(worst, share(x[..., :cin], p + ".bottleneck_block.norm1"), share(maps[f"bottleneck1.{l}"], p + ".output_block.norm2"))
    print("trips3-deep:" if deep else "trips3:", "largest share of a tensor at a PReLU kink:", worst)
    assert worst <= R.KINK_CAP
