"""The staged schedule of k_bwd1x1_fused_bf16 (bwd1x1_fused.hip: the next tile's Y and G rows requested under the weight-gradient MFMAs,
DU and x behind them, counted waits) in its steady state, and the narrow 1x1 forward (k_fwd1x1_fused_bf16<1|2>, fwd1x1_fused.hip) with
its next tile travelling under the epilogue.  Needs an MI355X.

Backward: the case `trips3` (test_bwd1x1_pipeline_cpu.py: cin = 520 and 552, grid 102 x 5, 206 tiles -- workgroups 0 and 1 take THREE
tiles, workgroup 1's third is the partial one), as layers 9 and 10 of `trips3-deep` (the same maps on a 232-channel stem: pool0 takes
no stem wider than 256 channels, see that file; its layers 0 .. 8 run the kernel at two to four slices and two trips besides), through the snapshot-hook comparison of test_densenet_layers_float64_gpu.py
(_run_layers_backward: eff rows, DU, norm2's link, db1, dW1, the read-add-write of G[:, :cin], norm1's link and P / Q against float64
on the state each layer found, everything else bit-unchanged; that test's own gates, no element excluded) on the validation library
without knobs in bf16.  The hook's report must show the fused kernel on a 102 x 5 grid over 206 tiles.  Then the same backward twice
more in the same process, unhooked: dW1, db1, G and the norm1 gradients of all three runs must agree bit for bit -- an LDS region
overwritten by an early request while it is still being read shows there or in the float64 gates.

Forward: `narrow3`, modelled on `many` of test_fwd1x1_wide_ring_gpu.py but at K <= 256: stem width 96, five layers (K = 96, 128 on
<1, ...>; 160, 192, 224 on <2, ...>), 151 maps of 28 x 24 = 101 472 pixels = 1585 full tiles + 32 rows on 768 workgroups: workgroups
0 .. 49 walk three tiles and workgroup 49's third is the partial one.  The 3x3 weights of the first four layers are zero, so every
layer sees identical inputs on both sides (that file's docstring); train and eval, every bottleneck map bit-identical to k_act_bf16 +
NT GEMM (TCVN_NO_FWD1_FUSE on the validation library)."""
import functools

import pytest
import torch

from oracle import tcvn_oracle as O
from test_bwd1x1_pipeline_cpu import DEEP_INIT, DEEP_LAYERS, M, N_IMG, WIDTHS, trips3_deep_case
from test_densenet_layer_reference_cpu import fused_grid
from test_densenet_gpu import PFX, _engine
from test_fwd1x1_wide_ring_gpu import _bits, _close, _f

pytestmark = pytest.mark.gpu

BF16 = 1
OWN = ("bottleneck_block.conv1.weight", "bottleneck_block.conv1.bias", "bottleneck_block.norm1.weight", "bottleneck_block.norm1.bias",
       "bottleneck_block.relu1.weight")


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def _state(eng, grads):
    """What the fused 1x1 backward and its reductions leave, as raw bytes: dW1, db1 and the norm1 / PReLU1 gradients of both layers, the
    block's G and (P, Q)."""
    torch.cuda.synchronize()
    out = {f"{l}.{k}": grads[f"features.dense1.layers.{l}.{k}"].contiguous().view(torch.uint8).cpu() for l in range(DEEP_LAYERS) for k in OWN}
    out["G"] = eng.tap("raw:grad1").contiguous().view(torch.uint8).cpu()
    out["PQ"] = eng.tap("raw:pq1").contiguous().view(torch.uint8).cpu()
    return out


def _plain_backward(T):
    """The backward of _run_layers_backward without the hook: same state, same seeds."""
    cfg, coords, values, n_img = trips3_deep_case()
    eng, _, grads = _engine(cfg, O.fill_state(cfg, 19), mode=BF16, with_grad=True)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=True, seed=T.SEED)
    eng.backward(torch.randn(n_img, eng.out_dim, generator=torch.Generator().manual_seed(5)).cuda())
    return _state(eng, grads)


def _backward_runs():
    """Child-process body: the hooked float64 comparison of trips3, then two unhooked backwards -> (report, [state, state, state])."""
    import test_densenet_layers_float64_gpu as T
    made = []
    case, engine = T._case, T._engine

    def engine_kept(*a, **k):
        made.append(engine(*a, **k))
        return made[-1]
    T._case = lambda name: trips3_deep_case() if name == "trips3" else case(name)      # that module's helpers know their own case names only
    T._engine = engine_kept
    try:
        rep = T._run_layers_backward("trips3", BF16)
    finally:
        T._case, T._engine = case, engine
    eng, _, grads = made[-1]
    return rep, [_state(eng, grads), _plain_backward(T), _plain_backward(T)]


@functools.lru_cache(maxsize=None)
def _backward_child():
    from variant_utils import run_on_debug_build
    return run_on_debug_build("import test_bwd1x1_pipeline_gpu as T\nresult = T._backward_runs()\n", {})


def test_three_trips_match_float64_on_the_state_each_layer_found():
    rep, _ = _backward_child()
    worst = {}
    for name, kernel, w, bad, numel, where, kinks, amax in rep["figures"]:
        if not w <= worst.get(kernel, (-1.0, ""))[0]:
            worst[kernel] = (w, name)
    print("trips3 worst |error| / gate per kernel:", {k: (round(v, 4), nm) for k, (v, nm) in sorted(worst.items())},
          "elements at a PReLU kink (left out):", sum(f[6] for f in rep["figures"]),
          "layers (block, layer, cin, dgrad kernel, fused 1x1, eff rows, fused grid, slices, M):", rep["reports"])
    bad = [f for f in rep["figures"] if f[3] or not f[2] <= 1.0]
    assert not bad, [f[:5] for f in bad[:12]]
    layers = DEEP_LAYERS
    assert [r[:3] for r in rep["reports"]] == [(0, l, DEEP_INIT + 32 * l) for l in range(layers)], rep["reports"]
    assert tuple(r[2] for r in rep["reports"][-2:]) == WIDTHS
    n_ey = len([f for f in rep["figures"] if f[1] == "eff rows"])
    assert len(rep["figures"]) == 15 * layers + n_ey + 6, len(rep["figures"])
    for kind, n in (("dgrad3x3", 1), ("norm2 link", 5), ("norm1 link", 5), ("untouched", 1), ("1x1 backward (fused)", 3)):
        assert len([f for f in rep["figures"] if f[1] == kind]) == n * layers, kind
    # ---- from the hook's report: the fused kernel ran everywhere; trips3's two launches on 102 x 5 workgroups over 206 tiles -- the third
    # trip is proven, not assumed
    for b, l, cin, kern, fused, eyv, nblk, slices, m in rep["reports"]:
        assert fused == 1 and m == M == N_IMG * 25 * 17 and (nblk, slices) == fused_grid(m, cin)[:2], rep["reports"]
    for b, l, cin, kern, fused, eyv, nblk, slices, m in rep["reports"][-2:]:
        assert (nblk, slices) == (102, 5), rep["reports"]
        tiles = -(-m // 64)
        assert tiles == 206 and tiles > 2 * nblk and tiles - 2 * nblk == 2 and m % 64 == 55, rep["reports"]
    assert sum("k_bwd1x1_fused_bf16" in k for k in rep["labels"]) == layers, rep["labels"]


def test_three_trips_give_the_same_bits_every_run():
    _, states = _backward_child()
    hooked, first, second = states
    assert set(hooked) == set(first) == set(second) and len(first) == 5 * DEEP_LAYERS + 2
    for k in sorted(first):
        assert first[k].numel() > 0 and bool(first[k].any()), k          # the run wrote it
        assert torch.equal(first[k], second[k]), k
        assert torch.equal(hooked[k], first[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
INIT, LAYERS, PRONGS = 96, 5, [76, 75]


def _fwd_case():
    cfg = O.tutorial_config(densenet_structure=[LAYERS], initial_pixel_dim=INIT, pixel_shape=(116, 100), num_encoder_layers=2, dropout=0.0,
                            pixel_noise_std=0.0)
    batch = O.synthetic_batch(PRONGS, 41, cfg, event_hits=(60, 200), prong_hits=(20, 120))
    sd = O.fill_state(cfg, 19)
    for l in range(LAYERS - 1):
        sd[f"{PFX}.features.dense1.layers.{l}.output_block.conv2.weight"].zero_()
    return cfg, batch, sd


def _forward(train):
    """One forward of narrow3; the maps as bf16 bit patterns (int16), the statistics rows as float64 (as test_fwd1x1_wide_ring_gpu._forward)."""
    cfg, batch, sd = _fwd_case()
    n_img = int(batch[7].sum())
    eng, _, _ = _engine(cfg, sd, mode=BF16)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(batch[5].cuda(), batch[6].cuda(), n_img, out, train=train, seed=1)
    torch.cuda.synchronize()
    d1 = eng.tap("dense1")
    res = dict(out=out.cpu(), dense1=_bits(d1), fused=[], shape=tuple(d1.shape[:3]))
    for l in range(LAYERS):
        try:
            eng.tap(f"xa1.{l}")
            res["fused"].append(False)
        except RuntimeError:                                # no activated copy of the layer's input: the 1x1 ran on the raw buffer
            res["fused"].append(True)
        res[f"y{l}"] = _bits(eng.tap(f"bottleneck1.{l}" if train else f"ya1.{l}"))
    if train:
        res["ystat"] = [eng.tap(f"raw:ystat1.{l}").double().cpu().flatten() for l in range(LAYERS)]
    return res


@functools.lru_cache(maxsize=None)
def _fwd_child(unfused):
    from variant_utils import run_on_debug_build
    knobs = dict(TCVN_NO_LF="1", TCVN_NO_FWD1_FUSE="1") if unfused else dict(TCVN_NO_LF="1")
    return run_on_debug_build("import test_bwd1x1_pipeline_gpu as T\nresult = dict((t, T._forward(t)) for t in (True, False))\n", knobs)


def _walks_three_tiles(res):
    n, h, w = res["shape"]
    pixels = n * h * w
    assert (n, h, w) == (151, 28, 24) and pixels == 101472 == 1585 * 64 + 32
    tiles = -(-pixels // 64)
    assert tiles - 2 * 768 == 50 and list(range(49, tiles, 768))[-1] == tiles - 1      # workgroups 0 .. 49, the partial tile is workgroup 49's third
    assert [INIT + 32 * l for l in range(LAYERS)] == [96, 128, 160, 192, 224]          # <1, ...> twice, <2, ...> three times


def test_narrow_forward_train_matches_act_plus_gemm():
    base, ref = _fwd_child(False)[True], _fwd_child(True)[True]
    _walks_three_tiles(base)
    assert all(base["fused"]) and not any(ref["fused"])
    for l in range(LAYERS):
        b, r = _f(base[f"y{l}"]), _f(ref[f"y{l}"])
        print(f"narrow3 layer {l} (K = {INIT + 32 * l}): fused vs GEMM max |diff|", (b - r).abs().max().item(), "of", r.abs().max().item())
        assert torch.isfinite(b).all() and (base["ystat"][l] != 0).any()
        assert torch.equal(base[f"y{l}"], ref[f"y{l}"]), l
        assert _close(base["ystat"][l], ref["ystat"][l], 1e-5), l        # kernel against kernel on identical values


def test_narrow_forward_eval_matches_act_plus_gemm():
    got, ref = _forward(False), _fwd_child(True)[False]
    _walks_three_tiles(got)
    assert all(got["fused"]) and not any(ref["fused"])
    for l in range(LAYERS):
        d = (_f(got[f"y{l}"]) - _f(ref[f"y{l}"])).abs().max().item()
        print(f"narrow3 eval, activated map of layer {l}: product vs GEMM max |diff|", d)
        assert torch.equal(got[f"y{l}"], ref[f"y{l}"]), l
    assert torch.equal(got["dense1"], ref["dense1"]) and torch.equal(got["out"], ref["out"])
