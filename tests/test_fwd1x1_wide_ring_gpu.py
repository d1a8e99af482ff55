"""k_fwd1x1_wide_bf16 (fwd1x1_fused.hip: bottleneck 1x1 forward for 256 < K <= 512 through a three-slot LDS ring, two chunks in flight)
against k_act_bf16 + the NT GEMM on the materialised operand (TCVN_NO_FWD1_FUSE on the validation build, separate process; same
arithmetic and summation order, so the same Y).  Needs an MI355X.

Bit for bit needs identical inputs, and the stem is at most 256 channels wide (pool0), so a wide layer is never a block's first layer: the
layers in front of it would hand the two sides inputs that differ by the statistics' summation-order noise.  The cases therefore zero the
3x3 weights of the first `exact - 1` layers: their new channels are the bias, whatever norm2's table is, and every layer up to index
`exact - 1` sees the same concat buffer and the same norm1 table on both sides (both on the validation build, with and without
TCVN_NO_FWD1_FUSE) -- its bottleneck map must agree BIT FOR BIT.  A layer behind them, and the product library's run (link-free
statistics: another table for the constant channels), is compared as test_fused_1x1_forward_matches_materialised_activation (test_densenet_gpu.py) compares it.

Cases (K = init + 32 l; a 104 x 72 map is 25 x 17 in block 1):
  k264   K = 232, 264 (exact: three chunks, 8 live columns in the last), 296 (noise); 3 x 25 x 17 = 1275 pixels: 20 tiles on 20
         workgroups, the last one partial
  k392   K = 232 .. 392, all exact: three chunks up to 384, four at 392
  k512   K = 256 .. 512, all exact: the last layer's four chunks completely full
  many   K = 232 .. 392 on 100 maps of 28 x 24 = 67 200 pixels: 1050 tiles on 512 workgroups -- workgroups 0..25 walk three tiles; at
         K = 392 (four chunks per tile on three slots) the ring crosses the tile boundaries with the slot index at 1 and 2
Train mode (OACT = false: raw Y + statistics) and eval mode (OACT = true: norm2 + PReLU2 in the epilogue; no batch statistics anywhere,
so every map of the block is compared bit for bit with the GEMM's activating epilogue)."""
import functools

import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import rel_err
from test_densenet_gpu import PFX, _engine

pytestmark = pytest.mark.gpu

# name: stem width, layers, pixel_shape, prongs per event, number of leading layers with identical inputs on both sides
CASES = {"k264": (232, 3, (104, 72), [2, 1], 2),
         "k392": (232, 6, (104, 72), [2, 1], 6),
         "k512": (256, 9, (104, 72), [2, 1], 9),
         "many": (232, 6, (116, 100), [50, 50], 6)}


def _case(name):
    init_ch, layers, hw, prongs, exact = CASES[name]
    cfg = O.tutorial_config(densenet_structure=[layers], initial_pixel_dim=init_ch, pixel_shape=hw, num_encoder_layers=2, dropout=0.0,
                            pixel_noise_std=0.0)
    batch = O.synthetic_batch(prongs, 41, cfg, event_hits=(60, 200), prong_hits=(20, 120))
    sd = O.fill_state(cfg, 19)
    for l in range(exact - 1):
        sd[f"{PFX}.features.dense1.layers.{l}.output_block.conv2.weight"].zero_()
    return cfg, batch, sd


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _forward(name, train, poison=False):
    """One forward of case `name`; the maps as bf16 bit patterns (int16), the statistics rows as float64."""
    cfg, batch, sd = _case(name)
    layers = cfg.densenet_structure[0]
    n_img = int(batch[7].sum())
    eng, _, _ = _engine(cfg, sd, mode=1)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    coords, values = batch[5].cuda(), batch[6].cuda()
    eng.forward(coords, values, n_img, out, train=train, seed=1)
    if poison:                                              # every workspace byte NaN (bf16, fp32, fp64), then the same forward again
        torch.cuda.synchronize()
        eng._ws.fill_(0xFF)
        eng.forward(coords, values, n_img, out, train=train, seed=1)
    torch.cuda.synchronize()
    res = dict(out=out.cpu(), dense1=_bits(eng.tap("dense1")), fused=[], pixels=n_img * eng.tap("dense1").shape[1] * eng.tap("dense1").shape[2])
    for l in range(layers):
        try:
            eng.tap(f"xa1.{l}")
            res["fused"].append(False)
        except RuntimeError:                                # no activated copy of the layer's input: the 1x1 ran on the raw buffer
            res["fused"].append(True)
        res[f"y{l}"] = _bits(eng.tap(f"bottleneck1.{l}" if train else f"ya1.{l}"))
    if train:
        res["ystat"] = [eng.tap(f"raw:ystat1.{l}").double().cpu().flatten() for l in range(layers)]
    return res


@functools.lru_cache(maxsize=None)
def _child(unfused):
    """Every case, train and eval, in ONE child process on the validation build with partial-row statistics (TCVN_NO_LF, as the test this
    one is modelled on: link-free fixed-point sums on one side only would add their own 1e-11), with or without the fused 1x1 forward."""
    from variant_utils import run_on_debug_build
    knobs = dict(TCVN_NO_LF="1", TCVN_NO_FWD1_FUSE="1") if unfused else dict(TCVN_NO_LF="1")
    return run_on_debug_build("import test_fwd1x1_wide_ring_gpu as T\n"
                              "result = dict(((c, t), T._forward(c, t)) for c in T.CASES for t in (True, False))\n", knobs)


@functools.lru_cache(maxsize=None)
def _product(name, train):
    return _forward(name, train)


def _f(bits):
    return bits.view(torch.bfloat16).float()


def _close(a, b, rtol):
    return ((a - b).abs() <= rtol * b.abs().clamp_min(1e-3)).all().item()


@pytest.mark.parametrize("name", list(CASES))
def test_wide_ring_train_matches_act_plus_gemm(name):
    got, base, ref = _product(name, True), _child(False)[(name, True)], _child(True)[(name, True)]
    init_ch, layers, _, _, exact = CASES[name]
    assert all(got["fused"]) and all(base["fused"]) and not any(ref["fused"])
    assert init_ch + 32 * (exact - 1) > 256                   # the last layer with identical inputs is a wide one
    if name == "many":
        assert got["pixels"] > 2 * 512 * 64                  # some workgroup walks three tiles
    else:
        assert got["pixels"] < 512 * 64 and got["pixels"] % 64 != 0      # fewer tiles than workgroups, the last one partial
    for l in range(exact):                                   # identical inputs: the same bits, and statistics that differ by their summation only
        y, b, r = _f(got[f"y{l}"]), _f(base[f"y{l}"]), _f(ref[f"y{l}"])
        e_cross = ((base["ystat"][l] - ref["ystat"][l]).abs() / ref["ystat"][l].abs().clamp_min(1e-3)).max().item()
        print(name, f"layer {l} (K = {init_ch + 32 * l}): fused vs GEMM max |diff|", (b - r).abs().max().item(), "of", r.abs().max().item(),
              "; ystat fused vs GEMM", e_cross, "; product (link-free statistics) vs GEMM max |diff|", (y - r).abs().max().item())
        assert torch.isfinite(y).all() and (got["ystat"][l] != 0).any()
        assert torch.equal(base[f"y{l}"], ref[f"y{l}"]), l
        assert _close(base["ystat"][l], ref["ystat"][l], 1e-5), l        # kernel against kernel on identical values
        # the product derives norm1's table from fixed-point sums (bn_lf.h): the zeroed layers' constant channels have a variance of
        # rounding noise only, so its table for them -- and with it single bf16 roundings -- may differ from the link kernels'
        assert rel_err(y, r) < 1e-2 and _close(got["ystat"][l], ref["ystat"][l], 2e-2), l
    for l in range(exact, layers):                           # behind them: the statistics' summation-order noise
        e = rel_err(_f(base[f"y{l}"]), _f(ref[f"y{l}"]))
        print(name, f"layer {l} (K = {init_ch + 32 * l}): bottleneck map, fused vs GEMM", e)
        assert e < 1e-2, l
        assert _close(base["ystat"][l], ref["ystat"][l], 2e-2) and _close(got["ystat"][l], ref["ystat"][l], 2e-2), l
    assert rel_err(_f(base["dense1"]), _f(ref["dense1"])) < 1e-2
    assert rel_err(_f(got["dense1"]), _f(ref["dense1"])) < 1e-2
    assert rel_err(base["out"], ref["out"]) < 1e-2


@pytest.mark.parametrize("name", list(CASES))
def test_wide_ring_eval_matches_act_plus_gemm(name):
    got, ref = _product(name, False), _child(True)[(name, False)]
    layers = CASES[name][1]
    assert all(got["fused"]) and not any(ref["fused"])
    for l in range(layers):
        d = (_f(got[f"y{l}"]) - _f(ref[f"y{l}"])).abs().max().item()
        print(name, f"eval, activated map of layer {l}: product vs GEMM max |diff|", d)
        assert torch.equal(got[f"y{l}"], ref[f"y{l}"]), l
    assert torch.equal(got["dense1"], ref["dense1"]) and torch.equal(got["out"], ref["out"])


@pytest.mark.parametrize("train", [True, False])
def test_wide_ring_reads_nothing_from_a_poisoned_workspace(train):
    """k264: a partial last tile and a last chunk with one live 16-B piece per row -- rows beyond M and columns beyond K must come from the
    zero line (which the forward writes itself), never from what the workspace held."""
    clean, dirty = _product("k264", train), _forward("k264", train, poison=True)
    assert torch.isfinite(dirty["out"]).all()
    for l in range(3):
        assert torch.equal(clean[f"y{l}"], dirty[f"y{l}"]), l
    assert torch.equal(clean["out"], dirty["out"])
