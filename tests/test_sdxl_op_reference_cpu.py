"""tests/sdxl_op_reference.py without a GPU: (1) the op list of the plan is consistent with its slots and kernel table; (2) the chained
reference with the roundings off IS the network (oracle/sdxl_oracle.py, float64, 1e-9); (3) its gates discriminate -- a simulated correct
kernel (bf16-rounded operands, fp32 torch arithmetic in two summation orders, one rounding to bf16) stays inside every gate on the shapes
of test_sdxl_ops_float64_gpu.py with ZERO elements out, and each simulated defect, forward and backward, leaves a gate on at least one
element."""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

import sdxl_op_reference as R
from densenet_layer_reference import bf16
from oracle import sdxl_oracle as S
from oracle import tcvn_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "sdxl_plan.json")) as f:
    GOLDEN = json.load(f)
PFX = "network.prong_embedding.prong_pixel_embedding"
CASES = R.CASES                          # the GPU test's cases; E is checked over stage 0 and its down-sampler only


def _engine(in_ch, out_dim, init_ch, H, W, mode):
    from transformercvn.hip.engine import SdxlEngine
    return SdxlEngine(in_ch, out_dim, init_ch, 2, 4, H, W, mode)


# ---------------------------------------------------------------------------------------------------------------------
# (1) the op list
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_op_list_is_consistent_with_slots_and_kernel_table(key):
    c = GOLDEN[key]["cfg"]
    eng = _engine(c["in_ch"], c["out_dim"], c["init_ch"], c["H"], c["W"], c["mode"])
    ops, slots = eng.ops(), eng.slots()
    names = [s[0] for s in slots]
    convs = [o for o in ops if o["kind"] == R.OP_CONV]
    gns = [o for o in ops if o["kind"] == R.OP_GN]
    assert len(ops) == len(convs) + len(gns)
    n = int(sorted(GOLDEN[key]["kernels"])[0])
    table = eng.conv_kernels(n)
    assert [o["conv_id"] for o in convs] == list(range(len(table)))            # one row per convolution, in conv_id order
    assert [o["gn_id"] for o in gns] == list(range(len(gns)))
    chan = {0: c["in_ch"]}
    used = set()
    for o in ops:
        assert names[o["w"]].endswith(".weight") and names[o["w"] + 1] == names[o["w"]][:-6] + "bias"
        assert o["w"] not in used
        used.add(o["w"])
        assert o["in"] in chan and o["out"] not in chan                            # every buffer has one producer, in front of its readers
        if o["kind"] == R.OP_CONV:
            cout = slots[o["w"] + 1][1]
            assert slots[o["w"]][1] == cout * chan[o["in"]] * o["ks"] ** 2, names[o["w"]]
            assert (o["act"], o["gn_id"], o["stats_given"]) == (-1, -1, -1)
            assert o["res"] == -1 or chan[o["res"]] == cout
            chan[o["out"]] = cout
        else:
            assert slots[o["w"]][1] == slots[o["w"] + 1][1] == chan[o["in"]]
            assert (o["ks"], o["stride"], o["pad"], o["conv_id"], o["stats_gn"], o["final_f32"], o["res"]) == (-1,) * 7
            chan[o["out"]] = chan[o["in"]]
    # slots no op uses: to_q / to_k of the one-token attention
    idle = sorted(names[i] for i in range(0, len(names), 2) if i not in used)
    assert idle == sorted(f"encoder.mid_block.attentions.0.{q}.weight" for q in ("to_q", "to_k"))
    assert [o["final_f32"] for o in convs] == [0] * (len(convs) - 1) + [1] and chan[convs[-1]["out"]] == c["out_dim"]
    assert table[0][1] is None and convs[0]["in"] == 0 and all(o["in"] != 0 for o in convs[1:])
    # statistics: a GroupNorm that is given them has exactly one convolution that delivers them, on its own input
    for g in gns:
        givers = [o for o in convs if o["stats_gn"] == g["gn_id"]]
        assert len(givers) == g["stats_given"] and all(o["out"] == g["in"] for o in givers)
    # regions: the queries agree with the taps and the workspace size, and exist exactly where the layout has them
    last = convs[-1]["out"]
    for wb in (False, True):
        total = eng.workspace_bytes(n, wb)
        for b in chan:
            spec = eng.region_spec("act", b, n, wb)
            assert (spec is None) == (b == last)
            if spec:
                assert spec[1][0] == n and spec[1][3] == chan[b] and spec[0] % 256 == 0 and spec[0] < total
            g = eng.region_spec("grad", b, n, wb)
            assert (g is None) == (not wb or b == 0)
        for o in convs:
            wk, wkt, gwk = (eng.region_spec(w, o["conv_id"], n, wb) for w in ("wk", "wkt", "gwk"))
            K = o["ks"] ** 2 * chan[o["in"]]
            assert wk[1] == (chan[o["out"]], -(-K // 32) * 32)
            assert (wkt is None) == (o["in"] == 0) and (gwk is None) == (not wb)
            if wkt:
                assert wkt[1] == (chan[o["in"]], -(-(o["ks"] ** 2 * chan[o["out"]]) // 32) * 32)
            if gwk:
                assert gwk[1] == wk[1] and gwk[2] == 4
        assert eng.region_spec("stats", 0, n, wb)[1] == (len(gns), n, 2) and (eng.region_spec("bstats", 0, n, wb) is None) == (not wb)
    for name, per_n in GOLDEN[key]["taps"].items():
        if name == "img" and str(n) in per_n:
            assert eng.region_spec("act", 0, n, False)[0] == per_n[str(n)][0]
    assert eng.region_spec("act", 10 ** 6, n) is None and eng.region_spec("wk", len(convs), n) is None


# ---------------------------------------------------------------------------------------------------------------------
# (2) the chained reference is the network
# ---------------------------------------------------------------------------------------------------------------------
def _params(cfg, seed):
    sd = O.fill_state(cfg, seed)
    return {k[len(PFX) + 1:]: v.double() for k, v in sd.items() if k.startswith(PFX + ".")}, sd


@pytest.mark.parametrize("init,emb", [(8, 64), (4, 36)])
def test_chained_reference_without_rounding_is_the_oracle(init, emb):
    cfg = O.tutorial_config(embedder="sdxl", initial_pixel_dim=init, pixel_embedding_dim=emb, hidden_dim=64, num_encoder_layers=2,
                            num_prong_decoder_layers=3, dropout=0.0, pixel_noise_std=0.0)
    P, sd = _params(cfg, 11)
    batch = O.synthetic_batch([2, 1], 5, cfg)
    px = O.preprocess_pixels(cfg, batch[5], batch[6].double(), False)                  # [n, 3, H, W]
    taps = {}
    ref = S.sdxl_forward({k: v.double() for k, v in sd.items() if k.startswith(PFX + ".")}, PFX, px, taps)
    out_dim = O.embed_dims(cfg)[0]
    eng = _engine(cfg.pixel_dim, out_dim, init, cfg.pixel_shape[0], cfg.pixel_shape[1], 0)
    ops, names = eng.ops(), [s[0] for s in eng.slots()]
    checks, bufs = R.run_forward(ops, names, P, px.permute(0, 2, 3, 1).contiguous(), False, exact_gn=True)
    convs = [o for o in ops if o["kind"] == R.OP_CONV]
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    assert rel(bufs[convs[-1]["out"]].reshape(ref.shape), ref) < 1e-9
    assert rel(bufs[convs[0]["out"]].permute(0, 3, 1, 2), taps[PFX + ":conv_in"]) < 1e-9
    # every down-sampler's input is a block tap, the buffer in front of conv_norm_out is "mid"
    blocks = [o["in"] for o in convs if o["stride"] == 2]
    for i, b in enumerate(blocks):
        assert rel(bufs[b].permute(0, 3, 1, 2), taps[f"{PFX}:block{i}"]) < 1e-9, i
    last_gn = [o for o in ops if o["kind"] == R.OP_GN][-1]
    assert rel(bufs[last_gn["in"]].permute(0, 3, 1, 2), taps[PFX + ":mid"]) < 1e-9
    # ... and the chained backward is its autograd
    sdd = {k: v.double().requires_grad_(True) for k, v in sd.items() if k.startswith(PFX + ".")}
    d_out = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3)).double()
    gs = torch.autograd.grad(S.sdxl_forward(sdd, PFX, px), list(sdd.values()), d_out, allow_unused=True)
    mine = R.run_backward(ops, names, P, bufs, d_out)
    for (k, v), gr in zip(sdd.items(), gs):
        k = k[len(PFX) + 1:]
        if "to_q" in k or "to_k" in k:
            assert k not in mine and (gr is None or gr.abs().max() < 1e-12)
            continue
        assert rel(mine[k].reshape(gr.shape), gr) < 1e-9, k


# ---------------------------------------------------------------------------------------------------------------------
# (3) the gates discriminate
# ---------------------------------------------------------------------------------------------------------------------
def _wide_cfg(H, W, out_dim=256):
    return O.tutorial_config(embedder="sdxl", initial_pixel_dim=64, pixel_embedding_dim=out_dim, dropout=0.0, pixel_noise_std=0.0,
                             pixel_shape=(H, W))


@functools.lru_cache(maxsize=None)
def _case(name):
    """The bf16-faithful chain of one GPU-test case on the CPU (width 64, out 256): ops, names, P, the produced buffers and the checks."""
    (n, H, W), coords, values = R.case_inputs(name)
    cfg = _wide_cfg(H, W)
    P, _ = _params(cfg, 13)
    img = bf16(R.dense_image((n, H, W), coords, values))
    eng = _engine(cfg.pixel_dim, 256, 64, H, W, 1)
    ops, names = eng.ops(), [s[0] for s in eng.slots()]
    if name == "E":                                                                    # stage 0 and its down-sampler only
        first_s2 = next(i for i, o in enumerate(ops) if o["kind"] == R.OP_CONV and o["stride"] == 2)
        ops = ops[:first_s2 + 1]
    kernels = eng.conv_kernels(n)
    checks, bufs = R.run_forward(ops, names, P, img, True, kernels)
    return ops, names, P, kernels, checks, bufs


def _sim_conv(a, w, b, res, o, order):
    """A correct kernel: bf16 operands (exact in fp32), fp32 conv2d in one of two memory orders, fp32 bias and residual, one rounding."""
    x = a.float().permute(0, 3, 1, 2)
    wr = bf16(w).float()
    if order == "channels_last":
        x, wr = x.contiguous(memory_format=torch.channels_last), wr.contiguous(memory_format=torch.channels_last)
    else:
        x = x.contiguous()
    if o["stride"] == 2:
        y = F.conv2d(F.pad(x, (0, max(1, 3 - x.shape[3]), 0, max(1, 3 - x.shape[2]))), wr, None, stride=2)      # a 1-pixel side stays 1
    else:
        y = F.conv2d(x, wr, None, padding=o["pad"])
    y = y.permute(0, 2, 3, 1) + b.float()
    if res is not None:
        y = y + res.float()
    return y


def _sim_stats(x, chunk):
    """fp32 sums over chunks of `chunk` stored values, double across them (the kernels widen per tile or per 8 values)."""
    n = x.shape[0]
    xf = x.float().reshape(n, -1)
    pad = (-xf.shape[1]) % chunk
    xf = F.pad(xf, (0, pad)).reshape(n, -1, chunk)
    return torch.stack([xf.sum(2).double().sum(1), (xf * xf).sum(2).double().sum(1)], 1)


def _sim_gn(x, stats, gamma, beta, act):
    n, H, W, C = x.shape
    mean, rstd = R.mean_rstd(stats, float(H * W * C))
    u = (x.float() - mean.float()[:, None, None, None]) * rstd.float()[:, None, None, None] * gamma.float() + beta.float()
    return u / (1 + torch.exp(-u)) if act else u


def _inputs(ops, names, P, bufs, i):
    o = ops[i]
    chan = {b: t.shape[-1] for b, t in bufs.items()}
    if o["kind"] == R.OP_CONV:
        w, b = R.conv_weight(P, names, o, chan)
        return bufs[o["in"]], w, b, (bufs[o["res"]] if o["res"] >= 0 else None)
    return bufs[o["in"]], P[names[o["w"]]], P[names[o["w"] + 1]], None


@pytest.mark.parametrize("name", sorted(CASES))
def test_simulated_correct_kernels_stay_inside_every_gate(name):
    ops, names, P, kernels, checks, bufs = _case(name)
    by_target = {}
    for chk, what in checks:
        by_target.setdefault(what, []).append(chk)
    stats_of = {what[1]: chk.ref for chk, what in checks if what[0] == "stats"}
    out_total = 0
    worst = {}
    for i, o in enumerate(ops):
        x, w, b, res = _inputs(ops, names, P, bufs, i)
        target = ("out",) if o["final_f32"] == 1 else ("act", o["out"])
        (chk,) = by_target[target]
        if o["kind"] == R.OP_CONV:
            for order in ("channels_first", "channels_last"):
                y = _sim_conv(x, w, b, res, o, order)
                got = y.double() if o["final_f32"] == 1 else y.bfloat16().double()
                wr, bad, where = chk.ratio(got)
                out_total += bad
                worst[(chk.kind, chk.family)] = max(worst.get((chk.kind, chk.family), 0), wr)
                assert bad == 0, (chk.name, order, wr, where)
            if o["stats_gn"] >= 0:
                (sc,) = by_target[("stats", o["stats_gn"])]
                for chunk in (8, 16384 if sc.kind == "stats fused" else 8):
                    wr, bad, where = sc.ratio(_sim_stats(bufs[o["out"]], chunk))
                    assert bad == 0, (sc.name, chunk, wr)
                    worst[(sc.kind, sc.family)] = max(worst.get((sc.kind, sc.family), 0), wr)
        else:
            got = _sim_gn(x, stats_of[o["gn_id"]], w, b, o["act"]).bfloat16().double()
            wr, bad, where = chk.ratio(got)
            worst[(chk.kind, chk.family)] = max(worst.get((chk.kind, chk.family), 0), wr)
            assert bad == 0, (chk.name, wr, where)
    print(name, {k: round(v, 3) for k, v in worst.items()})
    assert out_total == 0
    fams = {k[0] for k in kernels}
    if name in "ABC":
        assert {"in", "c64", "g", "s2"} <= fams


def _first(ops, kernels, pred):
    for i, o in enumerate(ops):
        if o["kind"] == R.OP_CONV and pred(o, kernels[o["conv_id"]][0]):
            return i
    raise AssertionError("no such op in this case")


def _check_of(checks, i, suffix=""):
    for chk, what in checks:
        if chk.name.startswith(f"op{i}:") and chk.name.endswith(":stats") == (suffix == ":stats"):
            return chk
    raise AssertionError(i)


def test_defect_overhang_row_and_column_of_the_last_tile_not_computed():
    ops, names, P, kernels, checks, bufs = _case("A")                                  # 44 x 72: tiles of 8 x 32 overhang both ways
    i = _first(ops, kernels, lambda o, k: k == "c64")
    x, w, b, res = _inputs(ops, names, P, bufs, i)
    chk = _check_of(checks, i)
    good = _sim_conv(x, w, b, res, ops[i], "channels_first").bfloat16().double()
    assert chk.ratio(good)[1] == 0
    for cut in ((slice(None), slice(40, 44), slice(None)), (slice(None), slice(None), slice(64, 72)), (slice(None), 43, 71)):
        bad = good.clone()
        bad[cut] = 0.0
        assert chk.ratio(bad)[1] > 0


def test_defect_packed_neighbour_read_instead_of_the_zero_column():
    ops, names, P, kernels, checks, bufs = _case("A")
    i = _first(ops, kernels, lambda o, k: k == "g" and R.tile_map(*bufs[o["in"]].shape[1:3])[0] > 1 and bufs[o["in"]].shape[2] > 1)
    x, w, b, res = _inputs(ops, names, P, bufs, i)
    n, H, W, C = x.shape
    chk = _check_of(checks, i)
    # images side by side WITHOUT the zero column: image k's right padding is image k + 1's first column
    strip = x.permute(1, 0, 2, 3).reshape(1, H, n * W, C)
    y = _sim_conv(strip, w, b, None, ops[i], "channels_first").reshape(H, n, W, -1).permute(1, 0, 2, 3)
    if res is not None:
        y = y + res.float()
    assert chk.ratio(_sim_conv(x, w, b, res, ops[i], "channels_first").bfloat16().double())[1] == 0
    assert chk.ratio(y.bfloat16().double())[1] > 0


def test_defect_stride2_far_row_clamped_instead_of_zero():
    """An even side reads the far row / column (44 -> 22: output row 21 covers rows 42 .. 44), an odd side does not (5 -> 2)."""
    ops, names, P, kernels, checks, bufs = _case("A")
    i = _first(ops, kernels, lambda o, k: o["stride"] == 2 and bufs[o["in"]].shape[1] % 2 == 0)
    x, w, b, res = _inputs(ops, names, P, bufs, i)
    chk = _check_of(checks, i)
    bad, _ = R.conv_forward(x, w, b, None, 3, 2, 0, True, clamp_far=True)
    assert chk.ratio(bf16(bad))[1] > 0
    j = _first(ops, kernels, lambda o, k: o["stride"] == 2 and bufs[o["in"]].shape[1] % 2 == 1 and bufs[o["in"]].shape[2] % 2 == 1)
    x, w, b, res = _inputs(ops, names, P, bufs, j)
    assert tuple(x.shape[1:3]) == (5, 9)
    same, _ = R.conv_forward(x, w, b, None, 3, 2, 0, True, clamp_far=True)
    assert _check_of(checks, j).ratio(bf16(same))[1] == 0


@pytest.mark.parametrize("name", ["A", "D"])
def test_defect_statistics_from_the_unrounded_value_or_of_the_neighbouring_image(name):
    ops, names, P, kernels, checks, bufs = _case(name)
    caught_unrounded = caught_neighbour = 0
    for i, o in enumerate(ops):
        if o["kind"] != R.OP_CONV or o["stats_gn"] < 0:
            continue
        x, w, b, res = _inputs(ops, names, P, bufs, i)
        sc = _check_of(checks, i, ":stats")
        unrounded = _sim_conv(x, w, b, res, o, "channels_first")                       # fp32, before its rounding to bf16
        n = unrounded.shape[0]
        s = unrounded.double().reshape(n, -1)
        caught_unrounded += sc.ratio(torch.stack([s.sum(1), (s * s).sum(1)], 1))[1] > 0
        good = _sim_stats(bufs[o["out"]], 8)
        assert sc.ratio(good)[1] == 0
        mixed = good.clone()
        mixed[1] += good[0]
        mixed[0] = 0
        caught_neighbour += sc.ratio(mixed)[1] > 0
    total = sum(1 for o in ops if o["kind"] == R.OP_CONV and o["stats_gn"] >= 0)
    print(name, "statistics defects caught at", caught_unrounded, "/", caught_neighbour, "of", total, "convolutions")
    assert caught_neighbour == total
    assert caught_unrounded >= 1


def test_defect_rstd_without_eps():
    """eps = 1e-6 matters where the variance is small: a map of nearly constant values (variance 1e-7)."""
    g = torch.Generator().manual_seed(5)
    x = bf16(1.0 + 2.0 ** -8 * torch.randint(-1, 2, (3, 5, 9, 64), generator=g).double())
    gamma, beta = 1.0 + 0.1 * torch.randn(64, generator=g).double(), 0.1 * torch.randn(64, generator=g).double()
    stats, _ = R.stored_stats(x, 0)
    for act in (0, 1):
        ref, d = R.gn_forward(x, stats, gamma, beta, act)
        chk = R.stored_check("gn", "gn", "gn", ref, d, True)
        assert chk.ratio(_sim_gn(x, stats, gamma, beta, act).bfloat16().double())[1] == 0
        bad, _ = R.gn_forward(x, stats, gamma, beta, act, eps=0.0)
        assert chk.ratio(bf16(bad))[1] > 0


def test_weight_pack_layout_and_padding():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(5, 3, 3, 3, generator=g).double()
    wk, wkt = R.weight_pack(w, 32, False, True), R.weight_pack(w, 64, True, True)
    assert wk.shape == (5, 32) and wkt.shape == (3, 64)
    for n_, c, t in ((0, 0, 0), (4, 2, 8), (2, 1, 5)):
        assert wk[n_, t * 3 + c] == bf16(w)[n_, c, t // 3, t % 3] == wkt[c, t * 5 + n_]
    assert wk[:, 27:].abs().max() == 0 and wkt[:, 45:].abs().max() == 0
    assert torch.equal(R.weight_pack(w, 32, False, False)[:, :27].reshape(5, 9, 3), w.reshape(5, 3, 9).permute(0, 2, 1))


def test_silu_gates_hold_for_a_correctly_rounded_fp32_evaluation():
    """The intrinsic assumption (1 ulp each) must at least admit an evaluation whose exp and reciprocal are correctly rounded."""
    u = torch.linspace(-40, 40, 1 << 16, dtype=torch.float32)
    ud = u.double()
    s32 = 1.0 / (1.0 + torch.exp(-u))
    ref, g = R.silu_gate(ud)
    assert bool(((u * s32).double() - ref).abs().le(g).all())
    ref, g = R.dsilu_gate(ud)
    assert bool(((s32 * (1 + u * (1 - s32))).double() - ref).abs().le(g).all())
    assert float((ref - R.dsilu_exact(ud)).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# backward: a simulated correct kernel (the same operation in fp32, another summation order than any kernel's) inside the gates, defects outside
# ---------------------------------------------------------------------------------------------------------------------
def _bwd_inputs(i, seed=9):
    ops, names, P, kernels, checks, bufs = _case("A")
    o = ops[i]
    g = torch.Generator().manual_seed(seed + i)
    shape = bufs[o["out"]].shape
    dO = bf16(torch.randn(shape, generator=g).double() * 0.05)
    earlier = bf16(torch.randn(bufs[o["in"]].shape, generator=g).double() * 0.05)
    return ops, names, P, kernels, bufs, o, dO, earlier


def _conv_ops(pred):
    ops, names, P, kernels, checks, bufs = _case("A")
    return [i for i, o in enumerate(ops) if o["kind"] == R.OP_CONV and pred(o, kernels[o["conv_id"]], bufs)]


def test_backward_convolution_gates_hold_and_catch_unflipped_taps_dropped_partials_and_a_repeated_bias():
    picks = {}
    for i in _conv_ops(lambda o, k, b: o["in"] != 0):
        ops, names, P, kernels, bufs, o, dO, earlier = _bwd_inputs(i)
        picks.setdefault((kernels[o["conv_id"]][1], kernels[o["conv_id"]][2], R.packs(*bufs[o["in"]].shape[1:3])), i)
    assert {k[0] for k in picks} == {"c64", "g", "s2", "generic"} and {k[1] for k in picks} == {"c64", "g", "s2", "generic"}
    caught = {"flip": 0, "partial": 0, "bias": 0}
    for (dg_f, wg_f, packed), i in sorted(picks.items()):
        ops, names, P, kernels, bufs, o, dO, earlier = _bwd_inputs(i)
        a = bufs[o["in"]]
        n, H, W, Cin = a.shape
        w, _ = R.conv_weight(P, names, o, {b: t.shape[-1] for b, t in bufs.items()})
        for acc in (None, earlier):
            ref, d = R.conv_dgrad(dO, w, acc, o["ks"], o["stride"], o["pad"], (H, W), True)
            chk = R.stored_check("dgrad", "dgrad", dg_f, ref, d, True)
            sim, _ = R.conv_dgrad(dO.float(), bf16(w).float(), None if acc is None else acc.float(), o["ks"], o["stride"], o["pad"], (H, W), False)
            assert chk.ratio(sim.bfloat16().double())[1] == 0, (i, dg_f)
            if o["ks"] == 3:
                bad, _ = R.conv_dgrad(dO, w, acc, o["ks"], o["stride"], o["pad"], (H, W), True, flip=False)
                caught["flip"] += chk.ratio(bf16(bad))[1] > 0
            if acc is not None:                                                    # defect 7 for a convolution: `accumulate` ignored
                assert chk.ratio(bf16(R.conv_dgrad(dO, w, None, o["ks"], o["stride"], o["pad"], (H, W), True)[0]))[1] > 0
        depth = R.wgrad_depth(wg_f, n, H, W, dO.shape[1], dO.shape[2], Cin, dO.shape[3], o["ks"])
        (dW, gW), (db, gb) = R.conv_wgrad(a, dO, o["ks"], o["stride"], o["pad"], True, depth=depth)
        cw, cb = R.stored_check("dW", "wgrad", wg_f, dW, gW, False), R.stored_check("db", "wgrad", wg_f, db, gb, False)
        (sW, _), (sb, _) = R.conv_wgrad(a.float(), dO.float(), o["ks"], o["stride"], o["pad"], True)
        assert cw.ratio(sW.double())[1] == 0 and cb.ratio(sb.double())[1] == 0, (i, wg_f)
        M = dO.shape[0] * dO.shape[1] * dO.shape[2]
        (bW, _), _ = R.conv_wgrad(a, dO, o["ks"], o["stride"], o["pad"], True, drop_partial=(M - min(M, 256), M))      # the last partial
        caught["partial"] += cw.ratio(bW)[1] > 0
        if Cin >= 128:                                                             # a bias gradient counted once per 64-channel input chunk
            _, (bb, _) = R.conv_wgrad(a, dO, o["ks"], o["stride"], o["pad"], True, bias_times=Cin // 64)
            assert cb.ratio(bb)[1] > 0
            caught["bias"] += 1
    print("backward convolution defects caught:", caught, "of", len(picks), "picked convolutions")
    assert caught["flip"] >= 1 and caught["partial"] == len(picks) and caught["bias"] >= 1


def test_backward_groupnorm_gates_hold_and_catch_an_ignored_accumulate():
    ops, names, P, kernels, checks, bufs = _case("A")
    stats_of = {what[1]: chk.ref for chk, what in checks if what[0] == "stats"}
    gns = [i for i, o in enumerate(ops) if o["kind"] == R.OP_GN]
    for i in (gns[0], gns[1], gns[len(gns) // 2], [j for j in gns if not ops[j]["act"]][0], gns[-1]):
        _, _, _, _, _, o, dO, earlier = _bwd_inputs(i)
        x, gamma, beta = bufs[o["in"]], P[names[o["w"]]], P[names[o["w"] + 1]]
        st = stats_of[o["gn_id"]]
        sim = R.gn_backward(x.float().double(), st, gamma, beta, o["act"], dO, None, None)      # for its bstats
        for acc in (None, earlier):
            res = R.gn_backward(x, st, gamma, beta, o["act"], dO, sim["bstats"][0], acc)
            # a correct kernel: the same formulas in fp32
            n, H, W, C = x.shape
            mean, rstd = (t.float()[:, None, None, None] for t in R.mean_rstd(st, float(H * W * C)))
            xh = (x.float() - mean) * rstd
            u = xh * gamma.float() + beta.float()
            sg = 1 / (1 + torch.exp(-u))
            dU = dO.float() * (sg * (1 + u * (1 - sg)) if o["act"] else 1.0)
            c1, c2 = ((sim["bstats"][0][:, j] / (H * W * C)).float()[:, None, None, None] for j in (0, 1))
            dx = rstd * (gamma.float() * dU - c1 - xh * c2)
            if acc is not None:
                dx = acc.float() + dx
            chk = R.stored_check("dx", "gn bwd dx", "-", *res["dx"], True)
            assert chk.ratio(dx.bfloat16().double())[1] == 0, (i, acc is None)
            if acc is not None:
                assert chk.ratio(bf16(R.gn_backward(x, st, gamma, beta, o["act"], dO, sim["bstats"][0], None)["dx"][0]))[1] > 0
        for key, got in (("dgamma", (dU * xh).reshape(-1, C).sum(0)), ("dbeta", dU.reshape(-1, C).sum(0)),
                         ("bstats", torch.stack([(gamma.float() * dU).reshape(n, -1).double().sum(1),
                                                 (gamma.float() * dU * xh).reshape(n, -1).double().sum(1)], 1))):
            ref, gate = res[key]
            chk = R.Check(key, key, "-", ref, gate) if key == "bstats" else R.stored_check(key, key, "-", ref, gate, False)
            assert chk.ratio(got.double())[1] == 0, (i, key)


def test_defect_slot_past_n_of_a_half_filled_packed_tile_written():
    """Packed px = 3 at 5 x 9 with 11 maps: the last tile holds 2 of 3 images.  A kernel that also stores the third slot writes one image
    behind its output buffer; the 'nothing else changes' predicate of the forward (sentinel bytes around the op's buffer) sees it."""
    ops, names, P, kernels, checks, bufs = _case("A")
    i = _first(ops, kernels, lambda o, k: k == "g" and R.tile_map(*bufs[o["in"]].shape[1:3]) == (3, 1))
    x, w, b, res = _inputs(ops, names, P, bufs, i)
    n, H, W, _ = x.shape
    px, py = R.tile_map(H, W)
    slots = -(-n // (px * py)) * px * py
    assert (n, slots) == (11, 12)
    good = _sim_conv(x, w, b, res, ops[i], "channels_first").bfloat16()
    per = good[0].numel() * 2
    own = n * per
    gap = (-own) % 256
    ws = torch.full((256 + own + gap + 4 * per,), R.SENTINEL, dtype=torch.uint8)          # [front guard][buffer][gap][what follows]
    ws[256:256 + own] = good.contiguous().view(torch.uint8).reshape(-1)
    assert R.changed_outside(ws, [(256, own)], 0, ws.numel()) == 0
    # the defective kernel: slot 11 is an image of zeros (the patch reads zero there), so it stores conv(0) + bias behind the buffer
    ghost = _sim_conv(torch.zeros_like(x[:1]), w, b, None, ops[i], "channels_first").bfloat16()
    assert bool(ghost.abs().max() > 0)
    ws[256 + own:256 + own + per] = ghost.contiguous().view(torch.uint8).reshape(-1)
    assert R.changed_outside(ws, [(256, own)], 0, ws.numel()) > 0
    assert _check_of(checks, i).ratio(good.double())[1] == 0                              # which no check of the op's own output can see


def test_product_library_has_none_of_the_validation_entry_points():
    import ctypes
    from transformercvn.hip import _lib
    assert os.path.basename(_lib.LIB_PATH) == "libtcvn_hip.so"
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tcvn_debug_sdxl_backward_stop", "tcvn_debug_sdxl_forward_stop", "tcvn_debug_sdxl_goff", "tcvn_debug_sdxl_silu_probe"):
        assert not hasattr(dll, name), name
    dbg = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libtcvn_hip_dbg.so"))
    assert all(hasattr(dbg, n_) for n_ in ("tcvn_debug_sdxl_backward_stop", "tcvn_debug_sdxl_forward_stop", "tcvn_debug_sdxl_goff",
                                            "tcvn_debug_sdxl_silu_probe"))


def test_replayed_gradient_regions_of_a_whole_backward():
    """R.replay_goff on the golden plan: which ops still find their dO after a whole backward (everything but conv2 of the same-width ResNet
    blocks and to_out), and that a residual pair shares one region."""
    c = GOLDEN[sorted(GOLDEN)[0]]["cfg"]
    eng = _engine(c["in_ch"], c["out_dim"], c["init_ch"], c["H"], c["W"], c["mode"])
    ops, names = eng.ops(), [s_[0] for s_ in eng.slots()]
    spec = {b: eng.region_spec("grad", b, 2, True) for b in {o["out"] for o in ops}}
    read, intact = R.replay_goff(ops, {b: sp[0] for b, sp in spec.items()}, lambda a, b: spec[a][1] == spec[b][1])
    gone = sorted(names[o["w"]] for i, o in enumerate(ops) if not intact[i])
    assert len(gone) == 17 and all(g.endswith(".conv2.weight") or g.endswith("to_out.0.weight") for g in gone)
    by_name = {names[o["w"]]: i for i, o in enumerate(ops)}
    for nm, i in by_name.items():
        if "conv_shortcut" in nm:                                  # conv_shortcut and its block's conv2 read one region, still intact
            j = by_name[nm.replace("conv_shortcut", "conv2")]
            assert read[i] == read[j] and intact[i] and intact[j]
    assert intact[by_name["encoder.conv_in.weight"]] and read[by_name["encoder.conv_in.weight"]] != spec[ops[0]["out"]][0]
