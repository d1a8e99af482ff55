"""The float64 reference of densenet_layer_reference.py, forward and backward, is right, and its gates bite.  No GPU.

Rounding off: the reference functions chained over a small net agree with oracle.tcvn_oracle.densenet_forward (float64) to 1e-9 relative
on every map the oracle exposes, in train and eval mode, without and with dropout keep masks fed to both sides; the chained deferred
(G, P, Q) backward agrees with the oracle's autograd on every parameter gradient behind the stem and on the gradient reaching block 1.

Rounding on: a "defective kernel" -- the reference with one deliberate defect, reading the same bf16-faithful stored inputs -- must leave
the gates of the intact reference on at least one element of the operation it sits in (and nowhere else); a simulated correct kernel
(operands rounded after a perturbation by +-tau, fp32 accumulation, one bf16 store) must stay inside them everywhere.

The frozen backward (hit gradients; run_backward_frozen): rounding off it is float64 autograd through the oracle's eval forward down to
the conv0 map and, behind the gather, the hit values, on the GPU test's cases narrow, wide and odd; each defect a schedule threaded
through the training one can have -- stale (P, Q), a dropout keep in the eff rows, batch-statistics tables, a non-zero odd edge behind
a transition, a 128-column slice of G[:, :cin] not accumulated, the gather reading DU0 at the fp32 stride in bf16 mode -- leaves the
gate of the check it affects at those sizes; and every GPU case stays under KINK_CAP on running-statistics tables."""
import functools

import pytest
import torch
import torch.nn.functional as F

import densenet_layer_reference as R
from oracle import tcvn_oracle as O

PFX = "network.prong_embedding.prong_pixel_embedding"


def _net(dropout=0.0, n_img=3, **over):
    """cin = 130, 162, 194 in block 1 (cin % 8 == 2, more than one 128-column slice), 9 x 13 maps (odd in front of the transition), and with
    three images 3 * 11 * 15 = 495 padded positions: the last partial 128-position tile (111 positions) holds real pixels."""
    cfg = O.tutorial_config(initial_pixel_dim=130, densenet_structure=[3, 2], pixel_shape=(40, 56), dropout=dropout, pixel_noise_std=0.0,
                            num_encoder_layers=2, **over)
    b = O.synthetic_batch([n_img], 31, cfg, prong_hits=(20, 120))
    return cfg, b[5], b[6], n_img


def _params(cfg, seed=19):
    sd = O.fill_state(cfg, seed)
    return sd, {k[len(PFX) + 1:]: v.double() for k, v in sd.items() if k.startswith(PFX + ".") and v.is_floating_point()}


def _conv0(cfg, P, coords, values, rnd):
    px = O.preprocess_pixels(cfg, coords, values.double(), False)
    if rnd:
        px = R.bf16(px)
    w = R.bf16(P["features.conv0.weight"]) if rnd else P["features.conv0.weight"]
    c0 = F.conv2d(px, w, P["features.conv0.bias"], stride=2, padding=3).permute(0, 2, 3, 1).contiguous()
    return R.bf16(c0) if rnd else c0


def _keeps(cfg, maps_hw, n_img, seed):
    """Random keep scales per 3x3 site, as tcvn_dropout_keep would report them: 0 or fl32(1 / (1 - p))."""
    gen = torch.Generator().manual_seed(seed)
    ks = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(cfg.dropout, dtype=torch.float32)))
    out = {}
    for b, layers in enumerate(cfg.densenet_structure):
        H, W = maps_hw[b]
        for l in range(layers):
            out[(b, l)] = (torch.rand(n_img, H, W, cfg.densenet_growth_rate, generator=gen) >= cfg.dropout).double() * ks
    return out


def _map_sizes(cfg):
    H, W = ((s + 6 - 7) // 2 + 1 for s in cfg.pixel_shape)
    H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out = []
    for _ in cfg.densenet_structure:
        out.append((H, W))
        H, W = H // 2, W // 2
    return out


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# rounding off: the chained reference is the oracle's network
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train,dropout", [(True, 0.0), (False, 0.0), (True, 0.1)])
def test_reference_without_rounding_is_the_oracle_network(train, dropout):
    cfg, coords, values, n_img = _net(dropout)
    sd, P = _params(cfg)
    keeps = _keeps(cfg, _map_sizes(cfg), n_img, 5) if dropout else None
    _, maps = R.run_forward(cfg, P, False, train, _conv0(cfg, P, coords, values, False), keeps)

    def provider(site, shape):
        if site.endswith(":out"):
            return torch.ones(shape, dtype=torch.float64)
        b, l = site.rsplit(":dense", 1)[1].split(".")
        return keeps[(int(b) - 1, int(l))].permute(0, 3, 1, 2)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ctx = O._Ctx(train, dropout, provider if dropout else None)
    with torch.no_grad():
        out = O.densenet_forward(sd64, PFX, cfg, O.preprocess_pixels(cfg, coords, values.double(), False), ctx)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    figures = {"conv0": _rel(nchw(maps["conv0"]), ctx.taps[PFX + ":conv0"]), "pool0": _rel(nchw(maps["pool0"]), ctx.taps[PFX + ":pool0"]),
               "condense": _rel(maps["condense"], ctx.taps[PFX + ":condense"])}
    ch = cfg.initial_pixel_dim
    for b, layers in enumerate(cfg.densenet_structure):
        figures[f"dense{b + 1}"] = _rel(nchw(maps[f"dense{b + 1}"]), ctx.taps[PFX + f":dense{b + 1}"])
        figures[f"bottleneck{b + 1}.0"] = _rel(nchw(maps[f"bottleneck{b + 1}.0"]), ctx.taps[PFX + f":dense{b + 1}.bottleneck0"])
        ch += layers * cfg.densenet_growth_rate
        if b + 1 < len(cfg.densenet_structure):
            ch //= 2
            figures[f"transition{b + 1}"] = _rel(nchw(maps[f"dense{b + 2}"][..., :ch]), ctx.taps[PFX + f":transition{b + 1}"])
    z = maps["output_linear"]                                     # the oracle exposes the Linear's rows only behind BatchNorm1d + PReLU
    o = "output_block.norm"
    sc, sh = R.bn_table(z, P[o + ".weight"], P[o + ".bias"], None if train else (P[o + ".running_mean"], P[o + ".running_var"]))
    figures["out"] = _rel(R._prelu(z * sc + sh, P["output_block.relu.weight"]), out)
    print(train, dropout, figures)
    assert max(figures.values()) < 1e-9, figures


def test_bf16_rounding_is_one_round_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -3.14159, 0.0, 1e-3, 255.5], dtype=torch.float64)
    assert torch.equal(R.bf16(x), torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625, 0.0, 0.00099945068359375, 256.0], dtype=torch.float64))
    y = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 37
    assert torch.equal(R.bf16(y.float().double()), y.float().to(torch.bfloat16).double())      # torch's own cast, from exact fp32 values
    assert torch.equal(R.f32(y), y.float().double())
    assert torch.equal(R.ulp(torch.tensor([1.0, 1.99, 2.0, 0.0, -0.75], dtype=torch.float64), 8),
                       torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0, 2.0 ** -8], dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# rounding on: the gates bite, and only where they should
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _faithful(n_img=3):
    """The bf16-faithful stored maps of the small net with dropout, and the intact reference's checks over them."""
    cfg, coords, values, n_img = _net(0.1, n_img)
    _, P = _params(cfg)
    keeps = _keeps(cfg, _map_sizes(cfg), n_img, 7)
    c0 = _conv0(cfg, P, coords, values, True)
    _, maps = R.run_forward(cfg, P, True, True, c0, keeps)
    stored = {k: v for k, v in maps.items() if k != "pool0"}
    checks, _ = R.run_forward(cfg, P, True, True, c0, keeps, stored=stored)
    return cfg, P, keeps, c0, stored, checks


def test_chained_maps_are_inside_their_own_gates():
    cfg, P, keeps, c0, stored, checks = _faithful()
    for c in checks:
        worst, bad, where = c.ratio(R.stored_counterpart(c, stored))
        assert bad == 0 and worst <= 1.0, (c.name, worst, bad, where)


DEFECTS = [("conv3x3.1.1", "row_leak"), ("conv3x3.1.1", "image_leak"), ("conv3x3.1.2", "stale_tail"), ("conv1x1.1.1", "drop_last_channel"),
           ("conv1x1.1.2", "slice_table"), ("conv3x3.1.1", "wrong_keep"), ("transition1", "ceil_pool")]
TARGET = {"conv3x3.1.1": "dense1[162:194]", "conv3x3.1.2": "dense1[194:226]", "conv1x1.1.1": "bottleneck1.1", "conv1x1.1.2": "bottleneck1.2",
          "transition1": "dense2[0:113]"}


@pytest.mark.parametrize("op,defect", DEFECTS)
def test_a_defective_kernel_leaves_the_gates(op, defect):
    cfg, P, keeps, c0, stored, checks = _faithful()
    assert _map_sizes(cfg)[0] == (9, 13) and cfg.initial_pixel_dim % 8 == 2 and (3 * 11 * 15) % 128 > 13 + 3
    wrong, _ = R.run_forward(cfg, P, True, True, c0, keeps, stored=stored, defects={op: defect})
    assert [c.name for c in wrong] == [c.name for c in checks]
    hit = {}
    for c, w in zip(checks, wrong):
        got = R.bf16(w.ref) if c.kernel not in ("head_pool", "linear") else R.f32(w.ref)     # what the defective kernel would store
        worst, bad, where = c.ratio(got)
        if bad:
            hit[c.name] = (bad, round(worst, 1), where)
    print(op, defect, hit)
    assert list(hit) == [TARGET[op]], hit


def test_simulated_correct_kernels_stay_inside_the_gates():
    """One dense layer and the transition as a correct bf16 kernel computes them: every self-computed operand is the bf16 rounding of the
    exact value moved by +tau or -tau (random sign: the worst an fp32 evaluation may do), products accumulate in fp32 (float32 matmul:
    some fma order), bias and keep scale in fp32, one bf16 store."""
    cfg, P, keeps, c0, stored, checks = _faithful()
    by_name = {c.name: c for c in checks}
    gen = torch.Generator().manual_seed(3)
    sign = lambda t: (torch.randint(0, 2, t.shape, generator=gen) * 2 - 1).double()
    b, l, g = 0, 1, cfg.densenet_growth_rate
    cin = cfg.initial_pixel_dim + l * g
    p = f"features.dense1.layers.{l}"
    tab = lambda norm, x: tuple(R.f32(t) for t in R.bn_table(x, P[norm + ".weight"], P[norm + ".bias"]))
    x = stored["dense1"][..., :cin]
    f, tau, _, _ = R.activation(x, *tab(p + ".bottleneck_block.norm1", x), P[p + ".bottleneck_block.relu1.weight"], True)
    a = R.bf16(f + sign(f) * tau).float()
    w1 = R.bf16(P[p + ".bottleneck_block.conv1.weight"].reshape(128, cin)).float()
    y = (a @ w1.T + P[p + ".bottleneck_block.conv1.bias"].float()).to(torch.bfloat16).double()
    worst, bad, where = by_name[f"bottleneck1.{l}"].ratio(y)
    print("simulated 1x1: worst |error| / gate", worst)
    assert bad == 0, (worst, bad, where)

    y = stored[f"bottleneck1.{l}"]
    f, tau, _, _ = R.activation(y, *tab(p + ".output_block.norm2", y), P[p + ".output_block.relu2.weight"], True)
    a = R.bf16(f + sign(f) * tau).float()
    w2 = R.bf16(P[p + ".output_block.conv2.weight"]).float()
    o = F.conv2d(a.permute(0, 3, 1, 2), w2, P[p + ".output_block.conv2.bias"].float(), padding=1).permute(0, 2, 3, 1)
    o = (o * keeps[(b, l)].float()).to(torch.bfloat16).double()
    worst, bad, where = by_name[f"dense1[{cin}:{cin + g}]"].ratio(o)
    print("simulated 3x3: worst |error| / gate", worst)
    assert bad == 0, (worst, bad, where)

    x = stored["dense1"]
    t = "features.transition1"
    f, tau, _, _ = R.pooled_activation(x, *tab(t + ".norm", x), P[t + ".relu.weight"], True)
    a = R.bf16(f + sign(f) * tau).float()
    C = x.shape[-1]
    o = (a @ R.bf16(P[t + ".conv.weight"].reshape(C // 2, C)).float().T + P[t + ".conv.bias"].float()).to(torch.bfloat16).double()
    worst, bad, where = by_name[f"dense2[0:{C // 2}]"].ratio(o)
    print("simulated transition: worst |error| / gate", worst)
    assert bad == 0, (worst, bad, where)


# ---------------------------------------------------------------------------------------------------------------------
# backward: the 3x3 data gradient
# ---------------------------------------------------------------------------------------------------------------------
def test_dgrad_reference_without_rounding_is_autograd():
    """DU = sc2 dA prelu'(u2) with dA the transposed 3x3 convolution of keep * G is the gradient of sum(G * keep * conv2(prelu(sc2 y + sh2)))
    with respect to y (tables held constant): pins the tap mirroring, the weight indexing and the PReLU branch."""
    gen = torch.Generator().manual_seed(2)
    n, H, W, mid, g = 2, 5, 7, 16, 8
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    y, Gt, w2, b2 = rn(n, H, W, mid).requires_grad_(True), rn(n, H, W, g), rn(g, mid, 3, 3), rn(g)
    sc, sh, sl = rn(mid), rn(mid), rn(mid).abs()
    keep = (torch.rand(n, H, W, g, generator=gen) > 0.3).double() / 0.7
    a = R._prelu(y * sc + sh, sl)
    out = F.conv2d(a.permute(0, 3, 1, 2), w2, b2, padding=1).permute(0, 2, 3, 1) * keep
    (out * Gt).sum().backward()
    ref, _ = R.conv3x3(a.detach(), torch.zeros_like(a.detach()), w2, b2, keep, False)
    assert _rel(ref, out.detach()) < 1e-12
    zero = torch.zeros(g, dtype=torch.float64)
    (chk,) = R.dgrad3_layer("t", Gt, torch.zeros_like(Gt), zero, zero, keep, y.detach(), sc, sh, sl, w2, False, 0)
    assert _rel(chk.ref, y.grad) < 1e-9, _rel(chk.ref, y.grad)
    w2.requires_grad_(True); b2.requires_grad_(True)
    out = F.conv2d(a.detach().permute(0, 3, 1, 2), w2, b2, padding=1).permute(0, 2, 3, 1) * keep
    (out * Gt).sum().backward()
    e = Gt * keep
    (dW, _), (db, _) = R.conv3x3_wgrad(e, torch.zeros_like(e), a.detach(), torch.zeros_like(a.detach()), False)
    assert _rel(dW, w2.grad) < 1e-9 and _rel(db, b2.grad) < 1e-9, (_rel(dW, w2.grad), _rel(db, b2.grad))


@functools.lru_cache(maxsize=None)
def _dgrad_inputs():
    """Layer (block 1, layer 1) of the faithful net with a synthetic bf16 gradient accumulator and fp32 (P, Q) rows of a realistic size."""
    cfg, P, keeps, c0, stored, checks = _faithful()
    gen = torch.Generator().manual_seed(9)
    X = stored["dense1"]
    G = R.bf16(torch.randn(X.shape, generator=gen, dtype=torch.float64) * 1e-2)
    Pr = R.f32(torch.randn(X.shape[-1], generator=gen, dtype=torch.float64) * 2e-3)
    Qr = R.f32(torch.randn(X.shape[-1], generator=gen, dtype=torch.float64) * 2e-3)
    l, p = 1, "features.dense1.layers.1"
    y = stored["bottleneck1.1"]
    sc2, sh2 = (R.f32(t) for t in R.bn_table(y, P[p + ".output_block.norm2.weight"], P[p + ".output_block.norm2.bias"]))
    args = dict(G=G, X=X, P=Pr, Q=Qr, keep=keeps[(0, l)], y=y, sc2=sc2, sh2=sh2, sl2=P[p + ".output_block.relu2.weight"],
                w2=P[p + ".output_block.conv2.weight"], rnd=True, c_off=cfg.initial_pixel_dim + l * cfg.densenet_growth_rate)
    return args, keeps[(0, 0)]


@pytest.mark.parametrize("defect", ["row_leak", "image_leak", "no_Q", "P_without_c_off", "wrong_keep", "no_sc2"])
def test_a_defective_data_gradient_leaves_the_gates(defect):
    args, other_keep = _dgrad_inputs()
    (intact,) = R.dgrad3_layer("l", **args)
    wrong_args = dict(args, keep=other_keep) if defect == "wrong_keep" else args
    (wrong,) = R.dgrad3_layer("l", defect=None if defect == "wrong_keep" else defect, **wrong_args)
    worst, bad, where = intact.ratio(R.bf16(wrong.ref))
    print(defect, "elements outside:", bad, "worst |error| / gate", worst, "kink set", int(intact.kink.sum()), "of", intact.kink.numel())
    assert bad > 0
    assert intact.ratio(R.bf16(intact.ref))[1] == 0


def test_simulated_correct_data_gradient_stays_inside_the_gates():
    """eff rows rounded after a move by +-tau, fp32 transposed convolution, fp32 epilogue (slope, scale), one bf16 store; the stored-operand
    variant (eff rows given) as well."""
    args, _ = _dgrad_inputs()
    g = args["w2"].shape[0]
    sl_ = slice(args["c_off"], args["c_off"] + g)
    gen = torch.Generator().manual_seed(4)
    f, tau, _, _ = R.eff_rows(args["G"][..., sl_], args["X"][..., sl_], args["P"][sl_], args["Q"][sl_], args["keep"], True)
    e = R.bf16(f + (torch.randint(0, 2, f.shape, generator=gen) * 2 - 1).double() * tau)
    w = R.bf16(args["w2"]).float()
    dA = F.conv_transpose2d(e.float().permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    y, sc, sh, sl = args["y"].float(), args["sc2"].float(), args["sh2"].float(), args["sl2"].float()
    u = y * sc + sh
    du = torch.where(u > 0, dA, sl * dA)
    DU = (sc * du).to(torch.bfloat16).double()
    for ey in (None, e):
        checks = R.dgrad3_layer("l", ey=ey, **args)
        worst, bad, where = checks[-1].ratio(DU)
        print("simulated data gradient, eff rows stored" if ey is not None else "simulated data gradient", "worst |error| / gate", worst)
        assert bad == 0, (worst, bad, where)
        if ey is not None:
            assert checks[0].ratio(e)[1] == 0


def test_weight_gradient_gates_bite_and_hold():
    """3x3 weight gradient: a tap that leaks across the row end leaves the gates; a simulated correct kernel (both operands rounded after a
    move by +-tau, fp32 sums, fp32 store) stays inside them."""
    args, _ = _dgrad_inputs()
    g = args["w2"].shape[0]
    sl_ = slice(args["c_off"], args["c_off"] + g)
    f, tau, e, de = R.eff_rows(args["G"][..., sl_], args["X"][..., sl_], args["P"][sl_], args["Q"][sl_], args["keep"], True)
    fa, taua, a, da = R.activation(args["y"], args["sc2"], args["sh2"], args["sl2"], True)
    (dW, dWd), (db, dbd) = R.conv3x3_wgrad(e, de, a, da, True)
    cW, cb = R.Check("dW2", "wgrad3x3", dW, dWd, False), R.Check("db2", "wgrad3x3", db, dbd, False)
    (wrong, _), _ = R.conv3x3_wgrad(e, de, a, da, True, "row_leak")
    worst, bad, where = cW.ratio(R.f32(wrong))
    print("row_leak in the weight gradient: elements outside", bad, "worst |error| / gate", worst)
    assert bad > 0
    gen = torch.Generator().manual_seed(6)
    sign = lambda t: (torch.randint(0, 2, t.shape, generator=gen) * 2 - 1).double()
    es, as_ = R.bf16(f + sign(f) * tau).float(), R.bf16(fa + sign(fa) * taua).float()
    M = es.numel() // g
    sim = torch.stack([es.reshape(M, g).T @ t.reshape(M, -1) for t in R._taps(as_)], -1).reshape(dW.shape).double()
    worst, bad, where = cW.ratio(sim)
    print("simulated weight gradient: worst |error| / gate", worst)
    assert bad == 0, (worst, bad, where)
    assert cb.ratio(es.reshape(M, g).sum(0).double())[1] == 0


def test_transition_data_gradient_reference():
    """Rounding off: the reference is autograd of the transition (tables held constant).  Rounding on: a value at a pixel no 2x2 window
    covers leaves the gates (the gate there is exactly 0); the intact result stays inside."""
    gen = torch.Generator().manual_seed(8)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    n, H, W, C, Nt = 2, 5, 7, 12, 6
    x, w, Gt = rn(n, H, W, C).requires_grad_(True), rn(Nt, C), rn(n, H // 2, W // 2, Nt)
    sc, sh, sl = rn(C), rn(C), rn(C).abs()
    a = R._prelu(x * sc + sh, sl)
    out = F.avg_pool2d(F.conv2d(a.permute(0, 3, 1, 2), w.reshape(Nt, C, 1, 1)), 2, 2).permute(0, 2, 3, 1)
    (out * Gt).sum().backward()
    zero = torch.zeros(Nt, dtype=torch.float64)
    for ch0 in (0, 8):
        DU, _, _ = R.transition_dgrad(Gt, torch.zeros_like(Gt), zero, zero, x.detach(), sc, sh, sl, w, False, ch0)
        assert _rel(DU, x.grad[..., ch0:]) < 1e-9
    assert bool((x.grad[:, 4:] == 0).all()) and bool((x.grad[:, :, 6:] == 0).all())
    b16 = lambda t: R.bf16(t)
    args = (b16(Gt * 1e-2), b16(rn(n, H // 2, W // 2, Nt)), R.f32(rn(Nt) * 1e-3), R.f32(rn(Nt) * 1e-3), b16(x.detach()), R.f32(sc), R.f32(sh), sl, w, True, 8)
    DU, d, kink = R.transition_dgrad(*args)
    chk = R.Check("t", "transition dgrad", DU, d, True, kink)
    assert chk.ratio(R.bf16(DU))[1] == 0
    wrong, _, _ = R.transition_dgrad(*args, defect="spill")
    worst, bad, where = chk.ratio(R.bf16(wrong))
    print("spill at uncovered pixels: elements outside", bad)
    assert bad > 0 and all(ix[1] == 4 or ix[2] == 6 for ix in where)


def test_head_pooling_backward_reference_is_autograd():
    gen = torch.Generator().manual_seed(12)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    n, H, W, C = 2, 3, 5, 9
    x, dF, sc, sh, sl = rn(n, H, W, C).requires_grad_(True), rn(n, C), rn(C), rn(C), rn(C).abs()
    (R._prelu(x * sc + sh, sl).mean((1, 2)) * dF).sum().backward()
    Gr, d, kink = R.head_pool_backward(dF, x.detach(), sc, sh, sl, 4)
    assert _rel(Gr, x.grad[..., 4:]) < 1e-9 and not kink.any()
    assert R.Check("h", "head pooling backward", Gr, d, True, kink).ratio(R.bf16(Gr * (1 + 3 * R.U)))[1] == 0
    assert R.Check("h", "head pooling backward", Gr, d, True, kink).ratio(R.bf16(Gr) * 1.02)[1] > 0


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_chained_backward_without_rounding_is_the_oracle_autograd(dropout):
    """The deferred (G, P, Q) formulation of tcvn_ops.h:118-136 and bn_link.h, chained over the small net in float64, against plain autograd
    of oracle.densenet_forward (the _oracle_grads pattern of test_densenet_gpu.py): every parameter gradient behind the stem and the
    gradient reaching block 1 (eff = G + P X + Q on its first channels = d loss / d pool0), 1e-9 relative, without and with keep masks."""
    cfg, coords, values, n_img = _net(dropout)
    sd, P = _params(cfg)
    keeps = _keeps(cfg, _map_sizes(cfg), n_img, 5) if dropout else None
    _, maps = R.run_forward(cfg, P, False, True, _conv0(cfg, P, coords, values, False), keeps)

    def provider(site, shape):
        if site.endswith(":out"):
            return torch.ones(shape, dtype=torch.float64)
        b, l = site.rsplit(":dense", 1)[1].split(".")
        return keeps[(int(b) - 1, int(l))].permute(0, 3, 1, 2)
    sub, leaves = {}, {}
    for k, v in sd.items():
        t = v.double() if v.is_floating_point() else v
        if k.startswith(PFX + ".") and v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            t = t.clone().requires_grad_(True)
            leaves[k[len(PFX) + 1:]] = t
        sub[k] = t
    ctx = O._Ctx(True, dropout, provider if dropout else None)
    out = O.densenet_forward(sub, PFX, cfg, O.preprocess_pixels(cfg, coords, values.double(), False), ctx)
    for tap in (":pool0", ":condense"):
        ctx.taps[PFX + tap].retain_grad()
    d_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (out * d_out).sum().backward()
    grads, g_pool0 = R.run_backward(cfg, P, maps, ctx.taps[PFX + ":condense"].grad, keeps)
    figures = {"pool0": _rel(g_pool0.permute(0, 3, 1, 2), ctx.taps[PFX + ":pool0"].grad)}
    zero_bias = []
    for k, v in grads.items():
        r = leaves[k].grad
        if k.endswith(("conv1.bias", "conv2.bias", "conv.bias")) and float(r.abs().max()) < 1e-9 * float(v.abs().max() + 1):      # exactly 0 in exact arithmetic where a train-mode BatchNorm follows
            zero_bias.append(k)
            assert float(v.abs().max()) < 1e-9, (k, float(v.abs().max()))
            continue
        figures[k] = _rel(v.reshape(r.shape), r)
    expected = [k for k in leaves if k.startswith(("features.dense", "features.transition", "features.final"))]
    assert sorted(grads) == sorted(expected), set(expected) ^ set(grads)
    print(dropout, "worst", max(figures.values()), "tensors", len(figures), "zero bias gradients", len(zero_bias))
    assert max(figures.values()) < 1e-9, {k: v for k, v in figures.items() if not v < 1e-9}


def test_1x1_backward_and_link_gates_bite_and_hold():
    """Rounding on, the 1x1 backward and a BatchNorm link of layer (block 1, layer 1): a correct kernel simulated in fp32 stays inside the
    gates of G[:, :cin], dW1 and the link's outputs; EY without the PY term, sums that miss one image, and a Q without its mean term leave them."""
    cfg, P, keeps, c0, stored, checks = _faithful()
    args, _ = _dgrad_inputs()
    gen = torch.Generator().manual_seed(21)
    y, cin, p = args["y"], args["c_off"], "features.dense1.layers.1"
    mid = y.shape[-1]
    DU = R.bf16(torch.randn(y.shape, generator=gen, dtype=torch.float64) * 1e-2)
    PY, QY = (R.f32(torch.randn(mid, generator=gen, dtype=torch.float64) * 2e-3) for _ in range(2))
    xin, Gb = args["X"][..., :cin], args["G"][..., :cin]
    n1 = p + ".bottleneck_block.norm1"
    sc1, sh1 = (R.f32(t) for t in R.bn_table(xin, P[n1 + ".weight"], P[n1 + ".bias"]))
    sl1 = P[p + ".bottleneck_block.relu1.weight"]
    w1 = P[p + ".bottleneck_block.conv1.weight"].reshape(mid, cin)
    _, _, a1, da1 = R.activation(xin, sc1, sh1, sl1, True)
    run = lambda py: R.conv1x1_backward(DU, y, py, QY, a1, da1, w1, Gb, xin, sc1, sh1, sl1, True)
    out, sums, gates = run(PY)
    cG = R.Check("G", "1x1 backward", out["G"][0], out["G"][1], True, out["G"][2])
    cW = R.Check("dW1", "1x1 backward", out["dW1"][0], out["dW1"][1], False)
    # a correct kernel in fp32
    e = (DU.float() + PY.float() * y.float() + QY.float()).to(torch.bfloat16).float()
    dX = e @ R.bf16(w1).float()
    u = xin.float() * sc1.float() + sh1.float()
    dU = torch.where(u > 0, dX, sl1.float() * dX)
    sim_G = (Gb.float() + sc1.float() * dU).to(torch.bfloat16).double()
    M = e.numel() // mid
    sim_W = (e.reshape(M, mid).T @ a1.float().reshape(M, cin)).double()
    assert cG.ratio(sim_G)[1] == 0 and cW.ratio(sim_W)[1] == 0, (cG.ratio(sim_G)[:2], cW.ratio(sim_W)[:2])
    # EY without PY * Y
    wrong, _, _ = run(torch.zeros_like(PY))
    assert cG.ratio(R.bf16(wrong["G"][0]))[1] > 0 and cW.ratio(R.f32(wrong["dW1"][0]))[1] > 0
    # the link
    xf = xin.reshape(M, cin)
    mu, var = xf.mean(0), ((xf - xf.mean(0)) ** 2).mean(0)
    lk = R.bn_link(sums, gates, mu, var, P[n1 + ".weight"], M)
    sim_sums = (dU.double().reshape(M, cin).sum(0), (dU.double() * xin).reshape(M, cin).sum(0),
                (dX.double() * torch.where(u > 0, torch.zeros_like(u), u).double()).reshape(M, cin).sum(0))
    sim = R.bn_link(sim_sums, gates, mu, var, P[n1 + ".weight"], M)
    for q in ("dgamma", "dbeta", "dslope", "P", "Q"):
        c = R.Check(q, "link", lk[q][0], lk[q][1], False)
        assert c.ratio(R.f32(sim[q][0]))[1] == 0, (q, c.ratio(R.f32(sim[q][0]))[:2])
    n = xin.shape[0]
    part = lambda t: t.reshape(n, -1, cin)[1:].reshape(-1, cin).sum(0)        # the first image's pixels missing from every sum
    missing = R.bn_link((part(dU.double()), part(dU.double() * xin), sim_sums[2]), gates, mu, var, P[n1 + ".weight"], M)
    for q in ("dgamma", "dbeta", "P", "Q"):
        assert R.Check(q, "link", lk[q][0], lk[q][1], False).ratio(R.f32(missing[q][0]))[1] > 0, q
    no_mean = R.bn_link(sim_sums, gates, torch.zeros_like(mu), var, P[n1 + ".weight"], M)
    assert R.Check("Q", "link", lk["Q"][0], lk["Q"][1], False).ratio(R.f32(no_mean["Q"][0]))[1] > 0


# ---------------------------------------------------------------------------------------------------------------------
# the fused 1x1 backward at the hook test's widths and trip counts
# ---------------------------------------------------------------------------------------------------------------------
def layer_case(name):
    """The hook test's own cases (test_densenet_layers_float64_gpu.py, LAYER_CASES) -> cfg, coords, values, n_img.
    mod4: one block, cin = 228 .. 388 (cin % 8 == 4: production block 4's widths, two to four 128-column slices), event map + two prong
    maps of 13 x 9 pixels.  trips: one block, cin = 232 .. 392, 27 prong maps of 25 x 17 pixels: M = 11 475 = 179 full 64-pixel tiles + 19
    rows, more than the fused 1x1 backward's grid cap at three slices (170 workgroups) and at four (128)."""
    base = dict(pixel_noise_std=0.0, num_encoder_layers=2, dropout=0.0)
    if name == "mod4":
        cfg = O.tutorial_config(initial_pixel_dim=228, densenet_structure=[6], pixel_shape=(56, 40), **base)
        b = O.synthetic_batch([2], 41, cfg, event_hits=(60, 200), prong_hits=(20, 120))
        pc = b[5].clone()
        pc[:, 0] += 1                                                     # image 0 = the event map
        return cfg, torch.cat([b[2], pc]).contiguous(), torch.cat([b[3], b[6]]).contiguous(), 3
    assert name == "trips"
    cfg = O.tutorial_config(initial_pixel_dim=232, densenet_structure=[6], pixel_shape=(104, 72), **base)
    b = O.synthetic_batch([14, 13], 43, cfg, prong_hits=(60, 400))
    return cfg, b[5], b[6], 27


def fused_grid(M, cin):
    """(row workgroups, 128-column slices, 64-pixel tiles) of the fused 1x1 backward: bwd1x1_fused.hip, bwd1x1_fused_nblk."""
    slices, tiles = -(-cin // 128), -(-M // 64)
    return min(tiles, max(64, 512 // slices)), slices, tiles


@pytest.mark.parametrize("case", ["mod4", "trips"])
def test_new_layer_cases_stay_under_the_kink_cap(case):
    """With the reference alone (the bf16-faithful forward, tables from its own maps): the PReLU kink sets of norm1 and norm2 of every
    layer and of final_norm -- they depend on the forward maps only -- hold at most KINK_CAP of their tensor."""
    cfg, coords, values, n_img = layer_case(case)
    _, P = _params(cfg)
    _, maps = R.run_forward(cfg, P, True, True, _conv0(cfg, P, coords, values, True))
    x, g = maps["dense1"], cfg.densenet_growth_rate
    assert x.shape[0] * x.shape[1] * x.shape[2] == {"mod4": 351, "trips": 11475}[case]

    def share(t, norm):
        sc, sh = (R.f32(v) for v in R.bn_table(t, P[norm + ".weight"], P[norm + ".bias"]))
        kink = (t * sc + sh).abs() <= R.R(2) * ((t * sc).abs() + sh.abs())
        return int(kink.sum()) / kink.numel()
    worst = share(x, "features.final_norm")
    for l in range(cfg.densenet_structure[0]):
        p = f"features.dense1.layers.{l}"
        cin = cfg.initial_pixel_dim + l * g
        assert cin % 8 == 4 or case == "trips"
        worst = max(worst, share(x[..., :cin], p + ".bottleneck_block.norm1"), share(maps[f"bottleneck1.{l}"], p + ".output_block.norm2"))
    print(case, "largest share of a tensor at a PReLU kink:", worst)
    assert worst <= R.KINK_CAP


@functools.lru_cache(maxsize=None)
def _fused_operands(M, cin):
    """Synthetic operands of one fused 1x1 backward launch at the hook cases' own M and cin (bf16 maps, fp32 rows and tables), the block's
    buffers 32 channels wider than cin (the layer's own 3x3 slice behind it), and the intact reference with its gates."""
    gen = torch.Generator().manual_seed(1000 * cin + M)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    mid, ld = 128, cin + 32
    o = dict(M=M, cin=cin, DU=R.bf16(rn(M, mid) * 1e-2), Y=R.bf16(rn(M, mid)), PY=R.f32(rn(mid) * 2e-3), QY=R.f32(rn(mid) * 2e-3),
             X=R.bf16(rn(M, ld)), G=R.bf16(rn(M, ld) * 1e-2), gamma=1.0 + 0.1 * rn(cin), w1=rn(mid, cin) * 0.05, sl=R.f32(0.25 + 0.05 * rn(cin)))
    xin = o["X"][:, :cin]
    o["sc"], o["sh"] = (R.f32(t) for t in R.bn_table(xin, o["gamma"], 0.1 * rn(cin)))
    _, _, a1, da1 = R.activation(xin, o["sc"], o["sh"], o["sl"], True)
    out, sums, gates = R.conv1x1_backward(o["DU"], o["Y"], o["PY"], o["QY"], a1, da1, o["w1"], o["G"][:, :cin], xin, o["sc"], o["sh"], o["sl"], True)
    o["mu"], o["var"] = xin.mean(0), ((xin - xin.mean(0)) ** 2).mean(0)
    lk = R.bn_link(sums, gates, o["mu"], o["var"], o["gamma"], M)
    checks = {"G": R.Check("G", "1x1 backward", out["G"][0], out["G"][1], True, out["G"][2]),
              "dW1": R.Check("dW1", "1x1 backward", out["dW1"][0], out["dW1"][1], False),
              "db1": R.Check("db1", "1x1 backward", out["db1"][0], out["db1"][1], False)}
    for q in ("dgamma", "dbeta", "dslope", "P", "Q"):
        checks[q] = R.Check(q, "norm1 link", lk[q][0], lk[q][1], False)
    return o, gates, checks


def _fused_kernel(o, defect=None):
    """k_bwd1x1_fused_bf16 (bwd1x1_fused.hip) in fp32, in the kernel's order: workgroup b of nblk takes the 64-pixel tiles b, b + nblk, ...;
    per tile EY = bf16(DU + PY Y + QY), dX = EY W1, the epilogue against x, G = bf16(G + sc dU); every thread keeps fp32 sums over its rows
    (row % 16) of all its workgroup's tiles and widens them to double at the end; the weight-gradient tile and the bias column sums stay
    in fp32 per workgroup over all its tiles and leave as one slab, added over the workgroups in fp32.
    defect: "slice_table" columns 256..383 read the table rows of columns 128..255; "drop_last4" the last four channels of a width with
    cin % 8 == 4 missing from G and dW1; "foreign_written" the four channels behind them stored with the chunk; "second_trip_missing"
    every tile of a second trip missing from dW1, db1 and the sums; "second_trip_rows" the second trip's G rows stored at the first
    trip's offsets; "reset_between_tiles" the weight-gradient accumulators zeroed in front of every tile; "one_tile_missing" tile 0
    missing from the three sums.  -> {G (all ld columns), dW1, db1, sums}, the results as stored."""
    M, cin = o["M"], o["cin"]
    nblk, slices, tiles = fused_grid(M, cin)
    trips = -(-tiles // nblk)
    f = lambda t: t.float()
    sc, sh, sl = f(o["sc"]).clone(), f(o["sh"]).clone(), f(o["sl"]).clone()
    if defect == "slice_table":
        k = min(384, cin) - 256
        assert k > 0
        for t in (sc, sh, sl):
            t[256:256 + k] = t[128:128 + k].clone()
    x = f(o["X"][:, :cin])
    e = (f(o["DU"]) + f(o["PY"]) * f(o["Y"]) + f(o["QY"])).to(torch.bfloat16).float()
    dX = e @ f(R.bf16(o["w1"]))
    u = x * sc + sh
    dU = torch.where(u > 0, dX, sl * dX)
    G = o["G"].clone()
    G[:, :cin] = (f(o["G"][:, :cin]) + sc * dU).to(torch.bfloat16).double()
    a = torch.where(u > 0, u, sl * u).to(torch.bfloat16).float()
    rows = trips * nblk * 64

    def tiled(t):                                                           # [M, C] -> [trip, workgroup, 64, C], rows behind M zero
        return torch.cat([t, t.new_zeros(rows - M, t.shape[1])]).reshape(trips, nblk, 64, t.shape[1])
    live = torch.ones(trips, nblk)                                          # tiles that reach the sums and the slabs
    if defect == "second_trip_missing":
        live[1:] = 0
    live_w = live.clone()
    if defect == "reset_between_tiles":                                     # only a workgroup's last tile survives
        last = torch.tensor([(tiles - 1 - b) // nblk for b in range(nblk)])
        live_w = (torch.arange(trips)[:, None] == last[None, :]).float()
    live_s = live.clone()
    if defect == "one_tile_missing":
        live_s[0, 0] = 0
    if defect == "second_trip_rows":
        assert trips == 2
        new, Gb = tiled(G[:, :cin]), tiled(o["G"][:, :cin])
        n2 = tiles - nblk                                                   # tiles of the second trip; the last one is partial
        mixed = torch.cat([new[0], Gb[1]]).clone()                          # [tile, 64, cin]: trip 0 as stored, trip 1 never written ...
        mixed[:n2 - 1] = new[1][:n2 - 1]                                    # ... its rows land on trip 0's tiles
        mixed[n2 - 1][:M - (tiles - 1) * 64] = new[1][n2 - 1][:M - (tiles - 1) * 64]
        G[:, :cin] = mixed.reshape(rows, cin)[:M]
    if defect == "drop_last4":
        assert cin % 8 == 4
        G[:, cin - 4:cin] = o["G"][:, cin - 4:cin]
        a = a.clone()
        a[:, cin - 4:] = 0
    if defect == "foreign_written":                                         # the 16-byte store of the last chunk, its foreign half with the
        assert cin % 8 == 4                                                 # values of the channels in front of it
        G[:, cin:cin + 4] = (f(o["G"][:, cin:cin + 4]) + sc[cin - 4:] * dU[:, cin - 4:]).to(torch.bfloat16).double()
    et, at = tiled(e), tiled(a)
    accW, accb = torch.zeros(nblk, 128, cin), torch.zeros(nblk, 16, 128)
    st = [torch.zeros(nblk, 16, cin) for _ in range(3)]
    terms = [tiled(t) for t in (dU, dU * x, torch.where(u > 0, torch.zeros_like(dX), dX) * u)]
    for t in range(trips):
        accW += live_w[t][:, None, None] * torch.bmm(et[t].transpose(1, 2), at[t])
        for i in range(4):
            accb += live[t][:, None, None] * et[t][:, 16 * i: 16 * i + 16]
            for s, term in zip(st, terms):
                s += live_s[t][:, None, None] * term[t][:, 16 * i: 16 * i + 16]
    return dict(G=G, dW1=accW.sum(0).double(), db1=accb.sum(1).sum(0).double(), sums=tuple(s.double().sum((0, 1)) for s in st))


def _outside(o, gates, checks, sim):
    """Elements outside the gate per result of a simulated launch (the link from the launch's own sums)."""
    lk = R.bn_link(sim["sums"], gates, o["mu"], o["var"], o["gamma"], o["M"])
    got = dict(G=sim["G"][:, :o["cin"]], dW1=sim["dW1"], db1=sim["db1"], **{q: R.f32(lk[q][0]) for q in ("dgamma", "dbeta", "dslope", "P", "Q")})
    return {k: (c.ratio(got[k])[1], round(c.ratio(got[k])[0], 3)) for k, c in checks.items()}


FUSED_SIZES = [(351, 260), (11475, 260), (11475, 392)]                      # mod4's layer 1; trips' M at three and at four slices


@pytest.mark.parametrize("M,cin", FUSED_SIZES)
def test_fused_1x1_backward_gates_hold_and_bite_at_the_hook_cases_sizes(M, cin):
    """The sum gates grow with M (R(M) of the sum of magnitudes), so what bites at 1 275 pixels need not bite at 11 475: at the hook
    cases' own sizes a correct kernel summing tile by tile and slab by slab stays inside every gate, and each defect of a column slice,
    of the half-foreign last chunk and of a workgroup's second tile leaves the gates it must.
    Resolution of the sum checks at M = 11 475 (printed below): ONE missing 64-row tile still leaves the gates of dgamma1, dbeta1,
    dslope1, P and Q -- on 154 .. 288 of the cin channels, worst |error| / gate 5.6 .. 8.7 on these operands."""
    o, gates, checks = _fused_operands(M, cin)
    nblk, slices, tiles = fused_grid(M, cin)
    assert slices == -(-cin // 128) >= 3 and (tiles > nblk) == (M == 11475)
    assert int(checks["G"].kink.sum()) <= R.KINK_CAP * checks["G"].kink.numel()
    ok = _outside(o, gates, checks, _fused_kernel(o))
    print(M, cin, "correct kernel, (elements outside, worst |error| / gate):", ok)
    assert all(v[0] == 0 for v in ok.values()), ok
    intact = _fused_kernel(o)
    assert torch.equal(intact["G"][:, cin:], o["G"][:, cin:])

    def bites(defect, *results):
        out = _outside(o, gates, checks, _fused_kernel(o, defect))
        print(M, cin, defect, out)
        for r in results:
            assert out[r][0] > 0, (defect, r, out)
        return out
    out = bites("slice_table", "G", "dbeta", "dgamma", "dslope")
    assert all(ix[1] >= 256 for ix in checks["G"].ratio(_fused_kernel(o, "slice_table")["G"][:, :cin])[2])
    if cin % 8 == 4:
        bites("drop_last4", "G", "dW1")
        wrong = _fused_kernel(o, "foreign_written")
        assert not torch.equal(wrong["G"][:, cin:], o["G"][:, cin:]) and checks["G"].ratio(wrong["G"][:, :cin])[1] == 0
    if tiles > nblk:
        assert tiles - nblk == {3: 10, 4: 52}[slices] and M % 64 == 19       # the partial last tile lands in the second trip
        bites("second_trip_missing", "dW1", "db1", "dbeta", "dgamma", "dslope", "P", "Q")
        bites("second_trip_rows", "G")
        bites("reset_between_tiles", "dW1")
        one = _outside(o, gates, checks, _fused_kernel(o, "one_tile_missing"))
        print(M, cin, "one 64-row tile missing from the sums (resolution of the sum checks at this size):", {q: one[q] for q in ("dgamma", "dbeta", "dslope", "P", "Q")})
        assert all(one[q][0] > 0 for q in ("dgamma", "dbeta", "dslope", "P", "Q")), one


# ---------------------------------------------------------------------------------------------------------------------
# the frozen backward (hit gradients): running statistics, P = Q = PY = QY = 0, no dropout
# ---------------------------------------------------------------------------------------------------------------------
def frozen_case(name):
    """The GPU test's cases (test_densenet_layers_float64_gpu._case) -> cfg, coords, values, n_img.  The frozen leg runs on running
    statistics, so its kink sets differ from the train leg's; FROZEN_WEIGHT_SEED gives a case another weight seed for the frozen leg
    should its share of kink elements exceed KINK_CAP (test_frozen_cases_stay_under_the_kink_cap; none does at seed 19)."""
    from test_densenet_layers_float64_gpu import _case
    return _case(name)


FROZEN_WEIGHT_SEED = {}      # case -> weight seed of the frozen leg where it is not 19


def frozen_seed(case):
    return FROZEN_WEIGHT_SEED.get(case, 19)


@functools.lru_cache(maxsize=None)
def _frozen_maps(case, rnd):
    """Eval-mode forward of the reference alone (running-statistics tables) -> cfg, P, maps, tables, n_img, coords, values."""
    cfg, coords, values, n_img = frozen_case(case)
    _, P = _params(cfg, frozen_seed(case))
    _, maps = R.run_forward(cfg, P, rnd, False, _conv0(cfg, P, coords, values, rnd))
    return cfg, P, maps, R.running_tables(cfg, P, rnd), n_img, coords, values


@pytest.mark.parametrize("case", ["narrow", "wide", "odd"])
def test_frozen_chain_without_rounding_is_the_oracle_autograd(case):
    """run_backward_frozen with rnd off against float64 autograd through O.densenet_forward in eval mode (running statistics, no dropout):
    the gradient reaching the conv0 map (DU0), every block's accumulator where the oracle exposes the concat buffer, and the hit-value
    gradient behind the gather -- to the 1e-9 relative of the train-mode pin."""
    import hit_gradients_reference as H
    cfg, P, maps, tables, n_img, coords, values = _frozen_maps(case, False)
    sd = O.fill_state(cfg, frozen_seed(case))
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    v = values.double().clone().requires_grad_(True)
    ctx = O._Ctx(False, 0.0, None)
    out = O.densenet_forward(sd64, PFX, cfg, O.preprocess_pixels(cfg, coords, v, False), ctx)
    ctx.taps[PFX + ":conv0"].retain_grad()
    d_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (out * d_out).sum().backward()
    du0, state = R.run_backward_frozen(cfg, P, maps, tables, d_out)
    o = "output_block.norm"
    sc, sh = R.bn_table(None, P[o + ".weight"], P[o + ".bias"], (P[o + ".running_mean"], P[o + ".running_var"]))
    figures = {"out": _rel(R._prelu(maps["output_linear"] * sc + sh, P["output_block.relu.weight"]), out.detach()),
               "du0": _rel(du0.permute(0, 3, 1, 2), ctx.taps[PFX + ":conv0"].grad)}
    got = H.gather(du0, P["features.conv0.weight"], coords, values, tuple(cfg.pixel_shape), 0)
    own = torch.tensor(H.owners(coords, n_img, *cfg.pixel_shape))
    # the oracle scatters a list with duplicates by index_put: the gradient lands on the entry that owns the pixel there too, or on all
    # of them; compare the owners only, the rest must be exactly zero on the library's side
    figures["d_values"] = _rel(got[own], v.grad[own])
    assert bool((got[~own] == 0).all())
    print(case, figures, "max |du0|", float(du0.abs().max()))
    assert float(du0.abs().max()) > 0 and max(figures.values()) < 1e-9, figures


@pytest.mark.parametrize("case", ["wide", "wide-dropout", "narrow", "narrow-one", "odd", "mod4", "trips"])
def test_frozen_cases_stay_under_the_kink_cap(case):
    """Under running-statistics tables, from the reference alone (the bf16-faithful eval forward): the share of elements at a PReLU kink of
    norm0, of every layer's norm1 and norm2, of every transition norm and of final_norm stays <= KINK_CAP; no row of the output block's
    BatchNorm1d sits at a kink."""
    cfg, P, maps, tables, n_img, _, _ = _frozen_maps(case, True)
    g = cfg.densenet_growth_rate

    def share(t, norm):
        sc, sh = tables[norm]
        kink = (t * sc + sh).abs() <= R.R(2) * ((t * sc).abs() + sh.abs())
        return int(kink.sum()) / kink.numel()
    worst = {"norm0": share(maps["conv0"], "features.norm0")}
    ch = cfg.initial_pixel_dim
    for b, layers in enumerate(cfg.densenet_structure):
        x = maps[f"dense{b + 1}"]
        for l in range(layers):
            p = f"features.dense{b + 1}.layers.{l}"
            worst[f"norm1 {b + 1}.{l}"] = share(x[..., :ch + l * g], p + ".bottleneck_block.norm1")
            worst[f"norm2 {b + 1}.{l}"] = share(maps[f"bottleneck{b + 1}.{l}"], p + ".output_block.norm2")
        ch += layers * g
        if b + 1 < len(cfg.densenet_structure):
            worst[f"transition{b + 1}"] = share(x, f"features.transition{b + 1}.norm")
            ch //= 2
        else:
            worst["final_norm"] = share(x, "features.final_norm")
    o = "output_block.norm"
    d_out = torch.randn(n_img, maps["output_linear"].shape[1], generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    _, _, krows = R.output_block_backward_frozen(d_out, maps["output_linear"], P[o + ".weight"], P[o + ".bias"], P[o + ".running_mean"],
                                                 P[o + ".running_var"], P["output_block.relu.weight"], P["output_block.linear.weight"])
    top = max(worst, key=worst.get)
    print(case, "largest share of a tensor at a PReLU kink under running statistics:", worst[top], top, "output-block kink rows", int(krows[:, 0].sum()))
    assert worst[top] <= R.KINK_CAP, (top, worst[top])
    assert not krows.any()


@functools.lru_cache(maxsize=None)
def _frozen_layer_state(case):
    """The bf16-faithful frozen forward of a case and the state its LAST layer of block 1 finds in the frozen backward: G of the block as
    its first writer left it (the unrounded frozen chain's, rounded to bf16), zero rows."""
    cfg, P, maps, tables, n_img, coords, values = _frozen_maps(case, True)
    d_out = torch.randn(n_img, maps["output_linear"].shape[1], generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    du0, state = R.run_backward_frozen(cfg, P, maps, tables, d_out)
    return cfg, P, maps, tables, n_img, coords, values, d_out, du0, state


def _stale_rows(x, G_first, d_cond, P, norm, relu, tables_batch):
    """(P, Q) of a block as the head's link of a TRAINING backward leaves them (bn_link on batch statistics of the same maps)."""
    sc, sh = tables_batch
    _, sums, gates = R.head_backward(d_cond, x, sc, sh, P[relu + ".weight"])
    xf = x.reshape(-1, x.shape[-1])
    mu, var = xf.mean(0), ((xf - xf.mean(0)) ** 2).mean(0)
    lk = R.bn_link(sums, gates, mu, var, P[norm + ".weight"], xf.shape[0])
    return R.f32(lk["P"][0]), R.f32(lk["Q"][0])


FROZEN_DEFECTS = ["stale_pq", "keep", "batch_tables", "odd_edge", "slice_not_accumulated", "gather_stride"]


@pytest.mark.parametrize("defect", FROZEN_DEFECTS)
def test_a_defective_frozen_schedule_leaves_the_gates(defect):
    """Each defect a frozen schedule threaded through the training one can have, at the GPU cases' own sizes (`odd`: one block, cin up to
    538, five 128-column slices; `wide`: the odd 9 x 69 map in front of the transition): the worst |error| / gate of the check it
    affects exceeds 1, and the intact result stays inside."""
    case = "wide" if defect == "odd_edge" else "odd"
    cfg, P, maps, tables, n_img, coords, values, d_out, du0, state = _frozen_layer_state(case)
    g, mid = cfg.densenet_growth_rate, cfg.densenet_batch_norm_size * cfg.densenet_growth_rate
    L = cfg.densenet_structure[0]
    l = L - 1
    cin = cfg.initial_pixel_dim + l * g
    p = f"features.dense1.layers.{l}"
    x, y = maps["dense1"], maps[f"bottleneck1.{l}"]
    Ct = x.shape[-1]
    zero = torch.zeros(Ct, dtype=torch.float64)
    G = R.bf16(state["G1:first"])
    sc2, sh2 = tables[p + ".output_block.norm2"]
    sl2, w2 = P[p + ".output_block.relu2.weight"], P[p + ".output_block.conv2.weight"]
    dgrad = lambda **kw: R.dgrad3_layer("l", **dict(dict(G=G, X=x, P=zero, Q=zero, keep=None, y=y, sc2=sc2, sh2=sh2, sl2=sl2, w2=w2, rnd=True,
                                                         c_off=cin), **kw))[0]
    if defect in ("stale_pq", "keep", "batch_tables"):
        intact = dgrad()
        if defect == "stale_pq":
            assert len(cfg.densenet_structure) == 1
            nf = "features.final_norm"
            Ps, Qs = _stale_rows(x, G, state["dcondense"], P, nf, "features.final_relu", R.bn_table(x, P[nf + ".weight"], P[nf + ".bias"]))
            assert float(Ps.abs().max()) > 0
            wrong = dgrad(P=Ps, Q=Qs)
        elif defect == "keep":
            ks = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(0.1, dtype=torch.float32)))
            keep = (torch.rand(G.shape[:3] + (g,), generator=torch.Generator().manual_seed(7)) >= 0.1).double() * ks
            wrong = dgrad(keep=keep)
        else:
            n2 = p + ".output_block.norm2"
            scb, shb = (R.f32(t) for t in R.bn_table(y, P[n2 + ".weight"], P[n2 + ".bias"]))
            wrong = dgrad(sc2=scb, sh2=shb)
        got = R.bf16(wrong.ref)
    elif defect == "odd_edge":
        assert x.shape[1:3] == (9, 69)
        t = "features.transition1"
        xn = maps["dense2"]
        zn = torch.zeros(xn.shape[-1], dtype=torch.float64)
        args = (R.bf16(state["G2"]), xn, zn, zn, x, *tables[t + ".norm"], P[t + ".relu.weight"], P[t + ".conv.weight"].reshape(Ct // 2, Ct), True, Ct - g)
        DU, d, kink = R.transition_dgrad(*args)
        intact = R.Check("t", "transition dgrad", DU, d, True, kink)
        got = R.bf16(R.transition_dgrad(*args, defect="spill")[0])
        assert float(intact.gate[:, 8].max()) == 0 and float(intact.gate[:, :, 68].max()) == 0      # exactly zero where no window covers
    elif defect == "slice_not_accumulated":
        DU = R.bf16(state[f"du1.{l}"])
        xin = x[..., :cin]
        sc1, sh1 = tables[p + ".bottleneck_block.norm1"]
        sl1 = P[p + ".bottleneck_block.relu1.weight"]
        _, _, a1, da1 = R.activation(xin, sc1, sh1, sl1, True)
        zy = torch.zeros(mid, dtype=torch.float64)
        out, _, _ = R.conv1x1_backward(DU, y, zy, zy, a1, da1, P[p + ".bottleneck_block.conv1.weight"].reshape(mid, cin), G[..., :cin], xin,
                                       sc1, sh1, sl1, True)
        intact = R.Check("G", "1x1 backward", out["G"][0], out["G"][1], True, out["G"][2])
        assert cin > 256
        got = R.bf16(out["G"][0]).clone()
        got[..., 128:256] = G[..., 128:256]
    else:
        N = du0.shape[-1]
        stored = R.bf16(du0)
        w0 = P["features.conv0.weight"]
        intact = R.hit_gradient_check(stored, w0, coords, values, tuple(cfg.pixel_shape), 0)
        flat = torch.cat([stored.reshape(-1), torch.zeros(stored.numel(), dtype=torch.float64)])
        rows = torch.arange(stored.numel() // N)
        strided = flat[(2 * rows[:, None] * N + torch.arange(N)[None, :]).reshape(-1)].reshape(stored.shape)      # row r read at byte offset r * N * 4
        import hit_gradients_reference as H
        got = R.f32(H.gather(strided, w0, coords, values, tuple(cfg.pixel_shape), 0))
    worst, bad, where = intact.ratio(got)
    ok = intact.ratio((R.f32 if defect == "gather_stride" else R.bf16)(intact.ref))
    print(defect, case, "elements outside:", bad, "worst |error| / gate", worst, "intact:", ok[:2], "max |ref|", float(intact.ref.abs().max()))
    assert float(intact.ref.abs().max()) > 0 and ok[1] == 0 and ok[0] <= 1.0
    assert bad > 0 and worst > 1.0
