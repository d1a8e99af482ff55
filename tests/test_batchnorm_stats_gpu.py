"""Train-mode BatchNorm state of the HIP DenseNet against a float64 recomputation over the engine's own stored maps.  Needs an MI355X.

Every producing kernel takes its statistics from the ROUNDED values it stores (fwd1x1_fused.hip "statistics of the rounded values", the
3x3 pair kernel's epilogue, k_pool0, the generic kernels), so mean / variance / (scale, shift) / running statistics recomputed in float64
from the tap() views are the specification of the operation itself -- no bf16 drift between the two sides, whichever build produced
the maps.  Checked for every BatchNorm of the net: its table in raw:tabs, its (mean, variance) row, running_mean / running_var after one
and after two train-mode forwards (the second on another image count), on three builds: the bf16 product path (link-free statistics,
bn_lf.h), bf16 with the link kernels (TCVN_NO_LF on the validation build, ONE child process for all cases) and fp32.

Gates (all from the arithmetic; u = 2^-24):
  * (mean, E[x^2]) rows: |mean - ref| <= 1e-9 s + W 2^-25 / n and |E2 - ref| <= 1e-9 s^2 + W 2^-17 / n (s = sqrt(ref E2)): the fixed-point
    resolution of one lf_add times the W = 1024 workgroups that add per channel at most (grid caps: 768 in fwd1x1_fused_nblk,
    fwd1x1_fused.hip:439; 256 in tile_grid, tile3x3.h).  PLUS one rounding step that bound leaves out: the producers sum a
    lane's values in fp32 before they widen to double -- the fused 1x1 kernels four rows per 64-row tile and workgroup
    (fwd1x1_fused.hip:195-201, :387-393), the 3x3 pair kernel the 16 positions of one epilogue (epilogue_impl of k_conv3x3_fwd_pair_bf16, conv3x3_fwd_tile.hip) -- which costs
    at most (L - 1) u mean|x| on the mean and L u E2 on E2 for an fp32 chain of L values.  The other producers (_chains):
      - k_pool0 / k_pool0_vec64 (elementwise.hip:189, :449), k_rows_bn_fwd (rows.hip:69), the generic k_conv_fwd (StatAcc is double for
        both types, conv_tile.h:160-161) and k_conv3x3_fwd_f32 (conv3x3_f32.hip:279) widen every value to double first: L = 1, no term;
      - k_stem_fwd2_bf16 adds one pixel per lane and 8 x 16 tile in fp32 (stem.hip:583-584): L = tiles per workgroup;
      - k_gemm_nt_bf16<fwd> (transition, unfused 1x1): 64-row instance (Kp <= 256) four rows per tile in fp32 running sums
        (gemm_nt.hip:88, :223), 128-row instance eight rows per tile, then double (gemm_nt.hip:250): L = 4 x tiles per workgroup, or 8;
      - k_conv1x1_fwd_f32 the 16 positions of one epilogue (conv1x1_f32.hip:390-401): L = 16, also taken where the generic kernel
        (L = 1) may have run instead (fp32 1x1 and transition convolutions).
    Tiles per workgroup = ceil(tiles / min(tiles, grid cap)), 1 at these shapes under every cap (the test asserts it).
  * tables and running statistics: 8 u of the magnitude of their terms (a handful of correctly rounded fp32 operations) plus the
    row gates above propagated through the formula.
"""
import functools

import pytest
import torch

from oracle import tcvn_oracle as O
from test_densenet_gpu import PFX, _conv0_activity, _engine

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
W_ADD = 1024          # workgroups that add to one channel's accumulators, at most (see the module docstring)
EPS = 1e-5
F32, BF16 = 0, 1


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _all_maps(batch):
    """One COO list over the event map and the prong maps of a synthetic batch with one event: image 0 = the event map."""
    pc = batch[5].clone()
    pc[:, 0] += 1
    n = 1 + int(batch[7].sum())
    return torch.cat([batch[2], pc]).contiguous(), torch.cat([batch[3], batch[6]]).contiguous(), n


def _case(name, dropout=0.1):
    """-> cfg, [(coords, values, n_img) per train step]"""
    base = dict(dropout=dropout, pixel_noise_std=0.0, num_encoder_layers=2)
    if name == "B":       # cin = 250 .. 538 (cin % 8 == 2); K extents pass 512 at the last layer, where the fused forward falls back
        cfg = O.tutorial_config(initial_pixel_dim=250, densenet_structure=[10], pixel_shape=(56, 40), **base)
        hits = dict(event_hits=(60, 200), prong_hits=(20, 120))
    else:                 # block 1: 26 x 18 positions per image, block 3: 6 x 4
        cfg = O.tutorial_config(pixel_shape=(104, 72), densenet_structure=[3, 3, 2], **base)
        hits = {}
    if name == "C":       # one image, a handful of hits: most conv0 rows are reached by no hit
        b = O.synthetic_batch([1], 53, cfg, prong_hits=(6, 10))
        return cfg, [(b[5], b[6], 1)]
    b1, b2 = O.synthetic_batch([2], 41, cfg, **hits), O.synthetic_batch([2], 43, cfg, **hits)
    return cfg, [_all_maps(b1), (b2[5], b2[6], 2)]


def _bn_list(cfg):
    """Every BatchNorm2d of the net in tab_off order (densenet.hip): (name, kind, block, layer, channels)."""
    g, mid = cfg.densenet_growth_rate, cfg.densenet_batch_norm_size * cfg.densenet_growth_rate
    out = [("features.norm0", "n0", -1, -1, cfg.initial_pixel_dim)]
    ch, nb = cfg.initial_pixel_dim, len(cfg.densenet_structure)
    for b, layers in enumerate(cfg.densenet_structure):
        for l in range(layers):
            p = f"features.dense{b + 1}.layers.{l}"
            out.append((p + ".bottleneck_block.norm1", "n1", b, l, ch + l * g))
            out.append((p + ".output_block.norm2", "n2", b, l, mid))
        ch += layers * g
        if b != nb - 1:
            out.append((f"features.transition{b + 1}.norm", "tn", b, -1, ch))
            ch //= 2
    out.append(("features.final_norm", "nf", nb - 1, -1, ch))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# reference and gates
# ---------------------------------------------------------------------------------------------------------------------
def _bn_reference(x64, gamma, beta, old_rm, old_rv):
    """nn.BatchNorm{1,2}d in train mode over x64 [positions, C] (float64): what the oracle and the goldens pin."""
    n = x64.shape[0]
    mean = x64.mean(0)
    var_b = ((x64 - mean) ** 2).mean(0)
    sc = gamma / torch.sqrt(var_b + EPS)
    sh = beta - mean * sc
    rm = 0.9 * old_rm + 0.1 * mean
    rv = 0.9 * old_rv + 0.1 * var_b * n / max(n - 1, 1)          # (one row: var_b = 0, as the oracle's max(n - 1, 1))
    return dict(mean=mean, var_b=var_b, sc=sc, sh=sh, rm=rm, rv=rv)


def _rstd(v):
    return 1.0 / torch.sqrt(v.clamp_min(0.0) + EPS)


def _gates(x64, ref, L, gamma, beta, old_rm, old_rv):
    """Allowed |error| of every published quantity of one BatchNorm; L [C]: longest fp32 summation chain of the channel's producer."""
    n = x64.shape[0]
    e2 = (x64 * x64).mean(0)
    s, am = e2.sqrt(), x64.abs().mean(0)
    chain = L > 1
    # fixed-point resolution of W adds + the producers' fp32 lane sums (module docstring): the issue's bound left the second term out
    d_mean = 1e-9 * s + W_ADD * 2.0 ** -25 / n + (L - 1).clamp_min(0) * U * am
    d_e2 = 1e-9 * e2 + W_ADD * 2.0 ** -17 / n + torch.where(chain, L * U * e2, torch.zeros_like(e2))
    mean, var = ref["mean"], ref["var_b"]
    d_var = d_e2 + 2 * mean.abs() * d_mean + d_mean * d_mean                       # var = E2 - mean^2
    r = _rstd(var)
    d_r = torch.maximum(_rstd(var - d_var) - r, r - _rstd(var + d_var))             # 1 / sqrt(var + eps) over var +- d_var
    d_sc = gamma.abs() * d_r
    unb = n / max(n - 1, 1)
    return dict(mean=d_mean, e2=d_e2, rstd=8 * U * r + d_r,
                sc=8 * U * ref["sc"].abs() + d_sc,
                sh=8 * U * (beta.abs() + (mean * ref["sc"]).abs()) + ref["sc"].abs() * d_mean + mean.abs() * d_sc + d_mean * d_sc,
                rm=8 * U * (0.9 * old_rm.abs() + 0.1 * mean.abs()) + 0.1 * d_mean,
                rv=8 * U * (0.9 * old_rv.abs() + 0.1 * var * unb) + 0.1 * unb * d_var), e2


def _raises(eng, name):
    try:
        eng.tap(name)
    except RuntimeError:
        return True
    return False


def _paths(eng, cfg, mode):
    """Per dense layer: did the fused 1x1 kernel run (no activated copy xa exists), did the 3x3 pair kernel with the activation in LDS run
    (no activated copy ya exists; conv3x3_act_fusable implies the pair kernel)?  fp32: neither kernel exists."""
    fused, pair = [], []
    for b, layers in enumerate(cfg.densenet_structure):
        fused.append([mode == BF16 and _raises(eng, f"xa{b + 1}.{l}") for l in range(layers)])
        pair.append([mode == BF16 and _raises(eng, f"ya{b + 1}.{l}") for l in range(layers)])
    return fused, pair


def _link_free_norm2(eng, cfg, mode):
    """LayerPath::lf2 of the last forward, per layer: the accumulators of a bottleneck map can be tapped only where norm2 was derived from them."""
    return [[mode == BF16 and not _raises(eng, f"raw:isumy{b + 1}.{l}") for l in range(layers)] for b, layers in enumerate(cfg.densenet_structure)]


def _chains(cfg, mode, fused, pair, n_img, hw0, n_blk):
    """Longest fp32 summation chain of every channel's producer (module docstring) -> L of norm0's input, per block the concat buffer's
    channels, per layer the bottleneck map's; with it a mask of the channels whose producer is one of the link-free pair (fused 1x1 / 3x3
    pair kernel), k_pool0 or k_rows_bn_fwd -- the figures are reported for those and for the other producers separately.  Last: the
    largest tiles-per-workgroup figure any chain above was built from (the grid caps are re-stated here: the test asserts it is 1, so a
    changed cap that made these chains longer or shorter than the kernels' shows as a failure, not as a wrong gate)."""
    g, init = cfg.densenet_growth_rate, cfg.initial_pixel_dim
    tpw = [1]
    def _tiles_per_wg(tiles, cap):
        tpw.append(-(-tiles // min(tiles, cap)))
        return tpw[-1]
    up32 = lambda c: -(-c // 32) * 32
    def gemm_nt(n, N, K):                                    # k_gemm_nt_bf16<EPI_FWD>; grid cap: gemm_nt_nblk (gemm_nt.hip:297-305)
        return 4 * _tiles_per_wg(-(-n // 64), max(64, 512 // -(-N // 128))) if up32(K) <= 256 else 8
    stem2 = mode == BF16 and init == 64 and cfg.pixel_dim == 3                    # stem_fwd_ok; grid cap 512 (stem_fwd_nblk, stem.hip:679-682)
    L0 = _tiles_per_wg(n_img * -(-hw0[0] // 8) * -(-hw0[1] // 16), 512) if stem2 else 1
    Lblock, Lmid, ch = [], [], init
    for b, layers in enumerate(cfg.densenet_structure):
        n = n_blk[b]
        L = torch.ones(ch + layers * g, dtype=torch.float64)                      # block 1: k_pool0
        own = torch.ones(ch + layers * g, dtype=torch.bool)
        if b > 0:                                                                  # the transition's output channels
            L[:ch] = gemm_nt(n, ch, 2 * ch) if mode == BF16 else 16
            own[:ch] = False
        mids = []
        for l in range(layers):
            new = slice(ch + l * g, ch + (l + 1) * g)
            if mode == BF16:
                assert pair[b][l], (b, l)                                          # the ring / strip 3x3 kernels' chains are not derived here
                L[new] = 16
                cin = ch + l * g                                                   # fused 1x1: the smaller of its two grid caps (fwd1x1_fused.hip:439)
                mids.append((4 * _tiles_per_wg(-(-n // 64), 512), True) if fused[b][l] else (gemm_nt(n, 128, cin), False))
            else:
                own[new] = False                                                   # k_conv3x3_fwd_f32 / generic: double
                mids.append((16, False))
        Lblock.append((L, own))
        Lmid.append(mids)
        ch = (ch + layers * g) // 2
    return L0, Lblock, Lmid, max(tpw)


def _check_step(eng, cfg, data, mode, coords, n_img, chain, step):
    """All BatchNorms after one train-mode forward.  `chain`: name -> (rm_ref, rv_ref, rm_gate, rv_gate) before the step (float64 reference
    chained from the first step's old values).  -> figures [(step, bn, quantity, worst |error| / gate)], the chain after the step."""
    g, mid, init = cfg.densenet_growth_rate, cfg.densenet_batch_norm_size * cfg.densenet_growth_rate, cfg.initial_pixel_dim
    cpu64 = lambda t: t.detach().double().cpu()
    tabs = cpu64(eng.tap("raw:tabs")).flatten()
    fused, pair = _paths(eng, cfg, mode)
    # the stored maps
    c0 = eng.tap("conv0").cpu()                                                   # [n, Hc, Wc, init]
    act = _conv0_activity(coords, n_img, c0.shape[1], c0.shape[2])
    bias_row = data["features.conv0.bias"].detach().cpu().to(c0.dtype)            # a row no hit reaches is the stored-precision bias row,
    c0 = torch.where(act[..., None], c0, bias_row.expand_as(c0))                  # whether or not the stem wrote it
    dense = []
    for b in range(len(cfg.densenet_structure)):
        d = eng.tap(f"dense{b + 1}")
        dense.append(cpu64(d).reshape(d.shape[0] * d.shape[1] * d.shape[2], -1))
    L0, Lblock, Lmid, tpw = _chains(cfg, mode, fused, pair, n_img, c0.shape[1:3], [d.shape[0] for d in dense])
    figures, new_chain, off = [], {}, 0
    bns = _bn_list(cfg) + [("output_block.norm", "head", -1, -1, O.embed_dims(cfg)[0])]
    for name, kind, b, l, C in bns:
        if kind == "n0":
            x = cpu64(c0).reshape(-1, C)
            L, own = torch.full((C,), float(L0), dtype=torch.float64), torch.zeros(C, dtype=torch.bool)
            rows = cpu64(eng.tap("raw:bstat0")).flatten()[:2 * C].view(C, 2)
        elif kind == "n2":
            y = eng.tap(f"bottleneck{b + 1}.{l}")
            x = cpu64(y).reshape(-1, C)
            L, own = torch.full((C,), float(Lmid[b][l][0]), dtype=torch.float64), torch.full((C,), Lmid[b][l][1])
            rows = cpu64(eng.tap(f"raw:ystat{b + 1}.{l}")).flatten()[:2 * C].view(C, 2)
        elif kind == "head":
            x = cpu64(eng.tap("output_linear")).reshape(n_img, C)
            L, own = torch.ones(C, dtype=torch.float64), torch.ones(C, dtype=torch.bool)      # k_rows_bn_fwd adds in double
            rows = None
        else:                                                                     # norm1 / transition norm / final_norm: a channel prefix of the concat buffer
            x = dense[b][:, :C]
            L, own = Lblock[b][0][:C], Lblock[b][1][:C]
            rows = cpu64(eng.tap(f"raw:bstat{b + 1}")).flatten()[:2 * C].view(C, 2)
        gamma, beta = cpu64(data[name + ".weight"]), cpu64(data[name + ".bias"])
        rm0, rv0, g_rm0, g_rv0 = chain[name]
        ref = _bn_reference(x, gamma, beta, rm0, rv0)
        gate, e2 = _gates(x, ref, L, gamma, beta, rm0, rv0)
        worst = lambda err, gt: err / gt
        fig = {}
        if kind == "head":       # the (mean, 1 / sqrt(var + eps)) rows backward reads are fp32 here: one more rounding each
            hs = cpu64(eng.tap("raw:head_stat")).flatten()
            fig["mean"] = worst((hs[:C] - ref["mean"]).abs(), gate["mean"] + U * ref["mean"].abs())
            fig["rstd"] = worst((hs[C:2 * C] - _rstd(ref["var_b"])).abs(), gate["rstd"])
        else:
            C8 = -(-C // 8) * 8
            fig["sc"] = worst((tabs[off: off + C] - ref["sc"]).abs(), gate["sc"])
            fig["sh"] = worst((tabs[off + C8: off + C8 + C] - ref["sh"]).abs(), gate["sh"])
            off += 2 * C8
            fig["mean"] = worst((rows[:, 0] - ref["mean"]).abs(), gate["mean"])
            fig["e2"] = worst((rows[:, 1] + rows[:, 0] ** 2 - e2).abs(), gate["e2"])      # never the variance alone: cancellation
        g_rm, g_rv = 0.9 * g_rm0 + gate["rm"], 0.9 * g_rv0 + gate["rv"]
        fig["running_mean"] = worst((cpu64(data[name + ".running_mean"]) - ref["rm"]).abs(), g_rm)
        fig["running_var"] = worst((cpu64(data[name + ".running_var"]) - ref["rv"]).abs(), g_rv)
        new_chain[name] = (ref["rm"], ref["rv"], g_rm, g_rv)
        for q, v in fig.items():                                 # worst channel of each producer group: (.., True) = fused 1x1 / pair / pool0 / rows kernel
            figures += [(step, name, q, float(v[m].max()), grp) for grp, m in ((True, own), (False, ~own)) if m.any()]
    assert off == tabs.numel(), (off, tabs.numel())                               # the Python offsets tile raw:tabs exactly
    return figures, new_chain, _link_free_norm2(eng, cfg, mode), tpw


@functools.lru_cache(maxsize=None)
def _run_case(case, mode):
    """The case's train-mode forwards on a fresh engine -> (report, state).  The report is plain data (it also travels from the child)."""
    cfg, steps = _case(case)
    sd = O.fill_state(cfg, 19)
    eng, data, _ = _engine(cfg, sd, mode=mode)
    names = [q[0] for q in _bn_list(cfg)] + ["output_block.norm"]
    zero = lambda t: torch.zeros_like(t, dtype=torch.float64)
    chain, trivial = {}, []
    for nm in names:
        rm, rv = data[nm + ".running_mean"].double().cpu(), data[nm + ".running_var"].double().cpu()
        if not (rm.abs().max() > 1e-2 and (rv - 1).abs().max() > 1e-2):           # else the 0.9 * old term would not be exercised
            trivial.append(nm)
        chain[nm] = (rm, rv, zero(rm), zero(rv))
    figures, lf2, tpw = [], None, 1
    for k, (coords, values, n_img) in enumerate(steps):
        out = torch.empty(n_img, eng.out_dim, device="cuda")
        eng.forward(coords.cuda(), values.cuda(), n_img, out, train=True, seed=1 + k)
        torch.cuda.synchronize()
        fig, chain, p, t = _check_step(eng, cfg, data, mode, coords, n_img, chain, k + 1)
        figures += fig
        tpw = max(tpw, t)
        lf2 = lf2 or p
        if k == 0:
            act = _conv0_activity(coords, n_img, eng.tap("conv0").shape[1], eng.tap("conv0").shape[2])
    report = dict(figures=figures, trivial=trivial, n_bn=len(names), conv0_active=float(act.float().mean()), lf2=lf2, tiles_per_wg=tpw)
    return report, (eng, data, cfg, sd, steps)


@functools.lru_cache(maxsize=None)
def _link_kernel_reports():
    """Cases A and B on the validation build with TCVN_NO_LF=1 (the link kernels of rounds 1-4) in ONE child process."""
    from variant_utils import run_on_debug_build
    return run_on_debug_build("import test_batchnorm_stats_gpu as S\nresult = dict((c, S._run_case(c, S.BF16)[0]) for c in 'AB')\n",
                              dict(TCVN_NO_LF="1"))


def _report(case, build):
    if build == "bf16-link-kernels":
        return _link_kernel_reports()[case]
    return _run_case(case, BF16 if build == "bf16" else F32)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2: every BatchNorm after one and after two train-mode forwards
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,build", [(c, b) for c in "AB" for b in ("bf16", "bf16-link-kernels", "fp32")] + [("C", "bf16")])
def test_every_batchnorm_matches_the_float64_statistics_of_its_stored_input(case, build):
    rep = _report(case, build)
    worst = {}
    for step, name, q, v, grp in rep["figures"]:
        if not v <= worst.get((grp, q), (-1.0, ""))[0]:
            worst[(grp, q)] = (v, name)
    for grp, label in ((True, "fused 1x1 / 3x3 pair / pool0 / rows kernel"), (False, "other producers")):
        print(case, build, "worst |error| / gate,", label + ":", {q: (round(v, 4), nm) for (g_, q), (v, nm) in sorted(worst.items()) if g_ == grp})
    assert rep["tiles_per_wg"] == 1, rep["tiles_per_wg"]            # _chains: one tile per workgroup under every grid cap it re-states
    assert not rep["trivial"], rep["trivial"]                       # fill_state's running statistics are non-trivial everywhere
    assert len(set(f[:3] for f in rep["figures"])) == len(_case(case)[1]) * (6 * (rep["n_bn"] - 1) + 4)
    bad = [f for f in rep["figures"] if not f[3] <= 1.0]             # (a NaN is bad)
    assert not bad, bad[:12]
    if case == "B" and build == "bf16":
        # both mechanisms inside one block: norm2 of layers 0-8 is derived in the 3x3 pair kernel's prologue; layer 9 (cin = 538 > 512:
        # fwd1x1_fused_ok rejects it) runs the GEMM, its norm2 and -- reading the pair kernel's accumulators -- its norm1 and final_norm
        # go through the link kernel
        assert rep["lf2"] == [[True] * 9 + [False]], rep["lf2"]
    if case == "A" and build == "bf16":
        assert all(all(b) for b in rep["lf2"]), rep["lf2"]
    if build != "bf16":
        assert not any(any(b) for b in rep["lf2"]), rep["lf2"]      # link kernels everywhere
    if case == "C":
        assert rep["conv0_active"] < 0.5, rep["conv0_active"]       # norm0's statistics must count the rows no hit reaches
        print("conv0 rows some hit reaches:", rep["conv0_active"])


def test_module_counts_one_batch_per_train_forward():
    """num_batches_tracked lives with the module (the plan's counter slots are host-side): one train-mode forward moves every BatchNorm's
    counter by exactly 1 and its running statistics with it; an eval forward moves neither."""
    from transformercvn.network.layers.dense_net import DenseNet
    from transformercvn.hip.pixels import SparsePixels
    cfg, steps = _case("A")
    sd = O.fill_state(cfg, 19)
    net = DenseNet(cfg.pixel_dim, O.embed_dims(cfg)[0], cfg.initial_pixel_dim, cfg.densenet_growth_rate, cfg.densenet_batch_norm_size,
                   list(cfg.densenet_structure), cfg.dropout)
    net.load_state_dict({k[len(PFX) + 1:]: v for k, v in sd.items() if k.startswith(PFX + ".")}, strict=True)
    net = net.cuda()
    net.hip_mode = BF16
    coords, values, n_img = steps[0]
    px = lambda: SparsePixels(coords.cuda(), values.cuda(), tuple(cfg.pixel_shape), count=n_img)
    bns = net.batch_norms()
    assert len(bns) == len(_bn_list(cfg)) + 1
    before = [(int(m.num_batches_tracked), m.running_mean.clone(), m.running_var.clone()) for m in bns]
    net.train()
    net(px())
    torch.cuda.synchronize()
    for m, (nbt, rm, rv) in zip(bns, before):
        assert int(m.num_batches_tracked) == nbt + 1
        assert not torch.equal(m.running_mean, rm) and not torch.equal(m.running_var, rv)
    after = [(int(m.num_batches_tracked), m.running_mean.clone(), m.running_var.clone()) for m in bns]
    net.eval()
    net(px())
    torch.cuda.synchronize()
    for m, (nbt, rm, rv) in zip(bns, after):
        assert int(m.num_batches_tracked) == nbt and torch.equal(m.running_mean, rm) and torch.equal(m.running_var, rv)


# ---------------------------------------------------------------------------------------------------------------------
# 3: train, then eval
# ---------------------------------------------------------------------------------------------------------------------
def _oracle(cfg, sd, coords, values, training, dtype):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        px = O.preprocess_pixels(cfg, coords, values.to(dtype), False)
        return O.densenet_forward(sd, PFX, cfg, px, O._Ctx(training, 0.0))


def test_eval_forward_uses_the_running_statistics_the_train_steps_wrote():
    """After the two train steps of case A (bf16): the engine's eval forward against the oracle's eval forward fed the engine's own updated
    tensors, in the bf16 band of test_densenet_bf16_close_to_fp32_oracle.  A running statistic written to the wrong parameter (or not at
    all) moves the embedding far outside it."""
    _, (eng, data, cfg, sd, steps) = _run_case("A", BF16)
    coords, values, n_img = steps[-1]
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=False)
    torch.cuda.synchronize()
    sd2 = dict(sd)
    moved = 0
    for k, v in data.items():
        moved += int("running_" in k and not torch.equal(v.cpu(), sd[PFX + "." + k]))
        sd2[PFX + "." + k] = v.detach().cpu()
    assert moved == 2 * (len(_bn_list(cfg)) + 1)
    ref = _oracle(cfg, sd2, coords, values, False, torch.float32)
    e_out = ((out.cpu() - ref).norm() / ref.norm()).item()
    print("eval after two train steps: bf16 rel L2 err of the embedding", e_out)
    assert e_out < 5e-2


# ---------------------------------------------------------------------------------------------------------------------
# 4: out-of-range and non-finite statistics
# ---------------------------------------------------------------------------------------------------------------------
def _range_case():
    """Case A's geometry and first batch without dropout (the oracle draws no masks): only values and weights change below."""
    cfg, steps = _case("A", dropout=0.0)
    return cfg, O.fill_state(cfg, 19), steps[0]


def _hip_train_forward(cfg, sd, coords, values, n_img):
    """-> embedding on the CPU, the engine, its tensors.  (The library has no path that refuses a step: an error here is a failure.)"""
    eng, data, _ = _engine(cfg, sd, mode=BF16)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=True, seed=1)
    torch.cuda.synchronize()
    return out.cpu(), eng, data


def test_non_finite_input_gives_a_non_finite_embedding():
    """One hit of one prong map is inf: the batch statistics are shared, so the float64 oracle's embedding is non-finite for EVERY image,
    and the link-free path (bn_lf.h: a NaN / Inf partial flags its channel, lf_table turns the flag into NaN) must not look finite.
    (norm0 is built by the link kernel from fp64 partial rows, so here the NaN also reaches every later map through the stored values
    themselves: the embedding was non-finite before the accumulators had a guard, too.  The test pins the outcome.)"""
    cfg, sd, (coords, values, n_img) = _range_case()
    values = values.clone()
    values[int((coords[:, 0] == 1).nonzero()[3]), 1] = float("inf")                # image 1 = the first prong map
    ref = _oracle(cfg, sd, coords, values, True, torch.float64)
    assert ref.shape[0] == n_img and not any(bool(torch.isfinite(ref[i]).all()) for i in range(n_img))
    out, _, _ = _hip_train_forward(cfg, sd, coords, values, n_img)
    finite_rows = [i for i in range(n_img) if bool(torch.isfinite(out[i]).all())]
    assert not finite_rows, (finite_rows, out[finite_rows[0]][:8])


def test_non_finite_bottleneck_map_gives_non_finite_statistics():
    """dense1.layers.1.conv1.weight x 3e38: the 1x1 convolution's fp32 sums pass the bf16 range at SOME positions, so the stored bottleneck
    map holds inf / NaN next to finite values and the first non-finite partial of the step goes into lf_add (no link kernel sees it
    first).  The float64 statistics of a stored column that holds a non-finite value are non-finite, and so must be what the step
    publishes for that channel: the (mean, variance) row, the (scale, shift) table and the running statistics of norm2 -- a partial
    converted to 0 or to a saturated integer would leave finite numbers there -- and the embedding of every image."""
    cfg, sd, (coords, values, n_img) = _range_case()
    nm = "features.dense1.layers.1.output_block.norm2"
    k = PFX + ".features.dense1.layers.1.bottleneck_block.conv1.weight"
    sd = dict(sd)
    sd[k] = sd[k] * 3e38
    assert torch.isfinite(sd[k]).all() and torch.isfinite(sd[k].to(torch.bfloat16)).all()
    out, eng, data = _hip_train_forward(cfg, sd, coords, values, n_img)
    y = eng.tap("bottleneck1.1").float().cpu().reshape(-1, 128)
    poisoned = ~torch.isfinite(y).all(0)                                          # channels whose stored column holds inf / NaN
    print("bottleneck1.1: non-finite entries", int((~torch.isfinite(y)).sum()), "of", y.numel(), "in", int(poisoned.sum()), "channels")
    assert poisoned.any() and torch.isfinite(y).any()
    rows = eng.tap("raw:ystat1.1").double().cpu().flatten()[:256].view(128, 2)
    tabs = eng.tap("raw:tabs").float().cpu().flatten()
    off = 0
    for name, _, _, _, C in _bn_list(cfg):
        if name == nm:
            break
        off += 2 * (-(-C // 8) * 8)
    published = dict(mean=rows[:, 0], var=rows[:, 1], sc=tabs[off: off + 128], sh=tabs[off + 128: off + 256],
                     running_mean=data[nm + ".running_mean"].cpu(), running_var=data[nm + ".running_var"].cpu())
    finite = {q: int(torch.isfinite(v[poisoned]).sum()) for q, v in published.items()}
    assert not any(finite.values()), finite
    finite_rows = [i for i in range(n_img) if bool(torch.isfinite(out[i]).all())]
    assert not finite_rows, finite_rows


def test_out_of_range_statistics_do_not_give_a_finite_wrong_embedding():
    """dense1.layers.1.conv1.weight x 1e6: the bottleneck map's sum of squares over the 1404 positions (~1e15) passes what the fixed-point
    accumulators hold (bn_lf.h).  The oracle normalises the scale away and stays finite.  The HIP step must either say so (a non-finite
    embedding for every image) or be right (the bf16 band of test_densenet_bf16_close_to_fp32_oracle)."""
    cfg, sd, (coords, values, n_img) = _range_case()
    k = PFX + ".features.dense1.layers.1.bottleneck_block.conv1.weight"
    sd = dict(sd)
    sd[k] = sd[k] * 1e6
    ref = _oracle(cfg, sd, coords, values, True, torch.float64)
    assert torch.isfinite(ref).all()
    out, _, _ = _hip_train_forward(cfg, sd, coords, values, n_img)
    finite_rows = [i for i in range(n_img) if bool(torch.isfinite(out[i]).all())]
    if not finite_rows:
        print("out of range: the embedding is non-finite for every image")
        return
    assert len(finite_rows) == n_img, finite_rows                    # shared statistics: no half-poisoned batch
    e_out = ((out.double() - ref).norm() / ref.norm()).item()
    print("out of range: finite embedding, bf16 rel L2 err", e_out)
    assert e_out < 5e-2
