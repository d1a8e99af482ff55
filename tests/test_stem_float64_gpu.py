"""The stem of the HIP DenseNet -- hit list -> map, conv0, BatchNorm0 / PReLU0 / AvgPool, and their backward, dense and sparse -- against a
float64 recomputation from each kernel's OWN stored inputs, element by element (stem_reference.py; test_stem_reference_cpu.py shows that
the listed defects leave these gates).  Needs an MI355X.

The other stem tests compare whole networks with the oracle (5e-2 on the embedding), the sparse stem with the dense one (4e-3 relative L2)
and two variants of one kernel bit for bit: none of them fails for one wrong tap out of 147, a wrong pooled window on the last row, a
gradient row written where no window reaches, or a band that mis-handles its records.

Cases (stem_reference.case_hits; structure [1], one encoder layer, no dropout), the smallest that reach each edge:
  partial     104 x 72, 3 maps: conv0 52 x 36 -- partial 8 x 16 forward and 8 x 32 backward tiles, an even extent whose last row and column lie
              in no pooling window (dz exactly 0 there) -- corners, borders, an empty map, entries outside the maps, 40 pixels listed twice
  odd         45 x 37: stem_fwd_ok needs Hin == 2 H, so the product bf16 build takes the generic conv0; 23 x 19: every row is pooled
  dense-band  40 x 280 with a fully set 24 x 120 block: sparse bands of more than SS_HCAP = 2048 records read them from the index
              (load_band's !in_lds path, stem_sparse.hip:216); the record counts per band are computed from the list and asserted
  many        150 maps: 2100 backward tiles (grid cap 2048 in pool0_bwd_vec_grid), 3150 forward tiles (512 in stem_fwd_nblk)
  many-tiny   12 x 16, 1030 maps: more sparse work units than the cap of 1024 in stem_sparse_plan
  wide-limit  24 x 384: the sparse stem's largest W (eval only)
Builds: product bf16 train, fp32, and the validation build with TCVN_DISABLE_TILE check img, conv0 (a position no hit reaches must be the
stored-precision bias exactly), pool0 and the backward (raw:du0, raw:pq0, dgamma0, dbeta0, dslope0, dW0, dbias0); TCVN_NO_STEM_SKIP and
TCVN_POOL0_BWD_FLAT the backward again; the product bf16 eval pass the sparse pooled map (img and conv0 must be absent);
TCVN_SPARSE_STEM_TRAIN raw:bstat0, the pooled map and, after backward, raw:pq0, the norm0 / relu0 gradients and dW0.  One child process per
validation-build variant runs all cases.  Every run asserts from the launch labels and the taps that it went through the kernel it is
meant to cover; nothing is skipped when a path is not taken.

Channel counts: every case above has the tutorial's three value channels per hit.  `partial` and `odd` run again with Cpix = 1, 2 and 4
(EXPECTED_PATH: which kernels each build takes there): the sparse stem keeps a three-channel weight table in LDS and must fill it from
the packed rows' k = tap * Cpix + c; four channels are past the hit-list weight gradient and the sparse stem, and take the generic kernels.

raw:du0 starts as NaN: with the activity bitmap on, rows no hit reaches are never stored and must still be NaN afterwards (they are
compared nowhere: nothing reads them); without it every row must have been written."""
import functools

import pytest
import torch

import densenet_layer_reference as L
import stem_reference as S
from oracle import tcvn_oracle as O
from test_densenet_gpu import _conv0_activity, _engine
from test_densenet_layers_float64_gpu import _count, _exists, _tap

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
SEED = 11
WEIGHT_SEED = 19
N0 = "features.norm0"
TRAIN_CASES = ["partial", "odd", "dense-band", "many", "many-tiny"]
ALL_CASES = TRAIN_CASES + ["wide-limit"]
SS_CROWS, SS_PROWS, SS_HCAP = 8, 4, 2048            # stem_sparse.hip: conv0 rows per band, pooled rows per band, records of a band kept in LDS


def _cfg(case, cpix=3):
    return O.tutorial_config(pixel_dim=cpix, pixel_shape=S.CASE_SHAPES[case][0], densenet_structure=[1], num_encoder_layers=1, dropout=0.0, pixel_noise_std=0.0)


def _kink_free(sc, sh, b0):
    """Is u_e = sc b0 + sh, the BatchNorm0 output of every position no hit reaches, outside the PReLU kink band for every channel?
    Otherwise all hit-free positions of a channel would sit on a kink."""
    return bool(((sc * b0 + sh).abs() > L.R(2) * ((sc * b0).abs() + sh.abs())).all())


def _band_records(coords, n, H, W, Hc, Ho):
    """Records (entries inside the maps, duplicates included: stem_sparse.hip:113-124) per band of every sparse pass -> the largest count of
    the conv0-row bands (statistics, backward: 21 input rows) and of the pooled-row bands (23 input rows)."""
    c = coords.long()
    ok = (c[:, 0] >= 0) & (c[:, 0] < n) & (c[:, 1] >= 0) & (c[:, 1] < H) & (c[:, 2] >= 0) & (c[:, 2] < W)
    rows = torch.zeros(n, H, dtype=torch.int64)
    rows.index_put_((c[ok, 0], c[ok, 1]), torch.ones(int(ok.sum()), dtype=torch.int64), accumulate=True)
    best = []
    for per, extent, lo, hi in ((SS_CROWS, Hc, lambda h0: 2 * h0 - 3, lambda h1: 2 * h1 + 3), (SS_PROWS, Ho, lambda q0: 4 * q0 - 3, lambda q1: 4 * q1 + 7)):
        m = 0
        for r0 in range(0, extent, per):
            r1 = min(r0 + per, extent) - 1
            m = max(m, int(rows[:, max(0, lo(r0)): min(H - 1, hi(r1)) + 1].sum(1).max()))
        best.append(m)
    return best


def _figure(figures, name, kernel, ref, delta, got, rnd_store, kink=None, mask=None):
    if mask is not None:
        ref, delta, got = ref[mask], delta[mask], got[mask]
        kink = kink[mask] if kink is not None else None
    c = L.Check(name, kernel, ref, delta, rnd_store, kink)
    worst, bad, where = c.ratio(got.reshape(ref.shape))
    figures.append((name, kernel, worst, bad, ref.numel(), where, 0 if kink is None else int(kink.sum()), float(ref.abs().max()) if ref.numel() else 0.0))


def _run(case, mode, train, value_mode=0, backward=True, cpix=3):
    """One forward (and, in train mode, one backward) of the case on a fresh engine; the float64 recomputation of every stem operation
    from its own stored inputs -> report (plain data: it also travels from a child process)."""
    from transformercvn.hip import _lib
    cfg = _cfg(case, cpix)
    coords, values, n, (H, W) = S.case_hits(case, cpix=cpix)
    sd = O.fill_state(cfg, WEIGHT_SEED)
    eng, data, grads = _engine(cfg, sd, mode=mode, with_grad=train)
    P = {k: v.detach().double().cpu() for k, v in data.items()}
    w0, b0, sl0, gamma0 = P["features.conv0.weight"], P["features.conv0.bias"], P["features.relu0.weight"], P[N0 + ".weight"]
    # ---- before any GPU work, from the parameters alone: with the running statistics (eval) no channel's hit-free positions sit on a kink
    sc_run = gamma0 / torch.sqrt(P[N0 + ".running_var"] + L.EPS)
    assert _kink_free(sc_run, P[N0 + ".bias"] - P[N0 + ".running_mean"] * sc_run, b0), "choose another weight seed"
    rnd = mode == BF16
    C0 = cfg.initial_pixel_dim
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Ho, Wo = (Hc - 3) // 2 + 1, (Wc - 3) // 2 + 1
    out = torch.empty(n, eng.out_dim, device="cuda")
    dev_c, dev_v = coords.cuda(), values.cuda()
    _lib.lib.tcvn_profile_filter(None); _lib.lib.tcvn_profile_reset(); _lib.lib.tcvn_profile_enable(1)
    eng.forward(dev_c, dev_v, n, out, train=train, seed=SEED, log_pixels=value_mode)
    torch.cuda.synchronize()
    fwd_labels = [r[0] for r in _lib.profile_records()]
    _lib.lib.tcvn_profile_reset()
    figures = []
    img, c0 = _tap(eng, "img"), _tap(eng, "conv0")
    sparse = c0 is None
    assert (img is None) == sparse
    dense1 = _tap(eng, "dense1")
    assert tuple(dense1.shape[:3]) == (n, Ho, Wo)
    tab = L.tables_from_tabs(cfg, _tap(eng, "raw:tabs").flatten())[N0]
    assert _kink_free(tab[0], tab[1], b0), "a channel's hit-free positions sit on a PReLU kink: choose another weight seed"
    act = _conv0_activity(coords[(coords[:, 0] >= 0) & (coords[:, 0] < n) & (coords[:, 1] >= 0) & (coords[:, 1] < H) & (coords[:, 2] >= 0) & (coords[:, 2] < W)],
                          n, Hc, Wc)
    bstat0 = _tap(eng, "raw:bstat0").flatten().view(C0, 2) if train else None
    info = dict(sparse=sparse, bias_rows_wrong=0, img_wrong=0, hit_free=int((~act).sum()), bands=_band_records(coords, n, H, W, Hc, Ho))
    if not sparse:
        assert tuple(img.shape) == (n, H, W, cpix) and tuple(c0.shape) == (n, Hc, Wc, C0)
        ref, d = S.image(coords, values, n, H, W, value_mode, rnd)
        if rnd:                               # bit for bit: the stored value is bf16(exact) (stem_reference.pixel_values)
            info["img_wrong"] = int((img != ref).sum())
            figures.append(("img", "scatter", float("inf") if info["img_wrong"] else 0.0, info["img_wrong"], ref.numel(), [], 0, float(ref.abs().max())))
        else:                                 # gate R(1) |ref|, no store rule on top: the division is the one rounding
            err = (img - ref).abs()
            bad = int((~(err <= d)).sum())
            worst = float(torch.where(err > 0, err / d, torch.zeros_like(err)).max())
            figures.append(("img", "scatter", worst, bad, ref.numel(), [], 0, float(ref.abs().max())))
        ref, d = S.conv0(img, w0, b0, rnd)
        _figure(figures, "conv0", "conv0", ref, d, c0, rnd)
        info["bias_rows_wrong"] = S.bias_exact(c0, act, b0, rnd)
        ref, d = L.pool0(c0, tab[0], tab[1], sl0)
        _figure(figures, "pool0", "pool0", ref, d, dense1[..., :C0], rnd)
        c0_used, dc0, img_used = c0, None, img
    else:
        c0_used, dc0 = S.conv0_from_hits(coords, values, n, H, W, value_mode, w0, b0, True)
        img_used, _ = S.image(coords, values, n, H, W, value_mode, True)
        ref, d = S.sparse_pool(c0_used, dc0, tab[0], tab[1], sl0)
        _figure(figures, "pooled", "sparse pool", ref, d, dense1[..., :C0], True)
        if train:
            (mean, gm), (e2, ge) = S.sparse_stats(c0_used, dc0)
            for nm, got, ref, gate in (("bstat0:mean", bstat0[:, 0], mean, gm), ("bstat0:E2", bstat0[:, 1] + bstat0[:, 0] ** 2, e2, ge)):
                err = (got - ref).abs()                                                   # double values: no store rule on top
                figures.append((nm, "sparse stats", float((err / gate).max()), int((~(err <= gate)).sum()), C0, [], 0, float(ref.abs().max())))
    bwd_labels, du0_nan_rows, du0_nan_active = [], 0, 0
    if train and backward:
        d_out = torch.randn(n, eng.out_dim, generator=torch.Generator().manual_seed(5)).cuda()
        eng.tap("raw:du0").fill_(float("nan"))
        _lib.lib.tcvn_profile_enable(1)
        eng.backward(d_out)
        torch.cuda.synchronize()
        bwd_labels = [r[0] for r in _lib.profile_records()]
        _lib.lib.tcvn_profile_reset()
        G, X = _tap(eng, "raw:grad1")[..., :C0], _tap(eng, "dense1")[..., :C0]
        pq1 = _tap(eng, "raw:pq1").flatten()
        ld = pq1.numel() // 2
        pq0 = _tap(eng, "raw:pq0").flatten()
        gr = {k: grads[k].detach().double().cpu() for k in ("features.conv0.weight", "features.conv0.bias", N0 + ".weight", N0 + ".bias", "features.relu0.weight")}
        inside = int(((coords[:, 0] >= 0) & (coords[:, 0] < n) & (coords[:, 1] >= 0) & (coords[:, 1] < H) & (coords[:, 2] >= 0) & (coords[:, 2] < W)).sum())
        hit_list = _count(bwd_labels, "k_stem_wgrad_sparse") > 0
        if not sparse:
            du0 = _tap(eng, "raw:du0")
            nan_row = torch.isnan(du0).all(-1)
            assert bool((torch.isnan(du0).any(-1) == nan_row).all())                       # a row is written whole or not at all
            du0_nan_rows, du0_nan_active = int(nan_row.sum()), int((nan_row & act).sum())
            o = S.stem_backward(G, X, pq1[:C0], pq1[ld: ld + C0], c0, None, tab, sl0, gamma0, (bstat0[:, 0], bstat0[:, 1]), img, du0=du0, pq0=pq0,
                                rnd=rnd, rnd_eff=rnd and not hit_list, terms=inside if hit_list else None)
            ref, d, kink = o["du0"]
            _figure(figures, "raw:du0", "pool0 backward", ref, d, du0, rnd, kink, mask=~nan_row[..., None].expand_as(du0))
            unc = S.uncovered(Hc, Wc)
            if bool(unc.any()):               # positions in no pooling window: the reference is exactly 0 with gate 0
                assert float(ref[:, unc].abs().max()) == 0.0 and float(d[:, unc].abs().max()) == 0.0
            if hit_list:
                _figure(figures, "dbias0", "conv0 wgrad (hit list)", *o["db0_zero"], gr["features.conv0.bias"], False)
            else:
                _figure(figures, "dbias0", "conv0 wgrad (generic)", *o["db0"], gr["features.conv0.bias"], False)
            kind = "conv0 wgrad (hit list)" if hit_list else "conv0 wgrad (generic)"
        else:
            o = S.stem_backward(G, X, pq1[:C0], pq1[ld: ld + C0], c0_used, dc0, tab, sl0, gamma0, (bstat0[:, 0], bstat0[:, 1]), img_used, pq0=pq0,
                                rnd=True, terms=inside, c=1025)
            kind = "sparse wgrad"
        link = "sparse backward sums" if sparse else "pool0 backward link"
        _figure(figures, "raw:pq0:P", link, *o["P0"], pq0[:C0], False)
        _figure(figures, "raw:pq0:Q", link, *o["Q0"], pq0[C0:], False)
        for q, k in (("dgamma", N0 + ".weight"), ("dbeta", N0 + ".bias"), ("dslope", "features.relu0.weight")):
            _figure(figures, q + "0", link, *o[q], gr[k], False)
        _figure(figures, "dW0", kind, *o["dW0"], gr["features.conv0.weight"], False)
    _lib.lib.tcvn_profile_enable(0)
    return dict(figures=figures, fwd_labels=fwd_labels, bwd_labels=bwd_labels, info=info, du0_nan_rows=du0_nan_rows, du0_nan_active=du0_nan_active,
                geometry=(n, H, W, Hc, Wc, Ho, Wo), d_out_rows=n)


BUILDS = {"generic": dict(TCVN_DISABLE_TILE="1"), "sparse-train": dict(TCVN_SPARSE_STEM_TRAIN="1"), "no-skip": dict(TCVN_NO_STEM_SKIP="1"),
          "flat": dict(TCVN_POOL0_BWD_FLAT="1"), "dense-stem": dict(TCVN_DENSE_STEM="1")}
EVAL_BUILDS = ("bf16-eval", "dense-stem")           # one eval forward; every other build runs a train forward and a backward

# ---- the stem at 1, 2 and 4 value channels per hit -------------------------------------------------------------------
CPIX = [1, 2, 4]
CPIX_CASES = ["partial", "odd"]                     # the two smallest cases
CPIX_CHILD_BUILDS = ["generic", "sparse-train", "no-skip", "dense-stem"]
# The kernels each build must be SEEN on, per channel count: (forward, conv0 weight gradient).
#   forward          "sparse"   k_stem_sparse_pool (+ k_stem_sparse_stats in a train pass): stem_sparse_ok, 1 <= Cpix <= 3, eval passes and
#                               the TCVN_SPARSE_STEM_TRAIN child;  "generic" k_conv_fwd<bf16,3,64>;  "generic f32" k_conv_fwd<float,3,64>.
#                               k_stem_fwd2_bf16 takes three channels only (stem_fwd_ok), so it -- and with it the activity bitmap --
#                               appears nowhere in this table.
#   weight gradient  "hit list" k_stem_wgrad_sparse (Cpix <= 3, in fp32 too);  "generic" k_conv_wgrad<bf16,3,64> / "generic f32"
#                               k_conv_wgrad<float,3,64>: Cpix = 4, and TCVN_DISABLE_TILE;  "sparse" k_stem_sparse_bwd<sums>, <wgrad>.
EXPECTED_PATH = {
    # build           Cpix = 1                   Cpix = 2                   Cpix = 4
    "bf16":         {1: ("generic", "hit list"), 2: ("generic", "hit list"), 4: ("generic", "generic")},
    "no-skip":      {1: ("generic", "hit list"), 2: ("generic", "hit list"), 4: ("generic", "generic")},
    "fp32":         {1: ("generic f32", "hit list"), 2: ("generic f32", "hit list"), 4: ("generic f32", "generic f32")},
    "generic":      {1: ("generic", "generic"), 2: ("generic", "generic"), 4: ("generic", "generic")},
    "sparse-train": {1: ("sparse", "sparse"), 2: ("sparse", "sparse"), 4: ("generic", "generic")},
    "bf16-eval":    {1: ("sparse", None), 2: ("sparse", None), 4: ("generic", None)},
    "dense-stem":   {1: ("generic", None), 2: ("generic", None), 4: ("generic", None)},
}


def _child_runs(build):
    """What one validation-build child computes: the three-channel train cases (not for the eval-only knob), then the channel-count cases."""
    train = build not in EVAL_BUILDS
    out = dict((c, _run(c, BF16, True)) for c in TRAIN_CASES) if train else {}
    if build in CPIX_CHILD_BUILDS:
        out.update(((c, cpix), _run(c, BF16, train, cpix=cpix)) for cpix in CPIX for c in CPIX_CASES)
    return out


@functools.lru_cache(maxsize=None)
def _child_reports(build):
    """All cases of one validation-build knob set in ONE child process (knobs are read once per process)."""
    from variant_utils import run_on_debug_build
    return run_on_debug_build(f"import test_stem_float64_gpu as T\nresult = T._child_runs({build!r})\n", BUILDS[build])


@functools.lru_cache(maxsize=None)
def _report(case, build, cpix=3):
    if build in BUILDS:
        return _child_reports(build)[case if cpix == 3 else (case, cpix)]
    return _run(case, F32 if build == "fp32" else BF16, build not in EVAL_BUILDS, cpix=cpix)


def _assert_figures(rep, case, build, kernels):
    figs = [f for f in rep["figures"] if f[1] in kernels]
    assert {f[1] for f in figs} == set(kernels), (sorted({f[1] for f in rep["figures"]}), kernels)
    print(case, build, "worst |error| / gate:", {f[0]: round(f[2], 4) for f in figs}, "elements at a PReLU kink (left out):", sum(f[6] for f in figs),
          "of", sum(f[4] for f in figs))
    bad = [f for f in figs if f[3] or not f[2] <= 1.0]
    assert not bad, [f[:6] for f in bad]


def _assert_case(rep, case):
    """The case is what it is there for (from the hit list and the sizes alone)."""
    n, H, W, Hc, Wc, Ho, Wo = rep["geometry"]
    cdiv = lambda a, b: -(-a // b)
    if case == "partial":
        assert (Hc, Wc) == (52, 36) and Hc % 8 and Wc % 16 and Wc % 32 and Hc == 2 * Ho + 2 and Wc == 2 * Wo + 2
    if case == "odd":
        assert (Hc, Wc) == (23, 19) and Hc == 2 * Ho + 1 and Wc == 2 * Wo + 1 and H != 2 * Hc
    if case == "dense-band":
        assert min(rep["info"]["bands"]) > SS_HCAP, rep["info"]["bands"]
    else:
        assert max(rep["info"]["bands"]) <= SS_HCAP, rep["info"]["bands"]
    if case == "many":
        assert n * cdiv(Hc, 8) * cdiv(Wc, 32) > 2048 and cdiv(n * Hc * Wc, 32) > 2048 and n * cdiv(Hc, 8) * cdiv(Wc, 16) > 512
    if case == "many-tiny":
        assert n > 1024                       # one work unit per map at least (stem_sparse_plan)
    if case == "wide-limit":
        assert W == 384
    assert rep["info"]["hit_free"] > 0 and rep["d_out_rows"] >= 2


@pytest.mark.parametrize("build", ["bf16", "fp32", "generic"])
@pytest.mark.parametrize("case", TRAIN_CASES)
def test_dense_stem_forward_matches_float64(case, build):
    rep = _report(case, build)
    _assert_case(rep, case)
    assert not rep["info"]["sparse"]                                   # img and conv0 exist: the dense stem ran
    _assert_figures(rep, case, build, ["scatter", "conv0", "pool0"])
    assert rep["info"]["img_wrong"] == 0 and rep["info"]["bias_rows_wrong"] == 0, rep["info"]
    labels = rep["fwd_labels"]
    n, H, W, Hc, Wc, Ho, Wo = rep["geometry"]
    if build == "bf16" and H == 2 * Hc:
        assert _count(labels, "k_stem_fwd_bf16") == 1 and not _count(labels, "k_conv_fwd<bf16,3"), labels      # (k_stem_fwd2_bf16 under its launcher's label)
    elif build == "bf16":                                              # the odd shape: stem_fwd_ok is false
        assert _count(labels, "k_conv_fwd<bf16,3") == 1 and not _count(labels, "k_stem_fwd_bf16"), labels
    elif build == "generic":
        assert _count(labels, "k_conv_fwd<bf16,3") == 1 and not _count(labels, "k_stem_fwd_bf16"), labels
    else:
        assert _count(labels, "k_conv_fwd<float,3") == 1 and not _count(labels, "bf16"), labels
    assert not _count(labels, "k_stem_sparse"), labels


@pytest.mark.parametrize("case,build", [(c, "bf16-eval") for c in ALL_CASES] + [(c, "sparse-train") for c in TRAIN_CASES])
def test_sparse_stem_pooled_map_and_statistics_match_float64(case, build):
    rep = _report(case, build)
    _assert_case(rep, case)
    assert rep["info"]["sparse"]                                       # neither img nor conv0 exists
    _assert_figures(rep, case, build, ["sparse pool"] + (["sparse stats"] if build == "sparse-train" else []))
    labels = rep["fwd_labels"]
    assert _count(labels, "k_stem_sparse_pool") == 1 and _count(labels, "k_stem_sparse_stats") == int(build == "sparse-train"), labels
    assert not _count(labels, "k_stem_fwd_bf16") and not _count(labels, "k_conv_fwd<bf16,3"), labels


@pytest.mark.parametrize("build", ["bf16", "no-skip", "flat", "generic", "fp32"])
@pytest.mark.parametrize("case", TRAIN_CASES)
def test_dense_stem_backward_matches_float64(case, build):
    rep = _report(case, build)
    _assert_case(rep, case)
    assert not rep["info"]["sparse"]
    hit_list = build != "generic"
    wg = "conv0 wgrad (hit list)" if hit_list else "conv0 wgrad (generic)"
    _assert_figures(rep, case, build, ["pool0 backward", "pool0 backward link", wg])
    assert len([f for f in rep["figures"] if f[1] == wg]) == 2 and len([f for f in rep["figures"] if f[1] == "pool0 backward link"]) == 5
    labels = rep["bwd_labels"]
    assert _count(labels, "k_stem_wgrad_sparse") == int(hit_list) and _count(labels, "k_conv_wgrad<bf16,3") == int(not hit_list), labels
    assert not _count(labels, "k_stem_sparse_bwd"), labels
    n, H, W, Hc, Wc, Ho, Wo = rep["geometry"]
    # the activity bitmap: on in the product bf16 build where the stem kernel ran -- rows no hit reaches are never stored -- off elsewhere
    skip = build == "bf16" and H == 2 * Hc
    assert rep["du0_nan_active"] == 0 and rep["du0_nan_rows"] == (rep["info"]["hit_free"] if skip else 0), (rep["du0_nan_rows"], rep["info"])


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_sparse_stem_backward_matches_float64(case):
    rep = _report(case, "sparse-train")
    assert rep["info"]["sparse"]
    _assert_figures(rep, case, "sparse-train", ["sparse backward sums", "sparse wgrad"])
    assert len([f for f in rep["figures"] if f[1] == "sparse backward sums"]) == 5
    labels = rep["bwd_labels"]
    assert _count(labels, "k_stem_sparse_bwd<sums>") == 1 and _count(labels, "k_stem_sparse_bwd<wgrad>") == 1 and not _count(labels, "k_stem_wgrad_sparse"), labels


@pytest.mark.parametrize("mode,value_mode", [(BF16, 1), (BF16, 2), (F32, 2)])
def test_value_modes_of_the_scatter_match_float64(mode, value_mode):
    """log(v + 1) and pre-scaled values on the `partial` list (fp32 log mode: nothing bounds logf, stem_reference.pixel_values)."""
    rep = _run("partial", mode, True, value_mode, backward=False)
    assert not rep["info"]["sparse"]
    _assert_figures(rep, "partial", f"mode {mode} values {value_mode}", ["scatter", "conv0", "pool0"])
    assert rep["info"]["img_wrong"] == 0 and rep["info"]["bias_rows_wrong"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2 and 4 value channels per hit
# ---------------------------------------------------------------------------------------------------------------------
def _assert_forward_path(labels, path, train):
    sparse = path == "sparse"
    assert _count(labels, "k_stem_sparse_pool") == int(sparse) and _count(labels, "k_stem_sparse_stats") == int(sparse and train), labels
    assert _count(labels, "k_conv_fwd<bf16,3") == int(path == "generic") and _count(labels, "k_conv_fwd<float,3") == int(path == "generic f32"), labels
    assert not _count(labels, "k_stem_fwd_bf16"), labels                # three channels only (stem_fwd_ok)


@pytest.mark.parametrize("build", ["bf16", "fp32", "bf16-eval", "generic", "dense-stem", "no-skip", "sparse-train"])
@pytest.mark.parametrize("case", CPIX_CASES)
@pytest.mark.parametrize("cpix", CPIX)
def test_stem_forward_matches_float64_at_other_channel_counts(cpix, case, build):
    rep = _report(case, build, cpix)
    _assert_case(rep, case)
    path = EXPECTED_PATH[build][cpix][0]
    train = build not in EVAL_BUILDS
    assert rep["info"]["sparse"] == (path == "sparse"), (path, rep["fwd_labels"])      # sparse: neither img nor conv0 exists
    _assert_forward_path(rep["fwd_labels"], path, train)
    if path == "sparse":
        _assert_figures(rep, case, f"{build} Cpix {cpix}", ["sparse pool"] + (["sparse stats"] if train else []))
    else:
        _assert_figures(rep, case, f"{build} Cpix {cpix}", ["scatter", "conv0", "pool0"])
        assert rep["info"]["img_wrong"] == 0 and rep["info"]["bias_rows_wrong"] == 0, rep["info"]


@pytest.mark.parametrize("build", ["bf16", "fp32", "generic", "no-skip", "sparse-train"])
@pytest.mark.parametrize("case", CPIX_CASES)
@pytest.mark.parametrize("cpix", CPIX)
def test_stem_backward_matches_float64_at_other_channel_counts(cpix, case, build):
    rep = _report(case, build, cpix)
    fwd, wgrad = EXPECTED_PATH[build][cpix]
    labels = rep["bwd_labels"]
    assert _count(labels, "k_stem_wgrad_sparse") == int(wgrad == "hit list") and _count(labels, "k_conv_wgrad<bf16,3") == int(wgrad == "generic") and \
        _count(labels, "k_conv_wgrad<float,3") == int(wgrad == "generic f32"), labels
    assert _count(labels, "k_stem_sparse_bwd<sums>") == int(wgrad == "sparse") and _count(labels, "k_stem_sparse_bwd<wgrad>") == int(wgrad == "sparse"), labels
    assert rep["info"]["sparse"] == (fwd == "sparse")
    if wgrad == "sparse":
        _assert_figures(rep, case, f"{build} Cpix {cpix}", ["sparse backward sums", "sparse wgrad"])
        assert len([f for f in rep["figures"] if f[1] == "sparse backward sums"]) == 5
        return
    wg = "conv0 wgrad (hit list)" if wgrad == "hit list" else "conv0 wgrad (generic)"
    _assert_figures(rep, case, f"{build} Cpix {cpix}", ["pool0 backward", "pool0 backward link", wg])
    assert len([f for f in rep["figures"] if f[1] == wg]) == 2 and len([f for f in rep["figures"] if f[1] == "pool0 backward link"]) == 5
    # no activity bitmap without the three-channel stem kernel: every row of raw:du0 has been written
    assert rep["du0_nan_active"] == 0 and rep["du0_nan_rows"] == 0, (rep["du0_nan_rows"], rep["info"])


@pytest.mark.parametrize("value_mode", [1, 2])
@pytest.mark.parametrize("cpix", CPIX)
def test_value_modes_of_the_eval_pass_match_float64_at_other_channel_counts(cpix, value_mode):
    """log(v + 1) and pre-scaled values through the product bf16 eval pass on the `partial` list (v / 255: the bf16-eval build above)."""
    rep = _run("partial", BF16, False, value_mode, cpix=cpix)
    path = EXPECTED_PATH["bf16-eval"][cpix][0]
    assert rep["info"]["sparse"] == (path == "sparse")
    _assert_forward_path(rep["fwd_labels"], path, False)
    if path == "sparse":
        _assert_figures(rep, "partial", f"eval Cpix {cpix} values {value_mode}", ["sparse pool"])
    else:
        _assert_figures(rep, "partial", f"eval Cpix {cpix} values {value_mode}", ["scatter", "conv0", "pool0"])
        assert rep["info"]["img_wrong"] == 0 and rep["info"]["bias_rows_wrong"] == 0
