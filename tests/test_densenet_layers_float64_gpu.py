"""Kernels of the HIP DenseNet, each against a float64 recomputation from its OWN stored inputs, element by element: every forward kernel, the
3x3 data- and weight-gradient kernels and the transition data gradient.  Needs an MI355X.

The whole-network tests (test_densenet_gpu.py) compare with an oracle through all layers, so their bounds must leave room for bf16 drift
(3e-2 on dense1, 5e-2 on the embedding) -- room enough for a kernel that is wrong on a few pixels or channels.  Here each operation is
recomputed in float64 (densenet_layer_reference.py) from the maps the engine stored (tap()), its (scale, shift) tables (raw:tabs) and the
bound fp32 parameters, so no drift accumulates and the gate of every element comes from the arithmetic alone (that module's docstring;
test_densenet_layer_reference_cpu.py shows that the listed defects leave these gates).  No element is excluded.

Operations: pool0 (where the conv0 map exists), every dense layer's 1x1 and 3x3 (with the dropout keep scale of tcvn_dropout_keep kind 1,
stream 64 b + l + 1), the materialised operands xa / ya where a build stores them, every transition, the head pooling, the output Linear.
Builds: the product library in bf16 train mode (fused 1x1 on the raw buffer, activation inside the 3x3 pair kernel), bf16 eval mode
(norm2 + PReLU2 in the 1x1 epilogue, stored ya) and fp32 mode; the validation library without the fusions (act_bf16 + NT GEMM, stored
xa / ya) and with the generic kernels (TCVN_DISABLE_TILE), one child process each for all cases.  Each run asserts from the taps and the
launch labels that it went through the kernels it is meant to cover.

Backward.  The backward pass reuses its scratch buffers layer after layer, so what can be read back without a hook is what stays: G and
(P, Q) of every layer's own slice (final once the layer has run: raw:grad<b>, raw:pq<b>), the eff rows the consecutive-tile kernel stores
per layer (raw:ey<b>.<l>), the parameter gradients, and DU of the layer that ran last (raw:du<b>).  The backward is issued block by block
(backward_part), and compared are:
  * 3x3 data gradient: DU = sc2 dA prelu'(u2) of the FIRST layer of every block, element by element (its slice starts at c_off = the
    block's first width, its keep stream is 64 b + 1), and the stored eff rows of every layer;
  * 3x3 weight and bias gradient of EVERY layer, from the eff rows recomputed from the final (G, P, Q) slices (or the stored rows) and
    the activated bottleneck map (or the stored ya);
  * transition data gradient and head pooling backward, the first writers of a block's accumulator: the last layer's slice of G[b]
    receives nothing but their contribution, so it is compared as the contribution alone -- for a transition exactly zero at the pixels
    of an odd edge that no 2x2 window covers (the head's input is raw:dcondense).
Builds: product (the kernel choice at these sizes), TCVN_DGRAD3_ANY_SIZE (the consecutive-tile data gradient with its eff rows feeding
the weight gradient; the odd-width case, whose slices are not 16-byte aligned, stays on the two-workgroup kernel), TCVN_DISABLE_TILE,
fp32.  With one image the output block's train-mode BatchNorm1d passes no gradient: every reference is exactly zero there, and so must
the kernels' results be.
The layers' transient state -- DU of any layer, (PY, QY), G[:, :cin] and (P, Q) in front of a layer's update -- is read through the snapshot
hook of the validation build (tcvn_debug_layer_snapshot, densenet_bwd.hip), armed in one backward for EVERY layer of
every block and for its transition or the head (test_every_layer_backward_...; test_first_and_last_layer_backward_... keeps its name and
assertions and reads the first and last layers' part of the same run, _first_and_last): eff rows, DU, norm2's link (dgamma2, dbeta2,
dslope2, PY, QY), db1, dW1, the read-add-write of G[:, :cin], norm1's link (dgamma1, dbeta1, dslope1, P / Q[:cin] +=), everything else of
G, P, Q bit-unchanged; for the block's first writer G and (P, Q) over all channels as the contribution alone, the transition's weight and
bias gradient and its norm's parameter gradients.  Builds: validation library without knobs (the product kernel choice; also in fp32
mode), TCVN_DGRAD3_ANY_SIZE, the unfused build (eff_materialize, TN and NT GEMMs on stored operands) and TCVN_DISABLE_TILE.  The hook's
report (which 3x3 data-gradient kernel ran, whether the fused 1x1 backward ran, whether the eff rows were stored) and the launch labels
are asserted per build.
The hook test has two cases of its own (LAYER_CASES; defined in test_densenet_layer_reference_cpu.layer_case, which also shows on the CPU
that the gates bite at these sizes), chosen along the three axes on which k_bwd1x1_fused_bf16 changes its behaviour:
  * column slices (grid.y = cdiv(cin, 128): own table rows, own slab columns): with every layer armed `odd` gives two to five slices at
    cin % 8 == 2, `mod4` and `trips` two to four;
  * cin % 8: `mod4` has cin = 228 .. 388, all % 8 == 4 -- production block 4's widths, where the last 16-byte chunk of a row is half
    foreign and the layer's 3x3 slice is 8-byte aligned only (the two-workgroup 3x3 data gradient, asserted);
  * tiles per workgroup (grid.x = min(tiles, max(64, 512 // slices)) workgroups of 64 pixels; a workgroup that takes a second tile keeps
    its weight-gradient accumulators, bias sums and statistics across tiles): `trips` has M = 11 475 pixels = 179 full tiles + 19 rows, so
    at three slices (cap 170) ten workgroups and at four slices (cap 128) fifty-two take a second tile, the partial tile among them.  The
    grid comes from tcvn_debug_layer_snapshot_grid and is asserted against the re-stated formula for every layer of every case: should
    the cap change, the test fails instead of going back to one tile per workgroup.  Layer 0 of `trips` (two slices, cap 256) stays at one
    tile: a second trip at one or two slices needs M > 16 384 and is left out to keep the float64 recomputation small.
The same cases run the unfused build's k_gemm_tn_bf16<conv1> / k_gemm_nt_bf16<dgrad1x1> (same cap formula), the generic kernels and fp32
mode (k_gemm_tn_f32 split-K, k_conv1x1_dgrad_f32) at these widths and trip counts.

The frozen schedule (hit gradients: forward_frozen + input_gradient, a second schedule threaded through the training one) runs on the
same cases (_run_frozen).  Every frozen run first does one training forward + backward with dropout 0.1 configured on the same engine and
workspace, so that stale (P, Q), (PY, QY), keep words, eff rows and batch-statistic rows are there to be picked up; the hit list carries
one pixel listed twice and one listed three times; the bound gradient tensors are filled with a NaN bit pattern.
  * forward (builds bf16-frozen, fp32-frozen, unfused-frozen, generic-frozen of the forward test): every operation under the gates of
    the train / eval legs; raw:tabs against float64 tables of the BOUND running statistics (8 u of the magnitude of their terms, the
    table gate of test_batchnorm_stats_gpu.py without its row terms: the statistics are exact fp32 inputs here); the conv0 map exists
    (dense stem), every Y is stored and no ya is fused, no element is dropped although the training step before did drop, the running
    statistics keep their bits (the engine binds no num_batches_tracked: those counters belong to the Python runtime).
  * backward without a hook (test_frozen_backward_..., builds bf16, fp32, TCVN_DGRAD3_ANY_SIZE, TCVN_DISABLE_TILE): raw:dcondense
    (k_rows_bn_bwd_frozen + the Linear), every block's first writer on the last layer's slice with an exactly zero odd edge, the FINAL
    G slice of every layer and the block's first channels as the end of the read-add-write chain (frozen_block_slices), DU of block 1's
    first layer (raw:du1), raw:du0 against stem_reference's pooling backward with P0 = Q0 = 0, and d_values against the gather of the
    STORED raw:du0 in value modes 0, 1 and 2 (non-owners exactly 0).  On `narrow` one more pass runs on a workspace filled with 0xFF
    bytes: its d_values must equal the clean run's bit for bit (no atomics anywhere in the frozen schedule).
  * backward through the hook (test_frozen_every_layer_..., input_gradient calls the same tcvn_debug_layer_snapshot): per first writer G
    over all channels; per layer the eff rows where stored, DU, the read-add-write of G[:, :cin] from the stored DU with PY = QY = 0,
    the rest of G bit-unchanged, (P, Q) of the block in front of and behind every launch and (PY, QY) behind it EXACTLY zero, the fused
    grid.  validation (bf16, fp32) and TCVN_DGRAD3_ANY_SIZE on all LAYER_CASES; unfused and TCVN_DISABLE_TILE on wide, narrow-one, odd, mod4.
  * schedule, per build: the bound gradient tensors bit-unchanged, no launch of a weight-gradient kernel or TN GEMM (k_conv3x3_wgrad*,
    k_conv_wgrad*, k_conv1x1_wgrad*, k_gemm_tn_*, k_stem_wgrad*; the link kernels, slab reducers and k_unpack carry no launch label --
    all they could write is those tensors), k_bwd1x1_fused_bf16 == layers in the fused builds, k_gemm_nt_bf16<dgrad1x1> == layers in the
    unfused one, k_hit_gradient == 1.  With running statistics one image passes a gradient too: every reference tensor's max is > 0.
The frozen reports ride in the same one-child-per-knob-set runs (_child_reports)."""
import copy
import ctypes as C
import functools

import pytest
import torch

import densenet_layer_reference as R
from oracle import tcvn_oracle as O
from test_densenet_gpu import _conv0_activity, _engine
from test_densenet_layer_reference_cpu import fused_grid, layer_case

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
SEED = 11


def _all_maps(batch):
    """One COO list over the event map and the prong maps of a synthetic batch with one event: image 0 = the event map."""
    pc = batch[5].clone()
    pc[:, 0] += 1
    return torch.cat([batch[2], pc]).contiguous(), torch.cat([batch[3], batch[6]]).contiguous(), 1 + int(batch[7].sum())


def _case(name):
    """-> cfg, coords, values, n_img"""
    base = dict(pixel_noise_std=0.0, num_encoder_layers=2)
    if name in ("mod4", "trips"):             # cin % 8 == 4 at production block 4's widths; M = 11 475 pixels, past the fused 1x1 backward's grid caps
        return layer_case(name)
    if name in ("wide", "wide-dropout"):      # block 1 as wide as production's: conv0 20 x 140, block 1 9 x 69 (odd in front of the transition), block 2 4 x 34
        cfg = O.tutorial_config(pixel_shape=(40, 280), densenet_structure=[3, 2], dropout=0.1 if name == "wide-dropout" else 0.0, **base)
        b = O.synthetic_batch([3], 47, cfg, prong_hits=(20, 400))
        return cfg, b[5], b[6], 3
    if name == "odd":                         # cin = 250 .. 538: cin % 8 == 2, two to five 128-column slices, cin > 512 at the last layer
        cfg = O.tutorial_config(initial_pixel_dim=250, densenet_structure=[10], pixel_shape=(56, 40), dropout=0.0, **base)
        return (cfg,) + _all_maps(O.synthetic_batch([2], 41, cfg, event_hits=(60, 200), prong_hits=(20, 120)))
    cfg = O.tutorial_config(pixel_shape=(104, 72), densenet_structure=[3, 3, 2], dropout=0.0, **base)      # block 1 26 x 18 ... block 3 6 x 4
    if name == "narrow-one":                  # one image: the last block has fewer padded positions than one 128-position tile
        b = O.synthetic_batch([1], 53, cfg, prong_hits=(60, 200))
        return cfg, b[5], b[6], 1
    assert name == "narrow"
    return (cfg,) + _all_maps(O.synthetic_batch([2], 41, cfg))


CASES = ["wide", "wide-dropout", "narrow", "narrow-one", "odd"]
FWD_CASES = CASES + ["mod4"]                  # the forward test
LAYER_CASES = CASES + ["mod4", "trips"]       # the snapshot-hook test


def _geometry(cfg):
    """Per block (H, W, first cin), from the config alone (the runs assert the tapped maps have these sizes)."""
    H, W = ((s - 1) // 2 + 1 for s in cfg.pixel_shape)
    H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out, ch = [], cfg.initial_pixel_dim
    for layers in cfg.densenet_structure:
        out.append((H, W, ch))
        ch = (ch + layers * cfg.densenet_growth_rate) // 2
        H, W = H // 2, W // 2
    return out


def _keep(p, seed, sid, rows, cols):
    from transformercvn.hip._lib import lib, check
    out = torch.empty(rows, cols, device="cuda")
    check(lib.tcvn_dropout_keep(1, float(p), C.c_uint64(seed), C.c_uint32(sid), rows, cols, C.c_void_p(out.data_ptr()),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dropout_keep")
    return out


def _exists(eng, name):
    """Does the plan have this tap?  Only the plan's own "no such tap" answer (code -1 of tcvn_densenet_tap) means no; any other error
    -- a HIP error among them -- is raised."""
    try:
        eng.tap(name)
    except RuntimeError as err:
        if str(err) != f"libtcvn_hip: tap {name} failed with code -1":
            raise
        return False
    return True


def _tap(eng, name):
    return eng.tap(name).detach().double().cpu() if _exists(eng, name) else None


def _run(case, mode, train):
    """One forward of the case on a fresh engine, the float64 recomputation of every operation, the comparison -> report (plain data: it
    also travels from a child process)."""
    from transformercvn.hip import _lib
    cfg, coords, values, n_img = _case(case)
    sd = O.fill_state(cfg, 19)
    eng, data, _ = _engine(cfg, sd, mode=mode)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    _lib.lib.tcvn_profile_filter(None); _lib.lib.tcvn_profile_reset(); _lib.lib.tcvn_profile_enable(1)
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=train, seed=SEED)
    torch.cuda.synchronize()
    _lib.lib.tcvn_profile_enable(0)
    labels = [r[0] for r in _lib.profile_records()]
    _lib.lib.tcvn_profile_reset()

    geo = _geometry(cfg)
    g = cfg.densenet_growth_rate
    P = {k: v.detach().double().cpu() for k, v in data.items()}
    stored, paths, keeps = {}, [], {}
    for b, layers in enumerate(cfg.densenet_structure):
        stored[f"dense{b + 1}"] = _tap(eng, f"dense{b + 1}")
        assert tuple(stored[f"dense{b + 1}"].shape[1:3]) == geo[b][:2], (stored[f"dense{b + 1}"].shape, geo[b])
        for l in range(layers):
            for nm in (f"bottleneck{b + 1}.{l}", f"xa{b + 1}.{l}", f"ya{b + 1}.{l}"):
                t = _tap(eng, nm)
                if t is not None:
                    stored[nm] = t
            paths.append((b, l, geo[b][2] + l * g, f"xa{b + 1}.{l}" in stored, f"ya{b + 1}.{l}" in stored, f"bottleneck{b + 1}.{l}" in stored,
                          _exists(eng, f"raw:isumy{b + 1}.{l}")))
            if train and cfg.dropout > 0:
                H, W, _ = geo[b]
                keeps[(b, l)] = _keep(cfg.dropout, SEED, 64 * b + l + 1, n_img * H * W, g).double().cpu().reshape(n_img, H, W, g)
    stored["condense"] = _tap(eng, "condense").reshape(n_img, -1)
    stored["output_linear"] = _tap(eng, "output_linear").reshape(n_img, -1)
    c0 = _tap(eng, "conv0")
    if c0 is not None:                        # a row no hit reaches is the stored-precision bias row, whether or not the stem wrote it
        act = _conv0_activity(coords, n_img, c0.shape[1], c0.shape[2])
        bias_row = P["features.conv0.bias"]
        c0 = torch.where(act[..., None], c0, (R.bf16(bias_row) if mode == BF16 else bias_row).expand_as(c0))
    tabs = _tap(eng, "raw:tabs").flatten()
    checks, _ = R.run_forward(cfg, P, mode == BF16, train, c0, keeps or None, stored=stored, tabs=tabs)
    figures = []
    for c in checks:
        worst, bad, where = c.ratio(R.stored_counterpart(c, stored))
        figures.append((c.name, c.kernel, worst, bad, c.ref.numel(), where))
    pp = [n_img * (H + 2) * (W + 2) for H, W, _ in geo]
    return dict(figures=figures, labels=labels, paths=paths, padded=pp, geometry=geo, conv0=c0 is not None,
                dropped=sum(int((k == 0).sum()) for k in keeps.values()))


def _run_backward(case, mode, generic=False):
    """Train-mode forward, then the backward block by block (last block first); after each block the 3x3 data gradient of its first layer
    and the stored eff rows of all its layers against float64 -> report."""
    from transformercvn.hip import _lib
    cfg, coords, values, n_img = _case(case)
    sd = O.fill_state(cfg, 19)
    eng, data, grads = _engine(cfg, sd, mode=mode, with_grad=True)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=True, seed=SEED)
    d_out = torch.randn(n_img, eng.out_dim, generator=torch.Generator().manual_seed(5)).cuda()
    geo, g, rnd = _geometry(cfg), cfg.densenet_growth_rate, mode == BF16
    P = {k: v.detach().double().cpu() for k, v in data.items()}
    tabd = R.tables_from_tabs(cfg, _tap(eng, "raw:tabs").flatten())
    for b, layers in enumerate(cfg.densenet_structure):           # the eff-row buffers start as NaN: a kernel that fills one leaves none
        for l in range(layers):
            if _exists(eng, f"raw:ey{b + 1}.{l}"):
                eng.tap(f"raw:ey{b + 1}.{l}").fill_(float("nan"))
    _lib.lib.tcvn_profile_filter(None); _lib.lib.tcvn_profile_reset(); _lib.lib.tcvn_profile_enable(1)
    figures, ey_filled = [], []
    for b in reversed(range(len(cfg.densenet_structure))):
        eng.backward_part(d_out, b)
        torch.cuda.synchronize()
        H, W, c0 = geo[b]
        G, X, pq = _tap(eng, f"raw:grad{b + 1}"), _tap(eng, f"dense{b + 1}"), _tap(eng, f"raw:pq{b + 1}").flatten()
        Pr, Qr = pq[:pq.numel() // 2], pq[pq.numel() // 2:]
        for l in range(cfg.densenet_structure[b]):
            p = f"features.dense{b + 1}.layers.{l}"
            c_off = c0 + l * g
            keep = _keep(cfg.dropout, SEED, 64 * b + l + 1, n_img * H * W, g).double().cpu().reshape(n_img, H, W, g) if cfg.dropout > 0 else None
            ey = _tap(eng, f"raw:ey{b + 1}.{l}")
            if ey is not None and bool(torch.isnan(ey).all()):
                ey = None                                          # untouched: another kernel ran
            ey_filled.append(ey is not None)
            # ---- 3x3 weight and bias gradient: every layer (the parameter gradients are the layer's own)
            c_sl = slice(c_off, c_off + g)
            fe, taue, e, de = R.eff_rows(G[..., c_sl], X[..., c_sl], Pr[c_sl], Qr[c_sl], keep, rnd)
            if ey is not None:
                e, de = ey, torch.zeros_like(ey)
            sc2, sh2 = tabd[p + ".output_block.norm2"]
            _, _, a2, da2 = R.activation(_tap(eng, f"bottleneck{b + 1}.{l}"), sc2, sh2, P[p + ".output_block.relu2.weight"], rnd)
            ya = _tap(eng, f"ya{b + 1}.{l}")
            if ya is not None:                                      # the materialised operand (checked by the forward test)
                a2, da2 = ya, torch.zeros_like(ya)
            (dW, dWd), (db, dbd) = R.conv3x3_wgrad(e, de, a2, da2, rnd, bias_terms=(fe, taue) if generic else None)
            for nm, ref, dl in ((".output_block.conv2.weight", dW, dWd), (".output_block.conv2.bias", db, dbd)):
                c = R.Check(p + nm, "wgrad3x3", ref, dl, False)
                worst, bad, where = c.ratio(grads[p + nm].detach().double().cpu().reshape(ref.shape))
                figures.append((c.name, c.kernel, worst, bad, ref.numel(), where, 0, float(ref.abs().max())))
            if l == 0:
                checks = R.dgrad3_layer(f"dense{b + 1}.{l}", G, X, Pr, Qr, keep, _tap(eng, f"bottleneck{b + 1}.{l}"), sc2, sh2,
                                        P[p + ".output_block.relu2.weight"], P[p + ".output_block.conv2.weight"], rnd, c_off, ey)
                got = [ey, _tap(eng, f"raw:du{b + 1}")] if ey is not None else [_tap(eng, f"raw:du{b + 1}")]
            elif ey is not None:
                checks, got = [R.Check(f"dense{b + 1}.{l}:ey", "eff rows", fe, taue, rnd)], [ey]
            else:
                continue
            for c, t in zip(checks, got):
                worst, bad, where = c.ratio(t)
                figures.append((c.name, c.kernel, worst, bad, c.ref.numel(), where, 0 if c.kink is None else int(c.kink.sum()),
                                float(c.ref.abs().max())))
    # ---- transition data gradients: the first writer of a block's accumulator.  The last layer's slice of G[b] receives nothing else, so
    # there the stored values are the transition's contribution alone (and exactly zero at the pixels no 2x2 window covers)
    for b in range(len(cfg.densenet_structure) - 1):
        t = f"features.transition{b + 1}"
        x, Gb = _tap(eng, f"dense{b + 1}"), _tap(eng, f"raw:grad{b + 1}")
        C = x.shape[-1]
        pq = _tap(eng, f"raw:pq{b + 2}").flatten()
        sc, sh = tabd[t + ".norm"]
        DU, d, kink = R.transition_dgrad(_tap(eng, f"raw:grad{b + 2}"), _tap(eng, f"dense{b + 2}"), pq[:pq.numel() // 2], pq[pq.numel() // 2:], x,
                                         sc, sh, P[t + ".relu.weight"], P[t + ".conv.weight"].reshape(C // 2, C), rnd, C - g)
        c = R.Check(f"transition{b + 1}:grad[{C - g}:{C}]", "transition dgrad", DU, d, rnd, kink)
        worst, bad, where = c.ratio(Gb[..., C - g:])
        H, W = x.shape[1:3]
        uncovered = int(H % 2) * W + int(W % 2) * H - int(H % 2) * int(W % 2)
        figures.append((c.name, c.kernel, worst, bad, DU.numel(), where, int(kink.sum()), float(DU.abs().max()), uncovered))
    # ---- head pooling backward: the first writer of the last block's accumulator, compared on the last layer's slice as above
    nb = len(cfg.densenet_structure)
    x, Gb = _tap(eng, f"dense{nb}"), _tap(eng, f"raw:grad{nb}")
    C = x.shape[-1]
    sc, sh = tabd["features.final_norm"]
    Gr, d, kink = R.head_pool_backward(_tap(eng, "raw:dcondense").reshape(n_img, C), x, sc, sh, P["features.final_relu.weight"], C - g)
    c = R.Check(f"head:grad[{C - g}:{C}]", "head pooling backward", Gr, d, rnd, kink)
    worst, bad, where = c.ratio(Gb[..., C - g:])
    figures.append((c.name, c.kernel, worst, bad, Gr.numel(), where, int(kink.sum()), float(Gr.abs().max())))
    _lib.lib.tcvn_profile_enable(0)
    labels = [r[0] for r in _lib.profile_records()]
    _lib.lib.tcvn_profile_reset()
    return dict(figures=figures, labels=labels, ey_filled=ey_filled, geometry=geo)


def _ru(v):
    return -(-v // 256) * 256


def _run_layers_backward(case, mode):
    """Validation build only: one backward with the snapshot hook (tcvn_debug_layer_snapshot, densenet_bwd.hip) armed for EVERY layer of
    every block and its transition / the head; every kernel of those layers against float64 on the state the layer found: eff rows (where stored), DU,
    norm2's link (dgamma2, dbeta2, dslope2, PY, QY), db1, dW1, the read-add-write of G[:, :cin], norm1's link (dgamma1, dbeta1, dslope1,
    P / Q[:cin] +=); the rest of G and (P, Q) must be bit-unchanged.  The report carries the fused 1x1 backward's grid per layer
    (tcvn_debug_layer_snapshot_grid).  -> report."""
    from transformercvn.hip import _lib
    lib = _lib.lib
    lib.tcvn_debug_layer_snapshot.restype = C.c_int
    lib.tcvn_debug_layer_snapshot.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64]
    lib.tcvn_debug_layer_snapshot_clear.restype = None
    lib.tcvn_debug_layer_snapshot_report.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    lib.tcvn_debug_layer_snapshot_grid.restype = C.c_int
    lib.tcvn_debug_layer_snapshot_grid.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    cfg, coords, values, n_img = _case(case)
    sd = O.fill_state(cfg, 19)
    eng, data, grads = _engine(cfg, sd, mode=mode, with_grad=True)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=True, seed=SEED)
    d_out = torch.randn(n_img, eng.out_dim, generator=torch.Generator().manual_seed(5)).cuda()
    geo, g, rnd = _geometry(cfg), cfg.densenet_growth_rate, mode == BF16
    mid, esz, dt = cfg.densenet_batch_norm_size * g, (2 if rnd else 4), (torch.bfloat16 if rnd else torch.float32)
    P = {k: v.detach().double().cpu() for k, v in data.items()}
    tabd = R.tables_from_tabs(cfg, _tap(eng, "raw:tabs").flatten())
    has_ey = rnd and g == 32
    armed = []
    lib.tcvn_debug_layer_snapshot_clear()
    for b, layers in enumerate(cfg.densenet_structure):
        H, W, _ = geo[b]
        M, ld = n_img * H * W, eng.tap(f"raw:pq{b + 1}").numel() // 2
        sizes = [_ru(M * ld * esz), _ru(ld * 8)] * 2 + [_ru(M * mid * esz), _ru(mid * 8)] + ([_ru(M * 32 * esz)] if has_ey else [])
        for l in [-1] + list(range(layers)):                             # -1: the block's transition, or the head
            buf = torch.zeros(sum(sizes), dtype=torch.uint8, device="cuda")
            idx = lib.tcvn_debug_layer_snapshot(b, l, buf.data_ptr(), buf.numel())
            armed.append((b, l, idx, buf, sizes, M, ld))
    _lib.lib.tcvn_profile_filter(None); _lib.lib.tcvn_profile_reset(); _lib.lib.tcvn_profile_enable(1)
    try:
        eng.backward(d_out)
        torch.cuda.synchronize()
    finally:
        _lib.lib.tcvn_profile_enable(0)
    labels = [r[0] for r in _lib.profile_records()]
    _lib.lib.tcvn_profile_reset()
    gr = {k: v.detach().double().cpu() for k, v in grads.items()}
    figures, reports, owners = [], [], []                                # owners[i]: the armed (block, layer) figure i belongs to

    def compare(name, kernel, ref, delta, got, rnd_store, kink=None):
        c = R.Check(name, kernel, ref, delta, rnd_store, kink)
        worst, bad, where = c.ratio(got.reshape(ref.shape))
        owners.append(owner)
        figures.append((name, kernel, worst, bad, ref.numel(), where, 0 if kink is None else int(kink.sum()), float(ref.abs().max())))

    for b, l, idx, buf, sizes, M, ld in armed:
        owner = (b, l)
        kern, fused, eyv, nbytes = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        assert lib.tcvn_debug_layer_snapshot_report(idx, C.byref(kern), C.byref(fused), C.byref(eyv), C.byref(nbytes)) == 0
        assert nbytes.value == buf.numel() - (0 if l >= 0 or not has_ey else sizes[-1]), (nbytes.value, buf.numel())      # (no eff rows around a transition)
        H, W, c0 = geo[b]
        cin = c0 + l * g
        if l >= 0:
            nblk, slices = C.c_int(-1), C.c_int(-1)
            assert lib.tcvn_debug_layer_snapshot_grid(idx, C.byref(nblk), C.byref(slices)) == 0
            reports.append((b, l, cin, kern.value, fused.value, eyv.value, nblk.value, slices.value, M))
        offs = [sum(sizes[:i]) for i in range(len(sizes))]
        raw = buf.cpu()
        sec = lambda i, nbytes_, d: raw[offs[i]: offs[i] + nbytes_].view(d).double()
        Gmap = lambda i: sec(i, M * ld * esz, dt).reshape(n_img, H, W, ld)
        G0, G1 = Gmap(0), Gmap(2)
        pq0, pq1 = sec(1, ld * 8, torch.float32), sec(3, ld * 8, torch.float32)
        DU = sec(4, M * mid * esz, dt).reshape(n_img, H, W, mid)
        pqy = sec(5, mid * 8, torch.float32)
        ey = sec(6, M * 32 * esz, dt).reshape(n_img, H, W, 32) if has_ey and eyv.value else None
        X = _tap(eng, f"dense{b + 1}")
        Ct = X.shape[-1]
        if l < 0:
            # ---- the first writer of G[b] and of its (P, Q): the stored state behind it is its contribution alone
            last = b == len(cfg.densenet_structure) - 1
            bs = _tap(eng, f"raw:bstat{b + 1}").flatten()[:2 * ld].view(ld, 2)[:Ct]
            if last:
                norm, relu, kind = "features.final_norm", "features.final_relu", "head pooling backward"
                sc, sh = tabd[norm]
                Gr, sums, gates = R.head_backward(_tap(eng, "raw:dcondense").reshape(n_img, Ct), X, sc, sh, P[relu + ".weight"])
            else:
                t = f"features.transition{b + 1}"
                norm, relu, kind = t + ".norm", t + ".relu", "transition backward"
                sc, sh = tabd[norm]
                pqn = _tap(eng, f"raw:pq{b + 2}").flatten()
                o, sums, gates = R.transition_backward(_tap(eng, f"raw:grad{b + 2}"), _tap(eng, f"dense{b + 2}"), pqn[:pqn.numel() // 2],
                                                       pqn[pqn.numel() // 2:], X, sc, sh, P[relu + ".weight"],
                                                       P[t + ".conv.weight"].reshape(Ct // 2, Ct), rnd)
                Gr = o["G"]
                compare(t + ".conv.bias", kind, o["db"][0], o["db"][1], gr[t + ".conv.bias"], False)
                compare(t + ".conv.weight", kind, o["dW"][0], o["dW"][1], gr[t + ".conv.weight"], False)
            compare(f"block{b + 1}:G after its first writer", kind, Gr[0], Gr[1], G1[..., :Ct], rnd, Gr[2])
            lk = R.bn_link(sums, gates, bs[:, 0], bs[:, 1], P[norm + ".weight"], M)
            for q, k in (("dgamma", norm + ".weight"), ("dbeta", norm + ".bias"), ("dslope", relu + ".weight")):
                compare(k, kind + " link", lk[q][0], lk[q][1], gr[k], False)
            for q, i0 in (("P", 0), ("Q", ld)):
                compare(f"block{b + 1}:{q} after its first writer", kind + " link", lk[q][0], lk[q][1], pq1[i0: i0 + Ct], False)
            continue
        p = f"features.dense{b + 1}.layers.{l}"
        nm = f"dense{b + 1}.{l}"
        y = _tap(eng, f"bottleneck{b + 1}.{l}")
        keep = _keep(cfg.dropout, SEED, 64 * b + l + 1, M, g).double().cpu().reshape(n_img, H, W, g) if cfg.dropout > 0 else None
        n2, n1 = p + ".output_block.norm2", p + ".bottleneck_block.norm1"
        sc2, sh2 = tabd[n2]
        sl2 = P[p + ".output_block.relu2.weight"]
        cs = slice(cin, cin + g)
        # ---- 3x3 data gradient -> DU
        f, tau, e, de = R.eff_rows(G0[..., cs], X[..., cs], pq0[:ld][cs], pq0[ld:][cs], keep, rnd)
        if ey is not None:
            compare(nm + ":ey", "eff rows", f, tau, ey, rnd)
            e, de = ey, torch.zeros_like(ey)
        dA, ddA = R.conv3x3_dgrad(e, de, P[p + ".output_block.conv2.weight"], rnd)
        ref, dl, kink = R.prelu_bn_backward(dA, ddA, y, sc2, sh2, sl2)
        compare(nm + ":du", "dgrad3x3", ref, dl, DU, rnd, kink)
        # ---- norm2's link
        ys = _tap(eng, f"raw:ystat{b + 1}.{l}").flatten()[:2 * mid].view(mid, 2)
        _, _, _, sums, gates = R.bn_sums(dA, ddA, y, sc2, sh2, sl2)
        lk = R.bn_link(sums, gates, ys[:, 0], ys[:, 1], P[n2 + ".weight"], M)
        for q, k in (("dgamma", n2 + ".weight"), ("dbeta", n2 + ".bias"), ("dslope", p + ".output_block.relu2.weight")):
            compare(k, "norm2 link", lk[q][0], lk[q][1], gr[k], False)
        compare(nm + ":PY", "norm2 link", lk["P"][0], lk["P"][1], pqy[:mid], False)
        compare(nm + ":QY", "norm2 link", lk["Q"][0], lk["Q"][1], pqy[mid:], False)
        # ---- 1x1 backward from the STORED DU and (PY, QY)
        xin = X[..., :cin]
        sc1, sh1 = tabd[n1]
        sl1 = P[p + ".bottleneck_block.relu1.weight"]
        _, _, a1, da1 = R.activation(xin, sc1, sh1, sl1, rnd)
        xa = _tap(eng, f"xa{b + 1}.{l}")
        if xa is not None:
            a1, da1 = xa, torch.zeros_like(xa)
        o1, sums1, gates1 = R.conv1x1_backward(DU, y, pqy[:mid], pqy[mid:], a1, da1, P[p + ".bottleneck_block.conv1.weight"].reshape(mid, cin),
                                               G0[..., :cin], xin, sc1, sh1, sl1, rnd)
        kind = "1x1 backward (fused)" if fused.value else "1x1 backward (GEMMs)" if xa is not None else "1x1 backward (generic)"
        compare(p + ".bottleneck_block.conv1.bias", kind, o1["db1"][0], o1["db1"][1], gr[p + ".bottleneck_block.conv1.bias"], False)
        compare(p + ".bottleneck_block.conv1.weight", kind, o1["dW1"][0], o1["dW1"][1], gr[p + ".bottleneck_block.conv1.weight"], False)
        compare(nm + f":G[0:{cin}]", kind, o1["G"][0], o1["G"][1], G1[..., :cin], rnd, o1["G"][2])
        Ct = X.shape[-1]                                               # (the columns behind Ctot are padding nobody initialises)
        same = bool(torch.equal(G1[..., cin:Ct], G0[..., cin:Ct])) and bool(torch.equal(pq1[:ld][cin:Ct], pq0[:ld][cin:Ct])) and \
            bool(torch.equal(pq1[ld:][cin:Ct], pq0[ld:][cin:Ct]))
        owners.append(owner)
        figures.append((nm + ":rest of G, P, Q unchanged", "untouched", 0.0 if same else float("inf"), 0 if same else 1, 1, [], 0, 1.0))
        # ---- norm1's link
        bs = _tap(eng, f"raw:bstat{b + 1}").flatten()[:2 * ld].view(ld, 2)[:cin]
        lk = R.bn_link(sums1, gates1, bs[:, 0], bs[:, 1], P[n1 + ".weight"], M)
        for q, k in (("dgamma", n1 + ".weight"), ("dbeta", n1 + ".bias"), ("dslope", p + ".bottleneck_block.relu1.weight")):
            compare(k, "norm1 link", lk[q][0], lk[q][1], gr[k], False)
        for q, i0 in (("P", 0), ("Q", ld)):
            inc, d_inc = lk[q]
            compare(nm + f":{q}[0:{cin}]", "norm1 link", pq0[i0: i0 + cin] + inc, d_inc + 0.5 * R.ulp(inc.abs() + d_inc, 24), pq1[i0: i0 + cin], False)
    lib.tcvn_debug_layer_snapshot_clear()
    return dict(figures=figures, labels=labels, reports=reports, owners=owners)


# ---------------------------------------------------------------------------------------------------------------------
# the frozen schedule (hit gradients): forward_frozen + input_gradient behind a training step on the same engine and workspace
# ---------------------------------------------------------------------------------------------------------------------
FROZEN_DROPOUT = 0.1                          # configured on every frozen engine: the frozen pass must ignore it
ARENA_PATTERN = 0x7FA5C3E1                    # the bound gradient tensors are filled with these bits (a NaN) in front of the frozen pass
NO_PARAMETER_GRADIENT = ("k_conv3x3_wgrad", "k_conv_wgrad", "k_conv1x1_wgrad", "k_gemm_tn_", "k_stem_wgrad")


def _frozen_case(case):
    """The case with dropout 0.1 configured and three entries more in its hit list: one pixel listed twice, one three times (the highest
    index owns the pixel) -> cfg, coords, values, n_img."""
    cfg, coords, values, n_img = _case(case)
    cfg = copy.copy(cfg)
    cfg.dropout = FROZEN_DROPOUT
    i, j = 3, coords.shape[0] // 2
    coords = torch.cat([coords, coords[[i, j, j]]]).contiguous()
    values = torch.cat([values, values[[i + 1, j + 1, j + 2]]]).contiguous()
    return cfg, coords, values, n_img


def _fig(figures, name, kernel, ref, delta, got, rnd_store, kink=None, **extra):
    c = R.Check(name, kernel, ref, delta, rnd_store, kink)
    worst, bad, where = c.ratio(got.reshape(ref.shape))
    figures.append(dict(name=name, kernel=kernel, worst=worst, bad=bad, numel=ref.numel(), where=where, kinks=0 if kink is None else int(kink.sum()),
                        amax=float(ref.abs().max()), **extra))
    return c


def _run_frozen(case, mode, parts=("fwd", "bwd"), value_modes=(0, 1, 2)):
    """One training forward + backward with dropout on a fresh engine, then forward_frozen + input_gradient on the same engine and
    workspace; every operation against float64 on its own stored state.  parts: "fwd" the forward operations, tables and side effects;
    "bwd" what stays readable behind the backward without a hook; "hook" (validation build) every layer and first writer through the
    snapshot hook.  value_modes beyond the first repeat the frozen pass for the gather alone; on `narrow` one more pass runs on a
    workspace filled with 0xFF bytes.  -> report (plain data)."""
    from transformercvn.hip import _lib
    from test_densenet_layer_reference_cpu import frozen_seed
    import hit_gradients_reference as HG
    import stem_reference as S
    lib = _lib.lib
    cfg, coords, values, n_img = _frozen_case(case)
    sd = O.fill_state(cfg, frozen_seed(case))
    eng, data, grads = _engine(cfg, sd, mode=mode, with_grad=True)
    cd, vd = coords.cuda(), values.cuda()
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    geo, g, rnd = _geometry(cfg), cfg.densenet_growth_rate, mode == BF16
    mid, esz, dt = cfg.densenet_batch_norm_size * g, (2 if rnd else 4), (torch.bfloat16 if rnd else torch.float32)
    nb, layers = len(cfg.densenet_structure), sum(cfg.densenet_structure)
    # ---- the training step whose state the frozen pass finds in the workspace
    eng.forward(cd, vd, n_img, out, train=True, seed=SEED)
    eng.backward(torch.randn(n_img, eng.out_dim, generator=torch.Generator().manual_seed(6)).cuda())
    torch.cuda.synchronize()
    H0, W0, _ = geo[0]
    train_dropped = int((_keep(cfg.dropout, SEED, 1, n_img * H0 * W0, g) == 0).sum())
    stale_pq = max(float(eng.tap(f"raw:pq{b + 1}").abs().max()) for b in range(nb))
    stats0 = {k: v.clone() for k, v in data.items() if "running_" in k}
    for t in grads.values():
        t.view(torch.int32).fill_(ARENA_PATTERN)
    P = {k: v.detach().double().cpu() for k, v in data.items()}
    d_out = torch.randn(n_img, eng.out_dim, generator=torch.Generator().manual_seed(5))
    d_out_d = d_out.cuda()
    rep = dict(geometry=geo, train_dropped=train_dropped, stale_pq=stale_pq, fwd=[], bwd=[], hook=[], owners=[], reports=[], gather={})

    armed = []
    if "hook" in parts:
        lib.tcvn_debug_layer_snapshot.restype = C.c_int
        lib.tcvn_debug_layer_snapshot.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64]
        lib.tcvn_debug_layer_snapshot_clear.restype = None
        lib.tcvn_debug_layer_snapshot_report.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
        lib.tcvn_debug_layer_snapshot_grid.restype = C.c_int
        lib.tcvn_debug_layer_snapshot_grid.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        has_ey = rnd and g == 32
        lib.tcvn_debug_layer_snapshot_clear()
        for b, L in enumerate(cfg.densenet_structure):
            H, W, _ = geo[b]
            M, ld = n_img * H * W, eng.tap(f"raw:pq{b + 1}").numel() // 2
            sizes = [_ru(M * ld * esz), _ru(ld * 8)] * 2 + [_ru(M * mid * esz), _ru(mid * 8)] + ([_ru(M * 32 * esz)] if has_ey else [])
            for l in [-1] + list(range(L)):
                buf = torch.zeros(sum(sizes), dtype=torch.uint8, device="cuda")
                armed.append((b, l, lib.tcvn_debug_layer_snapshot(b, l, buf.data_ptr(), buf.numel()), buf, sizes, M, ld))

    def frozen_pass(vm):
        lib.tcvn_profile_filter(None); lib.tcvn_profile_reset(); lib.tcvn_profile_enable(1)
        try:
            eng.forward_frozen(cd, vd, n_img, out, vm)
            n_fwd = lib.tcvn_profile_count()
            dv = eng.input_gradient(d_out_d)
            torch.cuda.synchronize()
        finally:
            lib.tcvn_profile_enable(0)
        labels = [r[0] for r in _lib.profile_records()]
        lib.tcvn_profile_reset()
        return dv, labels[:n_fwd], labels[n_fwd:]

    own = torch.tensor(HG.owners(coords, n_img, *cfg.pixel_shape))
    rep["non_owners"] = int((~own).sum())
    w0 = P["features.conv0.weight"]

    def gather_figures(vm, dv):
        c = R.hit_gradient_check(_tap(eng, "raw:du0"), w0, coords, values, tuple(cfg.pixel_shape), vm, f"d_values (value mode {vm})")
        worst, bad, where = c.ratio(dv.double().cpu())
        return [dict(name=c.name, kernel=c.kernel, worst=worst, bad=bad, numel=c.ref.numel(), where=where, kinks=0, amax=float(c.ref.abs().max()),
                     non_owner_max=float(dv.cpu()[~own].abs().max()), owner_min=float(c.ref[own].abs().min()), nan=int(torch.isnan(dv).sum()))]

    dv0, fwd_labels, bwd_labels = frozen_pass(value_modes[0])
    if armed:                                            # the hook's report per armed entry, then disarmed: the further passes below run without it
        told = []
        for b, l, idx, buf, sizes, M, ld in armed:
            kern, fused, eyv, nbytes, nblk, slices = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int(-1), C.c_int(-1)
            assert lib.tcvn_debug_layer_snapshot_report(idx, C.byref(kern), C.byref(fused), C.byref(eyv), C.byref(nbytes)) == 0
            assert lib.tcvn_debug_layer_snapshot_grid(idx, C.byref(nblk), C.byref(slices)) == 0
            told.append((b, l, (kern.value, fused.value, eyv.value, nbytes.value, nblk.value, slices.value), buf, sizes, M, ld))
        armed = told
        lib.tcvn_debug_layer_snapshot_clear()
    rep["fwd_labels"], rep["bwd_labels"] = fwd_labels, bwd_labels
    rep["stats_unchanged"] = all(torch.equal(v, data[k]) for k, v in stats0.items()) and len(stats0) > 0
    rep["arena_unchanged"] = all(bool((t.view(torch.int32) == ARENA_PATTERN).all()) for t in grads.values())
    tabs = _tap(eng, "raw:tabs").flatten()
    tabd = R.tables_from_tabs(cfg, tabs)

    # ---- taps
    stored, paths = {}, []
    for b, L in enumerate(cfg.densenet_structure):
        stored[f"dense{b + 1}"] = _tap(eng, f"dense{b + 1}")
        assert tuple(stored[f"dense{b + 1}"].shape[1:3]) == geo[b][:2]
        for l in range(L):
            for nm in (f"bottleneck{b + 1}.{l}", f"xa{b + 1}.{l}", f"ya{b + 1}.{l}"):
                t = _tap(eng, nm)
                if t is not None:
                    stored[nm] = t
            paths.append((b, l, geo[b][2] + l * g, f"xa{b + 1}.{l}" in stored, f"ya{b + 1}.{l}" in stored, f"bottleneck{b + 1}.{l}" in stored,
                          _exists(eng, f"raw:isumy{b + 1}.{l}")))
    stored["condense"] = _tap(eng, "condense").reshape(n_img, -1)
    stored["output_linear"] = _tap(eng, "output_linear").reshape(n_img, -1)
    c0 = _tap(eng, "conv0")
    rep["paths"], rep["conv0"] = paths, c0 is not None
    rep["padded"] = [n_img * (H + 2) * (W + 2) for H, W, _ in geo]

    if "fwd" in parts:
        # ---- tables from the bound running statistics: a handful of correctly rounded fp32 operations, 8 u of the magnitude of their terms
        # (test_batchnorm_stats_gpu.py; the statistics themselves are the exact fp32 inputs here, so no row gate is propagated)
        for name, (sc, sh) in R.running_tables(cfg, P).items():
            for q, ref, gate, got in (("sc", sc, 8 * R.U * sc.abs(), tabd[name][0]),
                                      ("sh", sh, 8 * R.U * (P[name + ".bias"].abs() + (P[name + ".running_mean"] * sc).abs()), tabd[name][1])):
                err = (got - ref).abs()
                bad = ~(err <= gate)
                rep["fwd"].append(dict(name=f"{name}:{q}", kernel="table", worst=float(torch.where(err > 0, err / gate, torch.zeros_like(err)).max()),
                                       bad=int(bad.sum()), numel=ref.numel(), where=[int(i) for i in bad.nonzero()[:4]], kinks=0, amax=float(ref.abs().max())))
        checks, _ = R.run_forward(cfg, P, rnd, False, c0, None, stored=stored, tabs=tabs)
        dropped = 0
        for c in checks:
            got = R.stored_counterpart(c, stored)
            worst, bad, where = c.ratio(got)
            rep["fwd"].append(dict(name=c.name, kernel=c.kernel, worst=worst, bad=bad, numel=c.ref.numel(), where=where, kinks=0, amax=float(c.ref.abs().max())))
            if c.kernel == "conv3x3":
                dropped += int(((got == 0) & (c.ref.abs() > c.gate)).sum())
        rep["dropped"] = dropped

    if "bwd" in parts or "hook" in parts:
        dcond = _tap(eng, "raw:dcondense").reshape(n_img, -1)
        G = {b: _tap(eng, f"raw:grad{b + 1}") for b in range(nb)}
        pq = {b: _tap(eng, f"raw:pq{b + 1}").flatten() for b in range(nb)}
        rep["pq_zero"] = all(float(v.abs().max()) == 0 for v in pq.values()) and float(_tap(eng, "raw:pq0").abs().max()) == 0

    def first_writer(b):
        """(ref, delta, kink) of block b's first writer over all channels, from the stored state."""
        x = stored[f"dense{b + 1}"]
        Ct = x.shape[-1]
        if b == nb - 1:
            sc, sh = tabd["features.final_norm"]
            return R.head_backward(dcond, x, sc, sh, P["features.final_relu.weight"])[0]
        t = f"features.transition{b + 1}"
        sc, sh = tabd[t + ".norm"]
        zn = torch.zeros(stored[f"dense{b + 2}"].shape[-1], dtype=torch.float64)
        o, _, _ = R.transition_backward(G[b + 1], stored[f"dense{b + 2}"], zn, zn, x, sc, sh, P[t + ".relu.weight"],
                                        P[t + ".conv.weight"].reshape(Ct // 2, Ct), rnd)
        return o["G"]

    if "bwd" in parts:
        figs = rep["bwd"]
        o = "output_block.norm"
        ref, d, krows = R.output_block_backward_frozen(d_out.double(), stored["output_linear"], P[o + ".weight"], P[o + ".bias"], P[o + ".running_mean"],
                                                       P[o + ".running_var"], P["output_block.relu.weight"], P["output_block.linear.weight"])
        _fig(figs, "raw:dcondense", "output block backward", ref, d, dcond, False, krows)
        for b in reversed(range(nb)):
            x = stored[f"dense{b + 1}"]
            H, W, cb = geo[b]
            Ct, L = x.shape[-1], cfg.densenet_structure[b]
            fw = first_writer(b)
            kind = "head pooling backward" if b == nb - 1 else "transition dgrad"
            sl_ = slice(Ct - g, Ct)
            uncovered = torch.zeros(H, W, dtype=torch.bool)
            if b != nb - 1:
                uncovered[2 * (H // 2):], uncovered[:, 2 * (W // 2):] = True, True
            edge = G[b][..., sl_][:, uncovered]
            _fig(figs, f"block{b + 1}:grad[{Ct - g}:{Ct}] after its first writer", kind, fw[0][..., sl_], fw[1][..., sl_], G[b][..., sl_], rnd, fw[2][..., sl_],
                 uncovered=int(uncovered.sum()), edge_max=float(edge.abs().max()) if edge.numel() else 0.0)
            pre = f"features.dense{b + 1}.layers."
            n1 = [tabd[pre + f"{l}.bottleneck_block.norm1"] for l in range(L)]
            n2 = [tabd[pre + f"{l}.output_block.norm2"] for l in range(L)]
            cks, got = R.frozen_block_slices(f"block{b + 1}", fw, G[b], x, [stored[f"bottleneck{b + 1}.{l}"] for l in range(L)], n1, n2,
                                             [P[pre + f"{l}.bottleneck_block.relu1.weight"] for l in range(L)],
                                             [P[pre + f"{l}.output_block.relu2.weight"] for l in range(L)],
                                             [P[pre + f"{l}.bottleneck_block.conv1.weight"].reshape(mid, cb + l * g) for l in range(L)],
                                             [P[pre + f"{l}.output_block.conv2.weight"] for l in range(L)], cb, g, rnd)
            for c, t in zip(cks, got):
                worst, bad, where = c.ratio(t)
                figs.append(dict(name=c.name, kernel=c.kernel, worst=worst, bad=bad, numel=c.ref.numel(), where=where, kinks=int(c.kink.sum()),
                                 amax=float(c.ref.abs().max())))
        # ---- DU of the layer that ran last: block 1, layer 0
        zero = torch.zeros(stored["dense1"].shape[-1], dtype=torch.float64)
        p = "features.dense1.layers.0"
        (c,) = R.dgrad3_layer("dense1.0", G[0], stored["dense1"], zero, zero, None, stored["bottleneck1.0"], *tabd[p + ".output_block.norm2"],
                              P[p + ".output_block.relu2.weight"], P[p + ".output_block.conv2.weight"], rnd, geo[0][2])
        worst, bad, where = c.ratio(_tap(eng, "raw:du1"))
        figs.append(dict(name="raw:du1", kernel="dgrad3x3", worst=worst, bad=bad, numel=c.ref.numel(), where=where, kinks=int(c.kink.sum()), amax=float(c.ref.abs().max())))
        # ---- the stem's pooling backward with P0 = Q0 = 0 -> DU0 over the whole conv0 map
        C0 = geo[0][2]
        z0 = torch.zeros(C0, dtype=torch.float64)
        sc, sh = tabd["features.norm0"]
        dz, ddz = S.pool_backward(G[0][..., :C0], stored["dense1"][..., :C0], z0, z0, c0.shape[1], c0.shape[2])
        dU, ddU, kink, _, _ = S.stem_sums(dz, ddz, c0, None, sc, sh, P["features.relu0.weight"])
        _fig(figs, "raw:du0", "pool0 backward", sc * dU, sc.abs() * ddU + R.R(1) * (sc * dU).abs(), _tap(eng, "raw:du0"), rnd, kink)

    if "hook" in parts:
        _frozen_hook_figures(rep, armed, eng, cfg, P, tabd, stored, G, first_writer, n_img, geo, rnd)

    # ---- the gather, per value mode, from the STORED DU0
    rep["gather"][value_modes[0]] = gather_figures(value_modes[0], dv0)
    for vm in value_modes[1:]:
        dv, _, lab = frozen_pass(vm)
        rep["gather"][vm] = gather_figures(vm, dv)
        rep["gather"][vm][0]["hit_launches"] = _count(lab, "k_hit_gradient")
    if case == "narrow":
        eng._ws.fill_(0xFF)
        dvp, _, _ = frozen_pass(value_modes[0])
        again = gather_figures(value_modes[0], dvp)
        rep["poison_equal"] = bool(torch.equal(dvp, dv0)) and again[0]["nan"] == 0
    return rep


def _frozen_hook_figures(rep, armed, eng, cfg, P, tabd, stored, G, first_writer, n_img, geo, rnd):
    """The snapshots of a frozen backward (validation build): per first writer G over all channels as the contribution alone; per layer
    the eff rows (where stored), DU, the read-add-write of G[:, :cin] from the STORED DU with PY = QY = 0, the rest of G bit-unchanged;
    (P, Q) of the block in front of and behind every launch and (PY, QY) behind it exactly zero."""
    from transformercvn.hip import _lib
    lib = _lib.lib
    g = cfg.densenet_growth_rate
    mid, esz, dt = cfg.densenet_batch_norm_size * g, (2 if rnd else 4), (torch.bfloat16 if rnd else torch.float32)
    has_ey = rnd and g == 32
    figs, owners = rep["hook"], rep["owners"]

    def compare(owner, name, kernel, ref, delta, got, rnd_store, kink=None):
        _fig(figs, name, kernel, ref, delta, got, rnd_store, kink)
        owners.append(owner)

    def flag(owner, name, kernel, ok):
        figs.append(dict(name=name, kernel=kernel, worst=0.0 if ok else float("inf"), bad=0 if ok else 1, numel=1, where=[], kinks=0, amax=1.0))
        owners.append(owner)

    for b, l, (kern, fused, eyv, nbytes, nblk, slices), buf, sizes, M, ld in armed:
        assert nbytes == buf.numel() - (0 if l >= 0 or not has_ey else sizes[-1]), (nbytes, buf.numel())
        H, W, c0 = geo[b]
        cin = c0 + l * g
        if l >= 0:
            rep["reports"].append((b, l, cin, kern, fused, eyv, nblk, slices, M))
        offs = [sum(sizes[:i]) for i in range(len(sizes))]
        raw = buf.cpu()
        sec = lambda i, nbytes_, d: raw[offs[i]: offs[i] + nbytes_].view(d).double()
        Gmap = lambda i: sec(i, M * ld * esz, dt).reshape(n_img, H, W, ld)
        G0, G1 = Gmap(0), Gmap(2)
        pq0, pq1 = sec(1, ld * 8, torch.float32), sec(3, ld * 8, torch.float32)
        X = stored[f"dense{b + 1}"]
        Ct = X.shape[-1]
        rows_zero = all(float(t[i0: i0 + Ct].abs().max()) == 0 for t in (pq0, pq1) for i0 in (0, ld))
        if l < 0:
            fw = first_writer(b)
            kind = "head pooling backward" if b == len(cfg.densenet_structure) - 1 else "transition backward"
            compare((b, l), f"block{b + 1}:G after its first writer", kind, fw[0], fw[1], G1[..., :Ct], rnd, fw[2])
            flag((b, l), f"block{b + 1}:(P, Q) exactly zero around its first writer", "zero rows", rows_zero)
            continue
        DU = sec(4, M * mid * esz, dt).reshape(n_img, H, W, mid)
        pqy = sec(5, mid * 8, torch.float32)
        ey = sec(6, M * 32 * esz, dt).reshape(n_img, H, W, 32) if has_ey and eyv else None
        p, nm = f"features.dense{b + 1}.layers.{l}", f"dense{b + 1}.{l}"
        y = stored[f"bottleneck{b + 1}.{l}"]
        cs = slice(cin, cin + g)
        zg = torch.zeros(g, dtype=torch.float64)
        f, tau, e, de = R.eff_rows(G0[..., cs], X[..., cs], zg, zg, None, rnd)
        if ey is not None:
            compare((b, l), nm + ":ey", "eff rows", f, tau, ey, rnd)
            e, de = ey, torch.zeros_like(ey)
        dA, ddA = R.conv3x3_dgrad(e, de, P[p + ".output_block.conv2.weight"], rnd)
        ref, dl, kink = R.prelu_bn_backward(dA, ddA, y, *tabd[p + ".output_block.norm2"], P[p + ".output_block.relu2.weight"])
        compare((b, l), nm + ":du", "dgrad3x3", ref, dl, DU, rnd, kink)
        xin = X[..., :cin]
        sc1, sh1 = tabd[p + ".bottleneck_block.norm1"]
        sl1 = P[p + ".bottleneck_block.relu1.weight"]
        _, _, a1, da1 = R.activation(xin, sc1, sh1, sl1, rnd)
        xa = stored.get(f"xa{b + 1}.{l}")
        if xa is not None:
            a1, da1 = xa, torch.zeros_like(xa)
        zy = torch.zeros(mid, dtype=torch.float64)
        o1, _, _ = R.conv1x1_backward(DU, y, zy, zy, a1, da1, P[p + ".bottleneck_block.conv1.weight"].reshape(mid, cin), G0[..., :cin], xin, sc1, sh1, sl1, rnd)
        kind = "1x1 backward (fused)" if fused else "1x1 backward (GEMMs)" if xa is not None else "1x1 backward (generic)"
        compare((b, l), nm + f":G[0:{cin}]", kind, o1["G"][0], o1["G"][1], G1[..., :cin], rnd, o1["G"][2])
        flag((b, l), nm + ":rest of G unchanged", "untouched", bool(torch.equal(G1[..., cin:Ct], G0[..., cin:Ct])))
        flag((b, l), nm + ":(P, Q) and (PY, QY) exactly zero", "zero rows", rows_zero and float(pqy.abs().max()) == 0)


def _first_and_last(rep, cfg):
    """The part of an every-layer report that belongs to the first and the last layer of every block and to the blocks' first writers, in
    the form the hook had before every layer was armed (reports without the grid): what test_first_and_last_layer_... reads."""
    keep = {(b, l) for b, L in enumerate(cfg.densenet_structure) for l in (-1, 0, L - 1)}
    return dict(figures=[f for f, o in zip(rep["figures"], rep["owners"]) if o in keep], labels=rep["labels"],
                reports=[r[:6] for r in rep["reports"] if r[:2] in keep])


BUILDS = {"validation": {}, "consec": dict(TCVN_DGRAD3_ANY_SIZE="1"), "unfused": dict(TCVN_NO_FWD1_FUSE="1", TCVN_NO_BWD1_FUSE="1", TCVN_NO_ACT_FUSE="1"), "generic": dict(TCVN_DISABLE_TILE="1")}


HOOK_CASES_NARROW_BUILDS = ["wide", "narrow-one", "odd", "mod4"]      # the frozen hook cases of the unfused and the generic build


def _frozen_child(case, build):
    """The frozen legs of one case in a validation-build child -> {mode: report} (parts as the module docstring's table), or None."""
    fwd, bwd = build in ("unfused", "generic") and case in FWD_CASES, build in ("consec", "generic") and case in CASES
    hook = build in ("validation", "consec") or case in HOOK_CASES_NARROW_BUILDS
    parts = tuple(p for p, on in (("fwd", fwd), ("bwd", bwd), ("hook", hook)) if on)
    if not parts:
        return None
    return {m: _run_frozen(case, m, parts, (0, 1, 2) if bwd else (0,)) for m in ((BF16, F32) if build == "validation" else (BF16,))}


@functools.lru_cache(maxsize=None)
def _child_reports(build):
    """All cases of one validation-build knob set in ONE child process (knobs are read once per process) -> {case: (forward report,
    backward report, {mode: first-and-last-layer view of the hook report}, {mode: hook report of every layer}, {mode: frozen report})}."""
    from variant_utils import run_on_debug_build
    fwd, bwd = build in ("unfused", "generic"), build in ("consec", "generic")
    modes = "(T.BF16, T.F32)" if build == "validation" else "(T.BF16,)"
    out = run_on_debug_build("import test_densenet_layers_float64_gpu as T\n"
                             f"result = dict((c, (T._run(c, T.BF16, True) if {fwd} and c in T.FWD_CASES else None,\n"
                             f"                       T._run_backward(c, T.BF16, {build == 'generic'}) if {bwd} and c in T.CASES else None,\n"
                             f"                       dict((m, T._run_layers_backward(c, m)) for m in {modes}),\n"
                             f"                       T._frozen_child(c, {build!r}))) for c in T.LAYER_CASES)\n",
                             BUILDS[build])
    return {c: (f, b, {m: _first_and_last(r, _case(c)[0]) for m, r in full.items()}, full, frozen) for c, (f, b, full, frozen) in out.items()}


@functools.lru_cache(maxsize=None)
def _frozen_report(case, build):
    """build: bf16 / fp32 (the product library, this process) or a validation-build knob set (its child), there "validation-fp32" too."""
    if build in ("bf16", "fp32"):
        return _run_frozen(case, F32 if build == "fp32" else BF16)
    child, mode = ("validation", F32) if build == "validation-fp32" else (build, BF16)
    return _child_reports(child)[case][4][mode]


def _frozen_as_forward(rep):
    """The forward part of a frozen report in the form of _run's."""
    return dict(figures=[(f["name"], f["kernel"], f["worst"], f["bad"], f["numel"], f["where"]) for f in rep["fwd"]], labels=rep["fwd_labels"],
                paths=rep["paths"], padded=rep["padded"], geometry=rep["geometry"], conv0=rep["conv0"], dropped=rep["dropped"])


@functools.lru_cache(maxsize=None)
def _report(case, build):
    if build.endswith("-frozen"):
        return _frozen_as_forward(_frozen_report(case, build[:-len("-frozen")]))
    if build in BUILDS:
        return _child_reports(build)[case][0]
    return _run(case, F32 if build == "fp32" else BF16, build != "bf16-eval")


@functools.lru_cache(maxsize=None)
def _backward_report(case, build):
    if build in BUILDS:
        return _child_reports(build)[case][1]
    return _run_backward(case, F32 if build == "fp32" else BF16)


def _count(labels, what):
    return sum(what in k for k in labels)


@pytest.mark.parametrize("build", ["bf16", "bf16-eval", "fp32", "unfused", "generic", "bf16-frozen", "fp32-frozen", "unfused-frozen", "generic-frozen"])
@pytest.mark.parametrize("case", FWD_CASES)
def test_every_forward_kernel_matches_float64_on_its_own_stored_input(case, build):
    rep = _report(case, build)
    cfg, _, _, n_img = _case(case)
    frozen = build.endswith("-frozen")
    if frozen:
        build = build[:-len("-frozen")]
    worst = {}
    for name, kernel, w, bad, numel, where in rep["figures"]:
        if not w <= worst.get(kernel, (-1.0, ""))[0]:
            worst[kernel] = (w, name)
    print(case, build + ("-frozen" if frozen else ""), "worst |error| / gate per kernel:", {k: (round(v, 4), nm) for k, (v, nm) in sorted(worst.items())},
          "elements", sum(f[4] for f in rep["figures"]))
    bad = [f for f in rep["figures"] if f[3] or not f[2] <= 1.0]
    assert not bad, bad[:8]

    # ---- the case is what it is there for
    geo, pp = rep["geometry"], rep["padded"]
    layers = sum(cfg.densenet_structure)
    if case.startswith("wide"):
        assert geo[0][:2] == (9, 69) and 128 < 2 * (69 + 2) and pp[0] % 128 != 0 and (pp[0] // n_img) % 128 != 0      # tiles straddle images
        assert geo[0][0] % 2 == 1 and geo[0][1] % 2 == 1                                                          # floor-pooling remainder
    if case == "wide-dropout" and build != "bf16-eval" and not frozen:
        assert rep["dropped"] > 0
    if case == "narrow-one":
        assert pp[-1] < 128
    if case.startswith("narrow"):
        assert geo[-1][:2] == (6, 4)
    if case == "odd":
        assert [p[2] % 8 for p in rep["paths"]] == [2] * 10 and rep["paths"][-1][2] > 512
    if case == "mod4":                        # production block 4's widths: the last 16-byte chunk of a row is half foreign
        assert [p[2] for p in rep["paths"]] == [228, 260, 292, 324, 356, 388] and all(p[2] % 8 == 4 for p in rep["paths"])
    # ---- every operation was compared
    n_ops = 2 * layers + len(cfg.densenet_structure) - 1 + 2 + int(rep["conv0"]) + sum(p[3] + (p[4] and p[5]) for p in rep["paths"])
    if frozen:
        n_ops += 2 * len(R.bn_names(cfg))                           # every table's scale and shift rows against the bound running statistics
    assert len(rep["figures"]) == n_ops, (len(rep["figures"]), n_ops)
    # ---- the run went through the kernels it is meant to cover
    labels = rep["labels"]
    wide1 = [p[2] > 512 for p in rep["paths"]]                     # fwd1x1_fused_ok rejects K > 512: NT GEMM on the materialised operand
    xa, ya, y, lf2 = ([p[i] for p in rep["paths"]] for i in (3, 4, 5, 6))
    if frozen:
        # the frozen schedule: an eval forward on running statistics that keeps what a backward needs, behind a training step with dropout
        full = _frozen_report(case, build)
        assert len([f for f in rep["figures"] if f[1] == "table"]) == 2 * len(R.bn_names(cfg))
        assert rep["conv0"], "a frozen pass takes the dense stem"
        assert all(y) and not any(lf2), rep["paths"]               # every Y stored (no norm2 in a 1x1 epilogue), no batch statistics derived
        assert full["train_dropped"] > 0 and rep["dropped"] == 0    # dropout 0.1 is configured, the training step drew it, the frozen pass dropped nothing
        assert full["stats_unchanged"], "running statistics moved"   # (the engine binds no num_batches_tracked: the counters are the Python runtime's)
        assert not any(_count(labels, k) for k in ("k_hit_gradient", "dgrad", "wgrad")), labels
    if build == "bf16":
        assert rep["conv0"] and xa == wide1 and not any(ya) and all(y) and lf2 == [not w and not frozen for w in wide1], rep["paths"]
        assert _count(labels, "k_fwd1x1_fused_bf16") == layers - sum(wide1) and _count(labels, "k_gemm_nt_bf16<fwd1x1>") == sum(wide1), labels
        assert _count(labels, "k_conv3x3_fwd_bf16") == layers and not _count(labels, "k_conv_fwd<bf16,2"), labels
    elif build == "bf16-eval":
        assert all(ya) and not any(y) and not any(lf2), rep["paths"]      # the activated map is the 1x1's only output
        assert _count(labels, "k_conv3x3_fwd_bf16") == layers, labels
    elif build == "fp32":
        assert not any(xa) and not any(ya) and all(y) and not any(lf2), rep["paths"]
        assert not _count(labels, "bf16"), labels
    elif build == "unfused":
        assert all(xa) and all(ya) and all(y), rep["paths"]
        assert not _count(labels, "k_fwd1x1_fused_bf16") and _count(labels, "k_gemm_nt_bf16<fwd1x1>") == layers, labels
        assert _count(labels, "k_gemm_nt_bf16<fwdtrans>") == len(cfg.densenet_structure) - 1, labels
    elif build == "generic":
        assert not _count(labels, "k_conv3x3_fwd_bf16") and _count(labels, "k_conv_fwd<bf16") >= layers, labels


@pytest.mark.parametrize("build", ["bf16", "consec", "generic", "fp32"])
@pytest.mark.parametrize("case", CASES)
def test_backward_kernels_match_float64_on_their_own_stored_inputs(case, build):
    rep = _backward_report(case, build)
    cfg, _, _, n_img = _case(case)
    nb, layers = len(cfg.densenet_structure), sum(cfg.densenet_structure)
    worst = {}
    for name, kernel, w, bad, numel, where, kinks, amax, *_ in rep["figures"]:
        if not w <= worst.get(kernel, (-1.0, ""))[0]:
            worst[kernel] = (w, name)
    print(case, build, "worst |error| / gate per kernel:", {k: (round(v, 4), nm) for k, (v, nm) in sorted(worst.items())},
          "elements at a PReLU kink (left out):", sum(f[6] for f in rep["figures"]), "of", sum(f[4] for f in rep["figures"] if f[1] in ("dgrad3x3", "transition dgrad", "head pooling backward")))
    bad = [f for f in rep["figures"] if f[3] or not f[2] <= 1.0]
    assert not bad, bad[:8]
    assert len([f for f in rep["figures"] if f[1] == "wgrad3x3"]) == 2 * layers
    if build in ("bf16", "consec"):
        assert _count(rep["labels"], "k_conv3x3_wgrad_bf16") == layers, rep["labels"]
    assert len([f for f in rep["figures"] if f[1] == "head pooling backward"]) == 1
    tr = [f for f in rep["figures"] if f[1] == "transition dgrad"]
    assert len(tr) == nb - 1
    if case.startswith("wide"):
        assert tr[0][8] == 9 + 69 - 1, tr[0]                            # the odd 9 x 69 map: a row and a column no window covers
    if build in ("bf16", "consec"):
        assert _count(rep["labels"], "k_gemm_nt_bf16<dgradtrans>") == nb - 1, rep["labels"]
    du = [f for f in rep["figures"] if f[1] == "dgrad3x3"]
    assert len(du) == nb, du                                           # one first layer per block
    if n_img == 1:      # the output block's train-mode BatchNorm1d over ONE row passes no gradient: every reference is exactly 0, and so must the kernels' be
        assert all(f[7] == 0 and f[2] == 0 for f in rep["figures"]), rep["figures"]
    else:
        assert all(f[7] > 0 for f in rep["figures"]), [f for f in rep["figures"] if not f[7] > 0]
    labels, filled = rep["labels"], rep["ey_filled"]
    aligned = cfg.initial_pixel_dim % 8 == 0                           # the LDS-DMA kernels need 16-byte aligned slices
    if build == "consec":
        assert filled == [aligned] * layers, filled                    # the consecutive-tile kernel ran (it alone stores the eff rows)
        assert len([f for f in rep["figures"] if f[1] == "eff rows"]) == (layers if aligned else 0)
    else:
        assert not any(filled), filled
    if build in ("bf16", "consec"):
        assert _count(labels, "k_conv3x3_dgrad_bf16") == layers and not _count(labels, "k_conv_dgrad<bf16,2"), labels
    elif build == "generic":
        assert _count(labels, "k_conv_dgrad<bf16,2") == layers and not _count(labels, "k_conv3x3_dgrad_bf16"), labels
        assert _count(labels, "k_conv_wgrad<bf16,2") == layers and not _count(labels, "k_conv3x3_wgrad_bf16"), labels
    else:
        assert not _count(labels, "bf16"), labels
        assert _count(labels, "k_conv3x3_dgrad_f32") + _count(labels, "k_conv_dgrad<float,2") == layers, labels


@pytest.mark.parametrize("build", ["validation", "validation-fp32", "consec", "unfused", "generic"])
@pytest.mark.parametrize("case", CASES)
def test_first_and_last_layer_backward_match_float64_on_the_state_they_found(case, build):
    """The snapshot hook of the validation build, armed for the first and the last layer of every block (_run_layers_backward)."""
    child, mode = ("validation", F32) if build == "validation-fp32" else (build, BF16)
    rep = _child_reports(child)[case][2][mode]
    cfg, _, _, n_img = _case(case)
    worst = {}
    for name, kernel, w, bad, numel, where, kinks, amax in rep["figures"]:
        if not w <= worst.get(kernel, (-1.0, ""))[0]:
            worst[kernel] = (w, name)
    print(case, build, "worst |error| / gate per kernel:", {k: (round(v, 4), nm) for k, (v, nm) in sorted(worst.items())},
          "elements at a PReLU kink (left out):", sum(f[6] for f in rep["figures"]), "layers (block, layer, cin, dgrad kernel, fused 1x1, eff rows):", rep["reports"])
    bad = [f for f in rep["figures"] if f[3] or not f[2] <= 1.0]
    assert not bad, [f[:5] for f in bad[:12]]
    armed = sum(len({0, L - 1}) for L in cfg.densenet_structure)
    assert len(rep["reports"]) == armed and [r[:2] for r in rep["reports"]] == [(b, l) for b, L in enumerate(cfg.densenet_structure) for l in sorted({0, L - 1})]
    labels = rep["labels"]
    layers = sum(cfg.densenet_structure)
    aligned = cfg.initial_pixel_dim % 8 == 0
    TWO_WG, PIPELINED, CONSEC = 1, 2, 3                                # Conv3x3Dgrad (tcvn_ops.h)
    for b, l, cin, kern, fused, eyv in rep["reports"]:
        if build in ("validation", "unfused"):
            assert kern == (PIPELINED if aligned else TWO_WG) and not eyv, rep["reports"]      # the product choice at these sizes
        elif build == "consec":
            assert kern == (CONSEC if aligned else TWO_WG) and eyv == int(aligned), rep["reports"]
        else:
            assert kern == 0 and not eyv, rep["reports"]
        assert fused == int(build in ("validation", "consec")), rep["reports"]
    if build == "unfused":
        assert _count(labels, "k_gemm_tn_bf16<conv1>") == layers and _count(labels, "k_gemm_nt_bf16<dgrad1x1>") == layers, labels
        assert not _count(labels, "k_bwd1x1_fused_bf16"), labels
    if build in ("validation", "consec"):
        assert _count(labels, "k_bwd1x1_fused_bf16") == layers, labels


@pytest.mark.parametrize("build", ["validation", "validation-fp32", "consec", "unfused", "generic"])
@pytest.mark.parametrize("case", LAYER_CASES)
def test_every_layer_backward_matches_float64_on_the_state_it_found(case, build):
    """The snapshot hook of the validation build, armed for every layer of every block (_run_layers_backward); the fused 1x1 backward's grid
    is asserted per layer, so that a changed cap cannot quietly take `trips` back to one tile per workgroup."""
    child, mode = ("validation", F32) if build == "validation-fp32" else (build, BF16)
    rep = _child_reports(child)[case][3][mode]
    cfg, _, _, n_img = _case(case)
    worst = {}
    for name, kernel, w, bad, numel, where, kinks, amax in rep["figures"]:
        if not w <= worst.get(kernel, (-1.0, ""))[0]:
            worst[kernel] = (w, name)
    print(case, build, "worst |error| / gate per kernel:", {k: (round(v, 4), nm) for k, (v, nm) in sorted(worst.items())},
          "elements at a PReLU kink (left out):", sum(f[6] for f in rep["figures"]),
          "layers (block, layer, cin, dgrad kernel, fused 1x1, eff rows, fused grid, slices, M):", rep["reports"])
    bad = [f for f in rep["figures"] if f[3] or not f[2] <= 1.0]
    assert not bad, [f[:5] for f in bad[:12]]
    layers = sum(cfg.densenet_structure)
    geo, g = _geometry(cfg), cfg.densenet_growth_rate
    assert len(rep["reports"]) == layers and [r[:3] for r in rep["reports"]] == \
        [(b, l, geo[b][2] + l * g) for b, L in enumerate(cfg.densenet_structure) for l in range(L)], rep["reports"]
    # every layer was compared: DU, norm2's link (5), db1, dW1, G[:, :cin], the rest unchanged, norm1's link (5) (+ the eff rows where stored);
    # per first writer G, three parameter gradients, P, Q (+ dW, db of a transition)
    n_first = 6 * len(cfg.densenet_structure) + 2 * (len(cfg.densenet_structure) - 1)
    n_ey = len([f for f in rep["figures"] if f[1] == "eff rows"])
    assert len(rep["figures"]) == 15 * layers + n_ey + n_first, (len(rep["figures"]), layers, n_ey, n_first)
    for kind, n in (("dgrad3x3", 1), ("norm2 link", 5), ("norm1 link", 5), ("untouched", 1)):
        assert len([f for f in rep["figures"] if f[1] == kind]) == n * layers, kind
    labels = rep["labels"]
    fused_build = build in ("validation", "consec")
    aligned = cfg.initial_pixel_dim % 8 == 0
    TWO_WG, PIPELINED, CONSEC = 1, 2, 3                                # Conv3x3Dgrad (tcvn_ops.h)
    for b, l, cin, kern, fused, eyv, nblk, slices, M in rep["reports"]:
        if build in ("validation", "unfused"):
            assert kern == (PIPELINED if aligned else TWO_WG) and not eyv, rep["reports"]      # the product choice at these sizes
        elif build == "consec":
            assert kern == (CONSEC if aligned else TWO_WG) and eyv == int(aligned), rep["reports"]
        else:
            assert kern == 0 and not eyv, rep["reports"]
        assert fused == int(fused_build), rep["reports"]
        # ---- the fused kernel's grid: bwd1x1_fused_nblk re-stated (max(64, 512 // slices) workgroups of 64 pixels, at most one per tile)
        assert M == n_img * geo[b][0] * geo[b][1] and slices == -(-cin // 128), rep["reports"]
        assert nblk == (min(-(-M // 64), max(64, 512 // slices)) if fused_build else 0) and (not fused_build or (nblk, slices) == fused_grid(M, cin)[:2]), rep["reports"]
        if case != "trips" and fused_build:
            assert nblk == -(-M // 64), rep["reports"]                  # one tile per workgroup everywhere else
    if case == "mod4":
        assert [r[2] for r in rep["reports"]] == [228, 260, 292, 324, 356, 388] and all(r[2] % 8 == 4 for r in rep["reports"])
        assert [r[7] for r in rep["reports"]] == [2, 3, 3, 3, 3, 4], rep["reports"]
        assert not aligned and all(r[3] == (TWO_WG if mode == BF16 and build != "generic" else 0) for r in rep["reports"]), rep["reports"]
    if case == "trips":
        assert [r[7] for r in rep["reports"]] == [2, 3, 3, 3, 3, 4] and all(r[8] == 11475 for r in rep["reports"]), rep["reports"]
        assert 11475 % 64 == 19 and -(-11475 // 64) == 180              # the partial last tile is tile 179: it lands in a second trip
        if fused_build:
            assert [r[6] for r in rep["reports"]] == [180, 170, 170, 170, 170, 128], rep["reports"]
            assert all(-(-r[8] // 64) > r[6] for r in rep["reports"] if r[7] >= 3), rep["reports"]      # a second tile per workgroup
    if build == "unfused":
        assert _count(labels, "k_gemm_tn_bf16<conv1>") == layers and _count(labels, "k_gemm_nt_bf16<dgrad1x1>") == layers, labels
        assert not _count(labels, "k_bwd1x1_fused_bf16"), labels
    if build in ("validation", "consec"):
        assert _count(labels, "k_bwd1x1_fused_bf16") == layers, labels


# ---------------------------------------------------------------------------------------------------------------------
# the frozen backward
# ---------------------------------------------------------------------------------------------------------------------
def _frozen_print(case, build, figs, rep):
    worst = {}
    for f in figs:
        if not f["worst"] <= worst.get(f["kernel"], (-1.0, ""))[0]:
            worst[f["kernel"]] = (f["worst"], f["name"])
    print(case, build, "frozen: worst |error| / gate per kernel:", {k: (round(v, 4), nm) for k, (v, nm) in sorted(worst.items())},
          "elements at a PReLU kink (left out):", sum(f["kinks"] for f in figs), "of", sum(f["numel"] for f in figs),
          "largest stale |P|, |Q| the training step left:", rep["stale_pq"])


def _frozen_schedule(rep, cfg, n_img):
    """What every frozen backward must show, whatever the build: nothing delivered to a parameter gradient, one gather."""
    assert rep["arena_unchanged"], "a frozen backward wrote into the bound gradient tensors"
    assert rep["stats_unchanged"], "running statistics moved"
    assert rep["pq_zero"], "(P, Q) or (P0, Q0) not zero behind a frozen backward"
    assert n_img == 1 or rep["stale_pq"] > 0                            # the training step did leave (P, Q) rows in this workspace
    labels = rep["fwd_labels"] + rep["bwd_labels"]
    assert not any(_count(labels, k) for k in NO_PARAMETER_GRADIENT), labels      # (links, slab reducers and k_unpack carry no launch label:
    assert _count(rep["bwd_labels"], "k_hit_gradient") == 1, rep["bwd_labels"]    #  what they would write is the arena, checked above)


@pytest.mark.parametrize("build", ["bf16", "fp32", "consec", "generic"])
@pytest.mark.parametrize("case", CASES)
def test_frozen_backward_matches_float64_on_its_own_stored_state(case, build):
    """forward_frozen + input_gradient behind a training step with dropout on the same engine and workspace, no hook: raw:dcondense, every
    block's first writer on the last layer's slice (odd edge exactly zero), the final G slices of every layer, DU of block 1's first
    layer, raw:du0, and d_values against the gather of the stored raw:du0 in value modes 0, 1, 2 with duplicate entries."""
    rep = _frozen_report(case, build)
    cfg, _, _, n_img = _case(case)
    nb, layers = len(cfg.densenet_structure), sum(cfg.densenet_structure)
    gather = [f for vm in (0, 1, 2) for f in rep["gather"][vm]]
    figs = rep["bwd"] + gather
    _frozen_print(case, build, figs, rep)
    bad = [f for f in figs if f["bad"] or not f["worst"] <= 1.0]
    assert not bad, [(f["name"], f["worst"], f["bad"], f["where"]) for f in bad[:8]]
    assert all(f["amax"] > 0 for f in figs), [f["name"] for f in figs if not f["amax"] > 0]      # running statistics pass a gradient with one image too
    count = lambda k: len([f for f in rep["bwd"] if f["kernel"] == k])
    assert count("output block backward") == 1 and count("head pooling backward") == 1 and count("transition dgrad") == nb - 1
    assert count("final G slice") == layers + nb and count("dgrad3x3") == 1 and count("pool0 backward") == 1
    tr = [f for f in rep["bwd"] if f["kernel"] == "transition dgrad"]
    assert all(f["edge_max"] == 0 for f in tr), tr
    if case.startswith("wide"):
        assert tr[-1]["uncovered"] == 9 + 69 - 1, tr[-1]                # the odd 9 x 69 map: a row and a column no window covers
    assert len(gather) == 3 and rep["non_owners"] == 3                  # one pixel listed twice, one three times
    assert all(f["non_owner_max"] == 0 and f["nan"] == 0 and f["owner_min"] > 0 for f in gather), gather
    assert all(f["hit_launches"] == 1 for f in gather[1:]), gather
    if case == "narrow":
        assert rep["poison_equal"], "a frozen pass read workspace bytes it did not write"
    _frozen_schedule(rep, cfg, n_img)
    labels = rep["bwd_labels"]
    if build in ("bf16", "consec"):
        assert _count(labels, "k_bwd1x1_fused_bf16") == layers and _count(labels, "k_conv3x3_dgrad_bf16") == layers, labels
        assert _count(labels, "k_gemm_nt_bf16<dgradtrans>") == nb - 1, labels
    elif build == "generic":
        assert _count(labels, "k_conv_dgrad<bf16,2") == layers and not _count(labels, "k_conv3x3_dgrad_bf16"), labels
    else:
        assert not _count(rep["fwd_labels"] + labels, "bf16"), labels
        assert _count(labels, "k_conv3x3_dgrad_f32") + _count(labels, "k_conv_dgrad<float,2") == layers, labels


FROZEN_HOOK = [(c, b) for b in ("validation", "validation-fp32", "consec") for c in LAYER_CASES] + \
              [(c, b) for b in ("unfused", "generic") for c in HOOK_CASES_NARROW_BUILDS]


@pytest.mark.parametrize("case,build", FROZEN_HOOK)
def test_frozen_every_layer_backward_matches_float64_on_the_state_it_found(case, build):
    """The snapshot hook in input_gradient (validation build), armed for every layer and first writer of the frozen backward."""
    rep = _frozen_report(case, build)
    mode = F32 if build == "validation-fp32" else BF16
    cfg, _, _, n_img = _case(case)
    figs = rep["hook"]
    _frozen_print(case, build, figs + rep["gather"][0], rep)
    print("    layers (block, layer, cin, dgrad kernel, fused 1x1, eff rows, fused grid, slices, M):", rep["reports"])
    bad = [f for f in figs + rep["gather"][0] if f["bad"] or not f["worst"] <= 1.0]
    assert not bad, [(f["name"], f["worst"], f["bad"], f["where"]) for f in bad[:12]]
    assert all(f["amax"] > 0 for f in figs), [f["name"] for f in figs if not f["amax"] > 0]
    nb, layers = len(cfg.densenet_structure), sum(cfg.densenet_structure)
    geo, g = _geometry(cfg), cfg.densenet_growth_rate
    assert [r[:3] for r in rep["reports"]] == [(b, l, geo[b][2] + l * g) for b, L in enumerate(cfg.densenet_structure) for l in range(L)], rep["reports"]
    n_ey = len([f for f in figs if f["kernel"] == "eff rows"])
    assert len(figs) == 4 * layers + n_ey + 2 * nb, (len(figs), layers, n_ey)
    for kind, n in (("dgrad3x3", layers), ("untouched", layers), ("zero rows", layers + nb)):
        assert len([f for f in figs if f["kernel"] == kind]) == n, kind
    _frozen_schedule(rep, cfg, n_img)
    labels = rep["bwd_labels"]
    fused_build = build in ("validation", "consec")
    aligned = cfg.initial_pixel_dim % 8 == 0
    TWO_WG, PIPELINED, CONSEC = 1, 2, 3                                # Conv3x3Dgrad (tcvn_ops.h)
    for b, l, cin, kern, fused, eyv, nblk, slices, M in rep["reports"]:
        if build in ("validation", "unfused"):
            assert kern == (PIPELINED if aligned else TWO_WG) and not eyv, rep["reports"]
        elif build == "consec":
            assert kern == (CONSEC if aligned else TWO_WG) and eyv == int(aligned), rep["reports"]
        else:
            assert kern == 0 and not eyv, rep["reports"]
        assert fused == int(fused_build), rep["reports"]
        assert M == n_img * geo[b][0] * geo[b][1] and slices == -(-cin // 128), rep["reports"]
        assert nblk == (min(-(-M // 64), max(64, 512 // slices)) if fused_build else 0) and (not fused_build or (nblk, slices) == fused_grid(M, cin)[:2]), rep["reports"]
    assert n_ey == (layers if build == "consec" and aligned else 0)
    if case == "mod4":
        assert [r[2] for r in rep["reports"]] == [228, 260, 292, 324, 356, 388] and [r[7] for r in rep["reports"]] == [2, 3, 3, 3, 3, 4]
        assert all(r[3] == (TWO_WG if mode == BF16 and build != "generic" else 0) for r in rep["reports"]), rep["reports"]
    if case == "trips" and fused_build:
        assert [r[6] for r in rep["reports"]] == [180, 170, 170, 170, 170, 128], rep["reports"]      # a second tile per workgroup at three and four slices
    if case == "odd":
        assert [r[7] for r in rep["reports"]] == [2, 3, 3, 3, 3, 4, 4, 4, 4, 5], rep["reports"]
    if fused_build:
        assert _count(labels, "k_bwd1x1_fused_bf16") == layers, labels
    if build == "unfused":
        assert _count(labels, "k_gemm_nt_bf16<dgrad1x1>") == layers and not _count(labels, "k_bwd1x1_fused_bf16"), labels
