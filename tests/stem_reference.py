"""Float64 reference of the stem -- COO hit list -> dense map -> conv0 7x7 / 2 -> BatchNorm0 -> PReLU0 -> AvgPool 3 / 2 -- and of its backward,
dense and sparse, one plain function per operation, each with the |error| a correct kernel may show per element.  The companion of
densenet_layer_reference.py (everything behind the stem), whose number formats, gate rules and BatchNorm link it uses: R(n), bf16, f32, ulp,
store_gate, KINK_CAP, prelu_bn_backward, bn_sums, bn_link, eff_rows, Check.  No GPU: every function takes the operation's ACTUAL inputs
as float64 -- the hit list, the tapped maps, the (scale, shift) table out of raw:tabs, the bound fp32 parameters.  `rnd` switches the bf16
roundings on (bf16 mode) or off (fp32 mode; with float64 inputs and the gates ignored it is the exact network, which
test_stem_reference_cpu.py pins against torch autograd).

Layouts: maps NHWC; coords [nnz, 3] = (image, y, x); conv0 weight [N, Cpix, 7, 7]; Hc = (H - 1) // 2 + 1, Ho = (Hc - 3) // 2 + 1.
Gates (u = 2^-24, R(n) = (1 + u)^n - 1; the store rule of densenet_layer_reference on top of every stored tensor) are derived in the
functions' docstrings, with the kernel lines they rest on.  The elements at a PReLU kink are the only ones ever left out of a comparison,
at most KINK_CAP of a tensor.  No gate carries a fitted factor."""
import torch
import torch.nn.functional as F

import densenet_layer_reference as L
from densenet_layer_reference import R, bf16, f32, ulp

TIE_MARGIN = 8        # fp32 ulps a pixel value must keep from every bf16 rounding tie (see pixel_values)


# ---------------------------------------------------------------------------------------------------------------------
# hit list -> dense map
# ---------------------------------------------------------------------------------------------------------------------
def owners(coords, n, H, W, defect=None):
    """The documented rule for the hit list (include/tcvn_hip.h): entries outside the maps are dropped, of the entries that list one pixel
    the one with the HIGHEST list index owns it.  -> list indices of the owners (ascending), their flat pixel indices.
    defects: "lowest" (the lowest index wins), "clamp" (an entry outside the maps is clamped onto the border instead of dropped)."""
    c = coords.long()
    img, y, x = c[:, 0], c[:, 1], c[:, 2]
    ok = (img >= 0) & (img < n) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
    if defect == "clamp":
        img, y, x, ok = img.clamp(0, n - 1), y.clamp(0, H - 1), x.clamp(0, W - 1), torch.ones_like(ok)
    idx = torch.arange(c.shape[0])[ok]
    pix = ((img * H + y) * W + x)[ok]
    sign = -1 if defect == "lowest" else 1
    best = torch.full((n * H * W,), -(1 << 62), dtype=torch.int64)
    best.scatter_reduce_(0, pix, sign * idx, "amax")
    own = best[pix] == sign * idx
    return idx[own], pix[own]


def pixel_values(values, mode, rnd):
    """Value arithmetic of k_scatter (elementwise.hip:100) = preprocess_value (stem_sparse.hip:65) without noise, for fp32 `values`:
    mode 0: v / 255 (one correctly rounded division), mode 1: logf(v + 1) (v + 1 exact for the integer pixel values), mode 2: v itself.
    bf16 mode: the stored value is bf16(fp32 result).  The fp32 result lies within 1/2 ulp (division) or a few ulps (logf; its error is
    not bounded here) of the exact value, so wherever the exact value keeps TIE_MARGIN = 8 fp32 ulps from every bf16 rounding tie the
    stored value is bf16(exact), with NO error allowed; the margin is asserted for the values given (for integer v in 1..255 it is 128
    ulps for v / 255 and 395 ulps for log(v + 1)).  Mode 2 has no arithmetic: bf16(v), ties to even, exactly.
    fp32 mode: modes 0 and 2 with gate R(1) |ref|; the log mode is left out -- nothing here bounds logf.  -> ref, delta."""
    v = values.double()
    exact = v / 255.0 if mode == 0 else torch.log1p(v) if mode == 1 else v
    if not rnd:
        assert mode in (0, 2), "fp32 log mode: nothing bounds logf, not covered"
        return exact, R(1) * exact.abs()
    if mode != 2:
        assert bool((exact > 0).all())
        lo = bf16(exact)                                                   # nearest bf16; the ties are the midpoints to its two neighbours
        up = ulp(lo, 8)
        dn = torch.where(torch.frexp(lo)[0] == 0.5, 0.5 * up, up)          # (below a power of two the spacing halves)
        dist = torch.minimum((exact - (lo - 0.5 * dn)).abs(), (exact - (lo + 0.5 * up)).abs())
        assert bool((dist >= TIE_MARGIN * ulp(exact, 24)).all()), "a pixel value sits at a bf16 rounding tie"
    return bf16(exact), torch.zeros_like(exact)


def image(coords, values, n, H, W, mode, rnd, defect=None):
    """Dense map [n, H, W, Cpix] under the documented rule (owners): the whole pixel from its owner, every unlisted pixel exactly 0.
    -> ref (as stored in bf16 mode: compare with delta = 0 and no store rule), delta."""
    idx, pix = owners(coords, n, H, W, defect)
    val, dv = pixel_values(values[idx], mode, rnd)
    C = values.shape[1]
    ref, delta = torch.zeros(n * H * W, C, dtype=torch.float64), torch.zeros(n * H * W, C, dtype=torch.float64)
    ref[pix], delta[pix] = val, dv
    return ref.reshape(n, H, W, C), delta.reshape(n, H, W, C)


# ---------------------------------------------------------------------------------------------------------------------
# conv0
# ---------------------------------------------------------------------------------------------------------------------
C_CONV0 = 1


def conv0(img, w, b, rnd, defect=None):
    """7x7, stride 2, pad 3 over the map as the kernel holds it (the `img` tap: already bf16 values in bf16 mode), bf16 weights in bf16
    mode.  One fp32 fma chain over the K = 49 Cpix products (147 at three channels; the MFMA is one; the padded contraction slots of
    k_stem_fwd2_bf16, stem.hip:500, and the sparse kernels' slots of the channels a map does not have, stem_sparse.hip load_weights,
    multiply zero weights: exact) plus c = 1 further operation, the bias add (stem.hip:582; generic k_conv_fwd, conv_fwd.hip:104; the
    sparse kernels start the chain AT the bias, stem_sparse.hip:346: no more roundings): delta = R(K + 1) S, S = sum |a_k| |w_k| + |b|.
    A position no hit reaches has S = |b| and ref = b: with the store rule it must be the stored-precision bias exactly (bias_exact).
    defects: "drop_tap" (tap (2, 5) of input channel 1 missing), "transpose" (ky and kx swapped), "tap3" (the weights read with a tap
    stride of 3 out of the packed rows, whatever Cpix is: tap3_weights).  -> ref [n, Hc, Wc, N], delta."""
    w = bf16(w) if rnd else w
    wk = w
    if defect == "tap3":
        wk = tap3_weights(w)
    if defect == "drop_tap":
        wk = w.clone(); wk[:, 1, 2, 5] = 0
    if defect == "transpose":
        wk = w.transpose(2, 3)
    x = img.permute(0, 3, 1, 2)
    ref = F.conv2d(x, wk, b, stride=2, padding=3).permute(0, 2, 3, 1).contiguous()
    S = F.conv2d(x.abs(), w.abs(), b.abs(), stride=2, padding=3).permute(0, 2, 3, 1).contiguous()
    return ref, R(49 * w.shape[1] + C_CONV0) * S


def packed_rows(w):
    """conv0 weight [N, Cpix, 7, 7] as k_pack lays it out (elementwise.hip:383-414): one row per output channel, k = tap * Cpix + c, padded
    with zeros to Kp = round_up(49 Cpix, 32).  -> [N, Kp]."""
    N, C = w.shape[:2]
    Kp = -(-49 * C // 32) * 32
    rows = torch.zeros(N, Kp, dtype=w.dtype)
    rows[:, :49 * C] = w.permute(0, 2, 3, 1).reshape(N, 49 * C)
    return rows


def tap3_weights(w):
    """The weights a kernel contracts with when it reads the packed rows as k = tap * 3 + c: w'[n][c][tap] = flat[n Kp + tap * 3 + c].  At
    Cpix = 3 the weights themselves; below, every tap but the first takes another tap's weights and the last taps run on into the row's
    padding and the next row (zero past the last row).  -> [N, Cpix, 7, 7]."""
    N, C = w.shape[:2]
    rows = packed_rows(w)
    flat = torch.cat([rows.flatten(), torch.zeros(147, dtype=w.dtype)])
    idx = (torch.arange(N)[:, None, None] * rows.shape[1] + torch.arange(49)[None, None, :] * 3 + torch.arange(C)[None, :, None])
    return flat[idx].reshape(N, C, 7, 7)


def tap3_wgrad(dW):
    """The weight gradient a kernel leaves when it stores its [tap * 3 + c] table into the packed row as it stands (slot k of the row takes
    table entry k): read back as k = tap * Cpix + c, dW'[n][c][tap] = dW[n][k % 3][k // 3] where k % 3 < Cpix, else 0.  At Cpix = 3 dW itself."""
    N, C = dW.shape[:2]
    k = torch.arange(49)[None, :] * C + torch.arange(C)[:, None]                        # [C, 49]
    tab = torch.zeros(N, 3, 49, dtype=dW.dtype)
    tab[:, :min(C, 3)] = dW.reshape(N, C, 49)[:, :3]
    return tab[:, k % 3, k // 3].reshape(N, C, 7, 7)


def conv0_from_hits(coords, values, n, H, W, mode, w, b, rnd):
    """The same map from the de-duplicated records, as the sparse kernels evaluate it (stem_sparse.hip:344-348 conv0_at): bias plus, per
    owner hit (y, x) and tap (ky, kx) with y + 3 - ky and x + 3 - kx even, v . w[:, :, ky, kx] at position ((y + 3 - ky) / 2,
    (x + 3 - kx) / 2).  Records hold bf16 values (HitRec::pack, stem_sparse.hip:46-49), so this is the bf16-mode map whatever `rnd` says about the
    weights.  Equal to conv0(image(...)) up to float64 summation order (test_stem_reference_cpu.py).  -> ref, delta."""
    idx, pix = owners(coords, n, H, W)
    val, _ = pixel_values(values[idx], mode, rnd)
    w = bf16(w) if rnd else w
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    N = w.shape[0]
    ref = b.expand(n * Hc * Wc, N).clone()
    S = b.abs().expand(n * Hc * Wc, N).clone()
    im, y, x = pix // (H * W), (pix // W) % H, pix % W
    for ky in range(7):
        for kx in range(7):
            ty, tx = y + 3 - ky, x + 3 - kx
            ok = (ty % 2 == 0) & (tx % 2 == 0) & (ty >= 0) & (tx >= 0) & (ty // 2 < Hc) & (tx // 2 < Wc)
            pos = ((im * Hc + ty // 2) * Wc + tx // 2)[ok]
            ref.index_add_(0, pos, val[ok] @ w[:, :, ky, kx].T)
            S.index_add_(0, pos, val[ok].abs() @ w[:, :, ky, kx].abs().T)
    return ref.reshape(n, Hc, Wc, N), (R(49 * w.shape[1] + C_CONV0) * S).reshape(n, Hc, Wc, N)


def bias_exact(c0_stored, act, b, rnd):
    """Number of positions no hit reaches (act false) whose stored row is NOT the stored-precision bias bit for bit."""
    row = bf16(b) if rnd else b
    return int(((c0_stored != row) & ~act[..., None]).any(-1).sum())


# ---------------------------------------------------------------------------------------------------------------------
# pooled output of the sparse stem, BatchNorm0 statistics of the sparse train pass
# ---------------------------------------------------------------------------------------------------------------------
def _pool3(t, defect=None):
    """AvgPool 3 / 2 without padding over NHWC.  defect "shift": every window starts one row lower (the last one wraps to the first)."""
    x = t.permute(0, 3, 1, 2)
    if defect == "shift":
        x = torch.roll(x, -1, 2)
    return F.avg_pool2d(x, 3, 2).permute(0, 2, 3, 1).contiguous()


def sparse_pool(c0, d0, sc, sh, sl, defect=None):
    """BN0 table + PReLU0 + AvgPool 3 / 2 of a conv0 map that stays fp32 on chip (k_stem_sparse_pool, stem_sparse.hip:438-446; the constant
    vector of an all-empty window makes the same nine additions, :404-407): c0 = the float64 map, d0 its allowed error (conv0_from_hits).
    f = prelu(fma(c0, sc, sh)): PReLU is continuous with slopes 1 and sl, so the conv0 error passes through |sc| max(1, |sl|) and no
    element is excluded; one fma and the slope multiply add R(2) |f|; nine additions from 0 and * fl(1 / 9) (two roundings: the constant,
    the product): delta = (1 + R(11)) mean9(|sc| max(1, |sl|) d0) + R(2 + 9 + 2) mean9 |f|.  -> ref, delta (bf16 store on top)."""
    f = L._prelu(c0 * sc + sh, sl)
    e = sc.abs() * torch.maximum(torch.ones_like(sl), sl.abs()) * d0
    return _pool3(f, defect), (1 + R(11)) * _pool3(e) + R(2 + 9 + 2) * _pool3(f.abs())


def sparse_stats(c0, d0):
    """raw:bstat0 of the sparse train pass (k_stem_sparse_stats, stem_sparse.hip:352-386): per channel the mean and E[x^2] = var + mean^2
    (never the variance alone: cancellation) of the fp32 on-chip conv0 values, every value widened to double before it is added.  Gate of
    a double accumulator as test_batchnorm_stats_gpu.py derives it (1e-9 s on the mean, 1e-9 s^2 on E2, s = sqrt(E2)) plus the conv0
    error itself: mean d0 on the mean, mean (2 |x| d0 + d0^2) on E2.  -> (mean, gate), (E2, gate)."""
    x, d = c0.reshape(-1, c0.shape[-1]), d0.reshape(-1, c0.shape[-1])
    mean, e2 = x.mean(0), (x * x).mean(0)
    return (mean, 1e-9 * e2.sqrt() + d.mean(0)), (e2, 1e-9 * e2 + (2 * x.abs() * d + d * d).mean(0))


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def pool_backward(G, X, P, Q, Hc, Wc, defect=None):
    """dz over the conv0 map from what reaches the pooled map: eff1 = G + P X + Q per pooled pixel (three fp32 roundings of a value no
    larger than |G| + |P X| + |Q|: stem.hip:76, :262; stem_sparse.hip:490), dz[p] = fl(1 / 9) * sum of eff1 over the <= 4 windows (rows
    2q .. 2q + 2) that hold p: at most three additions (stem.hip:302-303; four from 0 in the flat kernel, :76, and in the sparse one,
    stem_sparse.hip:505) and two roundings for * fl(1 / 9) (:82, :304; stem_sparse.hip:508):
        ddz = R(3 + 4 + 2) * 1/9 sum (|G| + |P X| + |Q|).
    A position no window covers -- the last row / column of an even extent -- has dz = 0 exactly and ddz = 0.
    G, X [n, Ho, Wo, C] (raw:grad1 / dense1, first C channels), P, Q [C].
    defects: "shift" (windows one row lower), "leak" (the uncovered last row takes the row above), "eighth" (1/8 instead of 1/9 on the
    windows at the map's border).  -> dz, ddz [n, Hc, Wc, C]."""
    n, Ho, Wo, C = G.shape
    e = G + P * X + Q
    a = G.abs() + (P * X).abs() + Q.abs()
    if defect == "eighth":
        border = torch.zeros(Ho, Wo, dtype=torch.bool)
        border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
        e = torch.where(border[None, :, :, None], e * 9.0 / 8.0, e)
    ones = torch.full((C, 1, 3, 3), 1.0 / 9.0, dtype=torch.float64)
    spread = lambda t: F.conv_transpose2d(t.permute(0, 3, 1, 2), ones, stride=2, groups=C).permute(0, 2, 3, 1)
    dz, ddz = torch.zeros(n, Hc, Wc, C, dtype=torch.float64), torch.zeros(n, Hc, Wc, C, dtype=torch.float64)
    off = 1 if defect == "shift" else 0
    h, w = min(2 * Ho + 1, Hc - off), 2 * Wo + 1
    dz[:, off:off + h, :w], ddz[:, off:off + h, :w] = spread(e)[:, :h], R(3 + 4 + 2) * spread(a)[:, :h]
    if defect == "leak":
        assert Hc == 2 * Ho + 2
        dz[:, -1] = dz[:, -2]
    return dz, ddz


def uncovered(Hc, Wc):
    """[Hc, Wc] bool: conv0 positions that lie in no 3 / 2 pooling window."""
    Ho, Wo = (Hc - 3) // 2 + 1, (Wc - 3) // 2 + 1
    m = torch.zeros(Hc, Wc, dtype=torch.bool)
    m[2 * Ho + 1:], m[:, 2 * Wo + 1:] = True, True
    return m


def stem_sums(dz, ddz, x, dx, sc, sh, sl):
    """The three sums the pooling backward leaves for BatchNorm0 -- s1 = sum dU, t2 = sum dU x, s3 = sum dz min(u, 0), dU = prelu'(u) dz,
    u = fma(x, sc, sh) -- over ALL conv0 positions (stem.hip:304-308; the sparse pass takes the hit-free positions in through the identity
    sum_p dz = sum_q eff, in double, stem_sparse.hip:562-568).  x: the conv0 map the kernel read, dx its uncertainty (0: the stored map;
    the sparse kernels rebuild it on chip: conv0_from_hits' delta).
    dx = 0: densenet_layer_reference.bn_sums as it stands.  dx > 0, on top of it: u is off by |sc| dx more, so the kink set grows to
    |u| <= R(2) (|sc x| + |sh|) + |sc| dx and each of its new members adds the difference between the two branches to the gates; t2 takes
    |dU| dx and s3 |dz| |sc| dx per element.  -> dU, ddU, kink, (s1, t2, s3), (gate1, gate2, gate3)."""
    dU, ddU, kink, sums, gates = L.bn_sums(dz, ddz, x, sc, sh, sl)
    if dx is None:
        return dU, ddU, kink, sums, gates
    C = x.shape[-1]
    u = x * sc + sh
    wide = (u.abs() <= R(2) * ((x * sc).abs() + sh.abs()) + sc.abs() * dx) & ~kink
    jump = torch.where(wide, (dz * (1 - sl)).abs(), torch.zeros_like(dz))
    flat = lambda t: t.reshape(-1, C).sum(0)
    gates = (gates[0] + flat(jump), gates[1] + flat(jump * (x.abs() + dx) + (dU.abs() + ddU) * dx), gates[2] + flat((dz.abs() + ddz) * sc.abs() * dx))
    return dU, ddU, kink | wide, sums, gates


def conv0_wgrad(e, de, img, terms, c=516, defect_img=None, bias_terms=None):
    """dW0[n][c][ky][kx] = sum over positions of eff0[pos][n] img[2 oy - 3 + ky][2 ox - 3 + kx][c] and db0[n] = sum eff0[pos][n]:
    e, de [n, Hc, Wc, N] the eff0 rows as the kernel holds them and their uncertainty, img the dense map [n, H, W, Cpix] with each listed
    pixel ONCE (image()).  The hit-list kernel (stem.hip:118-197) walks the owner entries -- fma chains per wave, at most one term per
    entry, then <= 3 LDS additions, the slab reduction over its 512 workgroups and the addition into the zeroed gradient -- and the
    generic kernel sums all positions with fp32 atomics; zero pixels contribute exact zeros, so a sum passes at most `terms` + c
    roundings, terms = the number of summands that can be nonzero (the caller's count), c = 3 + 512 + 1:
        delta = R(terms + c) (S + F) + F,  S = sum |eff0| |img|,  F = sum de |img|.
    defect_img: the map a wrong kernel would contract with (a duplicate counted twice: the sum of ALL listed entries).
    bias_terms = (f, tau): the generic kernel sums the fp32 eff0 rows in front of their bf16 rounding (conv_bwd.hip:375), cf.
    densenet_layer_reference.conv3x3_wgrad.
    -> (dW0 [N, Cpix, 7, 7], delta), (db0 [N], delta with S = sum |eff0|, F = sum de, `terms` = all positions)."""
    N, Cp = e.shape[-1], img.shape[-1]
    shape = (N, Cp, 7, 7)
    g = lambda t: t.permute(0, 3, 1, 2).contiguous()
    wg = lambda a, b: torch.nn.grad.conv2d_weight(g(a), shape, g(b), stride=2, padding=3)
    dW = wg(img if defect_img is None else defect_img, e)
    S, Fm = wg(img.abs(), e.abs()), wg(img.abs(), de)
    M = e.numel() // N
    ef, df = (t.reshape(M, N) for t in (bias_terms if bias_terms is not None else (e, de)))
    return (dW, R(terms + c) * (S + Fm) + Fm), (ef.sum(0), R(M + c) * (ef.abs().sum(0) + df.sum(0)) + df.sum(0))


def stem_backward(G, X, P, Q, c0, dc0, tab, sl, gamma, stats, img, du0=None, pq0=None, rnd=False, rnd_eff=False, terms=None, c=516, defect=None):
    """The stem's whole backward from what stays after a full backward pass:
      G, X, P, Q     raw:grad1[..., :C], dense1[..., :C], the rows of raw:pq1          -> eff1, dz (pool_backward)
      c0, dc0        the conv0 map the kernels read and its uncertainty (None: the stored map)
      tab, sl        BatchNorm0's (sc, sh) out of raw:tabs, PReLU0's slope              -> dU, the three sums (stem_sums)
      gamma, stats   norm0.weight, (mean, var) out of raw:bstat0                          -> dgamma0, dbeta0, dslope0, (P0, Q0) (bn_link)
      DU0 = sc dU: one more rounding on top of the slope multiply (stem.hip:309; prelu_bn_backward's gate)
      eff0 = DU0 + P0 c0 + Q0 (eff_rows; fma(sc, dU, fma(P0, x, Q0)) in the sparse pass, stem_sparse.hip:596: fewer roundings)
      dW0, db0 (conv0_wgrad) from the STORED du0 [n, Hc, Wc, C] and pq0 [2 C] where they are given (NaN rows of du0 -- never stored, no
      hit reaches them -- multiply zero pixels only and are taken as 0), so that one kernel's error is not charged to the next; without them
      (sparse pass) from the chain, whose per-element error |sc| ddU + |P0| dc0 goes into F.  rnd_eff: the generic bf16 kernel rounds the
      eff0 rows to bf16 before it multiplies them (conv_bwd.hip:373).  terms, c: see conv0_wgrad (default: all positions; the sparse pass
      reduces the slabs of up to 1024 workgroups: c = 1025).
    -> {name: (ref, delta[, kink])} for du0, dgamma, dbeta, dslope, P0, Q0, dW0, db0, and db0_zero: the hit-list path leaves the conv0 bias
    gradient at its exact value 0 (BatchNorm0 follows), gated around zero by R(M) sum |eff0|."""
    sc, sh = tab
    n, Hc, Wc, C = c0.shape
    M = n * Hc * Wc
    dz, ddz = pool_backward(G, X, P, Q, Hc, Wc, defect)
    dU, ddU, kink, sums, gates = stem_sums(dz, ddz, c0, dc0, sc, sh, sl)
    assert int(kink.sum()) <= L.KINK_CAP * kink.numel(), (int(kink.sum()), kink.numel())
    out = {"du0": (sc * dU, sc.abs() * ddU + R(1) * (sc * dU).abs(), kink)}
    lk = L.bn_link(sums, gates, stats[0], stats[1], gamma, M)
    out.update(dgamma=lk["dgamma"], dbeta=lk["dbeta"], dslope=lk["dslope"], P0=lk["P"], Q0=lk["Q"])
    if du0 is not None:
        DU, dDU = torch.where(torch.isnan(du0), torch.zeros_like(du0), du0), torch.zeros_like(du0)
    else:                                                                  # (an element at a kink may have taken either branch)
        DU, dDU = out["du0"][0], out["du0"][1] + torch.where(kink, (sc * dz * (1 - sl)).abs(), torch.zeros_like(dz))
    P0, Q0 = (pq0[:C], pq0[C:]) if pq0 is not None else (lk["P"][0], lk["Q"][0])
    f, tau, e, de = L.eff_rows(DU, c0, P0, Q0, None, rnd_eff)
    de = de + dDU + (P0.abs() * dc0 if dc0 is not None else 0)
    out["dW0"], out["db0"] = conv0_wgrad(e, de, img, M if terms is None else terms, c=c, bias_terms=(f, tau) if rnd_eff else None)
    out["db0_zero"] = (torch.zeros(C, dtype=torch.float64), R(M) * f.abs().reshape(M, C).sum(0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# hit lists of the test cases (shared by the GPU test and the CPU test of the gates)
# ---------------------------------------------------------------------------------------------------------------------
CASE_SHAPES = {"partial": ((104, 72), 3), "odd": ((45, 37), 3), "dense-band": ((40, 280), 2), "many": ((104, 72), 150),
               "many-tiny": ((12, 16), 1030), "wide-limit": ((24, 384), 2)}


def case_hits(name, seed=7, cpix=3):
    """-> coords int32 [nnz, 3], values fp32 [nnz, cpix] (integers 1 .. 255; the coordinates do not depend on cpix), n_img, (H, W).
    partial: all four corners, both borders, one EMPTY map, entries outside the maps (image -1, image n, y == H, x == W) and 40 pixels
    listed twice with different values, everything shuffled.  dense-band: every pixel of rows 8 .. 31, columns 100 .. 219 of map 0.
    many / many-tiny: 5 .. 40 / 1 .. 6 hits per map.  wide-limit: the sparse stem's widest map, hits in the first and last column."""
    import numpy as np
    (H, W), n = CASE_SHAPES[name]
    rng = np.random.default_rng(seed)
    rand = lambda k: [(int(f) // W, int(f) % W) for f in rng.choice(H * W, size=k, replace=False)]
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    if name == "partial":
        border = [(0, x) for x in range(0, W, 5)] + [(H - 1, x) for x in range(2, W, 7)] + [(y, 0) for y in range(0, H, 9)] + [(y, W - 1) for y in range(4, H, 6)]
        per = [sorted(set(corners + border + rand(60))), [], rand(80)]
    elif name == "odd":
        per = [sorted(set(corners + rand(50))), rand(30), rand(60)]
    elif name == "dense-band":
        per = [[(y, x) for y in range(8, 32) for x in range(100, 220)], rand(50)]
    elif name == "many":
        per = [rand(int(rng.integers(5, 41))) for _ in range(n)]
    elif name == "many-tiny":
        per = [rand(int(rng.integers(1, 7))) for _ in range(n)]
    else:
        per = [sorted(set(corners + [(y, W - 1) for y in range(2, H, 5)] + rand(100))), rand(100)]
    coords = np.array([(i, y, x) for i, p in enumerate(per) for y, x in p], dtype=np.int64).reshape(-1, 3)
    if name == "partial":
        dup = rng.choice(len(coords), size=40, replace=False)
        outside = np.array([(-1, 5, 5), (n, 0, 0), (0, H, 3), (2, 4, W), (0, -1, 2), (2, 7, -1)])
        coords = np.concatenate([coords, coords[dup], outside])
        coords = coords[rng.permutation(len(coords))]
    values = rng.integers(1, 256, size=(len(coords), cpix)).astype(np.float32)
    return torch.from_numpy(coords.astype(np.int32)), torch.from_numpy(values), n, (H, W)
