"""Float64 reference of the DenseNet embedder's forward and backward operations behind the stem (the stem itself -- hit list -> map, conv0,
the sparse pooled output, the stem's backward with its taps raw:du0 / raw:pq0 -- is stem_reference.py, built on this module's formats and
gate rules; pool0 below starts from the conv0 map that module checks), one plain function per operation,
each with the |error| a correct kernel may show per element.  No GPU: the functions take an operation's ACTUAL inputs (the maps the engine stored, its
(scale, shift) tables, the bound fp32 parameters) as float64 NHWC tensors, so nothing drifts between the two sides.  `rnd` switches the
bf16 roundings on (bf16 mode) or off (fp32 mode; with float64 inputs and the gates ignored it is the exact network, which
test_densenet_layer_reference_cpu.py pins against the oracle).

Gates (derived, u = 2^-24, R(n) = (1 + u)^n - 1 the compound of n fp32 roundings):
  * Operand the kernel computes itself, f = prelu(sc x + sh): one fma, one multiply by the slope (tile3x3.h:118 act8_apply,
    fwd1x1_fused.hip:144, elementwise.hip:258 k_act_bf16, conv_tile.h:111 act8) -> tau = R(2) |f|; rounding never changes a sign, so the
    fp32 evaluation takes the branch of the exact one.  Pooled operand (2x2 floor windows, elementwise.hip:326 / conv_tile.h:133-136):
    four such terms, four fp32 additions from 0, an exact * 0.25 -> tau = R(6) * 1/4 sum |f_k|.
    bf16 mode: the kernel's rounded operand is bf16(f - tau) or bf16(f + tau); where they differ the operand is uncertain by their
    difference da (one bf16 ulp), else da = 0.  fp32 mode: da = tau.
  * Convolution = fp32 fma chain over K products (the MFMA is one, k ascending; any order obeys the same bound) plus c further fp32
    operations: delta = R(K + c) (S + F) + F with S = sum |a_k| |w_k| + |bias| and F = sum da_k |w_k| (one more convolution with |w|).
      c = 1 for the 1x1 kernels: the bias add (fwd1x1_fused.hip:184, gemm_nt.hip:220, conv1x1_f32.hip:395, conv_fwd.hip:97-105);
      c = 3 for the 3x3 kernels: the pair kernel adds its two waves' partial chains and the bias (conv3x3_fwd_tile.hip:318) and
          multiplies by the dropout keep scale (:322); the single-wave kernels (:143-146, conv3x3_f32.hip:276-277) do less;
      c = 1 for the output Linear (rows.hip:36-43: one fma chain, alpha * acc + 0).
    Eval mode, norm2 + PReLU2 in the 1x1 epilogue (fwd1x1_fused.hip:185, gemm_nt.hip:221): delta' = max(1, |sl|) |sc| delta + R(2) |f|.
  * pool0 (elementwise.hip:180-186, :442-447): nine terms, nine additions, * fl(1/9): delta = R(2 + 9 + 2) * 1/9 sum |f_k|.
    Head pooling (elementwise.hip:214-215): HW terms and additions, one division: delta = R(2 + HW + 1) * 1/HW sum |f_k|.
  * Store: |hip - ref| <= delta + 1/2 ulp(|ref| + delta), the ulp of bf16 (bf16 mode maps) or fp32.
  * Stored operand (xa, ya): checked itself with delta = tau and the store rule, then used as the exact operand (da = 0).
  * Backward (3x3 data gradient, 3x3 weight and bias gradient, transition data gradient, head pooling): eff_rows, conv3x3_dgrad,
    prelu_bn_backward, conv3x3_wgrad, transition_dgrad, head_pool_backward, bn_sums, bn_link, conv1x1_backward, transition_backward and
    head_backward below carry their derivations; the elements
    at a PReLU kink (|u| within the fp32 evaluation error of 0, where prelu' may take either branch) are the only ones ever left out of
    a comparison, at most KINK_CAP of a tensor.
  * Frozen backward (hit gradients: running statistics, P = Q = PY = QY = 0, no dropout): output_block_backward_frozen
    (k_rows_bn_bwd_frozen + the Linear's data gradient), frozen_block_slices (the final accumulator of a block as the end of its chain
    of read-add-writes), hit_gradient_check (k_hit_gradient from the stored DU0) and the unrounded chain run_backward_frozen carry theirs.
No other element is excluded and no gate carries a fitted factor."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 1e-5
C_1X1, C_3X3, C_LINEAR = 1, 3, 1
KINK_CAP = 1e-3        # largest share of a tensor that may sit at a PReLU kink


def R(n):
    return (1.0 + U) ** n - 1.0


# ---------------------------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------------------------
def _rne(x, drop):
    """float64 -> the nearest value with `drop` fewer mantissa bits, ties to even (one rounding: never through float32 first)."""
    i = x.contiguous().view(torch.int64)
    i = (i + ((1 << (drop - 1)) - 1) + ((i >> drop) & 1)) & ~((1 << drop) - 1)
    return i.view(torch.float64)


def bf16(x):
    return _rne(x, 45)


def f32(x):
    return _rne(x, 29)


def ulp(x, p):
    """Spacing of the p-bit floating-point numbers at |x| (p = 8: bf16, 24: fp32); 0 at 0."""
    _, e = torch.frexp(x.abs())
    return torch.where(x != 0, torch.ldexp(torch.ones_like(x), e - p), torch.zeros_like(x))


def store_gate(ref, delta, rnd):
    return delta + 0.5 * ulp(ref.abs() + delta, 8 if rnd else 24)


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def _prelu(u, sl):
    return torch.where(u > 0, u, sl * u)


def _operand(f, tau, rnd):
    if not rnd:
        return f, tau
    return bf16(f), (bf16(f + tau) - bf16(f - tau)).abs()


def activation(x, sc, sh, sl, rnd):
    """-> f (exact), tau, the operand a as the kernel rounds it, its uncertainty da."""
    f = _prelu(x * sc + sh, sl)
    tau = R(2) * f.abs()
    return (f, tau) + _operand(f, tau, rnd)


def _pool2(t, edge_defect=False):
    """2x2 average over the windows that fit into t [n, H, W, C] (floor).  edge_defect: the last window of an odd extent also takes the
    remainder row / column in, as a ceil-mode window would."""
    if not edge_defect:
        return F.avg_pool2d(t.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    n, H, W, C = t.shape
    rows = [(2 * i, H if i == H // 2 - 1 else 2 * i + 2) for i in range(H // 2)]
    cols = [(2 * j, W if j == W // 2 - 1 else 2 * j + 2) for j in range(W // 2)]
    return torch.stack([torch.stack([t[:, r0:r1, c0:c1].mean((1, 2)) for c0, c1 in cols], 1) for r0, r1 in rows], 1)


def pooled_activation(x, sc, sh, sl, rnd, edge_defect=False):
    """2x2 average of prelu(sc x + sh); pixels of an odd edge that no window covers do not count."""
    f = _prelu(x * sc + sh, sl)
    p, s = _pool2(f, edge_defect), _pool2(f.abs(), edge_defect)
    tau = R(6) * s
    return (p, tau) + _operand(p, tau, rnd)


# ---------------------------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------------------------
def _weights(w, rnd):
    return bf16(w) if rnd else w


def conv1x1(a, da, w, bias, rnd):
    """a, da [..., K]; w [N, K] (the bound fp32 tensor; rounded here); -> ref (unrounded), delta."""
    w = _weights(w, rnd)
    K = a.shape[-1]
    ref = a @ w.T + bias
    S = a.abs() @ w.abs().T + bias.abs()
    Fm = da @ w.abs().T
    return ref, R(K + C_1X1) * (S + Fm) + Fm


def act_epilogue(v, dv, sc, sh, sl):
    """norm2 + PReLU2 applied to the fp32 1x1 result in the epilogue (eval mode)."""
    f = _prelu(v * sc + sh, sl)
    return f, torch.maximum(torch.ones_like(sl), sl.abs()) * sc.abs() * dv + R(2) * f.abs()


def padded_tail_mask(n, H, W, tile=128):
    """[n, H, W] bool: pixels whose position in the zero-padded map [n, H + 2, W + 2] lies in the last, partial tile."""
    pp = n * (H + 2) * (W + 2)
    i, h, w = torch.meshgrid(torch.arange(n), torch.arange(H), torch.arange(W), indexing="ij")
    return ((i * (H + 2) + h + 1) * (W + 2) + w + 1) >= (pp // tile) * tile if pp % tile else torch.zeros(n, H, W, dtype=torch.bool)


def _taps(a, defect=None):
    """The nine shifted copies of a [n, H, W, C] (zero outside the image), tap = 3 (dy + 1) + dx + 1, by flat position index as the
    padded-tile kernels address them.  defect "row_leak": the dx = +1 tap is not zeroed at the last column and reads the next row's first
    pixel; "image_leak": the same at an image's last pixel only, which reads the next image's first."""
    n, H, W, C = a.shape
    flat = torch.cat([a.reshape(-1, C), torch.zeros(1, C, dtype=a.dtype)])
    i, h, w = torch.meshgrid(torch.arange(n), torch.arange(H), torch.arange(W), indexing="ij")
    out = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vert = (h + dy >= 0) & (h + dy < H)
            ok = vert & (w + dx >= 0) & (w + dx < W)
            local = (h + dy) * W + w + dx
            if dx == 1 and defect == "row_leak":
                ok = vert & (local < H * W)
            if dx == 1 and defect == "image_leak":
                ok = ok | (vert & (local == H * W) & (i < n - 1))
            if dx == -1 and defect == "row_leak_back":                    # the same two leaks in the data gradient's mirrored taps
                ok = vert & (local >= 0)
            if dx == -1 and defect == "image_leak_back":
                ok = ok | (vert & (local == -1) & (i > 0))
            idx = torch.where(ok, i * H * W + local, torch.full_like(i, n * H * W))
            out.append(flat[idx.reshape(-1)].reshape(n, H, W, C))
    return out


def conv3x3(a, da, w, bias, keep, rnd, defect=None):
    """a, da [n, H, W, K]; w [N, K, 3, 3]; keep [n, H, W, N] dropout keep scale (0 or 1 / (1 - p)) or None -> ref, delta.
    defect "stale_tail": the pixels of the last partial 128-position tile of the padded map take the weights of the tap before."""
    w = _weights(w, rnd)
    n, H, W, K = a.shape
    wt = [w[:, :, t // 3, t % 3] for t in range(9)]
    ref = sum(x @ wk.T for x, wk in zip(_taps(a, defect), wt)) + bias
    if defect == "stale_tail":
        tail = padded_tail_mask(n, H, W)
        assert tail.any()
        stale = sum(x @ wt[(t - 1) % 9].T for t, x in enumerate(_taps(a))) + bias
        ref = torch.where(tail[..., None], stale, ref)
    S = sum(x @ wk.abs().T for x, wk in zip(_taps(a.abs()), wt)) + bias.abs()
    Fm = sum(x @ wk.abs().T for x, wk in zip(_taps(da), wt))
    delta = R(9 * K + C_3X3) * (S + Fm) + Fm
    if keep is not None:
        ref, delta = ref * keep, delta * keep
    return ref, delta


# ---------------------------------------------------------------------------------------------------------------------
# pooling and the head
# ---------------------------------------------------------------------------------------------------------------------
def pool0(c0, sc, sh, sl):
    """BN0 + PReLU0 + AvgPool(3, stride 2, no padding) of the conv0 map."""
    f = _prelu(c0 * sc + sh, sl).permute(0, 3, 1, 2)
    pool = lambda t: F.avg_pool2d(t, 3, 2).permute(0, 2, 3, 1).contiguous()
    return pool(f), R(2 + 9 + 2) * pool(f.abs())


def head_pool(x, sc, sh, sl):
    """final_norm + PReLU + global mean -> [n, C]."""
    f = _prelu(x * sc + sh, sl)
    hw = x.shape[1] * x.shape[2]
    return f.mean((1, 2)), R(2 + hw + 1) * f.abs().mean((1, 2))


def linear(x, w):
    """Output Linear without bias, fp32 in both modes: x [n, K] fp32 values, w [N, K] the bound fp32 tensor."""
    return x @ w.T, R(x.shape[-1] + C_LINEAR) * (x.abs() @ w.abs().T)


# ---------------------------------------------------------------------------------------------------------------------
# backward: the 3x3 data gradient of a dense layer
# ---------------------------------------------------------------------------------------------------------------------
def eff_rows(G, X, P, Q, keep, rnd):
    """Effective gradient of a layer's output slice, eff = keep (G + P X + Q) (tcvn_ops.h:118-121): fma(P, x, g) + Q, times the keep scale
    (tcvn_common.h:59 eff3; conv3x3_dgrad_tile.hip:80-83, :260-263, :433-436) -- three fp32 roundings, four where the product is rounded on
    its own (conv_bwd.hip:30-31, conv3x3_f32.hip:112-113), each of a value no larger than |g| + |P x| + |Q| (times the scale):
    tau = R(4) keep (|g| + |P x| + |Q|).  -> f, tau, operand, its uncertainty."""
    k = keep if keep is not None else torch.ones_like(G)
    f = (G + P * X + Q) * k
    tau = R(4) * k * (G.abs() + (P * X).abs() + Q.abs())
    return (f, tau) + _operand(f, tau, rnd)


def conv3x3_dgrad(e, de, w, rnd, defect=None):
    """dA[m][c] = sum_tap sum_n eff[m - shift(tap)][n] w[n][c][tap]: e, de [n, H, W, g]; w [g, C, 3, 3] the FORWARD weight (rounded here).
    One fma chain over 9 g products, nothing else (conv3x3_dgrad_tile.hip:96-107, :491-502): delta = R(9 g) (S + F) + F."""
    w = _weights(w, rnd)
    wt = [w[:, :, t // 3, t % 3] for t in range(9)]
    mirror = {"row_leak": "row_leak_back", "image_leak": "image_leak_back"}.get(defect)
    conv = lambda x, ws, d=None: sum(xs @ wk for xs, wk in zip(reversed(_taps(x, d)), ws))       # position m - shift(t) = tap 8 - t
    ref = conv(e, wt, mirror)
    S, Fm = conv(e.abs(), [k.abs() for k in wt]), conv(de, [k.abs() for k in wt])
    return ref, R(9 * e.shape[-1]) * (S + Fm) + Fm


def prelu_bn_backward(dA, ddA, y, sc, sh, sl, no_scale=False):
    """DU = sc dA prelu'(u), u = sc y + sh (conv3x3_dgrad_tile.hip:134-137, :523-527): the slope multiply and the scale multiply are two more
    roundings; the branch is that of the fp32 u -- a fused multiply-add keeps the sign of the exact u, a separate multiply and add is off by
    at most tau_u = R(2) (|sc y| + |sh|): elements with |u| <= tau_u form the kink set.  no_scale: the DEFECT of a missing sc.
    -> DU, delta, kink."""
    u = y * sc + sh
    kink = u.abs() <= R(2) * ((y * sc).abs() + sh.abs())
    du = torch.where(u > 0, dA, sl * dA)
    DU = du if no_scale else sc * du
    return DU, sc.abs() * torch.maximum(torch.ones_like(sl), sl.abs()) * ddA + R(2) * DU.abs(), kink


def transition_dgrad(Gn, Xn, Pn, Qn, x, sc, sh, sl, w, rnd, ch0, defect=None):
    """Data gradient of a transition for the channels [ch0, C) of its input block: the FIRST writer of that block's accumulator, so the
    reference is the contribution alone, and exactly zero at the pixels of an odd edge that no 2x2 window covers.
    Gn, Xn, Pn, Qn: accumulator, concat buffer and (P, Q) rows of the NEXT block, whose first Nt channels the transition produced (no
    dropout); x [n, H, W, C] the input block's concat buffer; (sc, sh, sl) the transition norm + PReLU; w [Nt, C] the bound 1x1 weight.
    dA = 1/4 sum_k eff[mo][k] w[k][c] at the four pixels of window mo (one chain of Nt products; * 0.25 is exact), then the slope and scale
    multiplies (gemm_nt.hip:196-200, conv_bwd.hip:257-270; the accumulate of the generic kernel adds to a zeroed buffer: exact).
    defect "spill": the remainder pixels take their neighbour's value.  -> DU [n, H, W, C - ch0], delta, kink."""
    Nt = w.shape[0]
    _, _, e, de = eff_rows(Gn[..., :Nt], Xn[..., :Nt], Pn[:Nt], Qn[:Nt], None, rnd)
    wk = _weights(w, rnd)[:, ch0:]
    dAp, S, Fm = e @ wk, e.abs() @ wk.abs(), de @ wk.abs()
    ddAp = R(Nt) * (S + Fm) + Fm
    n, H, W, _ = x.shape
    Hn, Wn = e.shape[1:3]
    assert (Hn, Wn) == (H // 2, W // 2)

    def up(t, spill=False):
        out = torch.zeros(n, H, W, t.shape[-1], dtype=t.dtype)
        out[:, :2 * Hn, :2 * Wn] = 0.25 * t.repeat_interleave(2, 1).repeat_interleave(2, 2)
        if spill:
            out[:, 2 * Hn:] = out[:, 2 * Hn - 1:2 * Hn]
            out[:, :, 2 * Wn:] = out[:, :, 2 * Wn - 1:2 * Wn]
        return out
    return prelu_bn_backward(up(dAp, defect == "spill"), up(ddAp), x[..., ch0:], sc[ch0:], sh[ch0:], sl[ch0:])


def head_pool_backward(dF, x, sc, sh, sl, ch0):
    """Head pooling backward for the channels [ch0, C) of the last block, its accumulator's first writer: G = sc prelu'(u) dF / HW per pixel
    (elementwise_bwd.hip:20-34: fl(1 / HW), dF * that, the slope multiply, the scale multiply -- four roundings).  dF [n, C]; x [n, H, W, C].
    -> G [n, H, W, C - ch0], delta, kink."""
    n, H, W, _ = x.shape
    dz = (dF[:, ch0:] / (H * W))[:, None, None, :].expand(n, H, W, -1)
    u = x[..., ch0:] * sc[ch0:] + sh[ch0:]
    kink = u.abs() <= R(2) * ((x[..., ch0:] * sc[ch0:]).abs() + sh[ch0:].abs())
    Gr = sc[ch0:] * torch.where(u > 0, dz, sl[ch0:] * dz)
    return Gr, R(4) * Gr.abs(), kink


def conv3x3_wgrad(e, de, a, da, rnd, defect=None, bias_terms=None):
    """dW[n][c][tap] = sum_m eff[m][n] a[m + shift(tap)][c], db[n] = sum_m eff[m][n]: e, de [n, H, W, g] the eff rows, a, da [n, H, W, C] the
    activated 3x3 input (both as the kernel rounds them, with their uncertainties).  fp32 sums of M = n H W products in some order -- per
    workgroup an MFMA chain over its tiles, then the slab reduction (conv3x3_wgrad_tile.hip:453-469, :476-482, :539-540; generic kernels:
    fp32 atomics) -- and one more addition into the zeroed gradient.  Padding rows contribute exact zeros, so a sum passes at most M
    roundings whatever the order: delta = R(M + 1) (S + F) + F, F = sum de |a| + |e| da + de da.  Both results are fp32.
    The bias gradient sums the eff rows AS ROUNDED in the tile kernel (conv3x3_wgrad_tile.hip:155-156) but the fp32 values in front of
    their bf16 store in the generic kernel (conv_bwd.hip:373-375): for that kernel pass bias_terms = (f, tau), the exact rows and their
    fp32 evaluation error.
    -> (dW [g, C, 3, 3], delta), (db [g], delta)."""
    g, C = e.shape[-1], a.shape[-1]
    M = e.numel() // g
    ef, def_ = e.reshape(M, g), de.reshape(M, g)
    flat = lambda ts: [t.reshape(M, C) for t in ts]
    ta, taa, tda = flat(_taps(a, defect)), flat(_taps(a.abs())), flat(_taps(da))
    dW = torch.stack([ef.T @ t for t in ta], -1).reshape(g, C, 3, 3)
    S = torch.stack([ef.abs().T @ t for t in taa], -1).reshape(g, C, 3, 3)
    Fm = torch.stack([def_.T @ t + ef.abs().T @ d + def_.T @ d for t, d in zip(taa, tda)], -1).reshape(g, C, 3, 3)
    if bias_terms is not None:
        ef, def_ = (t.reshape(M, g) for t in bias_terms)
    db, Sb, Fb = ef.sum(0), ef.abs().sum(0), def_.sum(0)
    return (dW, R(M + 1) * (S + Fm) + Fm), (db, R(M + 1) * (Sb + Fb) + Fb)


def dgrad3_layer(name, G, X, P, Q, keep, y, sc2, sh2, sl2, w2, rnd, c_off, ey=None, defect=None):
    """The 3x3 data gradient of one dense layer from its actual inputs: G, X [n, H, W, C] the block's gradient accumulator and concat
    buffer, P, Q [>= C] the block's rows, keep [n, H, W, g] or None, y the bottleneck map, (sc2, sh2, sl2) norm2 + PReLU2, w2 [g, mid, 3, 3].
    ey: the stored eff rows (checked, then used as the exact operand).  -> [Check]: the eff rows (where stored), DU."""
    g = w2.shape[0]
    sl_ = slice(c_off, c_off + g)
    Ps, Qs = P[sl_], Q[sl_]
    if defect == "no_Q":
        Qs = torch.zeros_like(Qs)
    if defect == "P_without_c_off":
        Ps = P[:g]
    f, tau, e, de = eff_rows(G[..., sl_], X[..., sl_], Ps, Qs, keep, rnd)
    checks = []
    if ey is not None:
        checks.append(Check(name + ":ey", "eff rows", f, tau, rnd))
        e, de = ey, torch.zeros_like(ey)
    dA, ddA = conv3x3_dgrad(e, de, w2, rnd, defect)
    DU, dDU, kink = prelu_bn_backward(dA, ddA, y, sc2, sh2, sl2, defect == "no_sc2")
    checks.append(Check(name + ":du", "dgrad3x3", DU, dDU, rnd, kink))
    return checks


# ---------------------------------------------------------------------------------------------------------------------
# backward: BatchNorm + PReLU links, the 1x1 backward, the whole chain
# ---------------------------------------------------------------------------------------------------------------------
def bn_sums(dA, ddA, x, sc, sh, sl):
    """The three per-channel sums a data-gradient kernel leaves for its consumer BatchNorm (tcvn_ops.h:135-136): s1 = sum dU,
    t2 = sum dU x, s3 = sum dA min(u, 0), with dU = dA prelu'(u), u = sc x + sh; dA [..., C] with its allowed error ddA.
    Gate of a sum: the per-element errors of its summands (delta_dU = max(1, |sl|) ddA + R(1) |dU| for the slope multiply; the fp32 u is
    off by at most tau_u = R(2) (|sc x| + |sh|)), plus R(L) sum |term| for an fp32 chain of L summands in front of the widening to double
    -- L is taken as the whole count M, an upper bound for every kernel (they widen per tile or per lane) -- plus, for the elements
    at a PReLU kink, the difference between the two branches.  -> dU, delta_dU, kink, (s1, t2, s3), (gate1, gate2, gate3)."""
    C = dA.shape[-1]
    u = x * sc + sh
    tau_u = R(2) * ((x * sc).abs() + sh.abs())
    kink = u.abs() <= tau_u
    dU = torch.where(u > 0, dA, sl * dA)
    ddU = torch.maximum(torch.ones_like(sl), sl.abs()) * ddA + R(1) * dU.abs()
    M = dA.numel() // C
    flat = lambda t: t.reshape(M, C)
    jump = torch.where(kink, (dA * (1 - sl)).abs(), torch.zeros_like(dA))
    neg = torch.where(u > 0, torch.zeros_like(u), u)
    t3 = dA * neg
    d3 = ddA * neg.abs() + dA.abs() * tau_u + R(1) * t3.abs()
    sums = (flat(dU).sum(0), flat(dU * x).sum(0), flat(t3).sum(0))
    gates = (flat(ddU + jump).sum(0) + R(M) * flat(dU.abs()).sum(0),
             flat((ddU + jump) * x.abs()).sum(0) + R(M + 1) * flat((dU * x).abs()).sum(0),
             flat(d3).sum(0) + R(M + 1) * flat(t3.abs()).sum(0))
    return dU, ddU, kink, sums, gates


def bn_link(sums, gates, mu, var, gamma, M):
    """BatchNorm backward link (bn_link.h:41-50, double arithmetic on the sums, results rounded to fp32):
        dgamma = r (t2 - mu s1), dbeta = s1, dslope = s3, P = -sc dgamma r / M, Q = -sc s1 / M + sc dgamma r mu / M,  r = 1 / sqrt(var + eps),
    sc = gamma r.  -> {name: (value, delta)}; the fp32 store is added by the caller's Check."""
    (s1, t2, s3), (g1, g2, g3) = sums, gates
    r = 1.0 / torch.sqrt(var + EPS)
    scg = gamma * r
    dgamma, g_dg = r * (t2 - mu * s1), r * (g2 + mu.abs() * g1)
    return dict(dgamma=(dgamma, g_dg), dbeta=(s1, g1), dslope=(s3, g3),
                P=(-scg * dgamma * r / M, scg.abs() * r / M * g_dg),
                Q=(-scg * s1 / M + scg * dgamma * r * mu / M, scg.abs() / M * g1 + scg.abs() * r * mu.abs() / M * g_dg))


def conv1x1_backward(DU, Y, PY, QY, a1, da1, w1, Gb, x, sc1, sh1, sl1, rnd):
    """Backward of a bottleneck 1x1 (bwd1x1_fused.hip:4-8; three-kernel path: eff_materialize, TN GEMM, NT GEMM with the same arithmetic):
    EY = bf16(DU + PY Y + QY); db1 = sum EY; dW1 = EY^T a1 (a1 [..., cin] the activated input with uncertainty da1); dX = EY W1 (one chain of
    mid products); G[:, :cin] = bf16(G_before + sc1 dU1) (gemm_nt.hip:242 one fma; the generic kernel rounds the product first: R(2)).
    The bias gradient may sum the rounded or the unrounded EY (cf. conv3x3_wgrad): its gate takes |f - e| per term in.
    Gb: G[:, :cin] before.  -> dict of (ref, delta[, kink]) and the norm1 sums."""
    f, tau, e, de = eff_rows(DU, Y, PY, QY, None, rnd)
    mid, cin = e.shape[-1], a1.shape[-1]
    M = e.numel() // mid
    ef, def_, af = e.reshape(M, mid), de.reshape(M, mid), a1.reshape(M, cin)
    out = {"EY": (f, tau)}
    slack = (f - e).abs().reshape(M, mid) + tau.reshape(M, mid)
    out["db1"] = (ef.sum(0), R(M + 1) * ef.abs().sum(0) + slack.sum(0))
    S = ef.abs().T @ af.abs()
    Fm = def_.T @ af.abs() + ef.abs().T @ da1.reshape(M, cin) + def_.T @ da1.reshape(M, cin)
    out["dW1"] = (ef.T @ af, R(M + 1) * (S + Fm) + Fm)
    w = _weights(w1, rnd)                                                    # [mid, cin]
    dX, Sx, Fx = e @ w, e.abs() @ w.abs(), de @ w.abs()
    ddX = R(mid) * (Sx + Fx) + Fx
    dU, ddU, kink, sums, gates = bn_sums(dX, ddX, x, sc1, sh1, sl1)
    ref = Gb + sc1 * dU
    out["G"] = (ref, sc1.abs() * ddU + R(2) * (Gb.abs() + (sc1 * dU).abs()), kink)
    return out, sums, gates


def transition_backward(Gn, Xn, Pn, Qn, x, sc, sh, sl, w, rnd):
    """Everything a transition's backward leaves: with ET = eff rows of the next block's first Nt channels (no dropout),
    db = sum ET (rounded or not, as conv1x1_backward's bias), dW = ET^T XP with XP the pooled activation the forward multiplied (sums over the
    Mn pooled positions), the data gradient of ALL input channels (transition_dgrad's arithmetic) and the three sums of the transition norm.
    -> dict of (ref, delta[, kink]), sums, gates."""
    Nt, C = w.shape
    f, tau, e, de = eff_rows(Gn[..., :Nt], Xn[..., :Nt], Pn[:Nt], Qn[:Nt], None, rnd)
    _, _, pa, dpa = pooled_activation(x, sc, sh, sl, rnd)
    Mn = e.numel() // Nt
    ef, def_, af, daf = e.reshape(Mn, Nt), de.reshape(Mn, Nt), pa.reshape(Mn, C), dpa.reshape(Mn, C)
    out = {"db": (ef.sum(0), R(Mn + 1) * ef.abs().sum(0) + ((f - e).abs() + tau).reshape(Mn, Nt).sum(0))}
    S = ef.abs().T @ af.abs()
    Fm = def_.T @ af.abs() + ef.abs().T @ daf + def_.T @ daf
    out["dW"] = (ef.T @ af, R(Mn + 1) * (S + Fm) + Fm)
    wk = _weights(w, rnd)
    dAp, Sp, Fp = e @ wk, e.abs() @ wk.abs(), de @ wk.abs()
    ddAp = R(Nt) * (Sp + Fp) + Fp
    n, H, W, _ = x.shape

    def up(t):
        o = torch.zeros(n, H, W, C, dtype=t.dtype)
        o[:, :2 * t.shape[1], :2 * t.shape[2]] = 0.25 * t.repeat_interleave(2, 1).repeat_interleave(2, 2)
        return o
    dA, ddA = up(dAp), up(ddAp)
    dU, ddU, kink, sums, gates = bn_sums(dA, ddA, x, sc, sh, sl)
    out["G"] = (sc * dU, sc.abs() * ddU + R(1) * (sc * dU).abs(), kink)
    return out, sums, gates


def head_backward(dF, x, sc, sh, sl):
    """Head pooling backward over all channels with the sums of final_norm: dz = dF fl(1 / HW) carries two roundings (elementwise_bwd.hip:20,
    :27), G = sc dU one more on top of bn_sums' slope multiply.  -> (G, delta, kink), sums, gates."""
    n, H, W, C = x.shape
    dz = (dF / (H * W))[:, None, None, :].expand(n, H, W, C)
    dU, ddU, kink, sums, gates = bn_sums(dz, R(2) * dz.abs(), x, sc, sh, sl)
    return (sc * dU, sc.abs() * ddU + R(1) * (sc * dU).abs(), kink), sums, gates


def run_backward(cfg, P, maps, d_cond, keeps=None):
    """The whole deferred (G, P, Q) backward in float64 without rounding, chained from the gradient of `condense`: maps = what run_forward
    returned with stored = None (train mode, rnd off).  -> parameter gradients by name, the gradient reaching pool0's output."""
    g, mid, nb = cfg.densenet_growth_rate, cfg.densenet_batch_norm_size * cfg.densenet_growth_rate, len(cfg.densenet_structure)
    grads = {}
    zero = lambda t: torch.zeros_like(t)

    def stats(x):
        xf = x.reshape(-1, x.shape[-1])
        mu = xf.mean(0)
        return mu, ((xf - mu) ** 2).mean(0), xf.shape[0]

    def link(norm, relu, sums, x):
        mu, var, M = stats(x)
        out = bn_link(sums, sums, mu, var, P[norm + ".weight"], M)
        grads[norm + ".weight"], grads[norm + ".bias"], grads[relu + ".weight"] = out["dgamma"][0], out["dbeta"][0], out["dslope"][0]
        return out["P"][0], out["Q"][0]

    widths, ch = [], cfg.initial_pixel_dim
    for layers in cfg.densenet_structure:
        widths.append(ch)
        ch = (ch + layers * g) // 2
    G, Pq, Qq = {}, {}, {}
    for b in reversed(range(nb)):
        x = maps[f"dense{b + 1}"]
        C = x.shape[-1]
        if b == nb - 1:
            sc, sh = bn_table(x, P["features.final_norm.weight"], P["features.final_norm.bias"])
            sl = P["features.final_relu.weight"]
            dz = (d_cond / (x.shape[1] * x.shape[2]))[:, None, None, :].expand_as(x)
            dU, _, _, sums, _ = bn_sums(dz, zero(dz), x, sc, sh, sl)
            G[b] = sc * dU
            Pq[b], Qq[b] = link("features.final_norm", "features.final_relu", sums, x)
        else:
            t = f"features.transition{b + 1}"
            xn = maps[f"dense{b + 2}"]
            Nt = C // 2
            sc, sh = bn_table(x, P[t + ".norm.weight"], P[t + ".norm.bias"])
            sl = P[t + ".relu.weight"]
            e = G[b + 1][..., :Nt] + Pq[b + 1][:Nt] * xn[..., :Nt] + Qq[b + 1][:Nt]
            pa, _, _, _ = pooled_activation(x, sc, sh, sl, False)
            ef = e.reshape(-1, Nt)
            grads[t + ".conv.bias"], grads[t + ".conv.weight"] = ef.sum(0), (ef.T @ pa.reshape(-1, C)).reshape(Nt, C, 1, 1)
            dAp = e @ P[t + ".conv.weight"].reshape(Nt, C)
            dA = zero(x)
            dA[:, :2 * dAp.shape[1], :2 * dAp.shape[2]] = 0.25 * dAp.repeat_interleave(2, 1).repeat_interleave(2, 2)
            dU, _, _, sums, _ = bn_sums(dA, zero(dA), x, sc, sh, sl)
            G[b] = sc * dU
            Pq[b], Qq[b] = link(t + ".norm", t + ".relu", sums, x)
        for l in reversed(range(cfg.densenet_structure[b])):
            p = f"features.dense{b + 1}.layers.{l}"
            cin = widths[b] + l * g
            cs = slice(cin, cin + g)
            y = maps[f"bottleneck{b + 1}.{l}"]
            n2, n1 = p + ".output_block.norm2", p + ".bottleneck_block.norm1"
            sc2, sh2 = bn_table(y, P[n2 + ".weight"], P[n2 + ".bias"])
            sl2 = P[p + ".output_block.relu2.weight"]
            _, _, e2, _ = eff_rows(G[b][..., cs], x[..., cs], Pq[b][cs], Qq[b][cs], keeps.get((b, l)) if keeps else None, False)
            _, _, a2, _ = activation(y, sc2, sh2, sl2, False)
            (dW2, _), (db2, _) = conv3x3_wgrad(e2, zero(e2), a2, zero(a2), False)
            grads[p + ".output_block.conv2.weight"], grads[p + ".output_block.conv2.bias"] = dW2, db2
            dA2, _ = conv3x3_dgrad(e2, zero(e2), P[p + ".output_block.conv2.weight"], False)
            dU2, _, _, sums2, _ = bn_sums(dA2, zero(dA2), y, sc2, sh2, sl2)
            PY, QY = link(n2, p + ".output_block.relu2", sums2, y)
            xin = x[..., :cin]
            sc1, sh1 = bn_table(xin, P[n1 + ".weight"], P[n1 + ".bias"])
            sl1 = P[p + ".bottleneck_block.relu1.weight"]
            _, _, a1, _ = activation(xin, sc1, sh1, sl1, False)
            out, sums1, _ = conv1x1_backward(sc2 * dU2, y, PY, QY, a1, zero(a1), P[p + ".bottleneck_block.conv1.weight"].reshape(mid, cin),
                                             G[b][..., :cin], xin, sc1, sh1, sl1, False)
            grads[p + ".bottleneck_block.conv1.bias"] = out["db1"][0]
            grads[p + ".bottleneck_block.conv1.weight"] = out["dW1"][0].reshape(mid, cin, 1, 1)
            G[b] = torch.cat([out["G"][0], G[b][..., cin:]], -1)
            dP, dQ = link(n1, p + ".bottleneck_block.relu1", sums1, xin)
            Pq[b] = torch.cat([Pq[b][:cin] + dP, Pq[b][cin:]])
            Qq[b] = torch.cat([Qq[b][:cin] + dQ, Qq[b][cin:]])
    c0 = widths[0]
    x = maps["dense1"]
    return grads, G[0][..., :c0] + Pq[0][:c0] * x[..., :c0] + Qq[0][:c0]


# ---------------------------------------------------------------------------------------------------------------------
# the frozen backward (hit gradients): running statistics, P = Q = PY = QY = 0, no dropout, data gradients alone
# ---------------------------------------------------------------------------------------------------------------------
def output_block_backward_frozen(dOut, Z, gamma, beta, rm, rv, slope, W):
    """Output block backward on running statistics -> the gradient of `condense` (raw:dcondense), its delta, the kink ROWS.
    k_rows_bn_bwd_frozen (input_grad.hip:92-97), all fp32:
        rstd = 1 / sqrtf(rv + eps)                 add, sqrt, divide: 3 roundings;
        u    = (z - rm) * rstd * gamma + beta      subtract, two multiplies, add: 4 roundings on top of rstd's 3, each of a value no
                                                   larger than |(z - rm) rstd gamma| + |beta|: tau_u = R(7) (|(z - rm) rstd gamma| + |beta|);
        dZ   = (u > 0 ? dOut : slope dOut) * gamma * rstd     the slope multiply, two multiplies, rstd's 3: |error| <= R(6) |dZ|.
    linear_bwd_dx (tcvn_rows.h:23-27 -> k_sgemm, rows.hip:36-43): dF[n][k] = sum_c dZ[n][c] W[c][k], one fma chain over the N = out_dim
    products and alpha * acc + 0: delta = R(N + 1) (S + F) + F, S = |dZ| |W|, F = R(6) |dZ| |W|.
    An element (n, c) with |u| <= tau_u may take either branch of prelu', and the Linear spreads it over the whole row n of the result:
    the kink set is those ROWS.  dOut, Z [n, N]; gamma, beta, rm, rv, slope [N]; W [N, K] the bound Linear weight."""
    rstd = 1.0 / torch.sqrt(rv + EPS)
    lin = (Z - rm) * rstd * gamma
    u = lin + beta
    kink = (u.abs() <= R(7) * (lin.abs() + beta.abs())).any(1)
    dZ = torch.where(u > 0, dOut, slope * dOut) * gamma * rstd
    N = Z.shape[1]
    S, Fm = dZ.abs() @ W.abs(), (R(6) * dZ.abs()) @ W.abs()
    return dZ @ W, R(N + 1) * (S + Fm) + Fm, kink[:, None].expand(-1, W.shape[1])


def running_tables(cfg, P, rnd=False):
    """{norm prefix: (sc, sh)} of every BatchNorm2d from the bound RUNNING statistics (rounded to fp32 when rnd: what raw:tabs holds)."""
    out = {}
    for name, _, C in bn_names(cfg):
        sc, sh = bn_table(None, P[name + ".weight"], P[name + ".bias"], (P[name + ".running_mean"], P[name + ".running_var"]))
        out[name] = (f32(sc), f32(sh)) if rnd else (sc, sh)
    return out


def run_backward_frozen(cfg, P, maps, tables, d_out, defects=None):
    """The whole frozen chain in float64 without rounding, composed from the functions above: output block on running statistics, head
    pooling backward, per layer eff rows with P = Q = 0 and keep = None, the 3x3 data gradient, DU = sc2 dA prelu'(u2), the 1x1 backward
    with PY = QY = 0, the transitions, down to DU0 over the conv0 map.  maps: what run_forward returned in eval mode with rnd off (they
    hold conv0 and output_linear); tables: {norm prefix: (sc, sh)} (running_tables); d_out [n, out_dim].
    defects (the gate tests): {"pq": {block: (P, Q)}} rows left in place instead of zero, {"keep": {(block, layer): keep}} a dropout keep
    applied in the eff rows.  -> DU0 [n, Hc, Wc, C0], {name: tensor} of the intermediate state (dcondense, G<b> after each writer, du<b>.<l>)."""
    import stem_reference as S
    g, mid, nb = cfg.densenet_growth_rate, cfg.densenet_batch_norm_size * cfg.densenet_growth_rate, len(cfg.densenet_structure)
    defects = defects or {}
    zero = lambda t: torch.zeros_like(t)
    widths, ch = [], cfg.initial_pixel_dim
    for layers in cfg.densenet_structure:
        widths.append(ch)
        ch = (ch + layers * g) // 2
    o = "output_block.norm"
    d_cond, _, _ = output_block_backward_frozen(d_out, maps["output_linear"], P[o + ".weight"], P[o + ".bias"], P[o + ".running_mean"],
                                                P[o + ".running_var"], P["output_block.relu.weight"], P["output_block.linear.weight"])
    state = {"dcondense": d_cond}
    G = {}
    for b in reversed(range(nb)):
        x = maps[f"dense{b + 1}"]
        C = x.shape[-1]
        Pb, Qb = defects.get("pq", {}).get(b, (torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)))
        if b == nb - 1:
            sc, sh = tables["features.final_norm"]
            (G[b], _, _), _, _ = head_backward(d_cond, x, sc, sh, P["features.final_relu.weight"])
        else:
            t = f"features.transition{b + 1}"
            sc, sh = tables[t + ".norm"]
            Cn = maps[f"dense{b + 2}"].shape[-1]
            Pn, Qn = defects.get("pq", {}).get(b + 1, (torch.zeros(Cn, dtype=torch.float64), torch.zeros(Cn, dtype=torch.float64)))
            out, _, _ = transition_backward(G[b + 1], maps[f"dense{b + 2}"], Pn, Qn, x, sc, sh, P[t + ".relu.weight"],
                                            P[t + ".conv.weight"].reshape(C // 2, C), False)
            G[b] = out["G"][0]
        state[f"G{b + 1}:first"] = G[b]
        for l in reversed(range(cfg.densenet_structure[b])):
            p = f"features.dense{b + 1}.layers.{l}"
            cin = widths[b] + l * g
            cs = slice(cin, cin + g)
            y = maps[f"bottleneck{b + 1}.{l}"]
            sc2, sh2 = tables[p + ".output_block.norm2"]
            _, _, e2, _ = eff_rows(G[b][..., cs], x[..., cs], Pb[cs], Qb[cs], defects.get("keep", {}).get((b, l)), False)
            dA2, _ = conv3x3_dgrad(e2, zero(e2), P[p + ".output_block.conv2.weight"], False)
            DU, _, _ = prelu_bn_backward(dA2, zero(dA2), y, sc2, sh2, P[p + ".output_block.relu2.weight"])
            state[f"du{b + 1}.{l}"] = DU
            xin = x[..., :cin]
            sc1, sh1 = tables[p + ".bottleneck_block.norm1"]
            sl1 = P[p + ".bottleneck_block.relu1.weight"]
            _, _, a1, _ = activation(xin, sc1, sh1, sl1, False)
            zy = torch.zeros(mid, dtype=torch.float64)
            out, _, _ = conv1x1_backward(DU, y, zy, zy, a1, zero(a1), P[p + ".bottleneck_block.conv1.weight"].reshape(mid, cin),
                                         G[b][..., :cin], xin, sc1, sh1, sl1, False)
            G[b] = torch.cat([out["G"][0], G[b][..., cin:]], -1)
        state[f"G{b + 1}"] = G[b]
    c0 = maps["conv0"]
    C0 = widths[0]
    P0, Q0 = defects.get("pq", {}).get(0, (torch.zeros(C0, dtype=torch.float64),) * 2)
    sc, sh = tables["features.norm0"]
    dz, ddz = S.pool_backward(G[0][..., :C0], maps["dense1"][..., :C0], P0[:C0], Q0[:C0], c0.shape[1], c0.shape[2])
    dU, _, _, _, _ = bn_sums(dz, zero(dz), c0, sc, sh, P["features.relu0.weight"])
    return sc * dU, state


def frozen_block_slices(name, first, G_final, x, ys, tabs1, tabs2, sl1s, sl2s, w1s, w2s, c0, g, rnd):
    """The FINAL accumulator of one block after a frozen backward (raw:grad<b>), every layer's slice and the block's first channels,
    without a hook: what stays readable is the end of a chain of read-add-writes, G[:, :cin_l] = store(G + sc1 dU1) for l = L - 1 .. 0,
    behind the first writer.  The chain is walked with a running reference A and the |error| dpre a correct schedule may have in front
    of a store (the buffer then holds a value within store_gate(A, dpre)):
      * the first writer's (ref, delta, kink) as head_backward / transition_backward give them: A = ref, dpre = delta;
      * layer l: its slice [cin, cin + g) is final -- Check(A, dpre) against the stored slice.  The STORED slice then feeds the layer's own
        3x3 data gradient (eff rows with P = Q = 0: fma(0, x, g) + 0 = g exactly), so no error is carried from one layer's check into the
        next through this path: DU = prelu_bn_backward(conv3x3_dgrad(...)) with its gate.  DU itself is gone (every layer overwrites it), so
        the 1x1 backward's operand is the reference DU with the uncertainty of its store, de = store_gate(DU, dDU); with PY = QY = 0 the
        eff row is DU itself (fma(0, y, du) + 0, already of the stored format).  dX = DU W1: one chain of mid products,
        ddX = R(mid) (S + F) + F, F = de |W1|; bn_sums gives dU1 and its error; the read-add-write (gemm_nt.hip:242, conv1x1_backward):
        A[:cin] += sc1 dU1,  dpre[:cin] = store_gate(A, dpre) + |sc1| ddU1 + R(2) (|A| + |sc1 dU1|);
      * an element whose history holds a PReLU kink is left out: the first writer's kink set, norm1's per element, and for a kink of norm2
        at one pixel the pixel's whole row of G[:, :cin] (the 1x1 spreads it); Check holds the set to KINK_CAP.
    first = (ref, delta, kink) over all Ct channels; G_final, x [n, H, W, Ct]; ys, tabs*, sl*, w* per layer (w1 [mid, cin], w2 [g, mid, 3, 3]).
    -> [Check] for every layer's slice (last layer first) and the first c0 channels, the stored counterparts."""
    A, dpre, skip = first[0].clone(), first[1].clone(), first[2].clone()
    L = len(ys)
    checks, got = [], []
    for l in reversed(range(L)):
        cin = c0 + l * g
        cs = slice(cin, cin + g)
        checks.append(Check(f"{name}:grad[{cin}:{cin + g}]", "final G slice", A[..., cs].clone(), dpre[..., cs].clone(), rnd, skip[..., cs].clone()))
        got.append(G_final[..., cs])
        zero = torch.zeros(g, dtype=torch.float64)
        _, _, e, de = eff_rows(G_final[..., cs], x[..., cs], zero, zero, None, rnd)
        dA2, ddA2 = conv3x3_dgrad(e, de, w2s[l], rnd)
        DU, dDU, kink2 = prelu_bn_backward(dA2, ddA2, ys[l], tabs2[l][0], tabs2[l][1], sl2s[l])
        de1 = store_gate(DU, dDU, rnd)
        w = _weights(w1s[l], rnd)
        dX = DU @ w
        Fx = de1 @ w.abs()
        ddX = R(DU.shape[-1]) * (DU.abs() @ w.abs() + Fx) + Fx
        xin = x[..., :cin]
        sc1, sh1 = tabs1[l]
        dU1, ddU1, kink1, _, _ = bn_sums(dX, ddX, xin, sc1, sh1, sl1s[l])
        c = sc1 * dU1
        Ain, din = A[..., :cin], dpre[..., :cin]
        dnew = store_gate(Ain, din, rnd) + sc1.abs() * ddU1 + R(2) * (Ain.abs() + c.abs())
        A = torch.cat([Ain + c, A[..., cin:]], -1)
        dpre = torch.cat([dnew, dpre[..., cin:]], -1)
        skip = torch.cat([skip[..., :cin] | kink1 | kink2.any(-1, keepdim=True), skip[..., cin:]], -1)
    checks.append(Check(f"{name}:grad[0:{c0}]", "final G slice", A[..., :c0], dpre[..., :c0], rnd, skip[..., :c0]))
    got.append(G_final[..., :c0])
    return checks, got


def hit_gradient_check(du0, w0, coords, values, shape, value_mode, name="d_values"):
    """k_hit_gradient (input_grad.hip:45-75) from the STORED DU0 (raw:du0: bf16 or fp32 values, exact in double) and the bound fp32 conv0
    weight: per hit and pixel channel at most 16 taps x N output channels of double fma (:60), 6 double additions of the xor-shuffle sum
    (:68), the value-mode factor formed in double (:74: at most an addition and a division) and its multiply, ONE rounding to fp32 (:75):
        delta = Rd(16 N + 6 + 3) S,  S = the same gather over |DU0| |W0| |factor|,  Rd(n) = (1 + 2^-53)^n - 1,
    then the fp32 store rule.  Entries that do not own their pixel (and entries outside the maps) are exactly 0: gate 0.
    The reference is hit_gradients_reference.gather.  -> Check."""
    import hit_gradients_reference as H
    ref = H.gather(du0, w0, coords, values, shape, value_mode)
    S = H.gather(du0.abs(), w0.abs(), coords, values, shape, value_mode).abs()
    n = 16 * du0.shape[-1] + 9
    return Check(name, "k_hit_gradient", ref, ((1.0 + 2.0 ** -53) ** n - 1.0) * S, False)


# ---------------------------------------------------------------------------------------------------------------------
# the network, operation by operation
# ---------------------------------------------------------------------------------------------------------------------
def bn_table(x, gamma, beta, running=None):
    """(scale, shift) of a BatchNorm over x [..., C]: batch statistics of the stored values (train) or the running ones."""
    if running is None:
        xf = x.reshape(-1, x.shape[-1])
        mean = xf.mean(0)
        var = ((xf - mean) ** 2).mean(0)
    else:
        mean, var = running
    sc = gamma / torch.sqrt(var + EPS)
    return sc, beta - mean * sc


def bn_names(cfg):
    """Every BatchNorm2d in the order of its table in raw:tabs -> (parameter prefix, activation prefix, channels)."""
    g, mid = cfg.densenet_growth_rate, cfg.densenet_batch_norm_size * cfg.densenet_growth_rate
    out = [("features.norm0", "features.relu0", cfg.initial_pixel_dim)]
    ch, nb = cfg.initial_pixel_dim, len(cfg.densenet_structure)
    for b, layers in enumerate(cfg.densenet_structure):
        for l in range(layers):
            p = f"features.dense{b + 1}.layers.{l}"
            out.append((p + ".bottleneck_block.norm1", p + ".bottleneck_block.relu1", ch + l * g))
            out.append((p + ".output_block.norm2", p + ".output_block.relu2", mid))
        ch += layers * g
        if b != nb - 1:
            out.append((f"features.transition{b + 1}.norm", f"features.transition{b + 1}.relu", ch))
            ch //= 2
    out.append(("features.final_norm", "features.final_relu", ch))
    return out


def tables_from_tabs(cfg, tabs):
    """raw:tabs (flat) -> {norm prefix: (sc, sh)}; the offsets must tile it exactly."""
    out, off = {}, 0
    for name, _, C in bn_names(cfg):
        C8 = -(-C // 8) * 8
        out[name] = (tabs[off: off + C], tabs[off + C8: off + C8 + C])
        off += 2 * C8
    assert off == tabs.numel(), (off, tabs.numel())
    return out


class Check:
    """One compared tensor: ref (unrounded), gate (store rule included), and -- once a stored counterpart is known -- the worst ratio."""
    def __init__(self, name, kernel, ref, delta, rnd_store, kink=None):
        self.name, self.kernel, self.ref = name, kernel, ref
        self.gate = store_gate(ref, delta, rnd_store)
        self.kink = kink                  # elements at a PReLU kink, where prelu' may take either branch: the ONLY exclusion there is
        assert kink is None or int(kink.sum()) <= KINK_CAP * kink.numel(), (name, int(kink.sum()), kink.numel())

    def ratio(self, got):
        """Worst |got - ref| / gate and the number of elements outside (a NaN is outside; 0 / 0 is inside)."""
        err = (got - self.ref).abs()
        bad = ~(err <= self.gate)
        if self.kink is not None:
            err, bad = torch.where(self.kink, torch.zeros_like(err), err), bad & ~self.kink
        r = torch.where(err > 0, err / self.gate, torch.zeros_like(err))
        worst = float(r.max()) if r.numel() else 0.0
        where = [tuple(int(v) for v in ix) for ix in bad.nonzero()[:4]]
        return worst, int(bad.sum()), where


def run_forward(cfg, P, rnd, train, c0, keeps=None, stored=None, tabs=None, defects=None):
    """Every forward operation behind conv0, in network order.  P: parameters by name (float64, no prefix); c0: the conv0 map [n, Hc, Wc,
    C0] or None (pool0 is then left out; needs `stored`); keeps: {(block, layer): [n, H, W, g] keep scale} or None.
    stored = None: each operation reads what the one before produced (rounded as the kernel stores it when rnd) and the tables are the
    statistics of those maps -- the bf16-faithful network without a GPU.
    stored = {tap name: tensor}: each operation reads the engine's OWN stored input, tables from `tabs` (raw:tabs); the materialised
    operands xa / ya are used, and checked, where they exist.
    defects: {operation name: defect} builds the deliberately wrong kernel of the gate tests.
    -> checks [Check], maps {tap name: produced map}."""
    g, mid, nb = cfg.densenet_growth_rate, cfg.densenet_batch_norm_size * cfg.densenet_growth_rate, len(cfg.densenet_structure)
    defects = defects or {}
    tabd = tables_from_tabs(cfg, tabs) if tabs is not None else None
    st = (lambda t: bf16(t)) if rnd else (lambda t: t)
    checks, maps = [], {"conv0": c0}

    def table(norm, x):
        if tabd is not None:
            return tabd[norm]
        run = None if train else (P[norm + ".running_mean"], P[norm + ".running_var"])
        sc, sh = bn_table(x, P[norm + ".weight"], P[norm + ".bias"], run)
        return (f32(sc), f32(sh)) if rnd else (sc, sh)

    def emit(name, kernel, ref, delta, rnd_store=rnd):
        checks.append(Check(name, kernel, ref, delta, rnd_store))
        return bf16(ref) if rnd_store else ref

    def have(name):
        return stored[name] if stored is not None and name in stored else None

    # ---- stem tail
    x = None
    if c0 is not None:                                                     # (the sparse stem materialises no conv0 map: nothing to start from)
        sc, sh = table("features.norm0", c0)
        ref, d = pool0(c0, sc, sh, P["features.relu0.weight"])
        x = emit(f"dense1[0:{cfg.initial_pixel_dim}]", "pool0", ref, d)
        maps["pool0"] = x
    ch = cfg.initial_pixel_dim
    for b, layers in enumerate(cfg.densenet_structure):
        if stored is not None:
            x = stored[f"dense{b + 1}"]
        for l in range(layers):
            p = f"features.dense{b + 1}.layers.{l}"
            cin = ch + l * g
            xin = x[..., :cin]
            # ---- BN1 - PReLU1 - 1x1
            sc, sh = table(p + ".bottleneck_block.norm1", xin)
            sl = P[p + ".bottleneck_block.relu1.weight"]
            dfc = defects.get(f"conv1x1.{b + 1}.{l}")
            if dfc == "drop_last_channel":
                sc = torch.cat([sc[:-1], sc[-1:] * 0]); sh = torch.cat([sh[:-1], sh[-1:] * 0])      # prelu(0) = 0: the channel is gone
            if dfc == "slice_table":                                       # columns [128, 256) take the table of columns [0, 128)
                k = min(256, cin) - 128
                sc, sh = sc.clone(), sh.clone()
                sc[128:128 + k], sh[128:128 + k] = sc[:k].clone(), sh[:k].clone()
            f, tau, a, da = activation(xin, sc, sh, sl, rnd)
            xa = have(f"xa{b + 1}.{l}")
            if xa is not None:
                checks.append(Check(f"xa{b + 1}.{l}", "act", f, tau, rnd))
                a, da = xa, torch.zeros_like(xa)
            w1 = P[p + ".bottleneck_block.conv1.weight"].reshape(mid, cin)
            v, dv = conv1x1(a, da, w1, P[p + ".bottleneck_block.conv1.bias"], rnd)
            n2, sl2 = p + ".output_block.norm2", P[p + ".output_block.relu2.weight"]
            epi = stored is not None and f"bottleneck{b + 1}.{l}" not in stored      # eval: the activated map is the 1x1's only output
            if epi:
                sc2, sh2 = table(n2, None)
                fe, de = act_epilogue(v, dv, sc2, sh2, sl2)
                emit(f"ya{b + 1}.{l}", "conv1x1+act", fe, de)
                a2 = stored[f"ya{b + 1}.{l}"]
                da2 = torch.zeros_like(a2)
            else:
                y = emit(f"bottleneck{b + 1}.{l}", "conv1x1", v, dv)
                maps[f"bottleneck{b + 1}.{l}"] = y
                if stored is not None:
                    y = stored[f"bottleneck{b + 1}.{l}"]
                # ---- BN2 - PReLU2
                sc2, sh2 = table(n2, y)
                f2, tau2, a2, da2 = activation(y, sc2, sh2, sl2, rnd)
                ya = have(f"ya{b + 1}.{l}")
                if ya is not None:
                    checks.append(Check(f"ya{b + 1}.{l}", "act", f2, tau2, rnd))
                    a2, da2 = ya, torch.zeros_like(ya)
            # ---- 3x3 - dropout
            keep = keeps.get((b, l)) if keeps else None
            dfc = defects.get(f"conv3x3.{b + 1}.{l}")
            if dfc == "wrong_keep":
                keep = keeps[(b, l - 1)]
            ref, d = conv3x3(a2, da2, P[p + ".output_block.conv2.weight"], P[p + ".output_block.conv2.bias"], keep, rnd,
                             dfc if dfc != "wrong_keep" else None)
            new = emit(f"dense{b + 1}[{cin}:{cin + g}]", "conv3x3", ref, d)
            if stored is None:
                x = torch.cat([x, new], -1)
        ch += layers * g
        maps[f"dense{b + 1}"] = x
        if b != nb - 1:
            # ---- transition: BN - PReLU - 2x2 pooling (commuted in front) - 1x1
            t = f"features.transition{b + 1}"
            sc, sh = table(t + ".norm", x)
            _, _, a, da = pooled_activation(x, sc, sh, P[t + ".relu.weight"], rnd, defects.get(f"transition{b + 1}") == "ceil_pool")
            ref, d = conv1x1(a, da, P[t + ".conv.weight"].reshape(ch // 2, ch), P[t + ".conv.bias"], rnd)
            x = emit(f"dense{b + 2}[0:{ch // 2}]", "transition", ref, d)
            ch //= 2
    # ---- head
    sc, sh = table("features.final_norm", x)
    ref, d = head_pool(x, sc, sh, P["features.final_relu.weight"])
    cond = emit("condense", "head_pool", ref, d, False)
    if rnd:
        cond = f32(cond)
    maps["condense"] = cond
    if stored is not None:
        cond = stored["condense"]
    ref, d = linear(cond, P["output_block.linear.weight"])
    maps["output_linear"] = emit("output_linear", "linear", ref, d, False)
    return checks, maps


def stored_counterpart(check, stored):
    """The stored tensor a Check's name addresses: a tap, or a channel slice 'dense<b>[lo:hi]' of one."""
    if "[" in check.name:
        tap, rng = check.name[:-1].split("[")
        lo, hi = (int(v) for v in rng.split(":"))
        return stored[tap][..., lo:hi]
    t = stored[check.name]
    return t.reshape(check.ref.shape)
