"""Float64 reference of the SDXL embedder's tape operations (csrc/sdxl.hip: CONV and GN ops over NHWC buffers), one plain function
per operation, each with the |error| a correct kernel may show per element.  No GPU: a function takes the operation's ACTUAL stored inputs
(the engine's activation buffers, its (sum, sum of squares) statistics, the bound fp32 parameters) as float64 tensors, so nothing drifts
between the two sides.  `rnd` switches the bf16 roundings on (bf16 mode) or off (fp32 mode; with the gates ignored and every operation
reading what the one before produced it is the exact network, which test_sdxl_op_reference_cpu.py pins against oracle/sdxl_oracle.py).
The number formats, R(n) and the store rule are those of densenet_layer_reference.py (imported, not copied).

The forward gates follow; the backward operations and their gates are derived in front of conv_dgrad below.

Gates (u = 2^-24, R(n) = (1 + u)^n - 1 the compound of n fp32 roundings; line numbers are those of csrc/ as it stands with this file; the validation-only code sits behind the cited lines):
  * Weight packs (elementwise.hip:383-412 k_pack): wk[n][tap Cin + c] = wkt[c][tap Cout + n] = bf16(w[n][c][tap]) (f2bf, :360) or w itself
    in fp32 mode (:363); every column from taps * inner up to Kp is written 0 (:351-352).  Bit for bit, no gate.
  * Convolution forward.  Operands are stored values, bf16 x bf16 products are exact in fp32, and every kernel is one fp32 accumulation
    chain over the K = ks ks Cin products of an output element (the MFMA is one, whatever its internal order: sdxl_conv3x3.hip:122-132
    tap_step, called over the nine taps at :258-259 C64 and :147-160 ring_taps -- G over its channel chunks without a break, :335, and
    S2, :405 --, sdxl_stem.hip:75-82 IN, sdxl_kernels.hip:109-119 generic), then
    c epilogue additions: the bias (sdxl_conv3x3.hip:171 acc_to_cs, sdxl_stem.hip:86-87, sdxl_kernels.hip:131) and, with a residual,
    one more (sdxl_conv3x3.hip:180 cs_store8, sdxl_kernels.hip:132): c = 1 or 2.
        delta = R(K + c) S,   S = sum |a| |w| + |bias| + |res|
    fp32 mode (generic kernel only): the fp32 MFMA may round a product before it adds it, one more rounding per term: R(K + c + 1).
    Store: bf16 (from_f / f2bf) or fp32 for the final convolution (sdxl_kernels.hip:133) and in fp32 mode: densenet's store_gate.
    Taps outside the map contribute exact zeros; behind a stride-2 convolution that is the far row and column, which an even side reads
    (output row H / 2 - 1 covers rows H - 2 .. H) and an odd side does not.
  * Statistics handed to a GroupNorm: (sum, sum of squares) over the STORED values of one image, exact in float64.  The kernel sums in
    fp32 first and widens to double per tile / per 8 values; a value passes at most D fp32 additions on that way, a square one
    multiplication more (its product f * f is rounded):  gate_sum = R(D) sum |x|,  gate_sq = R(D + 1) sum x^2,  plus 2^-48 of the same
    sums for the double atomics (fewer than 2^4 of them per value chain would already be generous).
        fused epilogue, C64 / G (512 threads): 2 passes x 2 rows x 8 values per thread (sdxl_conv3x3.hip:202-215 tile8x32_out, the
            sums at :187 cs_store8), six wave_sum steps and one LDS float atomic per wave of eight (:74-77), then double (:78-81):
                                                                                                                  D = 32 + 6 + 8 = 46
        fused epilogue, S2 (256 threads): 2 x 8 values (:410-416, :187), wave_sum, four waves:                    D = 16 + 6 + 4 = 26
        fused epilogue, IN (256 threads): 8 x 8 values (sdxl_stem.hip:93-103), wave_sum, four waves (:108-109):   D = 64 + 6 + 4 = 74
        stand-alone k_gn_stats after a generic or packed-G launch (sdxl_kernels.hip:817-820): groups of 8 values in fp32, then double
            (:387-390) when C % 8 == 0, else double throughout (:393-396):                                        D = 8 or 0
  * GroupNorm (+ SiLU) forward (k_gn_act sdxl_kernels.hip:428-429 / :435-436, k_gn_act_v :535-536): mean and rstd come from the engine's own
    statistics in double, rounded to float (gn_mean_rstd :403-409: m = s / cnt, var = max(ss / cnt - m m, 0), rstd = 1 / sqrt(var + eps),
    eps the float 1e-6f) -- exact inputs here.  u = (x - mean) rstd gamma + beta is three roundings on t = (x - mean) rstd gamma and one
    addition:  du = R(3) |t| + R(1) (|t| + |beta|)  (a contraction into an fma only removes one).
    silu(u) = u * rcp(1 + __expf(-u)) (:359).  ASSUMPTION -- neither intrinsic has an error bound in this repository or its guides:
    __expf(x) = exp2(x log2 e) is taken as one rounding of the argument (relative error u |x| of the result) plus EXP_ULP = 1 ulp, and
    v_rcp_f32 as RCP_ULP = 1 ulp (1 ulp = 2 u relative).  With sigma = 1 / (1 + e), e = exp(-u):
        rel(e) = u |u| (1 + 2 u) + 2 u EXP_ULP;  rel(sigma) = (1 - sigma) rel(e) + u [the addition] + 2 u RCP_ULP;
        |err silu| = |silu| (rel(sigma) + u) + |silu'(u)| du
    and dsilu(u) = s (1 + u (1 - s)) (:360) follows the same chain (dsilu_gate).  test_sdxl_ops_float64_gpu.py evaluates the file's own silu
    / dsilu on a dense sweep of [-40, 40] in the validation build (tcvn_debug_sdxl_silu_probe) and asserts exactly these two gates, so
    the assumption is tested on the intrinsics and never on the GroupNorm kernels.  Results below the fp32 normal range may flush to zero
    (rcp of more than 2^126, an overflowing exp): (1 + |u|) 2^-126 is added.
No element is excluded and no gate carries a fitted factor: SiLU has no kink."""
import torch

from densenet_layer_reference import bf16, f32, ulp, R, store_gate, U      # noqa: F401  (ulp: re-exported for the tests)

GN_EPS = float(torch.tensor(1e-6, dtype=torch.float32))        # kGnEps = 1e-6f (sdxl.hip:33), as the float the kernel receives
EXP_ULP, RCP_ULP = 1.0, 1.0                                   # assumed intrinsic errors in ulp (see above); asserted on the probe sweep
FLUSH = 2.0 ** -126
D_FUSED = {"c64": 46, "g": 46, "s2": 26, "in": 74}           # fp32 additions a value passes in a fused statistics epilogue
D_STANDALONE_VEC, D_STANDALONE = 8, 0
OP_CONV, OP_GN = 0, 1


# ---------------------------------------------------------------------------------------------------------------------
# TileMap (sdxl_conv3x3.hip:274-282 make_map, :507 packed) restated
# ---------------------------------------------------------------------------------------------------------------------
def tile_map(H, W):
    """-> (px, py): images side by side / stacked in one 8 x 32 tile of SCONV_G."""
    px = 32 // (W + 1) if W <= 15 else 1
    py = 8 // (H + 1) if (H <= 3 and px > 1) else 1
    return px, py


def packs(H, W):
    px, py = tile_map(H, W)
    return px > 1 or py > 1


def stats_depth(kernel, H, W, C):
    """Which statistics path follows a forward convolution kernel (sconv_fwd_kernel's fuses_stats, sdxl_kernels.hip:780; H, W the
    convolution's INPUT map, which is what sconv3_packs looks at) -> ("fused" | "standalone", D)."""
    if kernel != "generic" and not (kernel == "g" and packs(H, W)):
        return "fused", D_FUSED[kernel]
    return "standalone", (D_STANDALONE_VEC if C % 8 == 0 else D_STANDALONE)


# ---------------------------------------------------------------------------------------------------------------------
# weight packs
# ---------------------------------------------------------------------------------------------------------------------
def weight_pack(w, Kp, transpose, rnd):
    """w [Cout, Cin, ks, ks] (the bound fp32 values) -> the pack the forward (transpose False: [Cout][tap Cin + c]) or the data gradient
    (True: [Cin][tap Cout + n]) reads, zero padded to Kp columns.  Exact."""
    N, Ci, kh, kw = w.shape
    wr = bf16(w) if rnd else w
    t = wr.reshape(N, Ci, kh * kw)
    rows = t.permute(1, 2, 0).reshape(Ci, kh * kw * N) if transpose else t.permute(0, 2, 1).reshape(N, kh * kw * Ci)
    out = torch.zeros(rows.shape[0], Kp, dtype=torch.float64)
    out[:, :rows.shape[1]] = rows
    return out


# ---------------------------------------------------------------------------------------------------------------------
# convolution forward
# ---------------------------------------------------------------------------------------------------------------------
def _conv_nhwc(a, w, ks, stride, pad, far_zero=True, clamp_far=False):
    """sum over taps of a[img][ho stride + ky - pad][wo stride + kx - pad][:] @ w[:, :, ky, kx].T with zeros outside the map (top-left
    padding `pad`; the far side as far as the taps reach).  clamp_far: the DEFECT of a far row / column that repeats the last one."""
    n, H, W, C = a.shape
    far = 1 if stride == 2 else pad
    # sdxl.hip:117 (C division truncates: a 1-pixel side stays 1 behind a stride-2 convolution, whose third tap then lies beyond the far row too)
    Ho, Wo = int((H + pad + far - ks) / stride) + 1, int((W + pad + far - ks) / stride) + 1
    ap = torch.zeros(n, max(H + pad + far, (Ho - 1) * stride + ks), max(W + pad + far, (Wo - 1) * stride + ks), C, dtype=a.dtype)
    ap[:, pad:pad + H, pad:pad + W] = a
    if clamp_far and far:
        ap[:, pad + H:, pad:pad + W] = a[:, H - 1:H]
        ap[:, :, pad + W:] = ap[:, :, pad + W - 1:pad + W]
    out = torch.zeros(n, Ho, Wo, w.shape[0], dtype=a.dtype)
    for ky in range(ks):
        for kx in range(ks):
            sl = ap[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            out += (sl.reshape(-1, C) @ w[:, :, ky, kx].T).reshape(n, Ho, Wo, -1)
    return out


def conv_forward(a, w, bias, res, ks, stride, pad, rnd, clamp_far=False):
    """a [n, H, W, Cin] stored input; w [Cout, Cin, ks, ks] and bias [Cout] the bound fp32 values (w rounded here as k_pack does);
    res [n, Ho, Wo, Cout] stored residual or None.  -> ref (unrounded), delta (without the store rule)."""
    wr = bf16(w) if rnd else w
    K = ks * ks * a.shape[-1]
    c = 1 + (res is not None)
    ref = _conv_nhwc(a, wr, ks, stride, pad, clamp_far=clamp_far) + bias
    S = _conv_nhwc(a.abs(), wr.abs(), ks, stride, pad) + bias.abs()
    if res is not None:
        ref, S = ref + res, S + res.abs()
    return ref, R(K + c + (0 if rnd else 1)) * S


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
def stored_stats(x, D):
    """x [n, H, W, C] STORED values -> (sum, sum of squares) [n, 2] in float64 and their gates for a chain of depth D."""
    n = x.shape[0]
    xf = x.reshape(n, -1)
    s, sa, ss = xf.sum(1), xf.abs().sum(1), (xf * xf).sum(1)
    ref = torch.stack([s, ss], 1)
    gate = torch.stack([(R(D) + 2.0 ** -48) * sa, (R(D + 1) + 2.0 ** -48) * ss], 1)
    return ref, gate


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm (+ SiLU) forward
# ---------------------------------------------------------------------------------------------------------------------
def mean_rstd(stats, cnt, eps=GN_EPS, exact=False):
    """gn_mean_rstd: stats [n, 2] doubles -> (mean, rstd) [n], each rounded to float (exact: not rounded, for the pin against the oracle)."""
    m = stats[:, 0] / cnt
    var = (stats[:, 1] / cnt - m * m).clamp_min(0.0)
    r = 1.0 / torch.sqrt(var + eps)
    return (m, r) if exact else (f32(m), f32(r))


def _sigma(u):
    return torch.sigmoid(u)


def _rel_sigma(u):
    sg = _sigma(u)
    rel_e = U * u.abs() * (1 + 2 * U) + 2 * U * EXP_ULP
    return sg, (1 - sg) * rel_e + U + 2 * U * RCP_ULP


def silu_gate(u):
    """-> silu(u) exact, |error| of the kernel's silu evaluated AT the fp32 value u (no argument error)."""
    sg, rs = _rel_sigma(u)
    ref = u * sg
    return ref, ref.abs() * ((1 + rs) * (1 + U) - 1) + (1 + u.abs()) * FLUSH


def dsilu_exact(u):
    sg = _sigma(u)
    return sg * (1 + u * (1 - sg))


def dsilu_gate(u):
    """s (1 + u (1 - s)) with s = sigma (1 + rs): A = 1 - s, B = u A, Cc = 1 + B, result s Cc -- each step's absolute error carried on."""
    sg, rs = _rel_sigma(u)
    ds = sg * rs
    A = 1 - sg
    dA = ds + U * (A.abs() + ds)
    B = u * A
    dB = u.abs() * dA + U * (B.abs() + u.abs() * dA)
    Cc = 1 + B
    dC = dB + U * (Cc.abs() + dB)
    ref = sg * Cc
    return ref, ds * (Cc.abs() + dC) + sg * dC + U * (ref.abs() + ds * (Cc.abs() + dC) + sg * dC) + (1 + u.abs()) * FLUSH


def gn_forward(x, stats, gamma, beta, act, eps=GN_EPS, exact=False):
    """x [n, H, W, C] stored input, stats [n, 2] the engine's own statistics of it, gamma / beta [C] the bound fp32 values.
    -> ref (unrounded), delta (without the store rule)."""
    n, H, W, C = x.shape
    mean, rstd = mean_rstd(stats, float(H * W * C), eps, exact)
    t = (x - mean[:, None, None, None]) * rstd[:, None, None, None] * gamma
    u = t + beta
    du = R(3) * t.abs() + R(1) * (t.abs() + beta.abs())
    if not act:
        return u, du
    ref, g = silu_gate(u)
    # the kernel's argument is off by at most du: |silu'| is largest at the argument's end of [u - du, u + du] that lies farther out
    slope = torch.maximum(dsilu_exact(u - du).abs(), dsilu_exact(u + du).abs()).maximum(dsilu_exact(u).abs())
    return ref, g + slope * du * (1 + 4 * U)


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
class Check:
    """One compared tensor: ref (unrounded) and gate; ratio(got) -> worst |got - ref| / gate, elements outside, where."""
    def __init__(self, name, kind, family, ref, gate):
        self.name, self.kind, self.family, self.ref, self.gate = name, kind, family, ref, gate

    def ratio(self, got):
        err = (got.reshape(self.ref.shape) - self.ref).abs()
        bad = ~(err <= self.gate)                                            # a NaN is outside; 0 <= 0 is inside
        r = torch.where(err > 0, err / self.gate, torch.zeros_like(err))
        worst = float(r.max()) if r.numel() else 0.0
        return worst, int(bad.sum()), [tuple(int(v) for v in ix) for ix in bad.nonzero()[:4]]


def stored_check(name, kind, family, ref, delta, rnd_store):
    return Check(name, kind, family, ref, store_gate(ref, delta, rnd_store))


def exact_check(name, kind, family, ref):
    return Check(name, kind, family, ref, torch.zeros_like(ref))


def conv_weight(P, names, op, bufs_c):
    """The bound weight of a CONV op as [Cout, Cin, ks, ks] and its bias (the Linear layers of the tape are 1x1 convolutions)."""
    w = P[names[op["w"]]]
    return w.reshape(bufs_c[op["out"]], bufs_c[op["in"]], op["ks"], op["ks"]), P[names[op["w"] + 1]]


# ---------------------------------------------------------------------------------------------------------------------
# the tape, operation by operation
# ---------------------------------------------------------------------------------------------------------------------
def run_forward(ops, names, P, img, rnd, kernels=None, stored=None, stats=None, exact_gn=False):
    """Every forward operation of the tape `ops` (SdxlEngine.ops()), in order.  names: slot names (SdxlEngine.slots()); P: parameters by
    slot name, float64; img [n, H, W, 3]: buffer 0 as stored; kernels: SdxlEngine.conv_kernels() rows (forward family per conv_id), None =
    all generic.
    stored = None: every operation reads what the one before produced (rounded as the kernel stores it when rnd), statistics are those of
    the produced maps: the bf16-faithful network without a GPU (rnd off: the exact network).
    stored = {buffer index: tensor}, stats [n_gn, n, 2]: every operation reads the engine's OWN stored input and statistics.
    exact_gn: mean, rstd and eps = 1e-6 in double (with rnd off: the exact network, for the pin against the oracle).
    -> checks [(Check, what it addresses)], bufs {buffer index: produced map}; what = ("act", buf) | ("stats", gn_id) | ("out",)."""
    bufs = {0: img}
    chan = {0: img.shape[-1]}
    for o in ops:                                                              # channel counts, for the weight shapes
        if o["kind"] == OP_GN:
            chan[o["out"]] = chan[o["in"]]
        else:
            w = P[names[o["w"]]]
            chan[o["out"]] = w.shape[0]
    checks, own_stats = [], {}

    def src(b):
        return stored[b] if stored is not None else bufs[b]

    for i, o in enumerate(ops):
        if o["kind"] == OP_CONV:
            fam = kernels[o["conv_id"]][0] if kernels is not None else "generic"
            a = src(o["in"])
            w, b = conv_weight(P, names, o, chan)
            res = src(o["res"]) if o["res"] >= 0 else None
            ref, d = conv_forward(a, w, b, res, o["ks"], o["stride"], o["pad"], rnd)
            final = o["final_f32"] == 1
            name = f"op{i}:conv{o['conv_id']}:{names[o['w']][:-7]}"
            if final:
                checks.append((stored_check(name, "conv", fam, ref.reshape(ref.shape[0], -1), d.reshape(ref.shape[0], -1), False), ("out",)))
                bufs[o["out"]] = f32(ref) if rnd else ref
            else:
                checks.append((stored_check(name, "conv", fam, ref, d, rnd), ("act", o["out"])))
                bufs[o["out"]] = bf16(ref) if rnd else ref
            if o["stats_gn"] >= 0:
                x = src(o["out"]) if stored is not None else bufs[o["out"]]
                path, D = stats_depth(fam, a.shape[1], a.shape[2], x.shape[-1])
                sref, sgate = stored_stats(x, D)
                checks.append((Check(name + ":stats", "stats " + path, fam, sref, sgate), ("stats", o["stats_gn"])))
                own_stats[o["stats_gn"]] = sref
        else:
            x = src(o["in"])
            if not o["stats_given"]:
                sref, sgate = stored_stats(x, D_STANDALONE_VEC if x.shape[-1] % 8 == 0 else D_STANDALONE)
                checks.append((Check(f"op{i}:gn{o['gn_id']}:stats", "stats standalone", "gn", sref, sgate), ("stats", o["gn_id"])))
                own_stats[o["gn_id"]] = sref
            st = stats[o["gn_id"]] if stats is not None else own_stats[o["gn_id"]]
            ref, d = gn_forward(x, st, P[names[o["w"]]], P[names[o["w"] + 1]], o["act"], 1e-6 if exact_gn else GN_EPS, exact_gn)
            checks.append((stored_check(f"op{i}:gn{o['gn_id']}:{names[o['w']][:-7]}", "gn+silu" if o["act"] else "gn", "gn", ref, d, rnd),
                           ("act", o["out"])))
            bufs[o["out"]] = bf16(ref) if rnd else ref
    return checks, bufs


def pack_checks(ops, names, P, rnd, pack_shapes):
    """The two packs of every convolution: pack_shapes {("wk" | "wkt", conv_id): (rows, Kp)} as the engine lays them out."""
    out = []
    for o in ops:
        if o["kind"] != OP_CONV:
            continue
        w = P[names[o["w"]]]
        for what, tr in (("wk", False), ("wkt", True)):
            shp = pack_shapes.get((what, o["conv_id"]))
            if shp is None:
                continue
            cin = shp[0] if tr else None
            w4 = w.reshape(w.shape[0], -1, o["ks"], o["ks"]) if w.dim() != 4 else w
            if tr:
                assert w4.shape[1] == cin
            out.append((exact_check(f"conv{o['conv_id']}:{what}", "pack", what, weight_pack(w4, shp[1], tr, rnd)), (what, o["conv_id"])))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
# Gates of the backward operations (same conventions; every input is the engine's own stored tensor at the moment the op ran, which the
# validation build's stop point tcvn_debug_sdxl_backward_stop makes readable):
#   * Data gradient  dIn[y][x][c] = sum_{ky,kx,n} dO[(y + pad - ky) / s][(x + pad - kx) / s][n] w[n][c][ky][kx], exact divisions only
#     (sdxl_ops.h:35).  One fp32 chain over at most K = ks ks Cout products (C64 / G on the transposed pack with flipped taps,
#     sdxl_conv3x3.hip:111 ring_load, :801-802; S2 per parity class with 1, 2 or 4 of the 9 taps, :477-490; generic sdxl_kernels.hip:213-223),
#     no bias (launch_c64 / launch_g get bias = nullptr: acc + 0.f is exact), and with `accumulate` one addition of the earlier gradient
#     (the residual operand of C64 / G, sdxl_conv3x3.hip:799; :458, :498 S2, both through cs_store8 :177-181; sdxl_kernels.hip:235 generic):
#         delta = R(K + acc) S,  S = sum |dO| |w| + |earlier|;  bf16 / fp32 store.
#   * Weight and bias gradient  dW[n][c][tap] = sum_m dO[m][n] a[m + shift(tap)][c],  db[n] = sum_m dO[m][n] over the M = n Ho Wo output
#     pixels: fp32 sums in some order (per-workgroup MFMA chains and slab partials, k_sub_reduce / slab_reduce, sdxl_conv3x3.hip:807-833;
#     fp32 atomics of the generic split-K kernel, sdxl_kernels.hip:332, :346-350; one wave per hit in sdxl_stem.hip) -- padding positions
#     and empty partials add exact zeros, so any order passes at most M roundings -- then the addition into the zeroed kernel-layout
#     gradient and the one of unpack_wgrads into the (zeroed) bound gradient (elementwise_bwd.hip:254):
#         delta = R(M + 2) sum |dO| |a|;  fp32 store.
#     Where the launch geometry is read off the launcher, the longest chain a product passes is far shorter than M and replaces it for the
#     weight (wgrad_depth): a tile-family workgroup keeps its accumulators over its tiles t = lb, lb + gx, ... (sdxl_conv3x3.hip:629-638;
#     256 positions per 8 x 32 tile, 64 per 2 x 32 stride-2 tile) and writes one slab; gx slabs are summed (k_slab_reduce / k_sub_reduce):
#         D = positions per tile * ceil(ntiles / gx) + gx,  gx = min(ntiles, 256) below 512 tiles else 512 for C64 (:813),
#         gx = max(1, min(512 / nsub, ntiles)) with nsub = Cin / 64 * Cout / 64 for G and S2 (:819-822), ntiles as wgrad_args counts (:776-780);
#     the generic kernel sums `rows` pixels per z-workgroup and adds `split` partials by atomics (sdxl_kernels.hip:717-727): D = rows + split.
#     The bias gradient and SCONV_IN's hit-list weight gradient keep M.
#   * GroupNorm backward (sdxl_kernels.hip:465-469, :493-499, :583-587, :632-636): xh = (x - mean) rstd (two roundings), u = xh gamma + beta
#     (du as forward), dU = dA dsilu(u) (dsilu_gate at u, |dsilu'| <= 1/2 times du for the argument, one multiplication),
#         e_dU = |dA| (gate_dsilu + du / 2) (1 + u) + u |dU|
#     bstats = (sum gamma dU, sum gamma dU xhat) per image: fp32 runs of at most 8 pixels x 8 channels, then double (:636-639, :651-655; the
#     strided kernel widens every term, :469):  gate1 = sum (|gamma| e_dU + u |gamma dU|) + R(64) sum |gamma dU|,
#         gate2 = sum (|xh| (|gamma| e_dU + u |gamma dU|) + R(3) |gamma dU xh|) + R(64) sum |gamma dU xh|.
#     dgamma = sum dU xh, dbeta = sum dU over all M = n HW pixels of a channel: per-thread fp32 partials, LDS float atomics, global float
#     atomics (:472, :477, :657, :661) -- any order, at most M roundings, into the zeroed gradient:
#         gate = sum (per-term error) + R(M + 1) sum |term|.
#     dX = rstd (gamma dU - c1 - xh c2), c1 = float(bstats0 / cnt), c2 = float(bstats1 / cnt) from the engine's OWN bstats (:488, :566):
#         e = rstd (|gamma| e_dU + (R(2) + u) |xh c2| + 3 u (|gamma dU| + |c1| + |xh c2|)) + u |dX|;  with `accumulate` ref = earlier + dX and
#         one more rounding u |ref|;  bf16 / fp32 store.
#   * Glue: cast_f32_to (sdxl_kernels.hip:669) one rounding of d_out; add_into (:676) one fp32 addition, then the store; a residual input
#     that takes over its output's region (sdxl.hip: std::swap(goff...)) or receives a copy holds dO bit for bit.
def conv_dgrad(dO, w, earlier, ks, stride, pad, in_hw, rnd, flip=True):
    """dO [n, Ho, Wo, Cout] stored; w [Cout, Cin, ks, ks] bound (rounded here); earlier [n, H, W, Cin] the gradient so far or None.
    flip=False: the DEFECT of taps that are not flipped.  -> ref, delta."""
    wr = bf16(w) if rnd else w
    n, Ho, Wo, Co = dO.shape
    H, W = in_hw
    Hp, Wp = max(H + 2 * ks, (Ho - 1) * stride + ks), max(W + 2 * ks, (Wo - 1) * stride + ks)

    def run(d, wt):
        acc = torch.zeros(n, Hp, Wp, wt.shape[1], dtype=d.dtype)
        for ky in range(ks):
            for kx in range(ks):
                k2, k3 = (ky, kx) if flip else (ks - 1 - ky, ks - 1 - kx)
                acc[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] += \
                    (d.reshape(-1, Co) @ wt[:, :, k2, k3]).reshape(n, Ho, Wo, -1)
        return acc[:, pad:pad + H, pad:pad + W].contiguous()
    ref, S = run(dO, wr), run(dO.abs(), wr.abs())
    if earlier is not None:
        ref, S = ref + earlier, S + earlier.abs()
    return ref, R(ks * ks * Co + (earlier is not None) + (0 if rnd else 1)) * S


def wgrad_depth(family, n, H, W, Ho, Wo, Cin, Cout, ks):
    """The longest fp32 chain a product of the weight gradient passes, from the launch geometry (see above); M for families without one."""
    M = n * Ho * Wo
    cdiv = lambda a, b: -(-a // b)
    if family == "c64":
        ntiles = n * cdiv(Wo, 32) * cdiv(Ho, 8)
        gx = min(ntiles, 256) if ntiles < 512 else 512
        return min(M, 256 * cdiv(ntiles, gx) + gx)
    if family in ("g", "s2"):
        nsub = (Cin // 64) * (Cout // 64)
        if family == "g":
            px, py = tile_map(H, W)
            tx, ty = (1 if px > 1 else cdiv(W, 32)), (1 if py > 1 else cdiv(H, 8))
            ntiles, ppt = cdiv(n, px * py) * tx * ty, 256
        else:
            ntiles, ppt = n * cdiv(Wo, 32) * cdiv(Ho, 2), 64
        gx = max(1, min(512 // nsub, ntiles))
        return min(M, ppt * cdiv(ntiles, gx) + gx)
    if family == "generic":
        Kp = cdiv(ks * ks * Cin, 32) * 32
        jt, it = cdiv(Kp, 128), cdiv(Cout, 32 if Cout <= 32 else 64 if Cout <= 64 else 128)
        split = max(1, min(cdiv(1024, jt * it), cdiv(M, 512)))
        rows = cdiv(cdiv(M, split), 32) * 32
        return min(M, rows + cdiv(M, rows))
    return M


def conv_wgrad(a, dO, ks, stride, pad, rnd, drop_partial=None, bias_times=1, depth=None):
    """a [n, H, W, Cin] the stored forward input, dO [n, Ho, Wo, Cout] stored.  depth: wgrad_depth(...) or None = M.  drop_partial = (lo, hi): the DEFECT of the output pixels
    [lo, hi) of the flattened map missing from the sum; bias_times: the DEFECT of a bias gradient counted that often.
    -> (dW [Cout, Cin, ks, ks], delta), (db [Cout], delta)."""
    n, H, W, C = a.shape
    _, Ho, Wo, Co = dO.shape
    ap = torch.zeros(n, max(H + pad + ks, (Ho - 1) * stride + ks), max(W + pad + ks, (Wo - 1) * stride + ks), C, dtype=a.dtype)
    ap[:, pad:pad + H, pad:pad + W] = a
    d = dO.reshape(-1, Co)
    M = d.shape[0]
    dd = d
    if drop_partial is not None:
        dd = d.clone()
        dd[drop_partial[0]:drop_partial[1]] = 0
    dW = torch.zeros(Co, C, ks, ks, dtype=a.dtype)
    S = torch.zeros_like(dW)
    for ky in range(ks):
        for kx in range(ks):
            sl = ap[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride].reshape(-1, C)
            dW[:, :, ky, kx] = dd.T @ sl
            S[:, :, ky, kx] = d.abs().T @ sl.abs()
    extra = 0 if rnd else 1
    return (dW, R((M if depth is None else depth) + 2 + extra) * S), (bias_times * dd.sum(0), R(M + 2) * d.abs().sum(0))


def kernel_layout(dW, Kp):
    """[Cout, Cin, ks, ks] -> the kernel layout [Cout][tap Cin + c] padded to Kp columns."""
    Co, C, kh, kw = dW.shape
    out = torch.zeros(Co, Kp, dtype=dW.dtype)
    out[:, :kh * kw * C] = dW.reshape(Co, C, kh * kw).permute(0, 2, 1).reshape(Co, -1)
    return out


def gn_backward(x, stats, gamma, beta, act, dA, bstats, earlier, eps=GN_EPS, exact=False):
    """x, dA [n, H, W, C] stored; stats, bstats [n, 2] the engine's own; earlier: the gradient so far (accumulate) or None.
    bstats = None: c1, c2 from the exact sums (for a chained use); exact: mean, rstd, c1, c2 not rounded to float (pin against autograd).
    -> dict name -> (ref, delta): "bstats" [n, 2], "dgamma", "dbeta" [C], "dx" [n, H, W, C]."""
    n, H, W, C = x.shape
    cnt = float(H * W * C)
    mean, rstd = mean_rstd(stats, cnt, eps, exact)
    mean, rstd = mean[:, None, None, None], rstd[:, None, None, None]
    xh = (x - mean) * rstd
    t = xh * gamma
    u = t + beta
    du = R(3) * t.abs() + R(1) * (t.abs() + beta.abs())
    if act:
        ds, gds = dsilu_gate(u)
        gds = gds + 0.5 * du
    else:
        ds, gds = torch.ones_like(u), torch.zeros_like(u)
    dU = dA * ds
    e_dU = dA.abs() * gds * (1 + U) + U * dU.abs()
    gdu = gamma * dU
    e_g = gamma.abs() * e_dU + U * gdu.abs()
    flat = lambda v: v.reshape(n, -1)
    b_ref = torch.stack([flat(gdu).sum(1), flat(gdu * xh).sum(1)], 1)
    b_gate = torch.stack([flat(e_g).sum(1) + (R(64) + 2.0 ** -48) * flat(gdu.abs()).sum(1),
                          flat(xh.abs() * e_g + R(3) * (gdu * xh).abs()).sum(1) + (R(64) + 2.0 ** -48) * flat((gdu * xh).abs()).sum(1)], 1)
    M = n * H * W
    ch = lambda v: v.reshape(-1, C)
    out = {"bstats": (b_ref, b_gate),
           "dgamma": (ch(dU * xh).sum(0), ch(xh.abs() * e_dU + R(3) * (dU * xh).abs()).sum(0) + R(M + 1) * ch((dU * xh).abs()).sum(0)),
           "dbeta": (ch(dU).sum(0), ch(e_dU).sum(0) + R(M + 1) * ch(dU.abs()).sum(0))}
    bs = b_ref if bstats is None else bstats
    c1, c2 = (bs[:, 0] / cnt)[:, None, None, None], (bs[:, 1] / cnt)[:, None, None, None]
    if not exact:
        c1, c2 = f32(c1), f32(c2)
    dx = rstd * (gdu - c1 - xh * c2)
    e = rstd * (e_g + (R(2) + U) * (xh * c2).abs() + 3 * U * (gdu.abs() + c1.abs() + (xh * c2).abs())) + U * dx.abs()
    if earlier is not None:
        dx = earlier + dx
        e = e + U * dx.abs()
    out["dx"] = (dx, e)
    return out


def run_backward(ops, names, P, bufs, d_out):
    """The whole backward in float64 without rounding, chained from d_out [n, out]: bufs = what run_forward returned with rnd off and
    exact_gn.  -> parameter gradients by slot name (to_q / to_k receive none)."""
    g, grads = {ops[-1]["out"]: d_out.reshape(bufs[ops[-1]["out"]].shape)}, {}
    chan = {b: t.shape[-1] for b, t in bufs.items()}
    for o in reversed(ops):
        dO = g[o["out"]]
        if o["kind"] == OP_CONV:
            w, _ = conv_weight(P, names, o, chan)
            (dW, _), (db, _) = conv_wgrad(bufs[o["in"]], dO, o["ks"], o["stride"], o["pad"], False)
            grads[names[o["w"]]], grads[names[o["w"] + 1]] = dW.reshape(P[names[o["w"]]].shape), db
            if o["in"]:
                g[o["in"]], _ = conv_dgrad(dO, w, g.get(o["in"]), o["ks"], o["stride"], o["pad"], bufs[o["in"]].shape[1:3], False)
            if o["res"] >= 0:
                g[o["res"]] = g[o["res"]] + dO if o["res"] in g else dO
        else:
            st, _ = stored_stats(bufs[o["in"]], 0)
            r = gn_backward(bufs[o["in"]], st, P[names[o["w"]]], P[names[o["w"] + 1]], o["act"], dO, None, g.get(o["in"]), 1e-6, True)
            grads[names[o["w"]]], grads[names[o["w"] + 1]], g[o["in"]] = r["dgamma"][0], r["dbeta"][0], r["dx"][0]
    return grads


# ---------------------------------------------------------------------------------------------------------------------
# nothing else changes (forward): what an op stores OUTSIDE its own buffer
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def changed_outside(ws_bytes, produced, lo, hi):
    """ws_bytes: uint8 view of a workspace that held SENTINEL in every byte of [lo, hi) before the ops ran; produced: [(byte offset, bytes)]
    of the buffers those ops own.  -> number of bytes outside them that no longer hold the sentinel (0 for a correct kernel).  A store
    into an image slot img >= n of a half-filled packed tile lands behind the last image of the op's output: in the alignment gap and the
    buffers that follow, which a later op overwrites -- so the predicate is evaluated after EVERY op (forward stop point), and over the gaps
    alone where no stop point exists."""
    t = ws_bytes[lo:hi].clone()
    for off, nb in produced:
        t[max(off, lo) - lo: max(off + nb, lo) - lo] = SENTINEL
    return int((t != SENTINEL).sum())


def replay_goff(ops, nominal, same_shape):
    """The gradient regions of a whole backward, replayed from the tape as tcvn_sdxl::backward walks it (sdxl.hip backward(): `goff`,
    `written`, the std::swap for the first contribution to a residual input of its output's shape): ops in tape order; nominal {buffer: byte
    offset of its nominal gradient region}; same_shape(a, b) whether two buffers have one shape.
    -> read {op index: offset of the region the op read dO from}, intact {op index: no op processed later writes that region, so it still
    holds that dO when the whole backward has returned}."""
    goff = dict(nominal)
    written = {ops[-1]["out"]}
    read, writes = {}, []                                              # writes: (index of the writing op, region)
    for i in range(len(ops) - 1, -1, -1):
        o = ops[i]
        assert o["out"] in written
        read[i] = goff[o["out"]]
        if o["in"] != 0:                                               # GroupNorm dX / convolution data gradient: written or accumulated
            writes.append((i, goff[o["in"]]))
            written.add(o["in"])
        r = o["res"]
        if r >= 0:
            if r in written:
                writes.append((i, goff[r]))                            # add_into
            elif same_shape(r, o["out"]):
                goff[r], goff[o["out"]] = goff[o["out"]], goff[r]      # takes the region over: no store
            else:
                writes.append((i, goff[r]))                            # copy
            written.add(r)
    intact = {i: not any(j < i and reg == read[i] for j, reg in writes) for i in read}
    return read, intact


# the shapes of test_sdxl_ops_float64_gpu.py (n, H, W), shared with the CPU test so that both see the same inputs
CASES = {"A": (11, 44, 72), "B": (11, 36, 100), "C": (5, 52, 60), "D": (70, 12, 20), "E": (6, 120, 184)}
BORDER_MAP, EMPTY_MAP = 1, 3          # the map that gets hits on its corners and edges; the map of case D without any hit


def case_inputs(name, seed=6):
    """-> (n, H, W), coords int32 [nnz, 3] (image, y, x; one entry per pixel, ordered), values fp32 [nnz, 3] in 1 .. 255: the oracle's
    synthetic prong maps, plus hits at the four corners and the middle of each edge of map BORDER_MAP; case D's map EMPTY_MAP has none."""
    import numpy as np
    from oracle import tcvn_oracle as O
    n, H, W = CASES[name]
    cfg = O.tutorial_config(embedder="sdxl", pixel_shape=(H, W))
    batch = O.synthetic_batch([n], seed, cfg, event_hits=(20, min(800, H * W // 4)), prong_hits=(20, min(800, H * W // 4)))
    coords, values = batch[5].numpy(), batch[6].numpy()
    hits = {(int(i), int(y), int(x)): v for (i, y, x), v in zip(coords, values)}
    rng = np.random.Generator(np.random.Philox(key=seed + 1000))
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        hits[(BORDER_MAP, y, x)] = rng.integers(1, 256, size=3).astype(np.float32)
    if name == "D":
        hits = {k: v for k, v in hits.items() if k[0] != EMPTY_MAP}
    keys = sorted(hits)
    return (n, H, W), torch.tensor(keys, dtype=torch.int32), torch.from_numpy(np.stack([hits[k] for k in keys]))


def dense_image(shape, coords, values):
    """values / 255 scattered into [n, H, W, 3], float64, unrounded."""
    n, H, W = shape
    img = torch.zeros(n, H, W, values.shape[1], dtype=torch.float64)
    c = coords.long()
    img[c[:, 0], c[:, 1], c[:, 2]] = values.double() / 255.0
    return img


def worst_table(rows):
    """rows [(kind, family, worst ratio)] -> {(kind, family): worst} and a printable table."""
    tab = {}
    for kind, fam, w in rows:
        tab[(kind, fam)] = max(tab.get((kind, fam), 0.0), w)
    text = "\n".join(f"  {k:<18} {f:<8} {w:.3f}" for (k, f), w in sorted(tab.items()))
    return tab, text
