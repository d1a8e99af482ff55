"""Float64 restatement of the noise-averaged hit gradients (tests only, numpy): the Philox-4x32-10 call, the Box-Muller step, the noise
scale of a map, the perturbed values, the replicated hit list and the statistics over the samples.

Error bound of the statistics (`stat_bounds`).  `welford` is the update the device runs: mean_t = mean_{t-1} + (x_t - mean_{t-1}) / t,
M2_t = M2_{t-1} + (x_t - mean_{t-1}) (x_t - mean_t), in double, t ascending.  Every step is a handful of double operations on numbers no
larger than 2 max|x| (the mean is a convex combination of the samples) and, for M2, no larger than 4 max|x|^2 per term, T max-terms in
all.  With u = 2^-53, X = max_t |x_t| and T samples, first-order rounding analysis (Chan, Golub & LeVeque 1983, section 3, for the
updating formulas) gives
    |mean - exact|      <=  4 T u X
    |M2 - exact|        <= 16 T^2 u X^2     hence   |var - exact| <= 16 T^2 u X^2 / (T - 1)   and
    |mean_sq - exact|   <= 16 T u X^2 + 8 T u X^2 = 24 T u X^2      (mean^2 + M2 / T, both terms non-negative: no cancellation).
The bounds are crude (the constants cover a fused or an unfused multiply-add alike and the error of `numpy.var` itself) and still ten
orders of magnitude under the fp32 rounding of the results, which the comparisons add on top as 2^-24 of the value."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM = 0x4E54554E
MASK = np.uint64(0xFFFFFFFF)


def philox4(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on arrays of 32-bit words (broadcast) -> (w0, w1, w2, w3) as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def draw(seed, t, q, m, c):
    """The standard normal of (sample t, pixel q = y * W + x, map m = b * (1 + P) + s, channel c), float64; arguments broadcast."""
    t, q, m, c = np.broadcast_arrays(np.asarray(t, dtype=np.int64), np.asarray(q, dtype=np.int64), np.asarray(m, dtype=np.int64),
                                     np.asarray(c, dtype=np.int64))
    w = philox4(q, m, t, STREAM + (c >> 2), seed & 0xFFFFFFFF, seed >> 32)
    second = ((c & 3) >> 1) == 1
    wa = np.where(second, w[2], w[0]).astype(np.float64)
    wb = np.where(second, w[3], w[1]).astype(np.float64)
    u1, u2 = (wa + 1.0) * 2.0 ** -32, wb * 2.0 ** -32
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return rad * np.where((c & 1) == 1, np.sin(ang), np.cos(ang))


def inside(coords, n_img, H, W):
    c = np.asarray(coords, dtype=np.int64)
    return (c[:, 0] >= 0) & (c[:, 0] < n_img) & (c[:, 1] >= 0) & (c[:, 1] < H) & (c[:, 2] >= 0) & (c[:, 2] < W)


def sigma(coords, values, n_img, shape, img_bs, B, P, noise, out=None):
    """sigma [B, 1 + P] float32 = noise * (max(0, max v) - min(0, min v)) per map of this list; slots no image names keep `out` (default NaN);
    a map without hits 0.  The range is exact in double (two fp32 numbers added), the product is rounded to fp32 once."""
    out = np.full((B, 1 + P), np.nan, dtype=np.float32) if out is None else out
    c, v = np.asarray(coords, dtype=np.int64), np.asarray(values, dtype=np.float32).astype(np.float64)
    ok = inside(c, n_img, *shape)
    for img in range(n_img):
        b, s = (int(k) for k in img_bs[img])
        vv = v[ok & (c[:, 0] == img)]
        hi = max(0.0, float(np.nanmax(vv))) if vv.size and not np.isnan(vv).all() else 0.0
        lo = min(0.0, float(np.nanmin(vv))) if vv.size and not np.isnan(vv).all() else 0.0
        out[b, s] = np.float32(float(noise) * (hi - lo))
    return out


def replicate(coords, values, n_img, shape, img_bs, P, sig, seed, t0, reps):
    """Samples t0 .. t0 + reps - 1 of one hit list as one list over reps * n_img images -> (coords [reps * nnz, 3] int32, perturbed values
    [reps * nnz, C] float32, the same in float64 before the last rounding).  v' = max(v + sigma z, 0) in double, rounded to fp32 once;
    where sigma is 0 or the entry lies outside the maps, v' = v bit for bit.  An image index outside 0 .. n_img - 1 becomes -1."""
    c = np.asarray(coords, dtype=np.int64)
    v32 = np.asarray(values, dtype=np.float32)
    nnz, C = v32.shape
    H, W = shape
    ok = inside(c, n_img, H, W)
    img = np.where(ok, c[:, 0], 0)
    bs = np.asarray(img_bs, dtype=np.int64).reshape(-1, 2)
    m = bs[img, 0] * (1 + P) + bs[img, 1]
    sg = np.where(ok, np.asarray(sig, dtype=np.float32).reshape(-1)[m].astype(np.float64), 0.0)
    sg = np.where(sg > 0, sg, 0.0)                                  # (a NaN or zero sigma perturbs nothing)
    q = c[:, 1] * W + c[:, 2]
    out_c = np.empty((reps, nnz, 3), dtype=np.int32)
    out_v = np.empty((reps, nnz, C), dtype=np.float64)
    bad_img = (c[:, 0] < 0) | (c[:, 0] >= n_img)
    for r in range(reps):
        out_c[r, :, 0] = np.where(bad_img, -1, c[:, 0] + r * n_img)
        out_c[r, :, 1:] = c[:, 1:]
        z = draw(seed, t0 + r, q[:, None], m[:, None], np.arange(C)[None, :])
        out_v[r] = np.maximum(v32.astype(np.float64) + sg[:, None] * z, 0.0)
    v_out = out_v.astype(np.float32)
    keep = np.broadcast_to((sg == 0)[None, :, None], v_out.shape)
    v_out = np.where(keep, np.broadcast_to(v32[None], v_out.shape), v_out)
    out_v = np.where(keep, np.broadcast_to(v32[None].astype(np.float64), out_v.shape), out_v)
    return out_c.reshape(reps * nnz, 3), v_out.reshape(reps * nnz, C), out_v.reshape(reps * nnz, C)


def ulp32(x):
    """The spacing of fp32 at |x| (float64 array): one unit in the last place."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def welford(x):
    """x [T, ...] float64 -> (mean, M2) by the update the device runs, t ascending (see the module docstring)."""
    x = np.asarray(x, dtype=np.float64)
    mean, m2 = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for t in range(x.shape[0]):
        d = x[t] - mean
        mean = mean + d / float(t + 1)
        m2 = m2 + d * (x[t] - mean)
    return mean, m2


def stats(x):
    """x [T, ...] -> (mean, unbiased variance (NaN at T = 1), mean square) in float64."""
    T = np.asarray(x).shape[0]
    mean, m2 = welford(x)
    var = m2 / (T - 1) if T > 1 else np.full_like(m2, np.nan)
    return mean, var, mean * mean + m2 / T


def stat_bounds(x):
    """The absolute error bounds of (mean, variance, mean square) stated in the module docstring, per element."""
    x = np.asarray(x, dtype=np.float64)
    T, u = x.shape[0], 2.0 ** -53
    X = np.abs(x).max(0)
    return 4 * T * u * X, 16 * T * T * u * X * X / max(T - 1, 1), 24 * T * u * X * X


def within(got32, ref64, bound):
    """got (fp32 from the device) against the float64 reference: the double-precision bound plus one fp32 rounding of the result (half an
    ulp, or the smallest subnormal where the result underflows)."""
    got, ref = np.asarray(got32, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    tol = bound + np.maximum(2.0 ** -24 * np.abs(ref), 2.0 ** -149)
    return np.abs(got - ref) <= tol
