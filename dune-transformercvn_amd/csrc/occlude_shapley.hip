// Tile Shapley values (forward only): the class score of a pixel map shared among its n tiles that hold a hit.  A coalition is "this map
// with only the hits of these tiles", the replacement occlude.hip makes.  Maps with 1 <= n <= max_exact run all 2^n - 1 coalitions but the
// full one (coalition k: bit i = the i-th occupied tile in ascending tile index); wider maps run the empty map and the prefixes 1 .. n - 1
// of `samples` permutations drawn on the device.  As in occlude_curve.hip a permutation is a sort of 64-bit words (Philox key, tile index)
// that are all different, the only atomics are the integer ones of the occupancy count, and every sum is taken in a fixed order in double
// precision: two runs give the same bits.
#include "../../include/tcvn_hip.h"
#include "occlude_list.h"

namespace tcvn {

namespace {

constexpr uint32_t kTileShapStream = 0x54534850u;   // Philox stream constant of the tile permutation keys ("TSHP")
constexpr int RT = 1024;                            // threads of a rank workgroup
constexpr int VT = 256, VW = VT / 64;               // threads and waves of a values workgroup
constexpr int POS_WORDS = 16384;                    // 16-bit inverse-permutation entries a values workgroup keeps in LDS
constexpr unsigned long long NO_TILE = ~0ull;

bool shap_ok(int samples, int max_exact) {
    return samples >= 1 && samples <= TCVN_TSHAP_MAX_SAMPLES && max_exact >= 0 && max_exact <= TCVN_TSHAP_MAX_EXACT;
}

// ---- workspace: the list core's members (occlude_list.h) with rank = the int16 table [n_img][M][T], prefix = int32 [n_img][M][T + 1] (hits
// of the first r tiles of permutation m), nocc = n per map, and behind them ord [n_img][T] (ordinal of a tile among the occupied ones, -1),
// mode [n_img] (1: exact) and tiles [n_img][TCVN_TSHAP_MAX_EXACT] (the first occupied tiles, ascending).  R: candidate rows per map.
struct ShapLayout { ListLayout l; long ord, mode, tiles, R; };
bool shap_layout(int n_img, int H, int W, int th, int tw, int M, int E, int max_pass, ShapLayout& s) {
    s = ShapLayout{};
    ListLayout& o = s.l;
    if (n_img < 1 || H < 1 || W < 1 || th < 1 || tw < 1 || max_pass < 1 || max_pass > TCVN_OCC_MAX_PASS || !shap_ok(M, E)) return false;
    const long Ht = (H + th - 1) / th, Wt = (W + tw - 1) / tw, T = Ht * Wt;
    if (T > TCVN_TSHAP_MAX_TILES) return false;
    const long exact_rows = (1L << E) - 1, sampled_rows = 1 + (long)M * (T - 1);
    s.R = exact_rows > sampled_rows ? exact_rows : sampled_rows;
    o.cells = (long)n_img * T;
    o.rows = (long)n_img * s.R;
    if (o.cells > 0x7fffffffL - 1024 || o.rows > 0x7fffffffL - 1024) return false;
    o.Wt = (int)Wt; o.T = (int)T;
    o.nb = (int)((o.rows + max_pass - 1) / max_pass);
    long off = 0;
    auto take = [&](long bytes) { long at = off; off += round_up(bytes, 256); return at; };
    o.cnt = take(o.cells * 4); o.nnz_img = take((long)n_img * 4); o.flags = take(16); o.img_start = take(((long)n_img + 1) * 8);
    o.rank = take(o.cells * M * 2); o.prefix = take((long)n_img * M * (T + 1) * 4); o.nocc = take((long)n_img * 4);
    s.ord = take(o.cells * 4); s.mode = take((long)n_img * 4); s.tiles = take((long)n_img * TCVN_TSHAP_MAX_EXACT * 4);
    o.payload = take(o.rows * 4); o.voff = take((o.rows + 1) * 8); o.hdr = take((4L + o.nb + 1) * 8);
    o.total = off;
    return true;
}

// ---- 1. rank: one workgroup per (permutation m, map) sorts the keys of the map's occupied tiles in LDS (bitonic, ascending) ----------------
// word = key << 32 | tile with key = word 0 of philox4(tile, m, b * S + s, stream; seed).  Tiles without hits (and the padding up to N, the
// power of two >= T) carry the largest word; no occupied tile can (its low word < T).  The workgroup of m = 0 also writes what does not
// depend on m: n, the mode, ord and the first occupied tiles.
__global__ __launch_bounds__(RT) void k_tshap_rank(const int* __restrict__ cnt, const int* __restrict__ img_bs, int B, int S, int T, int N,
                                                   int M, int E, uint64_t seed, short* rank, int* prefix, int* nocc, int* ord, int* mode,
                                                   int* tiles, int* perms, int* n_tiles, int* exact) {
    __shared__ unsigned long long key[TCVN_TSHAP_MAX_TILES];
    __shared__ long wsum[RT / 64];
    const int img = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;     // grid.y holds at most 65 535 blocks: samples, not the maps
    const int b = img_bs[2 * img], s = img_bs[2 * img + 1];
    const bool named = b >= 0 && b < B && s >= 0 && s < S;                   // a map the outputs have no row for has no player
    const long map = named ? (long)b * S + s : 0;
    const int* c = cnt + (long)img * T;
    short* rk = rank + ((long)img * M + m) * T;
    for (int t = tid; t < N; t += RT) {
        unsigned long long k = NO_TILE;
        if (t < T) {
            rk[t] = -1;
            if (named && c[t] > 0)
                k = ((unsigned long long)philox4((uint32_t)t, (uint32_t)m, (uint32_t)map, kTileShapStream, (uint32_t)seed,
                                                 (uint32_t)(seed >> 32)).x << 32) | (unsigned)t;
        }
        key[t] = k;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= N; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += RT) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = key[i], z = key[l];
                    if ((a > z) == ((i & k2) == 0)) { key[i] = z; key[l] = a; }
                }
            }
            __syncthreads();
        }
    // the occupied tiles now stand in front, in the order of the permutation: rank, the permutation and prefix[r] (r = 0..T)
    long carry = 0, tot;
    for (int base = 0; base <= T; base += RT) {
        const int i = base + tid;
        const unsigned long long k = i < T ? key[i] : NO_TILE;
        const int tile = (int)(k & 0xffffffffull);
        const long v = k != NO_TILE ? c[tile] : 0;
        const long ex = block_scan_excl(v, wsum, tot);
        if (i <= T) prefix[((long)img * M + m) * (T + 1) + i] = (int)(carry + ex);
        if (k != NO_TILE) rk[tile] = (short)i;
        if (named && i < T) perms[(map * M + m) * T + i] = k != NO_TILE ? tile : -1;
        carry += tot;
    }
    if (m != 0) return;                                                      // the whole workgroup: no barrier below is skipped by a part
    carry = 0;
    for (int base = 0; base < T; base += RT) {
        const int t = base + tid;
        const bool occ = t < T && named && c[t] > 0;
        const long ex = block_scan_excl(occ ? 1 : 0, wsum, tot);
        if (t < T) ord[(long)img * T + t] = occ ? (int)(carry + ex) : -1;
        if (occ && carry + ex < TCVN_TSHAP_MAX_EXACT) tiles[(long)img * TCVN_TSHAP_MAX_EXACT + carry + ex] = t;
        carry += tot;
    }
    if (tid == 0) {
        const int n = (int)carry, ex = n >= 1 && n <= E ? 1 : 0;
        nocc[img] = n; mode[img] = ex;
        if (named) { n_tiles[map] = n; exact[map] = ex; }
    }
}

// ---- 2-3. the variant list (occlude_list.h): a row is an (image, m, k) candidate -----------------------------------------------------------
// Row r of a map: exact maps, coalition r < 2^n - 1; sampled maps, r = 0 the empty map and r = 1 + m (T - 1) + (k - 1) the prefix of length
// k = 1 .. n - 1 of permutation m.  The surviving hits are a sum over the set bits / a prefix sum along the permutation.
__global__ __launch_bounds__(LIST_T) void k_tshap_list(const int* __restrict__ cnt, const int* __restrict__ nnz_img, const int* flags,
                                                       const int* __restrict__ img_bs, const int* __restrict__ prefix,
                                                       const int* __restrict__ nocc, const int* __restrict__ mode,
                                                       const int* __restrict__ tiles, int n_img, int T, int M, long R, int max_pass,
                                                       long* img_start, int* vimg, int* payload, long* voff, int* index, long* hdr) {
    auto row = [=](long c) {
        const int img = (int)(c / R), n = nocc[img];
        const long r = c - (long)img * R;
        if (n < 1) return ListRow{false, 0, img, 0, 0, 0};
        if (mode[img]) {
            long surv = 0;
            for (int i = 0; i < n; ++i)
                if ((r >> i) & 1) surv += cnt[(long)img * T + tiles[(long)img * TCVN_TSHAP_MAX_EXACT + i]];
            return ListRow{r < (1L << n) - 1, surv, img, (int)r, 0, (int)r};
        }
        if (r == 0) return ListRow{true, 0, img, 0, 0, 0};
        if (T < 2) return ListRow{false, 0, img, 0, 0, 0};
        const int m = (int)((r - 1) / (T - 1)), k = (int)(r - 1 - (long)m * (T - 1)) + 1;
        if (m >= M || k > n - 1) return ListRow{false, 0, img, 0, 0, 0};
        return ListRow{true, (long)prefix[((long)img * M + m) * (T + 1) + k], img, m * (T + 1) + k, m, k};
    };
    variant_list(row, (long)n_img * R, nnz_img, flags, img_bs, n_img, max_pass, img_start, vimg, payload, voff, index, hdr);
}
// exact: the coalition holds the tile whose ordinal is a set bit of the payload; sampled: the payload is m (T + 1) + k and the prefix of
// length k holds the tiles ranked below k in permutation m.  A hit outside the map is dropped.
struct KeepCoalition {
    const short* rank; const int* ord; const int* mode; int T, M;
    __device__ bool operator()(bool in, int cell, int img, int word) const {
        if (!in) return false;
        if (mode[img]) {
            const int o = ord[(long)img * T + cell];
            return o >= 0 && o < TCVN_TSHAP_MAX_EXACT && ((word >> o) & 1) != 0;
        }
        const int m = word / (T + 1), k = word - m * (T + 1);
        if (m < 0 || m >= M) return false;
        const int r = rank[((long)img * M + m) * T + cell];
        return r >= 0 && r < k;
    }
};

// ---- 4. values ------------------------------------------------------------------------------------------------------------------------------
// the first variant of every map (index is ordered by map) and the value of every variant in double
__global__ __launch_bounds__(256) void k_tshap_value(const float* base_ev, const float* base_pr, const float* var_ev, const float* var_pr,
                                                     const int* index, long V, int B, int P, int Ce, int Cp, int prong, const int* cls,
                                                     int logit, long* start, double* vals) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int b = index[4 * v], s = index[4 * v + 1];
    vals[v] = __builtin_nan("");
    if (b < 0 || b >= B || s < 0 || s > P) return;
    if (v == 0 || index[4 * (v - 1)] != b || index[4 * (v - 1) + 1] != s) start[(long)b * (1 + P) + s] = v;
    const float *a, *o;
    int C, c;
    if (!class_choice(base_ev, base_pr, var_ev, var_pr, v, b, s, P, Ce, Cp, prong, cls, a, o, C, c)) return;
    vals[v] = logit ? (double)o[c] : softmax_at(o, C, c);
}
__device__ __forceinline__ long ins0(long r, int i) { return ((r >> i) << (i + 1)) | (r & ((1L << i) - 1)); }         // a zero bit at i
// |C|! (n - |C| - 1)! / n! = 1 / (n C(n - 1, |C|))
__device__ __forceinline__ double shap_weight(int n, int c) {
    double comb = 1.0;
    for (int j = 1; j <= c; ++j) comb = comb * (double)(n - 1 - c + j) / (double)j;         // an integer at every step
    return 1.0 / ((double)n * comb);
}
// one workgroup per map (b, s).  n_tiles < 0: a padded slot or a map not scanned, NaN.  Exact: wave w takes the players w, w + VW, ...,
// its lanes stride over the 2^(n-1) coalitions without the player, xor shuffles add them up.  Sampled: thread t takes the tiles t, t + VT,
// ... and walks the permutations in their order, twice (mean, then squared deviations); the position of a tile in a permutation comes
// from an inverse table that is built in LDS for as many permutations at a time as fit.
__global__ __launch_bounds__(VT) void k_tshap_phi(const float* base_ev, const float* base_pr, const int* __restrict__ exact,
                                                  const int* __restrict__ n_tiles, const int* __restrict__ perms,
                                                  const long* __restrict__ start, const double* __restrict__ vals, long V, int P, int Ce,
                                                  int Cp, int T, int M, int prong, const int* cls, int logit, float* phi, float* se,
                                                  double* full, double* empty) {
    __shared__ double vs[1 << TCVN_TSHAP_MAX_EXACT], W1[TCVN_TSHAP_MAX_EXACT + 1];
    __shared__ short pos[POS_WORDS];
    __shared__ int player[TCVN_TSHAP_MAX_EXACT];
    const long map = blockIdx.x;
    const int S = 1 + P, b = (int)(map / S), s = (int)(map - (long)b * S), tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = n_tiles[map];
    float* ph = phi + map * T;
    float* sd = se + map * T;
    const float nanf_ = __uint_as_float(0x7fc00000u);
    // the value of the map as it is, from the logits of the forward being explained
    double vfull = __builtin_nan("");
    bool have = n >= 0 && !(prong && s == 0);
    if (have) {
        const float* a = prong ? base_pr + ((long)b * P + (s - 1)) * Cp : base_ev + (long)b * Ce;
        const int C = prong ? Cp : Ce, c = prong || !cls ? argmax_row(a, C) : cls[b];
        have = c >= 0 && c < C;
        if (have) vfull = logit ? (double)a[c] : softmax_at(a, C, c);
    }
    const long st = have && n > 0 ? start[map] : -1;
    const long need = n < 1 ? 0 : exact[map] ? (1L << n) - 1 : 1 + (long)M * (n - 1);
    if (!have || n > T || (n > 0 && (st < 0 || st + need > V)) || (n > 0 && exact[map] && n > TCVN_TSHAP_MAX_EXACT)) {
        for (int t = tid; t < T; t += VT) { ph[t] = nanf_; sd[t] = nanf_; }      // nothing to compare (or a list that does not fit)
        if (tid == 0) { full[map] = __builtin_nan(""); empty[map] = __builtin_nan(""); }
        return;
    }
    for (int t = tid; t < T; t += VT) { ph[t] = 0.f; sd[t] = 0.f; }
    if (tid == 0) { full[map] = vfull; empty[map] = n > 0 ? vals[st] : vfull; }
    if (n == 0) return;
    const int* pm = perms + map * (long)M * T;
    __syncthreads();                                                         // the zeros stand before any player's value is written
    if (exact[map]) {
        const long all = (1L << n) - 1;
        for (long k = tid; k <= all; k += VT) vs[k] = k < all ? vals[st + k] : vfull;
        if (tid < TCVN_TSHAP_MAX_EXACT) player[tid] = -1;                    // permutations that do not list n tiles leave a player out
        __syncthreads();
        if (tid < n) {
            W1[tid] = shap_weight(n, tid);
            int o = 0;                                                       // the ordinal of the tile at position tid of permutation 0
            for (int j = 0; j < n; ++j) o += pm[j] < pm[tid] ? 1 : 0;
            player[o] = pm[tid];
        }
        __syncthreads();
        const long half = 1L << (n - 1);
        for (int i = w; i < n; i += VW) {
            const long bi = 1L << i;
            double acc = 0.0;
            for (long r = lane; r < half; r += 64) {
                const long k = ins0(r, i);
                acc += W1[__popcll((unsigned long long)k)] * (vs[k | bi] - vs[k]);
            }
            acc = wave_sum(acc);
            const int t = player[i];
            if (lane == 0 && t >= 0 && t < T) ph[t] = (float)acc;
        }
        return;
    }
    // sampled: prefix k of permutation m is variant st + 1 + m (n - 1) + k - 1; prefix 0 the empty map, prefix n the map as it is
    const double vempty = vals[st];
    const int chunk = POS_WORDS / T < M ? POS_WORDS / T : M;                 // T <= 1024: at least 16 permutations at a time
    double mean[TCVN_TSHAP_MAX_TILES / VT], acc[TCVN_TSHAP_MAX_TILES / VT];
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int q = 0; q < TCVN_TSHAP_MAX_TILES / VT; ++q) acc[q] = 0.0;
        for (int m0 = 0; m0 < M; m0 += chunk) {
            const int mc = M - m0 < chunk ? M - m0 : chunk;
            __syncthreads();                                                 // the previous chunk's table has been read
            for (int e = tid; e < mc * T; e += VT) pos[e] = -1;
            __syncthreads();
            for (int e = tid; e < mc * n; e += VT) {
                const int mi = e / n, j = e - mi * n, t = pm[(long)(m0 + mi) * T + j];
                if (t >= 0 && t < T) pos[mi * T + t] = (short)j;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < TCVN_TSHAP_MAX_TILES / VT; ++q) {
                const int t = q * VT + tid;
                if (t >= T) continue;
                for (int mi = 0; mi < mc; ++mi) {
                    const int j = pos[mi * T + t];
                    if (j < 0) continue;                                     // no player: in every permutation alike
                    const long row = st + 1 + (long)(m0 + mi) * (n - 1);
                    const double lo = j == 0 ? vempty : vals[row + j - 1], hi = j + 1 == n ? vfull : vals[row + j];
                    const double d = hi - lo;
                    acc[q] += pass == 0 ? d : (d - mean[q]) * (d - mean[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < TCVN_TSHAP_MAX_TILES / VT; ++q) {
            const int t = q * VT + tid;
            if (t >= T || pos[t] < 0) continue;                              // the last chunk's table is still there: pos[t] is its row 0
            if (pass == 0) { mean[q] = acc[q] / (double)M; ph[t] = (float)mean[q]; }
            else sd[t] = M > 1 ? (float)sqrt(acc[q] / (double)(M - 1) / (double)M) : 0.f;
        }
    }
}
__global__ __launch_bounds__(256) void k_tshap_clear(long* start, long maps) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < maps) start[i] = -1;
}

}  // namespace

}  // namespace tcvn

using namespace tcvn;

extern "C" {

int64_t tcvn_occlusion_shapley_workspace_bytes(int n_img, int height, int width, int tile_h, int tile_w, int samples, int max_exact,
                                               int max_pass) {
    ShapLayout s;
    return shap_layout(n_img, height, width, tile_h, tile_w, samples, max_exact, max_pass, s) ? s.l.total : -1;
}

int tcvn_occlusion_shapley_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                                    const int32_t* img_bs, int batch, int max_prongs, int samples, int max_exact, uint64_t seed,
                                    int32_t* permutations, int32_t* n_tiles, int32_t* exact, int max_pass, int32_t* vimg, int32_t* index,
                                    void* workspace, int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream) {
    const char* who = "occlusion_shapley_variants";
    ShapLayout s;
    if (!list_pointers_ok(coords, nnz, img_bs, vimg, index, workspace, host_out) || !permutations || !n_tiles || !exact || batch < 1 ||
        max_prongs < 0 || !shap_layout(n_img, height, width, tile_h, tile_w, samples, max_exact, max_pass, s)) {
        fprintf(stderr, "tcvn: %s: bad argument (NULL pointer, n_img / map / tile / batch < 1, samples outside 1..%d, max_exact outside 0..%d, max_pass outside 1..%d or more than %d tiles per map)\n",
                who, TCVN_TSHAP_MAX_SAMPLES, TCVN_TSHAP_MAX_EXACT, TCVN_OCC_MAX_PASS, TCVN_TSHAP_MAX_TILES);
        return -1;
    }
    const ListLayout& o = s.l;
    if (int rc = list_room(who, o, workspace_bytes, host_cap)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* w = reinterpret_cast<char*>(workspace);
    const int T = o.T;
    int N = 2;
    while (N < T) N <<= 1;
    const int* cnt = reinterpret_cast<const int*>(w + o.cnt);
    const int* nnz_img = reinterpret_cast<const int*>(w + o.nnz_img);
    int* prefix = reinterpret_cast<int*>(w + o.prefix);
    int* nocc = reinterpret_cast<int*>(w + o.nocc);
    int* mode = reinterpret_cast<int*>(w + s.mode);
    int* tiles = reinterpret_cast<int*>(w + s.tiles);
    if (int rc = list_count(o, w, coords, nnz, n_img, height, width, tile_h, tile_w, img_bs, nullptr, 0, 0, 0, 0, st)) return rc;
    hipLaunchKernelGGL(k_tshap_rank, dim3(n_img, samples), dim3(RT), 0, st, cnt, img_bs, batch, 1 + max_prongs, T, N, samples, max_exact,
                       seed, reinterpret_cast<short*>(w + o.rank), prefix, nocc, reinterpret_cast<int*>(w + s.ord), mode, tiles,
                       permutations, n_tiles, exact);
    TCVN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tshap_list, dim3(1), dim3(LIST_T), 0, st, cnt, nnz_img, reinterpret_cast<const int*>(w + o.flags), img_bs, prefix,
                       nocc, mode, tiles, n_img, T, samples, s.R, max_pass, reinterpret_cast<long*>(w + o.img_start), vimg,
                       reinterpret_cast<int*>(w + o.payload), reinterpret_cast<long*>(w + o.voff), index,
                       reinterpret_cast<long*>(w + o.hdr));
    TCVN_LAUNCH_CHECK();
    return list_read_header(o, w, host_out, st);
}

int tcvn_occlusion_shapley_build(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height, int width,
                                 int tile_h, int tile_w, int samples, int max_exact, int max_pass, const int32_t* vimg,
                                 const void* workspace, int64_t workspace_bytes, int first, int count, int32_t* out_coords,
                                 float* out_values, int64_t out_rows, void* stream) {
    ShapLayout s;
    if (!build_args_ok(coords, values, nnz, channels, vimg, workspace, max_pass, first, count, out_coords, out_values, out_rows) ||
        !shap_layout(n_img, height, width, tile_h, tile_w, samples, max_exact, max_pass, s) || (long)first + count > s.l.rows) {
        fprintf(stderr, "tcvn: occlusion_shapley_build: bad argument (NULL pointer, empty hit list, tile < 1, samples or max_exact out of range, more than %d tiles per map, count outside 1..max_pass or variants beyond the list's rows)\n",
                TCVN_TSHAP_MAX_TILES);
        return -1;
    }
    const char* w = reinterpret_cast<const char*>(workspace);
    const KeepCoalition keep{reinterpret_cast<const short*>(w + s.l.rank), reinterpret_cast<const int*>(w + s.ord),
                             reinterpret_cast<const int*>(w + s.mode), s.l.T, samples};
    return list_build_pass("occlusion_shapley_build", s.l, coords, values, channels, n_img, height, width, tile_h, tile_w, vimg, workspace,
                           workspace_bytes, first, count, keep, out_coords, out_values, out_rows, stream);
}

int tcvn_occlusion_shapley_values(const float* event_logits, const float* prong_logits, const float* coalition_event_logits,
                                  const float* coalition_prong_logits, const int32_t* index, int64_t n_variants, const int32_t* exact,
                                  const int32_t* n_tiles, const int32_t* permutations, int batch, int max_prongs, int event_classes,
                                  int prong_classes, int grid_h, int grid_w, int samples, int target, const int32_t* classes, int value,
                                  float* phi, float* std_err, double* full, double* empty, void* scratch, int64_t scratch_bytes,
                                  void* stream) {
    const bool prong = target == TCVN_OCC_TARGET_PRONG;
    const long maps = (long)batch * (1 + (long)max_prongs), T = (long)grid_h * grid_w;
    if (!phi || !std_err || !full || !empty || !exact || !n_tiles || !permutations || !scratch || n_variants < 0 || batch < 1 ||
        max_prongs < 0 || grid_h < 1 || grid_w < 1 || T > TCVN_TSHAP_MAX_TILES || samples < 1 || samples > TCVN_TSHAP_MAX_SAMPLES ||
        (target != TCVN_OCC_TARGET_EVENT && !prong) || (prong && classes) ||
        (value != TCVN_SHAP_VALUE_PROB && value != TCVN_SHAP_VALUE_LOGIT) ||
        (prong ? (max_prongs > 0 && (!prong_logits || prong_classes < 1)) : (!event_logits || event_classes < 1)) ||
        (n_variants > 0 && (!index || (prong ? (max_prongs > 0 && !coalition_prong_logits) : !coalition_event_logits)))) {
        fprintf(stderr, "tcvn: occlusion_shapley_values: bad argument (NULL pointer, batch / classes / grid < 1, more than %d tiles per map, samples outside 1..%d, unknown target or value, or a class list with the prong target)\n",
                TCVN_TSHAP_MAX_TILES, TCVN_TSHAP_MAX_SAMPLES);
        return -1;
    }
    if (scratch_bytes < 8 * (maps + (long)n_variants)) {
        fprintf(stderr, "tcvn: occlusion_shapley_values: scratch of %ld bytes, %ld needed\n", (long)scratch_bytes,
                8 * (maps + (long)n_variants));
        return -12;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    long* start = reinterpret_cast<long*>(scratch);
    double* vals = reinterpret_cast<double*>(start + maps);
    hipLaunchKernelGGL(k_tshap_clear, dim3(cdiv(maps, 256)), dim3(256), 0, st, start, maps);
    TCVN_LAUNCH_CHECK();
    if (n_variants > 0) {
        hipLaunchKernelGGL(k_tshap_value, dim3(cdiv(n_variants, 256)), dim3(256), 0, st, event_logits, prong_logits,
                           coalition_event_logits, coalition_prong_logits, index, (long)n_variants, batch, max_prongs, event_classes,
                           prong_classes, prong ? 1 : 0, classes, value == TCVN_SHAP_VALUE_LOGIT ? 1 : 0, start, vals);
        TCVN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_tshap_phi, dim3((unsigned)maps), dim3(VT), 0, st, event_logits, prong_logits, exact, n_tiles, permutations, start,
                       vals, (long)n_variants, max_prongs, event_classes, prong_classes, (int)T, samples, prong ? 1 : 0, classes,
                       value == TCVN_SHAP_VALUE_LOGIT ? 1 : 0, phi, std_err, full, empty);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
