// Deletion / insertion curves (forward only): the rank of every occupied tile of every map under a relevance map, the hit lists of the
// variants "this map without / with only the hits of its m_k first tiles", and the curve of class probabilities with its area.
// As in occlude.hip a variant is a filtered copy of its image's rows in their original order.  The ranking is a sort of 64-bit keys
// (relevance pattern, tile index) that are all different, so it is a pure function of the inputs; the only atomics are the integer
// ones of the occupancy count: every result is deterministic.
#include "../../include/tcvn_hip.h"
#include "occlude_dev.h"

namespace tcvn {

namespace {

// Workspace of the curve variants of one hit list (n_img images of T = Ht x Wt tiles, K + 1 variants each at most).
struct CurveLayout { long cnt, nnz_img, flags, img_start, rank, prefix, nocc, vm, voff, hdr, total; long cells, rows; int T, nb; };
bool curve_layout(int n_img, int H, int W, int th, int tw, int steps, int max_pass, CurveLayout& o) {
    const long Ht = (H + th - 1) / th, Wt = (W + tw - 1) / tw;
    if (Ht * Wt > TCVN_CURVE_MAX_TILES) return false;
    o.T = (int)(Ht * Wt);
    o.cells = (long)n_img * o.T;
    o.rows = (long)n_img * (steps + 1);
    if (o.cells > 0x7fffffffL - 1024 || o.rows > 0x7fffffffL - 1024) return false;
    o.nb = (int)((o.rows + max_pass - 1) / max_pass);
    long off = 0;
    auto take = [&](long bytes) { long at = off; off += round_up(bytes, 256); return at; };
    o.cnt = take(o.cells * 4); o.nnz_img = take((long)n_img * 4); o.flags = take(16); o.img_start = take(((long)n_img + 1) * 8);
    o.rank = take(o.cells * 4); o.prefix = take((long)n_img * (o.T + 1) * 4); o.nocc = take((long)n_img * 4);
    o.vm = take(o.rows * 4); o.voff = take((o.rows + 1) * 8); o.hdr = take((4L + o.nb + 1) * 8);
    o.total = off;
    return true;
}
bool curve_geometry_ok(int n_img, int H, int W, int th, int tw, int steps, int mode, int max_pass) {
    return n_img >= 1 && H >= 1 && W >= 1 && th >= 1 && tw >= 1 && steps >= 1 && steps <= TCVN_CURVE_MAX_STEPS &&
           (mode == TCVN_CURVE_DELETION || mode == TCVN_CURVE_INSERTION) && max_pass >= 1 && max_pass <= TCVN_OCC_MAX_PASS;
}

// ---- 1. rank: one workgroup per map sorts the keys of its tiles in LDS (bitonic, ascending) ------------------------------------------------
// key = (~ascending-orderable pattern of the relevance) << 32 | tile: ascending keys are descending relevances, ties by ascending tile.
// Tiles without hits (and the padding up to N, the power of two >= T) carry the largest key; no occupied tile can (its low word < T).
constexpr int RT = 1024;
constexpr unsigned long long NO_TILE = ~0ull;
__global__ __launch_bounds__(RT) void k_curve_rank(const int* __restrict__ cnt, const int* __restrict__ img_bs,
                                                   const float* __restrict__ rel, int B, int S, int T, int N, int* rank, int* prefix,
                                                   int* nocc, int* rank_map) {
    __shared__ unsigned long long key[TCVN_CURVE_MAX_TILES];
    __shared__ long wsum[RT / 64];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int b = img_bs[2 * img], s = img_bs[2 * img + 1];
    const bool named = b >= 0 && b < B && s >= 0 && s < S;                   // a map the relevance has no row for is not ranked
    const long map = named ? (long)b * S + s : 0;
    const int* c = cnt + (long)img * T;
    for (int t = tid; t < N; t += RT) {
        unsigned long long k = NO_TILE;
        if (t < T) {
            rank[(long)img * T + t] = -1;
            if (named && c[t] > 0) {
                unsigned u = __float_as_uint(rel[map * T + t]);
                if ((u << 1) == 0) u = 0;                                     // -0.0 counts as +0.0
                const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                k = ((unsigned long long)(~asc) << 32) | (unsigned)t;
            }
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
    // the occupied tiles now stand in front, in rank order: rank, n and prefix[r] = hits of the tiles ranked below r (r = 0..T)
    if (tid == 0 && key[0] == NO_TILE) nocc[img] = 0;
    long carry = 0, tot;
    for (int base = 0; base <= T; base += RT) {
        const int i = base + tid;
        const unsigned long long k = i < T ? key[i] : NO_TILE;
        const int tile = (int)(k & 0xffffffffull);
        const long v = k != NO_TILE ? c[tile] : 0;
        const long ex = block_scan_excl(v, wsum, tot);
        if (i <= T) prefix[(long)img * (T + 1) + i] = (int)(carry + ex);
        if (k != NO_TILE) {
            rank[(long)img * T + tile] = i;
            rank_map[map * T + tile] = i;
            if (i + 1 == T || key[i + 1] == NO_TILE) nocc[img] = i + 1;      // key has N >= T entries; i + 1 < T is read only
        }
        carry += tot;
    }
}

// ---- 2. variant list: the (image, k) pairs of the maps that hold a hit, their surviving hits and the pass boundaries ---------------------
constexpr int CT = 1024;
__global__ __launch_bounds__(CT) void k_curve_plan(const int* __restrict__ nnz_img, const int* flags, const int* __restrict__ img_bs,
                                                   const int* __restrict__ prefix, const int* __restrict__ nocc, int n_img, int T, int K,
                                                   int insertion, int max_pass, long* img_start, int* vimg, int* vm, long* voff,
                                                   int* index, long* hdr) {
    __shared__ long wsum[CT / 64];
    const int tid = threadIdx.x;
    long carry = 0, tot;
    for (int base = 0; base < n_img; base += CT) {           // first hit of every image (the list is sorted by image)
        const int i = base + tid;
        const long v = i < n_img ? nnz_img[i] : 0;
        const long ex = block_scan_excl(v, wsum, tot);
        if (i < n_img) img_start[i] = carry + ex;
        carry += tot;
    }
    if (tid == 0) img_start[n_img] = carry;
    const long rows = (long)n_img * (K + 1);
    long nv = 0, nh = 0;                                     // variants / surviving hits in front of this chunk
    long* bounds = hdr + 4;
    for (long base = 0; base < rows; base += CT) {
        const long c = base + tid;
        int img = 0, k = 0, n = 0, m = 0;
        long surv = 0;
        if (c < rows) {
            img = (int)(c / (K + 1)); k = (int)(c - (long)img * (K + 1)); n = nocc[img];
            m = (k * n + K - 1) / K;                         // k <= 64, n <= 4096
            const long below = prefix[(long)img * (T + 1) + m];
            surv = n > 0 ? (insertion ? below : (long)nnz_img[img] - below) : 0;
        }
        const long flag = n > 0 ? 1 : 0;
        long tv, th_;
        const long pos = nv + block_scan_excl(flag, wsum, tv);
        const long at = nh + block_scan_excl(surv, wsum, th_);
        if (flag) {
            vimg[pos] = img; vm[pos] = m; voff[pos] = at;
            index[4 * pos] = img_bs[2 * img]; index[4 * pos + 1] = img_bs[2 * img + 1]; index[4 * pos + 2] = k; index[4 * pos + 3] = m;
            if (pos % max_pass == 0) bounds[pos / max_pass] = at;
        }
        nv += tv; nh += th_;
    }
    if (tid == 0) {
        voff[nv] = nh;
        bounds[(nv + max_pass - 1) / max_pass] = nh;         // the end of the last pass (bounds[0] = 0 when there is no variant)
        hdr[0] = nv; hdr[1] = flags[0]; hdr[2] = flags[1]; hdr[3] = nh;
    }
}

// ---- 3. variant build: one workgroup per variant walks its image's hits in chunks; ballot + prefix keeps the order ---------------------
__global__ __launch_bounds__(256) void k_curve_build(const int* __restrict__ coords, const float* __restrict__ values, int C, int H, int W,
                                                     int th, int tw, int Wt, int T, const long* __restrict__ img_start,
                                                     const int* __restrict__ rank, const int* __restrict__ vimg,
                                                     const int* __restrict__ vm, const long* __restrict__ voff, int first, int n_img,
                                                     int deletion, int* out_coords, float* out_values, long out_cap) {
    __shared__ int wcnt[4];
    const int j = blockIdx.x, v = first + j, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int img = vimg[v], m = vm[v];
    if (img < 0 || img >= n_img) return;             // not a variant of this list (whole workgroup: no barrier is skipped by a part of it)
    const long lo = img_start[img], hi = img_start[img + 1];
    const int* rk = rank + (long)img * T;
    long dst = voff[v] - voff[first];
    for (long base = lo; base < hi; base += 256) {
        const long i = base + tid;
        bool keep = false;
        int y = 0, x = 0;
        if (i < hi) {
            y = coords[3 * i + 1]; x = coords[3 * i + 2];
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            keep = in && ((rk[(y / th) * Wt + x / tw] < m) != (deletion != 0));
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wcnt[w] = __popcll(mask);
        __syncthreads();
        int off = __popcll(mask & ((1ull << lane) - 1ull)), tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int n = wcnt[k]; if (k < w) off += n; tot += n; }
        const long o = dst + off;
        if (keep && o >= 0 && o < out_cap) {
            out_coords[3 * o] = j; out_coords[3 * o + 1] = y; out_coords[3 * o + 2] = x;
            for (int c = 0; c < C; ++c) out_values[o * C + c] = values[i * C + c];
        }
        dst += tot;
        __syncthreads();
    }
}

// ---- 4. curve and area -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_curve_nan(float* curve, long n_curve, float* auc, long n_auc) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_curve) curve[i] = __uint_as_float(0x7fc00000u);
    else if (i < n_curve + n_auc) auc[i - n_curve] = __uint_as_float(0x7fc00000u);
}
__global__ __launch_bounds__(256) void k_curve_prob(const float* base_ev, const float* base_pr, const float* step_ev, const float* step_pr,
                                                    const int* index, long V, int B, int P, int Ce, int Cp, int K, int prong,
                                                    const int* cls, float* curve) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int b = index[4 * v], s = index[4 * v + 1], k = index[4 * v + 2];
    if (b < 0 || b >= B || s < 0 || s > P || k < 0 || k > K) return;
    const float *a, *o;
    int C, c;
    if (prong) {
        if (s == 0) return;
        a = base_pr + ((long)b * P + (s - 1)) * Cp; o = step_pr + ((long)v * P + (s - 1)) * Cp; C = Cp;
        c = argmax_row(a, C);
    } else {
        a = base_ev + (long)b * Ce; o = step_ev + (long)v * Ce; C = Ce;
        c = cls ? cls[b] : argmax_row(a, C);
        if (c < 0 || c >= C) return;
    }
    curve[((long)b * (1 + P) + s) * (K + 1) + k] = (float)softmax_at(o, C, c);
}
// one thread per map: the trapezoid over x = k / K in the order of k (a NaN row gives NaN)
__global__ __launch_bounds__(256) void k_curve_auc(const float* __restrict__ curve, long maps, int K, float* auc) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= maps) return;
    const float* p = curve + i * (K + 1);
    double a = 0.5 * (double)p[0];
    for (int k = 1; k < K; ++k) a += (double)p[k];
    a += 0.5 * (double)p[K];
    auc[i] = (float)(a / (double)K);
}

}  // namespace

}  // namespace tcvn

using namespace tcvn;

extern "C" {

int64_t tcvn_occlusion_curve_workspace_bytes(int n_img, int height, int width, int tile_h, int tile_w, int steps, int max_pass) {
    CurveLayout o;
    if (!curve_geometry_ok(n_img, height, width, tile_h, tile_w, steps, TCVN_CURVE_DELETION, max_pass) ||
        !curve_layout(n_img, height, width, tile_h, tile_w, steps, max_pass, o))
        return -1;
    return o.total;
}

int tcvn_occlusion_curve_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                                  const int32_t* img_bs, const float* relevance, int batch, int max_prongs, int steps, int mode,
                                  int32_t* rank, int max_pass, int32_t* vimg, int32_t* index, void* workspace,
                                  int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream) {
    CurveLayout o;
    if ((!coords && nnz > 0) || !img_bs || !relevance || !rank || !vimg || !index || !workspace || !host_out || nnz < 0 || batch < 1 ||
        max_prongs < 0 || !curve_geometry_ok(n_img, height, width, tile_h, tile_w, steps, mode, max_pass) ||
        !curve_layout(n_img, height, width, tile_h, tile_w, steps, max_pass, o)) {
        fprintf(stderr, "tcvn: occlusion_curve_variants: bad argument (NULL pointer, n_img / map / tile / batch < 1, steps outside 1..%d, unknown mode, max_pass outside 1..%d or more than %d tiles per map)\n",
                TCVN_CURVE_MAX_STEPS, TCVN_OCC_MAX_PASS, TCVN_CURVE_MAX_TILES);
        return -1;
    }
    if (workspace_bytes < o.total || host_cap < 4 + o.nb + 1) {
        fprintf(stderr, "tcvn: occlusion_curve_variants: workspace of %lld bytes (%ld needed) or host buffer of %lld words (%d needed) too small\n",
                (long long)workspace_bytes, o.total, (long long)host_cap, 4 + o.nb + 1);
        return -12;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* w = reinterpret_cast<char*>(workspace);
    const int Wt = (width + tile_w - 1) / tile_w, T = o.T;
    int N = 2;
    while (N < T) N <<= 1;
    int* cnt = reinterpret_cast<int*>(w + o.cnt);
    int* nnz_img = reinterpret_cast<int*>(w + o.nnz_img);
    int* flags = reinterpret_cast<int*>(w + o.flags);
    int* rk = reinterpret_cast<int*>(w + o.rank);
    int* prefix = reinterpret_cast<int*>(w + o.prefix);
    int* nocc = reinterpret_cast<int*>(w + o.nocc);
    long* hdr = reinterpret_cast<long*>(w + o.hdr);
    TCVN_CHECK(hipMemsetAsync(w + o.cnt, 0, (size_t)(o.img_start - o.cnt), st));           // cnt, nnz_img and flags are adjacent
    TCVN_CHECK(hipMemsetAsync(hdr, 0, (size_t)(4 + o.nb + 1) * 8, st));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_occ_count, dim3(cdiv(nnz, 256)), dim3(256), 0, st, coords, (long)nnz, n_img, height, width, tile_h, tile_w,
                           Wt, T, cnt, nnz_img, flags);
        TCVN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_curve_rank, dim3(n_img), dim3(RT), 0, st, cnt, img_bs, relevance, batch, 1 + max_prongs, T, N, rk, prefix, nocc,
                       rank);
    TCVN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_curve_plan, dim3(1), dim3(CT), 0, st, nnz_img, flags, img_bs, prefix, nocc, n_img, T, steps,
                       mode == TCVN_CURVE_INSERTION ? 1 : 0, max_pass, reinterpret_cast<long*>(w + o.img_start), vimg,
                       reinterpret_cast<int*>(w + o.vm), reinterpret_cast<long*>(w + o.voff), index, hdr);
    TCVN_LAUNCH_CHECK();
    // V, the two flags and the pass boundaries: the one synchronisation of the curves over this hit list
    TCVN_CHECK(hipMemcpyAsync(host_out, hdr, (size_t)(4 + o.nb + 1) * 8, hipMemcpyDeviceToHost, st));
    TCVN_CHECK(hipStreamSynchronize(st));
    return 0;
}

int tcvn_occlusion_curve_build_pass(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height,
                                    int width, int tile_h, int tile_w, int steps, int mode, int max_pass, const int32_t* vimg,
                                    const void* workspace, int64_t workspace_bytes, int first, int count, int32_t* out_coords,
                                    float* out_values, int64_t out_rows, void* stream) {
    CurveLayout o;
    if (!coords || !values || !vimg || !workspace || !out_coords || !out_values || nnz < 1 || channels < 1 ||
        !curve_geometry_ok(n_img, height, width, tile_h, tile_w, steps, mode, max_pass) || first < 0 || count < 1 || count > max_pass ||
        out_rows < 0 || !curve_layout(n_img, height, width, tile_h, tile_w, steps, max_pass, o) || (long)first + count > o.rows) {
        fprintf(stderr, "tcvn: occlusion_curve_build_pass: bad argument (NULL pointer, empty hit list, tile < 1, steps or mode out of range, count outside 1..max_pass or variants beyond n_img * (steps + 1))\n");
        return -1;
    }
    if (workspace_bytes < o.total) {
        fprintf(stderr, "tcvn: occlusion_curve_build_pass: workspace of %lld bytes, %ld needed\n", (long long)workspace_bytes, o.total);
        return -12;
    }
    const char* w = reinterpret_cast<const char*>(workspace);
    const int Wt = (width + tile_w - 1) / tile_w;
    hipLaunchKernelGGL(k_curve_build, dim3(count), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), coords, values, channels, height,
                       width, tile_h, tile_w, Wt, o.T, reinterpret_cast<const long*>(w + o.img_start),
                       reinterpret_cast<const int*>(w + o.rank), vimg, reinterpret_cast<const int*>(w + o.vm),
                       reinterpret_cast<const long*>(w + o.voff), first, n_img, mode == TCVN_CURVE_DELETION ? 1 : 0, out_coords,
                       out_values, (long)out_rows);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_occlusion_curve(const float* event_logits, const float* prong_logits, const float* step_event_logits,
                         const float* step_prong_logits, const int32_t* index, int64_t n_variants, int batch, int max_prongs,
                         int event_classes, int prong_classes, int steps, int target, const int32_t* classes, float* curve, float* auc,
                         void* stream) {
    const bool prong = target == TCVN_OCC_TARGET_PRONG;
    if (!curve || !auc || n_variants < 0 || batch < 1 || max_prongs < 0 || steps < 1 || steps > TCVN_CURVE_MAX_STEPS ||
        (target != TCVN_OCC_TARGET_EVENT && !prong) || (prong && classes) ||
        (n_variants > 0 && (!index || (prong ? (!prong_logits || !step_prong_logits || prong_classes < 1)
                                             : (!event_logits || !step_event_logits || event_classes < 1))))) {
        fprintf(stderr, "tcvn: occlusion_curve: bad argument (NULL pointer, batch / classes < 1, steps outside 1..%d, unknown target or a class list with the prong target)\n",
                TCVN_CURVE_MAX_STEPS);
        return -1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long maps = (long)batch * (1 + max_prongs), cells = maps * (steps + 1);
    hipLaunchKernelGGL(k_curve_nan, dim3(cdiv(cells + maps, 256)), dim3(256), 0, st, curve, cells, auc, maps);
    TCVN_LAUNCH_CHECK();
    if (n_variants == 0) return 0;
    hipLaunchKernelGGL(k_curve_prob, dim3(cdiv(n_variants, 256)), dim3(256), 0, st, event_logits, prong_logits, step_event_logits,
                       step_prong_logits, index, (long)n_variants, batch, max_prongs, event_classes, prong_classes, steps,
                       prong ? 1 : 0, classes, curve);
    TCVN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_curve_auc, dim3(cdiv(maps, 256)), dim3(256), 0, st, curve, maps, steps, auc);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
