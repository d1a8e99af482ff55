// Deletion / insertion curves (forward only): the rank of every occupied tile of every map under a relevance map, the hit lists of the
// variants "this map without / with only the hits of its m_k first tiles", and the curve of class probabilities with its area.
// As in occlude.hip a variant is a filtered copy of its image's rows in their original order.  The ranking is a sort of 64-bit keys
// (relevance pattern, tile index) that are all different, so it is a pure function of the inputs; the only atomics are the integer
// ones of the occupancy count: every result is deterministic.
#include "../../include/tcvn_hip.h"
#include "occlude_list.h"

namespace tcvn {

namespace {

// steps and mode of a curve list; the rest of its geometry is list_layout's to check (occlude_list.h)
bool curve_ok(int steps, int mode) {
    return steps >= 1 && steps <= TCVN_CURVE_MAX_STEPS && (mode == TCVN_CURVE_DELETION || mode == TCVN_CURVE_INSERTION);
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

// ---- 2-3. the variant list (occlude_list.h): a row is an (image, k) pair, a variant every pair of a map that holds a hit -----------------------
__global__ __launch_bounds__(LIST_T) void k_curve_list(const int* __restrict__ nnz_img, const int* flags, const int* __restrict__ img_bs,
                                                       const int* __restrict__ prefix, const int* __restrict__ nocc, int n_img, int T,
                                                       int K, int insertion, int max_pass, long* img_start, int* vimg, int* vm,
                                                       long* voff, int* index, long* hdr) {
    auto step_row = [=](long c) {
        const int img = (int)(c / (K + 1)), k = (int)(c - (long)img * (K + 1)), n = nocc[img];
        const int m = (k * n + K - 1) / K;                   // k <= 64, n <= 4096
        const long below = prefix[(long)img * (T + 1) + m];
        return ListRow{n > 0, insertion ? below : (long)nnz_img[img] - below, img, m, k, m};
    };
    variant_list(step_row, (long)n_img * (K + 1), nnz_img, flags, img_bs, n_img, max_pass, img_start, vimg, vm, voff, index, hdr);
}
// deletion keeps the hits of all but the m top-ranked tiles, insertion those of the m top-ranked tiles; a hit outside the map is dropped
struct KeepRanked {
    const int* rank; int T, deletion;
    __device__ bool operator()(bool in, int cell, int img, int m) const {
        return in && ((rank[(long)img * T + cell] < m) != (deletion != 0));
    }
};

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
    if (!class_choice(base_ev, base_pr, step_ev, step_pr, v, b, s, P, Ce, Cp, prong, cls, a, o, C, c)) return;
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
    ListLayout o;
    return curve_ok(steps, TCVN_CURVE_DELETION) && list_layout(n_img, height, width, tile_h, tile_w, steps, max_pass, o) ? o.total : -1;
}

int tcvn_occlusion_curve_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                                  const int32_t* img_bs, const float* relevance, int batch, int max_prongs, int steps, int mode,
                                  int32_t* rank, int max_pass, int32_t* vimg, int32_t* index, void* workspace,
                                  int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream) {
    const char* who = "occlusion_curve_variants";
    ListLayout o;
    if (!list_pointers_ok(coords, nnz, img_bs, vimg, index, workspace, host_out) || !relevance || !rank || batch < 1 || max_prongs < 0 ||
        !curve_ok(steps, mode) || !list_layout(n_img, height, width, tile_h, tile_w, steps, max_pass, o)) {
        fprintf(stderr, "tcvn: %s: bad argument (NULL pointer, n_img / map / tile / batch < 1, steps outside 1..%d, unknown mode, max_pass outside 1..%d or more than %d tiles per map)\n",
                who, TCVN_CURVE_MAX_STEPS, TCVN_OCC_MAX_PASS, TCVN_CURVE_MAX_TILES);
        return -1;
    }
    if (int rc = list_room(who, o, workspace_bytes, host_cap)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* w = reinterpret_cast<char*>(workspace);
    const int T = o.T;
    int N = 2;
    while (N < T) N <<= 1;
    const int* nnz_img = reinterpret_cast<const int*>(w + o.nnz_img);
    int* prefix = reinterpret_cast<int*>(w + o.prefix);
    int* nocc = reinterpret_cast<int*>(w + o.nocc);
    if (int rc = list_count(o, w, coords, nnz, n_img, height, width, tile_h, tile_w, img_bs, nullptr, 0, 0, 0, 0, st)) return rc;
    hipLaunchKernelGGL(k_curve_rank, dim3(n_img), dim3(RT), 0, st, reinterpret_cast<const int*>(w + o.cnt), img_bs, relevance, batch,
                       1 + max_prongs, T, N, reinterpret_cast<int*>(w + o.rank), prefix, nocc, rank);
    TCVN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_curve_list, dim3(1), dim3(LIST_T), 0, st, nnz_img, reinterpret_cast<const int*>(w + o.flags), img_bs, prefix,
                       nocc, n_img, T, steps, mode == TCVN_CURVE_INSERTION ? 1 : 0, max_pass, reinterpret_cast<long*>(w + o.img_start),
                       vimg, reinterpret_cast<int*>(w + o.payload), reinterpret_cast<long*>(w + o.voff), index,
                       reinterpret_cast<long*>(w + o.hdr));
    TCVN_LAUNCH_CHECK();
    return list_read_header(o, w, host_out, st);
}

int tcvn_occlusion_curve_build_pass(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height,
                                    int width, int tile_h, int tile_w, int steps, int mode, int max_pass, const int32_t* vimg,
                                    const void* workspace, int64_t workspace_bytes, int first, int count, int32_t* out_coords,
                                    float* out_values, int64_t out_rows, void* stream) {
    ListLayout o;
    if (!build_args_ok(coords, values, nnz, channels, vimg, workspace, max_pass, first, count, out_coords, out_values, out_rows) ||
        !curve_ok(steps, mode) || !list_layout(n_img, height, width, tile_h, tile_w, steps, max_pass, o) ||
        (long)first + count > o.rows) {
        fprintf(stderr, "tcvn: occlusion_curve_build_pass: bad argument (NULL pointer, empty hit list, tile < 1, steps or mode out of range, count outside 1..max_pass or variants beyond n_img * (steps + 1))\n");
        return -1;
    }
    const KeepRanked keep{reinterpret_cast<const int*>(reinterpret_cast<const char*>(workspace) + o.rank), o.T,
                          mode == TCVN_CURVE_DELETION ? 1 : 0};
    return list_build_pass("occlusion_curve_build_pass", o, coords, values, channels, n_img, height, width, tile_h, tile_w, vimg,
                           workspace, workspace_bytes, first, count, keep, out_coords, out_values, out_rows, stream);
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
