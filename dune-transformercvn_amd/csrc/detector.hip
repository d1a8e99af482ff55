// Detector-effect scans (forward only): the variants "this map as a detector with effect k would have recorded it" of one COO hit list --
// hit inefficiency, dead wires / ticks, a charge scale, a hit threshold and a shifted window, applied per hit in that order --, their hit
// lists pass by pass, and the response statistics (class probability, its change and the flipped arg-max) in double precision.
// Unlike the occlusion variants these transform coordinates and values, so the list has a layout and a build kernel of its own; the
// ordered compaction, the header and the class choice are those of occlude_list.h.  det_hit() is the one place that decides what becomes
// of a hit under an effect: the count and the build both call it.  Integer atomics only: every result is deterministic.
#include "../../include/tcvn_hip.h"
#include "occlude_list.h"
#include <math.h>
#include <string.h>

namespace tcvn {

namespace {

// ---- workspace: rows (image, k), one counter per row; the tile members of ListLayout stay zero ------------------------------------------------
struct DetLayout { ListLayout l; long effects; };
bool det_layout(int n_img, int K, int max_pass, DetLayout& d) {
    d = DetLayout{};
    ListLayout& o = d.l;
    if (n_img < 1 || K < 1 || K > TCVN_DET_MAX_EFFECTS || max_pass < 1 || max_pass > TCVN_OCC_MAX_PASS) return false;
    o.cells = o.rows = (long)n_img * K;
    if (o.rows > 0x7fffffffL - 1024) return false;
    o.nb = (int)((o.rows + max_pass - 1) / max_pass);
    long off = 0;
    auto take = [&](long bytes) { long at = off; off += round_up(bytes, 256); return at; };
    o.cnt = take(o.rows * 4); o.nnz_img = take((long)n_img * 4); o.flags = take(16); o.img_start = take(((long)n_img + 1) * 8);
    o.payload = take(o.rows * 4); o.voff = take((o.rows + 1) * 8); o.hdr = take((4L + o.nb + 1) * 8);
    d.effects = take((long)K * sizeof(tcvn_detector_effect));
    o.total = off;
    return true;
}

bool effect_ok(const tcvn_detector_effect& e, int H, int W) {
    auto range = [](int lo, int hi, int n) { return 0 <= lo && lo <= hi && hi <= n; };
    auto shift = [](int d) { return d >= -32767 && d <= 32767; };
    return isfinite(e.scale) && e.scale >= 0.f && isfinite(e.threshold) && e.threshold >= 0.f && e.drop >= 0.f && e.drop <= 1.f &&
           range(e.dead_y0, e.dead_y1, H) && range(e.dead_x0, e.dead_x1, W) && shift(e.shift_y) && shift(e.shift_x);
}

// ---- the effects travel as a launch argument and are kept in the workspace: the caller's array is not read after the call ----------------------
constexpr int EFFECT_WORDS = sizeof(tcvn_detector_effect) / 4;
struct EffectTable { uint32_t w[TCVN_DET_MAX_EFFECTS * EFFECT_WORDS]; };
static_assert(sizeof(tcvn_detector_effect) % 8 == 0 && sizeof(EffectTable) <= 3584, "the effect table must fit the kernel arguments");
__global__ __launch_bounds__(256) void k_det_effects(EffectTable t, int words, uint32_t* out) {
    for (int i = threadIdx.x; i < words; i += 256) out[i] = t.w[i];
}

// ---- what becomes of one hit under one effect --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float det_value(const tcvn_detector_effect& e, float raw) {
    const float v = raw * e.scale;
    return (e.threshold > 0.f && v < e.threshold) ? 0.f : v;
}
// (y, x) inside the map, (b, s) its map's event and token slot, v its C raw values -> does it survive, and where
__device__ __forceinline__ bool det_hit(const tcvn_detector_effect& e, int y, int x, int b, int s, int H, int W, const float* v, int C,
                                        int& oy, int& ox) {
    if (e.drop > 0.f) {
        const uint4 r = philox4((uint32_t)(y * W + x), (uint32_t)b, (uint32_t)s, 0x44455453u, (uint32_t)e.seed, (uint32_t)(e.seed >> 32));
        if ((r.x >> 8) * (1.0f / 16777216.0f) < e.drop) return false;
    }
    if ((y >= e.dead_y0 && y < e.dead_y1) || (x >= e.dead_x0 && x < e.dead_x1)) return false;
    if (e.threshold > 0.f) {
        bool any = false;
        for (int c = 0; c < C; ++c) any = any || det_value(e, v[c]) != 0.f;
        if (!any) return false;
    }
    oy = y + e.shift_y; ox = x + e.shift_x;
    return oy >= 0 && oy < H && ox >= 0 && ox < W;
}

// ---- 1. count: one thread per hit, a loop over the effects ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_det_count(const int* __restrict__ coords, const float* __restrict__ values, long nnz, int n_img,
                                                   int H, int W, int C, const int* __restrict__ img_bs,
                                                   const tcvn_detector_effect* __restrict__ effects, int K, int* cnt, int* nnz_img,
                                                   int* flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const int img = coords[3 * i], y = coords[3 * i + 1], x = coords[3 * i + 2];
    if (i > 0 && coords[3 * (i - 1)] > img) atomicOr(&flags[0], 1);                      // the list is not sorted by image
    if (img < 0 || img >= n_img || y < 0 || y >= H || x < 0 || x >= W) { atomicOr(&flags[1], 1); return; }   // a hit the embedders drop
    atomicAdd(&nnz_img[img], 1);
    const int b = img_bs[2 * img], s = img_bs[2 * img + 1];
    const float* v = values + i * C;
    for (int k = 0; k < K; ++k) {
        int oy, ox;
        if (det_hit(effects[k], y, x, b, s, H, W, v, C, oy, ox)) atomicAdd(&cnt[(long)img * K + k], 1);
    }
}

// ---- 2. the variant list (occlude_list.h): a row is an (image, k) pair, a variant every pair of a map that holds a hit ----------------------
__global__ __launch_bounds__(LIST_T) void k_det_list(const int* __restrict__ cnt, const int* __restrict__ nnz_img, const int* flags,
                                                     const int* __restrict__ img_bs, int n_img, int K, int max_pass, long* img_start,
                                                     int* vimg, int* vk, long* voff, int* index, long* hdr) {
    auto effect_row = [=](long c) {
        const int img = (int)(c / K), k = (int)(c - (long)img * K), n = cnt[c];
        return ListRow{nnz_img[img] > 0, (long)n, img, k, k, n};
    };
    variant_list(effect_row, (long)n_img * K, nnz_img, flags, img_bs, n_img, max_pass, img_start, vimg, vk, voff, index, hdr);
}

// ---- 3. build: one workgroup per variant walks its map's hits in chunks of 256; ballot + prefix over the four waves keeps the order ----------
__global__ __launch_bounds__(256) void k_det_build(const int* __restrict__ coords, const float* __restrict__ values, int C, int H, int W,
                                                   const int* __restrict__ img_bs, const tcvn_detector_effect* __restrict__ effects,
                                                   int K, const long* __restrict__ img_start, const int* __restrict__ vimg,
                                                   const int* __restrict__ vk, const long* __restrict__ voff, int first, int n_img,
                                                   int* out_coords, float* out_values, long out_cap) {
    __shared__ int wcnt[4];
    const int j = blockIdx.x, v = first + j, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int img = vimg[v], k = vk[v];
    if (img < 0 || img >= n_img || k < 0 || k >= K) return;    // not a variant of this list (whole workgroup: no barrier is skipped by a part of it)
    const tcvn_detector_effect e = effects[k];
    const int b = img_bs[2 * img], s = img_bs[2 * img + 1];
    const long lo = img_start[img], hi = img_start[img + 1];
    long dst = voff[v] - voff[first];
    for (long base = lo; base < hi; base += 256) {
        const long i = base + tid;
        bool keep = false;
        int oy = 0, ox = 0;
        if (i < hi) {
            const int y = coords[3 * i + 1], x = coords[3 * i + 2];
            keep = y >= 0 && y < H && x >= 0 && x < W && det_hit(e, y, x, b, s, H, W, values + i * C, C, oy, ox);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int off = __popcll(m & ((1ull << lane) - 1ull)), tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int n = wcnt[q]; if (q < w) off += n; tot += n; }
        const long o = dst + off;
        if (keep && o >= 0 && o < out_cap) {
            out_coords[3 * o] = j; out_coords[3 * o + 1] = oy; out_coords[3 * o + 2] = ox;
            for (int c = 0; c < C; ++c) out_values[o * C + c] = det_value(e, values[i * C + c]);
        }
        dst += tot;
        __syncthreads();
    }
}

// ---- 4. response: probability of the compared class, its change and the flipped arg-max; one thread per entry, no atomics ---------------------
__global__ __launch_bounds__(256) void k_det_nan(float* prob, float* delta, unsigned char* flipped, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    prob[i] = delta[i] = __uint_as_float(0x7fc00000u);
    flipped[i] = 0;
}
__global__ __launch_bounds__(256) void k_det_response(const float* base_ev, const float* base_pr, const float* var_ev, const float* var_pr,
                                                      const int* index, const int* valid, long n, int B, int P, int Ce, int Cp, int K,
                                                      int by_map, int prong, const int* cls, float* prob, float* delta,
                                                      unsigned char* flipped) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long v, out;
    int b, s;
    if (by_map) {                                // entry = variant: written at (k, b, s)
        v = i; b = index[4 * v]; s = index[4 * v + 1];
        const int k = index[4 * v + 2];
        if (b < 0 || b >= B || s < 0 || s > P || k < 0 || k >= K) return;
        out = ((long)k * B + b) * (1 + P) + s;
    } else if (prong) {                          // entry = (k, b, p): the slot's own row of the event's varied prediction
        const int p = (int)(i % P);
        v = i / P; b = (int)(v % B); s = 1 + p; out = i;
        if (valid[(long)b * (1 + P) + s] < 0) return;
    } else {                                     // entry = (k, b)
        v = i; b = (int)(v % B); s = 0; out = i;
    }
    const float *a, *o;
    int C, c;
    if (!class_choice(base_ev, base_pr, var_ev, var_pr, v, b, s, P, Ce, Cp, prong, cls, a, o, C, c)) return;
    const double pb = softmax_at(a, C, c), pv = softmax_at(o, C, c);
    prob[out] = (float)pv;
    delta[out] = (float)(pv - pb);
    flipped[out] = argmax_row(o, C) != argmax_row(a, C) ? 1 : 0;
}

}  // namespace

}  // namespace tcvn

using namespace tcvn;

extern "C" {

int64_t tcvn_detector_workspace_bytes(int n_img, int n_effects, int max_pass) {
    DetLayout d;
    return det_layout(n_img, n_effects, max_pass, d) ? d.l.total : -1;
}

int tcvn_detector_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int channels, const float* values,
                           const int32_t* img_bs, const tcvn_detector_effect* effects, int n_effects, int max_pass, int32_t* vimg,
                           int32_t* index, void* workspace, int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream) {
    const char* who = "detector_variants";
    DetLayout d;
    bool ok = list_pointers_ok(coords, nnz, img_bs, vimg, index, workspace, host_out) && (values || nnz == 0) && effects && height >= 1 &&
              width >= 1 && (long)height * width <= 0x7fffffffL && channels >= 1 && det_layout(n_img, n_effects, max_pass, d);
    for (int k = 0; ok && k < n_effects; ++k) ok = effect_ok(effects[k], height, width);
    if (!ok) {
        fprintf(stderr, "tcvn: %s: bad argument (NULL pointer, n_img / map / channels < 1, n_effects outside 1..%d, max_pass outside 1..%d or an effect out of range)\n",
                who, TCVN_DET_MAX_EFFECTS, TCVN_OCC_MAX_PASS);
        return -1;
    }
    const ListLayout& o = d.l;
    if (int rc = list_room(who, o, workspace_bytes, host_cap)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* w = reinterpret_cast<char*>(workspace);
    tcvn_detector_effect* d_effects = reinterpret_cast<tcvn_detector_effect*>(w + d.effects);
    EffectTable table{};
    memcpy(table.w, effects, (size_t)n_effects * sizeof(tcvn_detector_effect));
    hipLaunchKernelGGL(k_det_effects, dim3(1), dim3(256), 0, st, table, n_effects * EFFECT_WORDS, reinterpret_cast<uint32_t*>(d_effects));
    TCVN_LAUNCH_CHECK();
    int* cnt = reinterpret_cast<int*>(w + o.cnt);
    int* nnz_img = reinterpret_cast<int*>(w + o.nnz_img);
    int* flags = reinterpret_cast<int*>(w + o.flags);
    TCVN_CHECK(hipMemsetAsync(w + o.cnt, 0, (size_t)(o.img_start - o.cnt), st));               // cnt, nnz_img and flags are adjacent
    TCVN_CHECK(hipMemsetAsync(w + o.hdr, 0, (size_t)(4 + o.nb + 1) * 8, st));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_det_count, dim3(cdiv(nnz, 256)), dim3(256), 0, st, coords, values, (long)nnz, n_img, height, width, channels,
                           img_bs, d_effects, n_effects, cnt, nnz_img, flags);
        TCVN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_det_list, dim3(1), dim3(LIST_T), 0, st, cnt, nnz_img, flags, img_bs, n_img, n_effects, max_pass,
                           reinterpret_cast<long*>(w + o.img_start), vimg, reinterpret_cast<int*>(w + o.payload),
                           reinterpret_cast<long*>(w + o.voff), index, reinterpret_cast<long*>(w + o.hdr));
        TCVN_LAUNCH_CHECK();
    }
    return list_read_header(o, w, host_out, st);
}

int tcvn_detector_build_pass(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height, int width,
                             const int32_t* img_bs, int n_effects, int max_pass, const int32_t* vimg, const void* workspace,
                             int64_t workspace_bytes, int first, int count, int32_t* out_coords, float* out_values, int64_t out_rows,
                             void* stream) {
    DetLayout d;
    if (!build_args_ok(coords, values, nnz, channels, vimg, workspace, max_pass, first, count, out_coords, out_values, out_rows) ||
        !img_bs || height < 1 || width < 1 || !det_layout(n_img, n_effects, max_pass, d) || (long)first + count > d.l.rows) {
        fprintf(stderr, "tcvn: detector_build_pass: bad argument (NULL pointer, empty hit list, map < 1, n_effects outside 1..%d, count outside 1..max_pass or variants beyond n_img * n_effects)\n",
                TCVN_DET_MAX_EFFECTS);
        return -1;
    }
    const ListLayout& o = d.l;
    if (workspace_bytes < o.total) {
        fprintf(stderr, "tcvn: detector_build_pass: workspace of %ld bytes, %ld needed\n", (long)workspace_bytes, o.total);
        return -12;
    }
    const char* w = reinterpret_cast<const char*>(workspace);
    hipLaunchKernelGGL(k_det_build, dim3(count), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), coords, values, channels, height,
                       width, img_bs, reinterpret_cast<const tcvn_detector_effect*>(w + d.effects), n_effects,
                       reinterpret_cast<const long*>(w + o.img_start), vimg, reinterpret_cast<const int*>(w + o.payload),
                       reinterpret_cast<const long*>(w + o.voff), first, n_img, out_coords, out_values, (long)out_rows);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_detector_response(const float* event_logits, const float* prong_logits, const float* varied_event_logits,
                           const float* varied_prong_logits, const int32_t* index, int64_t n_variants, const int32_t* valid, int batch,
                           int max_prongs, int event_classes, int prong_classes, int n_effects, int scope, int target,
                           const int32_t* classes, float* prob, float* delta, uint8_t* flipped, void* stream) {
    const bool prong = target == TCVN_OCC_TARGET_PRONG, by_map = scope == TCVN_DET_SCOPE_MAP;
    bool ok = prob && delta && flipped && n_variants >= 0 && batch >= 1 && max_prongs >= 0 && n_effects >= 1 &&
              n_effects <= TCVN_DET_MAX_EFFECTS && (by_map || scope == TCVN_DET_SCOPE_EVENT) &&
              (prong || target == TCVN_OCC_TARGET_EVENT) && !(prong && classes);
    long entries = 0, work = 0;                  // entries of the outputs; threads of the response kernel
    if (ok) {
        const long kb = (long)n_effects * batch;
        entries = by_map ? kb * (1 + max_prongs) : prong ? kb * max_prongs : kb;
        work = by_map ? (long)n_variants : entries;
        if (!by_map && n_variants != kb) ok = false;
        if (work > 0 && ((by_map && !index) || (!by_map && prong && !valid) ||
                         (prong ? (!prong_logits || !varied_prong_logits || prong_classes < 1)
                                : (!event_logits || !varied_event_logits || event_classes < 1))))
            ok = false;
    }
    if (!ok) {
        fprintf(stderr, "tcvn: detector_response: bad argument (NULL pointer, batch / classes < 1, n_effects outside 1..%d, unknown scope or target, a class list with the prong target, or a whole-event scan whose rows are not n_effects * batch)\n",
                TCVN_DET_MAX_EFFECTS);
        return -1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (entries == 0) return 0;
    hipLaunchKernelGGL(k_det_nan, dim3(cdiv(entries, 256)), dim3(256), 0, st, prob, delta, flipped, entries);
    TCVN_LAUNCH_CHECK();
    if (work == 0) return 0;
    hipLaunchKernelGGL(k_det_response, dim3(cdiv(work, 256)), dim3(256), 0, st, event_logits, prong_logits, varied_event_logits,
                       varied_prong_logits, index, valid, work, batch, max_prongs, event_classes, prong_classes, n_effects,
                       by_map ? 1 : 0, prong ? 1 : 0, classes, prob, delta, flipped);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
