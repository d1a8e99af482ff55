// The variant-list core of the occlusion kernels (occlude.hip: one variant per occupied tile; occlude_curve.hip: steps + 1 variants per
// occupied map): workspace layout, occupancy count, the ordered compaction into (vimg, payload, voff, index, bounds), the build of a
// pass's hit lists, the host routines around them, and the class choice and double-precision softmax of the heat map and the curves.
// A list supplies only what one of its rows is (ListRow) and which hits a variant keeps.  Every translation unit gets its own copy.
#pragma once
#include "../../include/tcvn_hip.h"
#include "tcvn_common.h"

namespace tcvn {

namespace {

// ---- workspace of the variant list of one hit list: n_img images of T = Ht x Wt tiles, `rows` candidate variants ---------------------------
// steps = 0: the tile list, one row per tile.  steps > 0: the curve list, steps + 1 rows per image, and the only members it adds
// (rank, prefix, nocc).  payload: one word per variant (its tile / its m).  false: bad geometry or more than 2^31 - 1024 cells or rows.
struct ListLayout { long cnt, nnz_img, flags, img_start, rank, prefix, nocc, payload, voff, hdr, total; long cells, rows; int Wt, T, nb; };
bool list_layout(int n_img, int H, int W, int th, int tw, int steps, int max_pass, ListLayout& o) {
    o = ListLayout{};
    if (n_img < 1 || H < 1 || W < 1 || th < 1 || tw < 1 || max_pass < 1 || max_pass > TCVN_OCC_MAX_PASS) return false;
    const long Ht = (H + th - 1) / th, Wt = (W + tw - 1) / tw;
    if (steps > 0 && Ht * Wt > TCVN_CURVE_MAX_TILES) return false;
    o.cells = (long)n_img * Ht * Wt;
    o.rows = steps > 0 ? (long)n_img * (steps + 1) : o.cells;
    if (o.cells > 0x7fffffffL - 1024 || o.rows > 0x7fffffffL - 1024) return false;
    o.Wt = (int)Wt; o.T = (int)(Ht * Wt);
    o.nb = (int)((o.rows + max_pass - 1) / max_pass);
    long off = 0;
    auto take = [&](long bytes) { long at = off; off += round_up(bytes, 256); return at; };
    o.cnt = take(o.cells * 4); o.nnz_img = take((long)n_img * 4); o.flags = take(16); o.img_start = take(((long)n_img + 1) * 8);
    if (steps > 0) { o.rank = take(o.cells * 4); o.prefix = take((long)n_img * (o.T + 1) * 4); o.nocc = take((long)n_img * 4); }
    o.payload = take(o.rows * 4); o.voff = take((o.rows + 1) * 8); o.hdr = take((4L + o.nb + 1) * 8);
    o.total = off;
    return true;
}

// ---- 1. occupancy: one thread per hit -----------------------------------------------------------------------------------------------------
// keep_map == nullptr: every hit inside its map counts.  Refinement: a hit enters cnt only where the parent level's keep_map is set at its
// parent tile (tiles of 2*th x 2*tw); nnz_img and the two flags still see every hit, so a variant's surviving hits stay "the whole image
// minus that one tile".
__global__ __launch_bounds__(256) void k_occ_count(const int* __restrict__ coords, long nnz, int n_img, int H, int W, int th, int tw,
                                                   int Wt, int T, const int* __restrict__ img_bs,
                                                   const unsigned char* __restrict__ keep_map, int B, int S, int pHt, int pWt, int* cnt,
                                                   int* nnz_img, int* flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const int img = coords[3 * i], y = coords[3 * i + 1], x = coords[3 * i + 2];
    if (i > 0 && coords[3 * (i - 1)] > img) atomicOr(&flags[0], 1);                      // the list is not sorted by image
    if (img < 0 || img >= n_img || y < 0 || y >= H || x < 0 || x >= W) { atomicOr(&flags[1], 1); return; }   // a hit the embedders drop
    atomicAdd(&nnz_img[img], 1);
    if (keep_map) {
        const int b = img_bs[2 * img], s = img_bs[2 * img + 1], py = y / (2 * th), px = x / (2 * tw);
        if (b < 0 || b >= B || s < 0 || s >= S || py >= pHt || px >= pWt) return;        // no such parent: never a variant
        if (!keep_map[(((long)b * S + s) * pHt + py) * pWt + px]) return;
    }
    atomicAdd(&cnt[(long)img * T + (y / th) * Wt + x / tw], 1);
}

__device__ __forceinline__ long shfl_up64(long v, int d) {
    const int lo = __shfl_up((int)(v & 0xffffffffL), d), hi = __shfl_up((int)(v >> 32), d);
    return ((long)hi << 32) | (long)(unsigned)lo;
}
// exclusive prefix sum over the workgroup (wave64 shuffles, then the wave totals through LDS); total: the sum over all threads
__device__ __forceinline__ long block_scan_excl(long v, long* wsum, long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const long t = shfl_up64(inc, d); if (lane >= d) inc += t; }
    __syncthreads();                       // wsum may still be read from the previous call
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    long base = 0, tot = 0;
    for (int i = 0; i < nw; ++i) { const long s = wsum[i]; if (i < w) base += s; tot += s; }
    total = tot;
    return base + inc - v;
}

// ---- 2. variant list: ordered compaction of the rows that are variants; one workgroup of LIST_T threads walks the rows in chunks -----------
// row_of(c) says what row c is: whether it is a variant, how many hits survive in it, its image, its payload word and the last two words
// of its index row (the first two are the image's (b, s)).  hdr = (V, unsorted, bad, surviving hits), then the pass boundaries.
constexpr int LIST_T = 1024;
struct ListRow { bool flag; long surv; int img, payload, i2, i3; };
template <class RowOf>
__device__ __forceinline__ void variant_list(RowOf row_of, long rows, const int* __restrict__ nnz_img, const int* flags,
                                             const int* __restrict__ img_bs, int n_img, int max_pass, long* img_start, int* vimg,
                                             int* payload, long* voff, int* index, long* hdr) {
    __shared__ long wsum[LIST_T / 64];
    const int tid = threadIdx.x;
    long carry = 0, tot;
    for (int base = 0; base < n_img; base += LIST_T) {       // first hit of every image (the list is sorted by image)
        const int i = base + tid;
        const long v = i < n_img ? nnz_img[i] : 0;
        const long ex = block_scan_excl(v, wsum, tot);
        if (i < n_img) img_start[i] = carry + ex;
        carry += tot;
    }
    if (tid == 0) img_start[n_img] = carry;
    long nv = 0, nh = 0;                                     // variants / surviving hits in front of this chunk
    long* bounds = hdr + 4;
    for (long base = 0; base < rows; base += LIST_T) {
        const long c = base + tid;
        const ListRow r = c < rows ? row_of(c) : ListRow{false, 0, 0, 0, 0, 0};
        long tv, th_;
        const long pos = nv + block_scan_excl(r.flag ? 1 : 0, wsum, tv);
        const long at = nh + block_scan_excl(r.flag ? r.surv : 0, wsum, th_);
        if (r.flag) {
            vimg[pos] = r.img; payload[pos] = r.payload; voff[pos] = at;
            index[4 * pos] = img_bs[2 * r.img]; index[4 * pos + 1] = img_bs[2 * r.img + 1];
            index[4 * pos + 2] = r.i2; index[4 * pos + 3] = r.i3;
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
// keep(in, cell, img, payload): does the variant with this payload word keep a hit of tile `cell` (in: the hit lies inside the map)
template <class Keep>
__global__ __launch_bounds__(256) void k_list_build(const int* __restrict__ coords, const float* __restrict__ values, int C, int H, int W,
                                                    int th, int tw, int Wt, const long* __restrict__ img_start,
                                                    const int* __restrict__ vimg, const int* __restrict__ payload,
                                                    const long* __restrict__ voff, int first, int n_img, Keep keep_of, int* out_coords,
                                                    float* out_values, long out_cap) {
    __shared__ int wcnt[4];
    const int j = blockIdx.x, v = first + j, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int img = vimg[v], word = payload[v];
    if (img < 0 || img >= n_img) return;             // not a variant of this list (whole workgroup: no barrier is skipped by a part of it)
    const long lo = img_start[img], hi = img_start[img + 1];
    long dst = voff[v] - voff[first];
    for (long base = lo; base < hi; base += 256) {
        const long i = base + tid;
        bool keep = false;
        int y = 0, x = 0;
        if (i < hi) {
            y = coords[3 * i + 1]; x = coords[3 * i + 2];
            keep = keep_of(y >= 0 && y < H && x >= 0 && x < W, (y / th) * Wt + x / tw, img, word);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int off = __popcll(m & ((1ull << lane) - 1ull)), tot = 0;
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

// ---- class choice and softmax of the heat map and the curves ---------------------------------------------------------------------------------
__device__ __forceinline__ int argmax_row(const float* a, int C) {
    int c = 0;
    for (int k = 1; k < C; ++k) if (a[k] > a[c]) c = k;
    return c;
}
__device__ __forceinline__ double softmax_at(const float* a, int C, int c) {
    float m = a[0];
    for (int k = 1; k < C; ++k) m = fmaxf(m, a[k]);
    double s = 0.0;
    for (int k = 0; k < C; ++k) s += exp((double)a[k] - (double)m);
    return exp((double)a[c] - (double)m) / s;
}
// Variant v = (event b, token slot s): the base row a, the variant's row o, their width C and the class c that is compared.  prong: the
// predicted class of slot s - 1 from its own base logits; otherwise cls[b], or the predicted event class.  false: nothing to compare.
__device__ __forceinline__ bool class_choice(const float* base_ev, const float* base_pr, const float* var_ev, const float* var_pr, long v,
                                             int b, int s, int P, int Ce, int Cp, int prong, const int* cls, const float*& a,
                                             const float*& o, int& C, int& c) {
    if (prong) {
        if (s == 0) return false;
        a = base_pr + ((long)b * P + (s - 1)) * Cp; o = var_pr + ((long)v * P + (s - 1)) * Cp; C = Cp;
        c = argmax_row(a, C);
        return true;
    }
    a = base_ev + (long)b * Ce; o = var_ev + (long)v * Ce; C = Ce;
    c = cls ? cls[b] : argmax_row(a, C);
    return c >= 0 && c < C;
}

// ---- host routines of a list call and of a build call ------------------------------------------------------------------------------------------
inline bool list_pointers_ok(const void* coords, long nnz, const void* img_bs, const void* vimg, const void* index, const void* workspace,
                             const void* host_out) {
    return (coords || nnz == 0) && img_bs && vimg && index && workspace && host_out && nnz >= 0;
}
inline int list_room(const char* who, const ListLayout& o, long workspace_bytes, long host_cap) {
    if (workspace_bytes >= o.total && host_cap >= 4 + o.nb + 1) return 0;
    fprintf(stderr, "tcvn: %s: workspace of %ld bytes (%ld needed) or host buffer of %ld words (%d needed) too small\n", who,
            workspace_bytes, o.total, host_cap, 4 + o.nb + 1);
    return -12;
}
// zero the counters and the header, then count (keep_map: see k_occ_count)
inline int list_count(const ListLayout& o, char* w, const int* coords, long nnz, int n_img, int H, int W, int th, int tw,
                      const int* img_bs, const unsigned char* keep_map, int B, int S, int pHt, int pWt, hipStream_t st) {
    TCVN_CHECK(hipMemsetAsync(w + o.cnt, 0, (size_t)(o.img_start - o.cnt), st));           // cnt, nnz_img and flags are adjacent
    TCVN_CHECK(hipMemsetAsync(w + o.hdr, 0, (size_t)(4 + o.nb + 1) * 8, st));
    if (nnz == 0) return 0;
    hipLaunchKernelGGL(k_occ_count, dim3(cdiv(nnz, 256)), dim3(256), 0, st, coords, nnz, n_img, H, W, th, tw, o.Wt, o.T, img_bs, keep_map,
                       B, S, pHt, pWt, reinterpret_cast<int*>(w + o.cnt), reinterpret_cast<int*>(w + o.nnz_img),
                       reinterpret_cast<int*>(w + o.flags));
    TCVN_LAUNCH_CHECK();
    return 0;
}
// V, the two flags and the pass boundaries: the one synchronisation of a scan over this hit list
inline int list_read_header(const ListLayout& o, const char* w, int64_t* host_out, hipStream_t st) {
    TCVN_CHECK(hipMemcpyAsync(host_out, w + o.hdr, (size_t)(4 + o.nb + 1) * 8, hipMemcpyDeviceToHost, st));
    TCVN_CHECK(hipStreamSynchronize(st));
    return 0;
}
inline bool build_args_ok(const void* coords, const void* values, long nnz, int channels, const void* vimg, const void* workspace,
                          int max_pass, int first, int count, const void* out_coords, const void* out_values, long out_rows) {
    return coords && values && vimg && workspace && out_coords && out_values && nnz >= 1 && channels >= 1 && first >= 0 && count >= 1 &&
           count <= max_pass && out_rows >= 0;
}
// the hit lists of variants first .. first + count - 1 of a list laid out as `o` (the caller has checked the arguments)
template <class Keep>
int list_build_pass(const char* who, const ListLayout& o, const int* coords, const float* values, int channels, int n_img, int H, int W,
                    int th, int tw, const int* vimg, const void* workspace, long workspace_bytes, int first, int count, Keep keep,
                    int* out_coords, float* out_values, long out_rows, void* stream) {
    if (workspace_bytes < o.total) {
        fprintf(stderr, "tcvn: %s: workspace of %ld bytes, %ld needed\n", who, workspace_bytes, o.total);
        return -12;
    }
    const char* w = reinterpret_cast<const char*>(workspace);
    hipLaunchKernelGGL(k_list_build<Keep>, dim3(count), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), coords, values, channels, H,
                       W, th, tw, o.Wt, reinterpret_cast<const long*>(w + o.img_start), vimg,
                       reinterpret_cast<const int*>(w + o.payload), reinterpret_cast<const long*>(w + o.voff), first, n_img, keep,
                       out_coords, out_values, out_rows);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

}  // namespace tcvn
