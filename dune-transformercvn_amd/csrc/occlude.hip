// Occlusion maps (forward only): which tiles of which pixel maps hold hits, the hit lists of the variants "this map without the hits of
// that tile", the variant rows / sequences of the token path and the heat map of softmax differences.
// The maps are COO hit lists, so a variant is a filtered copy of its image's rows in their original order (the stem's rule for duplicate
// coordinates is "highest index wins"); only tiles that hold a hit are variants.  Integer atomics only: every result is deterministic.
#include "../../include/tcvn_hip.h"
#include "tcvn_occlude.h"
#include "occlude_dev.h"

namespace tcvn {

namespace {

// Workspace of the variant list of one hit list (n_img images, Ht x Wt tiles each).
struct OccLayout { long cnt, nnz_img, flags, img_start, vtile, voff, hdr, total; long cells; int nb; };
bool occ_layout(int n_img, int H, int W, int th, int tw, int max_pass, OccLayout& o) {
    const long Ht = (H + th - 1) / th, Wt = (W + tw - 1) / tw;
    o.cells = (long)n_img * Ht * Wt;
    if (o.cells > 0x7fffffffL - 1024) return false;
    o.nb = (int)((o.cells + max_pass - 1) / max_pass);
    long off = 0;
    auto take = [&](long bytes) { long at = off; off += round_up(bytes, 256); return at; };
    o.cnt = take(o.cells * 4); o.nnz_img = take((long)n_img * 4); o.flags = take(16); o.img_start = take(((long)n_img + 1) * 8);
    o.vtile = take(o.cells * 4); o.voff = take((o.cells + 1) * 8); o.hdr = take((4L + o.nb + 1) * 8);
    o.total = off;
    return true;
}

// ---- 1. occupancy: one thread per hit (k_occ_count, occlude_dev.h) ------------------------------------------------------------------
// refinement: the same pass, but a hit enters cnt only where the parent level's keep_map is set at its parent tile (tiles of 2*th x 2*tw);
// nnz_img and the two flags still see every hit, so a variant's surviving hits stay "the whole image minus that one tile"
__global__ __launch_bounds__(256) void k_occ_count_kept(const int* __restrict__ coords, long nnz, int n_img, int H, int W, int th, int tw,
                                                        int Wt, int T, const int* __restrict__ img_bs,
                                                        const unsigned char* __restrict__ keep_map, int B, int S, int pHt, int pWt,
                                                        int* cnt, int* nnz_img, int* flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const int img = coords[3 * i], y = coords[3 * i + 1], x = coords[3 * i + 2];
    if (i > 0 && coords[3 * (i - 1)] > img) atomicOr(&flags[0], 1);
    if (img < 0 || img >= n_img || y < 0 || y >= H || x < 0 || x >= W) { atomicOr(&flags[1], 1); return; }
    atomicAdd(&nnz_img[img], 1);
    const int b = img_bs[2 * img], s = img_bs[2 * img + 1], py = y / (2 * th), px = x / (2 * tw);
    if (b < 0 || b >= B || s < 0 || s >= S || py >= pHt || px >= pWt) return;            // no such parent: never a variant
    if (keep_map[(((long)b * S + s) * pHt + py) * pWt + px]) atomicAdd(&cnt[(long)img * T + (y / th) * Wt + x / tw], 1);
}

// ---- 2. variant list: ordered compaction of the occupied cells; one workgroup walks the cells in chunks -----------------------------------
// (block_scan_excl: occlude_dev.h)
constexpr int CT = 1024;
__global__ __launch_bounds__(CT) void k_occ_compact(const int* __restrict__ cnt, const int* __restrict__ nnz_img, const int* flags,
                                                    const int* __restrict__ img_bs, int n_img, int T, int Wt, long cells, int max_pass,
                                                    long* img_start, int* vimg, int* vtile, long* voff, int* index, long* hdr) {
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
    long nv = 0, nh = 0;                                     // variants / surviving hits in front of this chunk
    long* bounds = hdr + 4;
    for (long base = 0; base < cells; base += CT) {
        const long c = base + tid;
        int k = 0, img = 0;
        if (c < cells) { k = cnt[c]; img = (int)(c / T); }
        const long flag = k > 0 ? 1 : 0, surv = k > 0 ? (long)(nnz_img[img] - k) : 0;
        long tv, th_;
        const long pos = nv + block_scan_excl(flag, wsum, tv);
        const long at = nh + block_scan_excl(surv, wsum, th_);
        if (flag) {
            const int tile = (int)(c - (long)img * T);
            vimg[pos] = img; vtile[pos] = tile; voff[pos] = at;
            index[4 * pos] = img_bs[2 * img]; index[4 * pos + 1] = img_bs[2 * img + 1];
            index[4 * pos + 2] = tile / Wt; index[4 * pos + 3] = tile - (tile / Wt) * Wt;
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
__global__ __launch_bounds__(256) void k_occ_build(const int* __restrict__ coords, const float* __restrict__ values, int C, int H, int W,
                                                   int th, int tw, int Wt, const long* __restrict__ img_start,
                                                   const int* __restrict__ vimg, const int* __restrict__ vtile,
                                                   const long* __restrict__ voff, int first, int n_img, int* out_coords,
                                                   float* out_values, long out_cap) {
    __shared__ int wcnt[4];
    const int j = blockIdx.x, v = first + j, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int img = vimg[v], tile = vtile[v];
    if (img < 0 || img >= n_img) return;             // not a variant of this list (whole workgroup: no barrier is skipped by a part of it)
    const long lo = img_start[img], hi = img_start[img + 1];
    long dst = voff[v] - voff[first];
    for (long base = lo; base < hi; base += 256) {
        const long i = base + tid;
        bool keep = false;
        int y = 0, x = 0;
        if (i < hi) {
            y = coords[3 * i + 1]; x = coords[3 * i + 2];
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            keep = !(in && (y / th) * Wt + x / tw == tile);
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

// ---- 5. token path: variant rows and variant sequences ----------------------------------------------------------------------------------
__global__ void k_occ_rows(const float* rows, const int* vimg, int row_base, const float* emb, long emb_ld, int col0, int width,
                           float* vrows, int* ident, int in_dim, int n_rows) {
    const int j = blockIdx.x;
    const int r = row_base + vimg[j];
    const float* src = rows + (long)(r >= 0 && r < n_rows ? r : 0) * in_dim;
    const float* e = emb + (long)j * emb_ld;
    for (int c = threadIdx.x; c < in_dim; c += blockDim.x)
        vrows[(long)j * in_dim + c] = (c >= col0 && c < col0 + width) ? e[c - col0] : src[c];
    if (threadIdx.x == 0) ident[j] = j;
}
__global__ void k_occ_gather(const float* tokens, const int* tok_row, const int* index, const float* vtok, float* X0, int* vrow, int n,
                             int B, int S, int D) {
    const int t = blockIdx.x;                       // t = s*n + j
    const int s = t / n, j = t - s * n;
    const int b = index[4 * j], slot = index[4 * j + 1];
    const bool valid = b >= 0 && b < B && tok_row[b * S + s] >= 0;
    const float* src = s == slot ? vtok + (long)j * D : tokens + ((long)b * S + s) * D;
    for (int d = threadIdx.x; d < D; d += blockDim.x) X0[(long)t * D + d] = valid ? src[d] : 0.f;
    if (threadIdx.x == 0) vrow[j * S + s] = valid ? 0 : -1;
}

// ---- 6. heat map: softmax(base)[c] - softmax(occluded)[c] at every variant's position -------------------------------------------------
__global__ __launch_bounds__(256) void k_occ_heat(const float* base_ev, const float* base_pr, const float* occ_ev, const float* occ_pr,
                                                  const int* index, long V, int P, int Ce, int Cp, int Ht, int Wt, int prong,
                                                  const int* cls, float* out) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int b = index[4 * v], s = index[4 * v + 1], ty = index[4 * v + 2], tx = index[4 * v + 3];
    const float *a, *o;
    int C, c;
    if (prong) {
        if (s == 0) return;
        a = base_pr + ((long)b * P + (s - 1)) * Cp; o = occ_pr + ((long)v * P + (s - 1)) * Cp; C = Cp;
        c = argmax_row(a, C);
    } else {
        a = base_ev + (long)b * Ce; o = occ_ev + (long)v * Ce; C = Ce;
        c = cls ? cls[b] : argmax_row(a, C);
        if (c < 0 || c >= C) return;
    }
    out[(((long)b * (1 + P) + s) * Ht + ty) * Wt + tx] = (float)(softmax_at(a, C, c) - softmax_at(o, C, c));
}

}  // namespace

int occ_rows(const float* rows, const int* vimg, int row_base, const float* emb, long emb_ld, int col0, int width, float* vrows,
             int* ident, int n, int in_dim, int n_rows, hipStream_t st) {
    hipLaunchKernelGGL(k_occ_rows, dim3(n), dim3(128), 0, st, rows, vimg, row_base, emb, emb_ld, col0, width, vrows, ident, in_dim,
                       n_rows);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int occ_gather(const float* tokens, const int* tok_row, const int* index, const float* vtok, float* X0, int* vrow, int n, int B, int S,
               int D, hipStream_t st) {
    hipLaunchKernelGGL(k_occ_gather, dim3(S * n), dim3(128), 0, st, tokens, tok_row, index, vtok, X0, vrow, n, B, S, D);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace tcvn

using namespace tcvn;

extern "C" {

int64_t tcvn_occlusion_workspace_bytes(int n_img, int height, int width, int tile_h, int tile_w, int max_pass) {
    OccLayout o;
    if (n_img < 1 || height < 1 || width < 1 || tile_h < 1 || tile_w < 1 || max_pass < 1 || max_pass > TCVN_OCC_MAX_PASS ||
        !occ_layout(n_img, height, width, tile_h, tile_w, max_pass, o))
        return -1;
    return o.total;
}

// The variant list of one hit list: flat (keep_map == NULL) or restricted to the children of the parent level's selected tiles.
static int occ_variant_list(const char* who, const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                            const int32_t* img_bs, const uint8_t* keep_map, int batch, int max_prongs, int parent_grid_h,
                            int parent_grid_w, int max_pass, int32_t* vimg, int32_t* index, void* workspace, int64_t workspace_bytes,
                            int64_t* host_out, int64_t host_cap, void* stream) {
    OccLayout o;
    if ((!coords && nnz > 0) || !img_bs || !vimg || !index || !workspace || !host_out || nnz < 0 || n_img < 1 || height < 1 ||
        width < 1 || tile_h < 1 || tile_w < 1 || max_pass < 1 || max_pass > TCVN_OCC_MAX_PASS ||
        !occ_layout(n_img, height, width, tile_h, tile_w, max_pass, o)) {
        fprintf(stderr, "tcvn: %s: bad argument (NULL pointer, n_img / map / tile < 1, max_pass outside 1..%d or more than 2^31 tiles)\n",
                who, TCVN_OCC_MAX_PASS);
        return -1;
    }
    if (workspace_bytes < o.total || host_cap < 4 + o.nb + 1) {
        fprintf(stderr, "tcvn: %s: workspace of %lld bytes (%ld needed) or host buffer of %lld words (%d needed) too small\n", who,
                (long long)workspace_bytes, o.total, (long long)host_cap, 4 + o.nb + 1);
        return -12;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* w = reinterpret_cast<char*>(workspace);
    const int Wt = (width + tile_w - 1) / tile_w, T = ((height + tile_h - 1) / tile_h) * Wt;
    int* cnt = reinterpret_cast<int*>(w + o.cnt);
    int* nnz_img = reinterpret_cast<int*>(w + o.nnz_img);
    int* flags = reinterpret_cast<int*>(w + o.flags);
    long* hdr = reinterpret_cast<long*>(w + o.hdr);
    TCVN_CHECK(hipMemsetAsync(w + o.cnt, 0, (size_t)(o.img_start - o.cnt), st));           // cnt, nnz_img and flags are adjacent
    TCVN_CHECK(hipMemsetAsync(hdr, 0, (size_t)(4 + o.nb + 1) * 8, st));
    if (nnz > 0 && !keep_map) {
        hipLaunchKernelGGL(k_occ_count, dim3(cdiv(nnz, 256)), dim3(256), 0, st, coords, (long)nnz, n_img, height, width, tile_h, tile_w,
                           Wt, T, cnt, nnz_img, flags);
        TCVN_LAUNCH_CHECK();
    } else if (nnz > 0) {
        hipLaunchKernelGGL(k_occ_count_kept, dim3(cdiv(nnz, 256)), dim3(256), 0, st, coords, (long)nnz, n_img, height, width, tile_h,
                           tile_w, Wt, T, img_bs, keep_map, batch, 1 + max_prongs, parent_grid_h, parent_grid_w, cnt, nnz_img, flags);
        TCVN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_occ_compact, dim3(1), dim3(CT), 0, st, cnt, nnz_img, flags, img_bs, n_img, T, Wt, o.cells, max_pass,
                       reinterpret_cast<long*>(w + o.img_start), vimg, reinterpret_cast<int*>(w + o.vtile),
                       reinterpret_cast<long*>(w + o.voff), index, hdr);
    TCVN_LAUNCH_CHECK();
    // V, the two flags and the pass boundaries: the one synchronisation of the scan over this hit list
    TCVN_CHECK(hipMemcpyAsync(host_out, hdr, (size_t)(4 + o.nb + 1) * 8, hipMemcpyDeviceToHost, st));
    TCVN_CHECK(hipStreamSynchronize(st));
    return 0;
}

int tcvn_occlusion_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                            const int32_t* img_bs, int max_pass, int32_t* vimg, int32_t* index, void* workspace,
                            int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream) {
    return occ_variant_list("occlusion_variants", coords, nnz, n_img, height, width, tile_h, tile_w, img_bs, nullptr, 0, 0, 0, 0,
                            max_pass, vimg, index, workspace, workspace_bytes, host_out, host_cap, stream);
}

int tcvn_occlusion_refine_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                                   const int32_t* img_bs, const uint8_t* keep_map, int batch, int max_prongs, int parent_grid_h,
                                   int parent_grid_w, int max_pass, int32_t* vimg, int32_t* index, void* workspace,
                                   int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream) {
    // the parent level's tiles are (2 * tile_h, 2 * tile_w): its grid is fixed by the map, and every hit inside the map has a parent
    if (!keep_map || batch < 1 || max_prongs < 0 || height < 1 || width < 1 || tile_h < 1 || tile_w < 1 || tile_h > 0x3fffffff ||
        tile_w > 0x3fffffff || parent_grid_h != (height + 2 * tile_h - 1) / (2 * tile_h) ||
        parent_grid_w != (width + 2 * tile_w - 1) / (2 * tile_w)) {
        fprintf(stderr, "tcvn: occlusion_refine_variants: bad argument (no keep_map, batch < 1, max_prongs < 0 or a parent grid that is not that of tiles twice the size)\n");
        return -1;
    }
    return occ_variant_list("occlusion_refine_variants", coords, nnz, n_img, height, width, tile_h, tile_w, img_bs, keep_map, batch,
                            max_prongs, parent_grid_h, parent_grid_w, max_pass, vimg, index, workspace, workspace_bytes, host_out,
                            host_cap, stream);
}

int tcvn_occlusion_build_pass(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height, int width,
                              int tile_h, int tile_w, int max_pass, const int32_t* vimg, const void* workspace, int64_t workspace_bytes,
                              int first, int count, int32_t* out_coords, float* out_values, int64_t out_rows, void* stream) {
    OccLayout o;
    if (!coords || !values || !vimg || !workspace || !out_coords || !out_values || nnz < 1 || channels < 1 || n_img < 1 || height < 1 ||
        width < 1 || tile_h < 1 || tile_w < 1 || max_pass < 1 || max_pass > TCVN_OCC_MAX_PASS || first < 0 || count < 1 ||
        count > max_pass || out_rows < 0 || !occ_layout(n_img, height, width, tile_h, tile_w, max_pass, o) ||
        (long)first + count > o.cells) {
        fprintf(stderr, "tcvn: occlusion_build_pass: bad argument (NULL pointer, empty hit list, tile < 1, count outside 1..max_pass or variants beyond the tile count)\n");
        return -1;
    }
    if (workspace_bytes < o.total) {
        fprintf(stderr, "tcvn: occlusion_build_pass: workspace of %lld bytes, %ld needed\n", (long long)workspace_bytes, o.total);
        return -12;
    }
    const char* w = reinterpret_cast<const char*>(workspace);
    const int Wt = (width + tile_w - 1) / tile_w;
    hipLaunchKernelGGL(k_occ_build, dim3(count), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), coords, values, channels, height,
                       width, tile_h, tile_w, Wt, reinterpret_cast<const long*>(w + o.img_start), vimg,
                       reinterpret_cast<const int*>(w + o.vtile), reinterpret_cast<const long*>(w + o.voff), first, n_img,
                       out_coords, out_values, (long)out_rows);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_occlusion_heatmap(const float* event_logits, const float* prong_logits, const float* occluded_event_logits,
                           const float* occluded_prong_logits, const int32_t* index, int64_t n_variants, int batch, int max_prongs,
                           int event_classes, int prong_classes, int grid_h, int grid_w, int target, const int32_t* classes,
                           float* heatmap, void* stream) {
    const bool prong = target == TCVN_OCC_TARGET_PRONG;
    if (!heatmap || n_variants < 0 || batch < 1 || max_prongs < 0 || grid_h < 1 || grid_w < 1 ||
        (target != TCVN_OCC_TARGET_EVENT && !prong) || (prong && classes) ||
        (n_variants > 0 && (!index || (prong ? (!prong_logits || !occluded_prong_logits || prong_classes < 1)
                                             : (!event_logits || !occluded_event_logits || event_classes < 1))))) {
        fprintf(stderr, "tcvn: occlusion_heatmap: bad argument (NULL pointer, batch / grid / classes < 1, unknown target or a class list with the prong target)\n");
        return -1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    TCVN_CHECK(hipMemsetAsync(heatmap, 0, (size_t)batch * (1 + max_prongs) * grid_h * grid_w * 4, st));
    if (n_variants == 0) return 0;
    hipLaunchKernelGGL(k_occ_heat, dim3(cdiv(n_variants, 256)), dim3(256), 0, st, event_logits, prong_logits, occluded_event_logits,
                       occluded_prong_logits, index, (long)n_variants, max_prongs, event_classes, prong_classes, grid_h, grid_w,
                       prong ? 1 : 0, classes, heatmap);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
