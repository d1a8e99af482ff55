// Occlusion maps (forward only): which tiles of which pixel maps hold hits, the hit lists of the variants "this map without the hits of
// that tile", the variant rows / sequences of the token path and the heat map of softmax differences.
// The maps are COO hit lists, so a variant is a filtered copy of its image's rows in their original order (the stem's rule for duplicate
// coordinates is "highest index wins"); only tiles that hold a hit are variants.  Integer atomics only: every result is deterministic.
#include "../../include/tcvn_hip.h"
#include "tcvn_occlude.h"
#include "occlude_list.h"

namespace tcvn {

namespace {

// ---- 1-3. the variant list (occlude_list.h): a row is a tile, a variant every tile that holds an admitted hit ----------------------------------
__global__ __launch_bounds__(LIST_T) void k_occ_list(const int* __restrict__ cnt, const int* __restrict__ nnz_img, const int* flags,
                                                     const int* __restrict__ img_bs, int n_img, int T, int Wt, long cells, int max_pass,
                                                     long* img_start, int* vimg, int* vtile, long* voff, int* index, long* hdr) {
    auto tile_row = [=](long c) {
        const int k = cnt[c], img = (int)(c / T), tile = (int)(c - (long)img * T);
        return ListRow{k > 0, (long)(nnz_img[img] - k), img, tile, tile / Wt, tile - (tile / Wt) * Wt};
    };
    variant_list(tile_row, cells, nnz_img, flags, img_bs, n_img, max_pass, img_start, vimg, vtile, voff, index, hdr);
}
// the variant of a tile keeps every hit but that tile's (a hit outside the map is in no tile)
struct KeepOtherTiles {
    __device__ bool operator()(bool in, int cell, int, int tile) const { return !(in && cell == tile); }
};

// ---- 4. token path: variant rows and variant sequences ----------------------------------------------------------------------------------
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

// ---- 5. heat map: softmax(base)[c] - softmax(occluded)[c] at every variant's position -------------------------------------------------
__global__ __launch_bounds__(256) void k_occ_heat(const float* base_ev, const float* base_pr, const float* occ_ev, const float* occ_pr,
                                                  const int* index, long V, int P, int Ce, int Cp, int Ht, int Wt, int prong,
                                                  const int* cls, float* out) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int b = index[4 * v], s = index[4 * v + 1], ty = index[4 * v + 2], tx = index[4 * v + 3];
    const float *a, *o;
    int C, c;
    if (!class_choice(base_ev, base_pr, occ_ev, occ_pr, v, b, s, P, Ce, Cp, prong, cls, a, o, C, c)) return;
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
    ListLayout o;
    return list_layout(n_img, height, width, tile_h, tile_w, 0, max_pass, o) ? o.total : -1;
}

// The variant list of one hit list: flat (keep_map == NULL) or restricted to the children of the parent level's selected tiles.
static int occ_variant_list(const char* who, const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                            const int32_t* img_bs, const uint8_t* keep_map, int batch, int max_prongs, int parent_grid_h,
                            int parent_grid_w, int max_pass, int32_t* vimg, int32_t* index, void* workspace, int64_t workspace_bytes,
                            int64_t* host_out, int64_t host_cap, void* stream) {
    ListLayout o;
    if (!list_pointers_ok(coords, nnz, img_bs, vimg, index, workspace, host_out) ||
        !list_layout(n_img, height, width, tile_h, tile_w, 0, max_pass, o)) {
        fprintf(stderr, "tcvn: %s: bad argument (NULL pointer, n_img / map / tile < 1, max_pass outside 1..%d or more than 2^31 tiles)\n",
                who, TCVN_OCC_MAX_PASS);
        return -1;
    }
    if (int rc = list_room(who, o, workspace_bytes, host_cap)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* w = reinterpret_cast<char*>(workspace);
    if (int rc = list_count(o, w, coords, nnz, n_img, height, width, tile_h, tile_w, img_bs, keep_map, batch, 1 + max_prongs,
                            parent_grid_h, parent_grid_w, st))
        return rc;
    hipLaunchKernelGGL(k_occ_list, dim3(1), dim3(LIST_T), 0, st, reinterpret_cast<const int*>(w + o.cnt),
                       reinterpret_cast<const int*>(w + o.nnz_img), reinterpret_cast<const int*>(w + o.flags), img_bs, n_img, o.T, o.Wt,
                       o.cells, max_pass, reinterpret_cast<long*>(w + o.img_start), vimg, reinterpret_cast<int*>(w + o.payload),
                       reinterpret_cast<long*>(w + o.voff), index, reinterpret_cast<long*>(w + o.hdr));
    TCVN_LAUNCH_CHECK();
    return list_read_header(o, w, host_out, st);
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
    ListLayout o;
    if (!build_args_ok(coords, values, nnz, channels, vimg, workspace, max_pass, first, count, out_coords, out_values, out_rows) ||
        !list_layout(n_img, height, width, tile_h, tile_w, 0, max_pass, o) || (long)first + count > o.rows) {
        fprintf(stderr, "tcvn: occlusion_build_pass: bad argument (NULL pointer, empty hit list, tile < 1, count outside 1..max_pass or variants beyond the tile count)\n");
        return -1;
    }
    return list_build_pass("occlusion_build_pass", o, coords, values, channels, n_img, height, width, tile_h, tile_w, vimg, workspace,
                           workspace_bytes, first, count, KeepOtherTiles{}, out_coords, out_values, out_rows, stream);
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
