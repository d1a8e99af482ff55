// Coarse-to-fine occlusion maps (forward only): which variants of one level are refined, which tiles of a level were evaluated, which
// cells of the finest grid hold a hit, and the final map painted from the levels' stored heat values.  The variant list of a refined
// level itself is built in occlude.hip (k_occ_count with the parent level's keep_map in front of the same list and build kernels).
// The only atomic is an integer atomicMax on the bit pattern of a non-negative float: every result is deterministic.
#include "../../include/tcvn_hip.h"
#include "tcvn_common.h"

namespace tcvn {

namespace {

// (b, s, ty, tx) of variant v -> its place in a [B, S, Ht, Wt] map and its group, or false when the row lies outside the map
__device__ __forceinline__ bool variant_at(const int* __restrict__ index, long v, int B, int S, int Ht, int Wt, int per_map, long& at,
                                           int& group) {
    const int b = index[4 * v], s = index[4 * v + 1], ty = index[4 * v + 2], tx = index[4 * v + 3];
    if (b < 0 || b >= B || s < 0 || s >= S || ty < 0 || ty >= Ht || tx < 0 || tx >= Wt) return false;
    at = (((long)b * S + s) * Ht + ty) * Wt + tx;
    group = per_map ? b * S + s : b;
    return true;
}

// ---- 1. selection: group maxima of score = |h|, then the threshold -------------------------------------------------------------------------
// The bit patterns of non-negative floats order as the floats do, so an unsigned atomicMax gives the maximum whatever the order.
__global__ __launch_bounds__(256) void k_sel_max(const float* __restrict__ heat, const int* __restrict__ index, long V, int B, int S,
                                                 int Ht, int Wt, int per_map, unsigned* gmax) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    long at;
    int g;
    if (!variant_at(index, v, B, S, Ht, Wt, per_map, at, g)) return;
    atomicMax(&gmax[g], __float_as_uint(fabsf(heat[at])));
}
__global__ __launch_bounds__(256) void k_sel_mark(const float* __restrict__ heat, const int* __restrict__ index, long V, int B, int S,
                                                  int Ht, int Wt, int per_map, const unsigned* __restrict__ gmax, float keep,
                                                  unsigned char* keep_map) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    long at;
    int g;
    if (!variant_at(index, v, B, S, Ht, Wt, per_map, at, g)) return;
    const float score = fabsf(heat[at]), bound = __fmul_rn(keep, __uint_as_float(gmax[g]));      // one float32 multiplication
    keep_map[at] = (score >= bound && (keep == 0.f || score > 0.f)) ? 1 : 0;
}

// ---- 2. which tiles of a level were evaluated: one thread per variant ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_occ_mark(const int* __restrict__ index, long V, int B, int S, int Ht, int Wt,
                                                  unsigned char* map) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    long at;
    int g;
    if (variant_at(index, v, B, S, Ht, Wt, 0, at, g)) map[at] = 1;
}

// ---- 3. occupancy of a grid: one thread per hit (every writer of a cell stores the same byte) ----------------------------------------------
__global__ __launch_bounds__(256) void k_occ_occupied(const int* __restrict__ coords, long nnz, int n_img, int H, int W, int th, int tw,
                                                      const int* __restrict__ img_bs, int B, int S, int Ht, int Wt,
                                                      unsigned char* map) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const int img = coords[3 * i], y = coords[3 * i + 1], x = coords[3 * i + 2];
    if (img < 0 || img >= n_img || y < 0 || y >= H || x < 0 || x >= W) return;               // a hit the embedders drop
    const int b = img_bs[2 * img], s = img_bs[2 * img + 1];
    if (b < 0 || b >= B || s < 0 || s >= S) return;
    map[(((long)b * S + s) * Ht + y / th) * Wt + x / tw] = 1;
}

// ---- 4. painting: one thread per cell of the finest grid; a pure selection of stored values ------------------------------------------------
struct PaintLevels {
    const float* heat[TCVN_OCC_MAX_LEVELS];
    const unsigned char* evaluated[TCVN_OCC_MAX_LEVELS];
    int gh[TCVN_OCC_MAX_LEVELS], gw[TCVN_OCC_MAX_LEVELS];
    int levels;
};
__global__ __launch_bounds__(256) void k_occ_paint(PaintLevels L, const unsigned char* __restrict__ occupied, long cells, int maps,
                                                   float* out) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const int last = L.levels - 1, Hf = L.gh[last], Wf = L.gw[last];
    const int x = (int)(c % Wf), y = (int)((c / Wf) % Hf);
    const long m = c / ((long)Hf * Wf);                                                      // the map (b, s)
    float h = 0.f;
    if (m < maps && occupied[c]) {
        for (int l = last; l >= 0; --l) {                                                    // the deepest evaluated tile that holds the cell
            const int sh = last - l;
            const long at = (m * L.gh[l] + (y >> sh)) * L.gw[l] + (x >> sh);
            if (L.evaluated[l][at]) { h = L.heat[l][at]; break; }
        }
    }
    out[c] = h;
}

}  // namespace

}  // namespace tcvn

using namespace tcvn;

extern "C" {

int tcvn_occlusion_select(const float* heat, const int32_t* index, int64_t n_variants, int batch, int max_prongs, int grid_h,
                          int grid_w, int group, float keep, uint32_t* group_max, uint8_t* keep_map, void* stream) {
    if (!heat || !group_max || !keep_map || (n_variants > 0 && !index) || n_variants < 0 || batch < 1 || max_prongs < 0 || grid_h < 1 ||
        grid_w < 1 || (group != TCVN_OCC_GROUP_EVENT && group != TCVN_OCC_GROUP_MAP) || !(keep >= 0.f && keep <= 1.f)) {
        fprintf(stderr, "tcvn: occlusion_select: bad argument (NULL pointer, batch / grid < 1, unknown group or keep outside [0, 1])\n");
        return -1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int S = 1 + max_prongs;
    TCVN_CHECK(hipMemsetAsync(group_max, 0, (size_t)batch * S * 4, st));
    TCVN_CHECK(hipMemsetAsync(keep_map, 0, (size_t)batch * S * grid_h * grid_w, st));
    if (n_variants == 0) return 0;
    const int per_map = group == TCVN_OCC_GROUP_MAP ? 1 : 0;
    hipLaunchKernelGGL(k_sel_max, dim3(cdiv(n_variants, 256)), dim3(256), 0, st, heat, index, (long)n_variants, batch, S, grid_h, grid_w,
                       per_map, group_max);
    TCVN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sel_mark, dim3(cdiv(n_variants, 256)), dim3(256), 0, st, heat, index, (long)n_variants, batch, S, grid_h, grid_w,
                       per_map, group_max, keep, keep_map);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_occlusion_mark(const int32_t* index, int64_t n_variants, int batch, int max_prongs, int grid_h, int grid_w, uint8_t* evaluated,
                        void* stream) {
    if (!evaluated || (n_variants > 0 && !index) || n_variants < 0 || batch < 1 || max_prongs < 0 || grid_h < 1 || grid_w < 1) {
        fprintf(stderr, "tcvn: occlusion_mark: bad argument (NULL pointer or batch / grid < 1)\n");
        return -1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    TCVN_CHECK(hipMemsetAsync(evaluated, 0, (size_t)batch * (1 + max_prongs) * grid_h * grid_w, st));
    if (n_variants == 0) return 0;
    hipLaunchKernelGGL(k_occ_mark, dim3(cdiv(n_variants, 256)), dim3(256), 0, st, index, (long)n_variants, batch, 1 + max_prongs, grid_h,
                       grid_w, evaluated);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_occlusion_occupancy(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                             const int32_t* img_bs, int batch, int max_prongs, uint8_t* occupied, void* stream) {
    if ((!coords && nnz > 0) || !img_bs || !occupied || nnz < 0 || n_img < 1 || height < 1 || width < 1 || tile_h < 1 || tile_w < 1 ||
        batch < 1 || max_prongs < 0) {
        fprintf(stderr, "tcvn: occlusion_occupancy: bad argument (NULL pointer or n_img / map / tile / batch < 1)\n");
        return -1;
    }
    if (nnz == 0) return 0;
    hipLaunchKernelGGL(k_occ_occupied, dim3(cdiv(nnz, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), coords, (long)nnz,
                       n_img, height, width, tile_h, tile_w, img_bs, batch, 1 + max_prongs, (height + tile_h - 1) / tile_h,
                       (width + tile_w - 1) / tile_w, occupied);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_occlusion_paint(int levels, const float* const* heat, const uint8_t* const* evaluated, const int32_t* grid_h,
                         const int32_t* grid_w, const uint8_t* occupied, int batch, int max_prongs, float* out, void* stream) {
    bool ok = heat && evaluated && grid_h && grid_w && occupied && out && levels >= 1 && levels <= TCVN_OCC_MAX_LEVELS && batch >= 1 &&
              max_prongs >= 0;
    PaintLevels L;
    for (int l = 0; ok && l < levels; ++l) {
        const int sh = levels - 1 - l;                 // tiles halve from level to level: grid l = ceil(finest grid / 2^sh)
        ok = heat[l] && evaluated[l] && grid_h[l] >= 1 && grid_w[l] >= 1 &&
             grid_h[l] == (int)(((long)grid_h[levels - 1] + (1L << sh) - 1) >> sh) &&
             grid_w[l] == (int)(((long)grid_w[levels - 1] + (1L << sh) - 1) >> sh);
        L.heat[l] = heat[l]; L.evaluated[l] = evaluated[l]; L.gh[l] = grid_h[l]; L.gw[l] = grid_w[l];
    }
    if (!ok) {
        fprintf(stderr, "tcvn: occlusion_paint: bad argument (NULL pointer, levels outside 1..%d, batch < 1 or grids that do not halve from level to level)\n",
                TCVN_OCC_MAX_LEVELS);
        return -1;
    }
    L.levels = levels;
    const int maps = batch * (1 + max_prongs);
    const long cells = (long)maps * grid_h[levels - 1] * grid_w[levels - 1];
    hipLaunchKernelGGL(k_occ_paint, dim3(cdiv(cells, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), L, occupied, cells, maps,
                       out);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
