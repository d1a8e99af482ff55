// Device code shared by the occlusion kernels (occlude.hip, occlude_curve.hip): the occupancy count of a hit list, the workgroup prefix sum
// of the ordered compactions and the double-precision softmax of the heat map and the curves.  Every translation unit gets its own copy.
#pragma once
#include "tcvn_common.h"

namespace tcvn {

namespace {

// ---- occupancy: one thread per hit -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_occ_count(const int* __restrict__ coords, long nnz, int n_img, int H, int W, int th, int tw,
                                                   int Wt, int T, int* cnt, int* nnz_img, int* flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const int img = coords[3 * i], y = coords[3 * i + 1], x = coords[3 * i + 2];
    if (i > 0 && coords[3 * (i - 1)] > img) atomicOr(&flags[0], 1);                      // the list is not sorted by image
    if (img < 0 || img >= n_img || y < 0 || y >= H || x < 0 || x >= W) { atomicOr(&flags[1], 1); return; }   // a hit the embedders drop
    atomicAdd(&cnt[(long)img * T + (y / th) * Wt + x / tw], 1);
    atomicAdd(&nnz_img[img], 1);
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

}  // namespace

}  // namespace tcvn
