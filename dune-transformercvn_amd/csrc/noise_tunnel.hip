// Noise-averaged hit gradients (SmoothGrad, SmoothGrad^2, VarGrad): the element-wise kernels around the frozen pass of input_grad.hip.
//   * k_noise_range / k_noise_sigma: per map (b, s) the range max(0, max v) + max(0, -min v) over every value channel of every listed hit, and
//     sigma = noise * range.  max(v, 0) and max(-v, 0) are not negative, so their bit patterns order as unsigned integers: the two maxima
//     are integer atomics, order-independent, and sigma is exact whatever the launch does.
//   * k_noise_replicate: samples t0 .. t0 + R - 1 of one list as ONE list over R * n_img images, so that a frozen pass takes R samples at
//     once.  The draw of (sample t, pixel q = y * W + x, map m = b * (1 + P) + s, channel c) is one Philox-4x32-10 call with the counters
//     (q, m, t, 0x4e54554e + (c >> 2)) and a Box-Muller step in double; it knows nothing of the entry's place in the list, of the other
//     maps or of t0 / R, so duplicates share their draw and every split into passes gives the same bits.
//   * k_noise_accumulate: Welford's update of (mean, M2) in double for the gradient and for gradient x perturbed value; one thread owns an
//     element and folds the samples of the pass in ascending order.  The state lives in memory as doubles between samples, so a split at
//     any t0 runs the very same operations.
//   * k_noise_finish: mean, unbiased variance M2 / (T - 1) (NaN at T = 1) and mean square mean^2 + M2 / T, rounded to fp32 once.
// None of this is near the hot path: a few thousand hits times T against embedder passes of milliseconds.
#include <math.h>

#include "../../include/tcvn_hip.h"
#include "tcvn_common.h"

namespace tcvn {
namespace {

constexpr uint32_t NOISE_STREAM = 0x4e54554eu;
constexpr int NOISE_MAXC = 16;       // value channels per hit this file takes (the stem serves 1 .. 4)

// (b, s) of an image, or false where the table does not name a map of [batch, 1 + max_prongs]
__device__ __forceinline__ bool map_of(const int* __restrict__ img_bs, int img, int batch, int max_prongs, int& m) {
    const int b = img_bs[2 * img], s = img_bs[2 * img + 1];
    m = b * (1 + max_prongs) + s;
    return b >= 0 && b < batch && s >= 0 && s <= max_prongs;
}

__global__ __launch_bounds__(256) void k_noise_range(const int* __restrict__ coords, const float* __restrict__ values, long nnz, int C,
                                                     int n_img, int H, int W, uint32_t* range) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    int img, y, x;
    if (!hit_in_map(coords, i, n_img, H, W, img, y, x)) return;
    float hi = 0.f, lo = 0.f;
    for (int c = 0; c < C; ++c) {
        const float v = values[i * C + c];
        hi = fmaxf(hi, v);                 // (fmaxf drops a NaN: it moves neither bound)
        lo = fmaxf(lo, -v);
    }
    if (hi > 0.f) atomicMax(&range[2 * img], __float_as_uint(hi));
    if (lo > 0.f) atomicMax(&range[2 * img + 1], __float_as_uint(lo));
}

__global__ __launch_bounds__(256) void k_noise_sigma(const uint32_t* __restrict__ range, const int* __restrict__ img_bs, int n_img, int batch,
                                                     int max_prongs, double noise, float* sigma) {
    const int img = blockIdx.x * 256 + threadIdx.x;
    if (img >= n_img) return;
    int m;
    if (!map_of(img_bs, img, batch, max_prongs, m)) return;
    const double r = (double)__uint_as_float(range[2 * img]) + (double)__uint_as_float(range[2 * img + 1]);
    sigma[m] = (float)(noise * r);
}

__global__ __launch_bounds__(256) void k_noise_replicate(const int* __restrict__ coords, const float* __restrict__ values, long nnz, int C,
                                                         int n_img, int H, int W, const int* __restrict__ img_bs, int batch, int max_prongs,
                                                         const float* __restrict__ sigma, uint64_t seed, int t0, int reps, int* coords_out,
                                                         float* values_out) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nnz * reps) return;
    const int r = (int)(j / nnz);
    const long i = j - (long)r * nnz;
    int img, y, x, m = 0;
    const bool in = hit_in_map(coords, i, n_img, H, W, img, y, x);
    // an image index outside 0 .. n_img - 1 must not land on a map of another sample
    coords_out[3 * j] = (img < 0 || img >= n_img) ? -1 : img + r * n_img;
    coords_out[3 * j + 1] = y;
    coords_out[3 * j + 2] = x;
    const double sg = (in && map_of(img_bs, img, batch, max_prongs, m)) ? (double)sigma[m] : 0.0;
    const float* v = values + i * C;
    float* o = values_out + j * C;
    if (!(sg > 0.0)) {                     // outside the maps, an empty range or noise 0: the values as they are, bit for bit
        for (int c = 0; c < C; ++c) o[c] = v[c];
        return;
    }
    uint4 w = make_uint4(0, 0, 0, 0);
    for (int c = 0; c < C; ++c) {
        if ((c & 3) == 0)
            w = philox4((uint32_t)(y * W + x), (uint32_t)m, (uint32_t)(t0 + r), NOISE_STREAM + (uint32_t)(c >> 2), (uint32_t)seed,
                        (uint32_t)(seed >> 32));
        const uint32_t wa = (c & 2) ? w.z : w.x, wb = (c & 2) ? w.w : w.y;
        const double u1 = ((double)wa + 1.0) * 0x1p-32, u2 = (double)wb * 0x1p-32;
        const double rad = sqrt(-2.0 * log(u1)), ang = 2.0 * M_PI * u2;
        const double z = rad * ((c & 1) ? sin(ang) : cos(ang));
        o[c] = (float)fmax((double)v[c] + sg * z, 0.0);
    }
}

__device__ __forceinline__ void welford(double& mean, double& m2, double x, double n) {
    const double d = x - mean;
    mean += d / n;
    m2 += d * (x - mean);
}

// acc [4][count]: gradient mean, gradient M2, attribution mean, attribution M2
__global__ __launch_bounds__(256) void k_noise_accumulate(double* acc, const float* __restrict__ grads, const float* __restrict__ values,
                                                          long count, int t0, int reps) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double gm = acc[e], g2 = acc[count + e], am = acc[2 * count + e], a2 = acc[3 * count + e];
    if (t0 == 0) gm = g2 = am = a2 = 0.0;
    for (int r = 0; r < reps; ++r) {
        const double g = (double)grads[(long)r * count + e];
        const double a = g * (double)values[(long)r * count + e];       // exact: 24 x 24 bits
        const double n = (double)(t0 + r + 1);
        welford(gm, g2, g, n);
        welford(am, a2, a, n);
    }
    acc[e] = gm; acc[count + e] = g2; acc[2 * count + e] = am; acc[3 * count + e] = a2;
}

// stats [6][count]: gradient mean, variance, mean square; attribution mean, variance, mean square
__global__ __launch_bounds__(256) void k_noise_finish(const double* __restrict__ acc, long count, int T, float* stats) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    for (int k = 0; k < 2; ++k) {
        const double mean = acc[(2 * k) * count + e], m2 = acc[(2 * k + 1) * count + e];
        stats[(3 * k) * count + e] = (float)mean;
        stats[(3 * k + 1) * count + e] = T > 1 ? (float)(m2 / (double)(T - 1)) : __builtin_nanf("");
        stats[(3 * k + 2) * count + e] = (float)(mean * mean + m2 / (double)T);
    }
}

bool list_ok(const int32_t* coords, const float* values, int64_t nnz, int in_ch, int n_img, int height, int width, const int32_t* img_bs,
             int batch, int max_prongs) {
    return nnz >= 0 && (nnz == 0 || (coords && values)) && in_ch >= 1 && in_ch <= NOISE_MAXC && n_img >= 1 && height >= 1 && width >= 1 &&
           (long)height * width <= 0x7fffffffL && img_bs && batch >= 1 && max_prongs >= 0 && (long)batch * (1 + max_prongs) <= 0x7fffffffL;
}

}  // namespace
}  // namespace tcvn

using namespace tcvn;

extern "C" {

int64_t tcvn_noise_workspace_bytes(int n_img) { return n_img < 1 ? -1 : round_up((long)n_img * 8, 256); }

int tcvn_noise_sigma(const int32_t* coords, const float* values, int64_t nnz, int in_ch, int n_img, int height, int width,
                     const int32_t* img_bs, int batch, int max_prongs, double noise, float* sigma, void* workspace,
                     int64_t workspace_bytes, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!list_ok(coords, values, nnz, in_ch, n_img, height, width, img_bs, batch, max_prongs) || !sigma || !workspace || !(noise >= 0.0) ||
        !isfinite(noise)) {
        fprintf(stderr, "tcvn: noise_sigma: bad arguments\n");
        return -1;
    }
    const int64_t need = tcvn_noise_workspace_bytes(n_img);
    if (workspace_bytes < need) { fprintf(stderr, "tcvn: noise_sigma: workspace too small (%ld < %ld)\n", (long)workspace_bytes, (long)need); return -12; }
    uint32_t* range = reinterpret_cast<uint32_t*>(workspace);
    TCVN_CHECK(hipMemsetAsync(range, 0, (size_t)n_img * 8, st));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_noise_range, dim3(cdiv(nnz, 256)), dim3(256), 0, st, coords, values, (long)nnz, in_ch, n_img, height, width, range);
        TCVN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_noise_sigma, dim3(cdiv(n_img, 256)), dim3(256), 0, st, range, img_bs, n_img, batch, max_prongs, noise, sigma);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_noise_replicate(const int32_t* coords, const float* values, int64_t nnz, int in_ch, int n_img, int height, int width,
                         const int32_t* img_bs, int batch, int max_prongs, const float* sigma, uint64_t seed, int t0, int reps,
                         int32_t* coords_out, float* values_out, void* stream) {
    if (!list_ok(coords, values, nnz, in_ch, n_img, height, width, img_bs, batch, max_prongs) || !sigma || t0 < 0 || reps < 1 ||
        (long)t0 + reps > 0x7fffffffL || (long)reps * n_img > 0x7fffffffL || (nnz > 0 && (!coords_out || !values_out))) {
        fprintf(stderr, "tcvn: noise_replicate: bad arguments\n");
        return -1;
    }
    if (nnz == 0) return 0;
    hipLaunchKernelGGL(k_noise_replicate, dim3(cdiv((long)nnz * reps, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), coords, values,
                       (long)nnz, in_ch, n_img, height, width, img_bs, batch, max_prongs, sigma, seed, t0, reps, coords_out, values_out);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_noise_accumulate(double* acc, const float* grads, const float* values, int64_t count, int t0, int reps, void* stream) {
    if (count < 0 || t0 < 0 || reps < 1 || (long)t0 + reps > 0x7fffffffL || (count > 0 && (!acc || !grads || !values))) {
        fprintf(stderr, "tcvn: noise_accumulate: bad arguments\n");
        return -1;
    }
    if (count == 0) return 0;
    hipLaunchKernelGGL(k_noise_accumulate, dim3(cdiv(count, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), acc, grads, values,
                       (long)count, t0, reps);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_noise_finish(const double* acc, int64_t count, int samples, float* stats, void* stream) {
    if (count < 0 || samples < 1 || (count > 0 && (!acc || !stats))) {
        fprintf(stderr, "tcvn: noise_finish: bad arguments\n");
        return -1;
    }
    if (count == 0) return 0;
    hipLaunchKernelGGL(k_noise_finish, dim3(cdiv(count, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), acc, (long)count, samples, stats);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
