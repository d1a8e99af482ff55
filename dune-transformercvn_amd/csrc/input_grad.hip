// Hit gradients: the kernels behind tcvn_densenet_input_gradient that no training step has.
//   * k_hit_gradient: the data gradient of conv0 (7x7, stride 2, pad 3), formed only where it is asked for -- at the hits of the COO list.
//     A pixel (y, x) is read by the conv0 outputs (oy, ky) with 2*oy - 3 + ky = y, so ky has the parity of y + 3: 3 or 4 rows, 3 or 4
//     columns, at most 16 outputs of N channels each.  One wave owns a hit: lane = output channel, so a tap is one contiguous row of E0
//     (256 B fp32 / 128 B bf16 at N = 64) against one conflict-free row of the weights in LDS ([pixel channel][tap][output channel]); the
//     lanes are summed by xor-shuffles in a fixed order and lanes 0 .. Cpix-1 store the hit's values.  Every hit is written exactly once,
//     no atomics: two runs agree bit for bit.  Sums run in double and are rounded to fp32 once (the terms cancel: an fp32 sum of
//     16 x N x 1 products would be exact to 1e-7 of the LARGEST partial sum, not of the result).
//     The kernel is latency-bound, not a roofline kernel: a hit list is a few thousand entries of <= 16 dependent 256-B reads behind one
//     coordinate read, 16 x 64 x 3 multiply-adds each -- a few microseconds of launch and L2 latency beside an embedder backward of
//     milliseconds.  It is left as simple as this on purpose.
//   * k_rows_bn_bwd_frozen: BatchNorm1d + PReLU backward on RUNNING statistics (an affine map per channel: no batch terms).
//   * k_ig_*: integrated gradients, acc += w_k * grad in double over the steps, attr = acc * v at the end.
#include <algorithm>

#include "tcvn_input_grad.h"
#include "../../include/tcvn_hip.h"
#include "prof.h"

namespace tcvn {
namespace {

constexpr int HG_MAXC = 4;      // pixel channels per hit (as the hit-list weight gradient, stem.hip)

template <typename T>
__global__ __launch_bounds__(256) void k_hit_gradient(const HitGradArgs a) {
    extern __shared__ float w_lds[];                         // [Cpix * 49][N]: W0[co][k] transposed, k = c * 49 + ky * 7 + kx
    const int tid = threadIdx.x, lane = tid & 63;
    const int K = a.Cpix * 49;
    for (int i = tid; i < K * a.N; i += 256) {                 // consecutive lanes read consecutive floats of W0; the transpose happens in the LDS store
        const int co = i / K, k = i - co * K;
        w_lds[k * a.N + co] = a.W0[i];
    }
    __syncthreads();
    const T* E0 = reinterpret_cast<const T*>(a.E0);
    const bool dups = a.o.base != nullptr && *a.o.ndup() != 0;          // (uniform)
    const long nw = (long)gridDim.x * 4;
    for (long hit = (long)blockIdx.x * 4 + (tid >> 6); hit < a.nnz; hit += nw) {      // wave-uniform from here on
        int im, y, x;
        bool owned = hit_in_map(a.coords, hit, a.n_img, a.H, a.W, im, y, x);
        if (owned && dups) {
            const long pix = ((long)im * a.H + y) * a.W + x;
            if ((a.o.dup()[pix >> 5] >> (pix & 31)) & 1u) owned = a.o.own()[pix] == (int)hit;
        }
        double acc[HG_MAXC] = {0.0, 0.0, 0.0, 0.0};
        if (owned) {
            const int py = (y + 3) & 1, px = (x + 3) & 1;
            for (int ky = py; ky < 7; ky += 2) {
                const int oy = (y + 3 - ky) >> 1;                        // (y + 3 - ky is even; negative stays negative)
                if ((unsigned)oy >= (unsigned)a.Hc) continue;
                for (int kx = px; kx < 7; kx += 2) {
                    const int ox = (x + 3 - kx) >> 1;
                    if ((unsigned)ox >= (unsigned)a.Wc) continue;
                    const T* row = E0 + (((long)im * a.Hc + oy) * a.Wc + ox) * a.lde;
                    const float* w = w_lds + (ky * 7 + kx) * a.N;
                    for (int co = lane; co < a.N; co += 64) {
                        const double e = (double)to_f<T>(row[co]);
#pragma unroll
                        for (int c = 0; c < HG_MAXC; ++c)
                            if (c < a.Cpix) acc[c] = fma(e, (double)w[c * 49 * a.N + co], acc[c]);
                    }
                }
            }
        }
        double mine = 0.0;
#pragma unroll
        for (int c = 0; c < HG_MAXC; ++c) {
            const double s = wave_sum(acc[c]);
            if (lane == c) mine = s;
        }
        if (lane < a.Cpix) {
            const long i = hit * a.Cpix + lane;
            const double v = (double)a.values[i];
            const double pre = a.value_mode == 0 ? 1.0 / 255.0 : a.value_mode == 1 ? 1.0 / (v + 1.0) : 1.0;
            a.d_values[i] = owned ? (float)(mine * pre) : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void k_rows_bn_bwd_frozen(const RowsBnFrozenBwdArgs a) {
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;      // 16 columns x 16 row lanes per workgroup (as k_rows_bn_fwd)
    const int c = blockIdx.x * 16 + cl;
    if (c >= a.C) return;
    const float sl = a.slope ? a.slope[c] : 0.f;
    if (a.no_norm) {
        for (int r = rg; r < a.R; r += 16) {
            const float dz = a.dY[(long)r * a.lddy + c];
            a.dX[(long)r * a.lddx + c] = a.X[(long)r * a.ldx + c] > 0.f ? dz : sl * dz;
        }
        return;
    }
    const float mean = a.running_mean[c], rstd = 1.0f / sqrtf(a.running_var[c] + a.eps);      // the eval forward's arithmetic
    const float g = a.gamma ? a.gamma[c] : 1.f, b = a.beta ? a.beta[c] : 0.f;
    for (int r = rg; r < a.R; r += 16) {
        const float u = (a.X[(long)r * a.ldx + c] - mean) * rstd * g + b;
        const float dz = a.dY[(long)r * a.lddy + c];
        a.dX[(long)r * a.lddx + c] = (u > 0.f ? dz : sl * dz) * g * rstd;
    }
}

// seed[r][c] = d score_r / d logits[r][c] for score = logit of class cls[r] (kind 1: the one-hot row) or its softmax probability (kind 0:
// the softmax Jacobian row p_t (delta_ct - p_c), in double, max-subtracted); cls[r] < 0 (a padded slot): a zero row.  One thread per row.
__global__ void k_hit_seed(const float* logits, const int* cls, int R, int C, int kind, float* seed) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const float* lg = logits + (long)r * C;
    float* o = seed + (long)r * C;
    const int t = cls[r];
    if (t < 0 || t >= C) { for (int c = 0; c < C; ++c) o[c] = 0.f; return; }
    if (kind == 1) { for (int c = 0; c < C; ++c) o[c] = c == t ? 1.f : 0.f; return; }
    double m = (double)lg[0], z = 0.0;
    for (int c = 1; c < C; ++c) m = fmax(m, (double)lg[c]);
    for (int c = 0; c < C; ++c) z += exp((double)lg[c] - m);
    const double pt = exp((double)lg[t] - m) / z;
    for (int c = 0; c < C; ++c) {
        const double pc = exp((double)lg[c] - m) / z;
        o[c] = (float)(pt * ((c == t ? 1.0 : 0.0) - pc));
    }
}

__global__ void k_ig_scale(const float* v, float alpha, float* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = alpha * v[i];
}
__global__ void k_ig_accumulate(double* acc, const float* g, double w, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acc[i] = fma(w, (double)g[i], acc[i]);
}
__global__ void k_ig_finish(const double* acc, const float* v, float* attr, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) attr[i] = (float)(acc[i] * (double)v[i]);
}

}  // namespace

int hit_gradient(const HitGradArgs& a, hipStream_t st) {
    if (a.value_mode == 3) { fprintf(stderr, "tcvn: hit gradient: one-hot pixels are class indices and have no gradient\n"); return -22; }
    if (a.value_mode < 0 || a.value_mode > 2 || (a.mode != MODE_F32 && a.mode != MODE_BF16)) return -1;
    // the transposed conv0 weight in LDS: 37 KB at the product's 3 x 64 channels; wider stems (up to 160 KB: 3 x 278 channels) raise the 64 KB default
    const long lds = (long)a.Cpix * 49 * a.N * 4;
    if (a.Cpix < 1 || a.Cpix > HG_MAXC || a.N < 1 || lds > 160 * 1024 || a.lde < a.N) {
        fprintf(stderr, "tcvn: hit gradient: %d pixel channels x %d conv0 channels not supported\n", a.Cpix, a.N);
        return -2;
    }
    if (a.nnz <= 0) return 0;
    if (a.nnz > 0x7fffffffL) return -2;                      // the owner words hold 32-bit list indices
    const int nb = (int)std::min<long>(cdiv(a.nnz, 32), 1024);      // >= 8 hits per wave where the list allows: a workgroup loads the weights (37 KB) once
    if (lds > 64 * 1024) {
        static bool wide = false;
        if (!wide) {
            TCVN_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_hit_gradient<float>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            TCVN_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_hit_gradient<bf16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            wide = true;
        }
    }
    ProfScope ps("k_hit_gradient", 2.0 * a.nnz * 12.25 * a.Cpix * a.N, 0.0, st);
    if (a.mode == MODE_F32) hipLaunchKernelGGL(k_hit_gradient<float>, dim3(nb), dim3(256), (size_t)lds, st, a);
    else hipLaunchKernelGGL(k_hit_gradient<bf16>, dim3(nb), dim3(256), (size_t)lds, st, a);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int rows_bn_bwd_frozen(const RowsBnFrozenBwdArgs& a, hipStream_t st) {
    if (a.R <= 0) return 0;
    hipLaunchKernelGGL(k_rows_bn_bwd_frozen, dim3(cdiv(a.C, 16)), dim3(256), 0, st, a);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace tcvn

using namespace tcvn;

extern "C" {

int64_t tcvn_hit_gradient_workspace_bytes(int n_img, int height, int width, int in_ch) {
    if (n_img < 1 || height < 1 || width < 1 || in_ch < 1) return -1;
    const long npix = (long)n_img * height * width;
    return round_up(npix * in_ch * 4, 256) + round_up(pixel_owners_bytes(npix), 256);
}

int tcvn_hit_gradient_gather(int mode, const int32_t* coords, const float* values, int64_t nnz, int n_img, int height, int width,
                             int in_ch, int value_mode, const void* e0, int64_t lde, int init_ch, const float* conv0_weight,
                             float* d_values, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t need = tcvn_hit_gradient_workspace_bytes(n_img, height, width, in_ch);
    if (!coords || !values || !e0 || !conv0_weight || !d_values || !workspace || need < 0 || nnz < 0) {
        fprintf(stderr, "tcvn: hit_gradient_gather: bad arguments\n");
        return -1;
    }
    if (workspace_bytes < need) { fprintf(stderr, "tcvn: hit_gradient_gather: workspace too small (%ld < %ld)\n", (long)workspace_bytes, (long)need); return -12; }
    HitGradArgs a{};
    a.mode = mode; a.coords = coords; a.values = values; a.nnz = nnz; a.n_img = n_img; a.H = height; a.W = width; a.Cpix = in_ch;
    a.value_mode = value_mode; a.E0 = e0; a.lde = lde; a.Hc = (height + 6 - 7) / 2 + 1; a.Wc = (width + 6 - 7) / 2 + 1; a.N = init_ch;
    a.W0 = conv0_weight; a.d_values = d_values;
    if (value_mode == 3) return hit_gradient(a, st);           // refused there, in front of any launch
    // the duplicate record is the dense stem's: scatter the list into a scratch map, as a forward would have
    const long npix = (long)n_img * height * width;
    char* ws = reinterpret_cast<char*>(workspace);
    char* own = ws + round_up(npix * in_ch * 4, 256);
    TCVN_CHECK(hipMemsetAsync(ws, 0, (size_t)(own - ws + pixel_owners_zero_bytes(npix)), st));
    a.o = PixelOwners{reinterpret_cast<uint32_t*>(own), npix};
    ScatterArgs sc{MODE_F32, coords, values, nnz, n_img, ws, height, width, in_ch, value_mode, 0.f, 0, a.o};
    if (int rc = scatter_pixels(sc, st)) return rc;
    return hit_gradient(a, st);
}

int tcvn_hit_gradient_seed(const float* logits, const int32_t* classes, int rows, int n_classes, int value_kind, float* seed, void* stream) {
    if (rows <= 0) return 0;
    if (!logits || !classes || !seed || n_classes < 1 || (value_kind != 0 && value_kind != 1)) { fprintf(stderr, "tcvn: hit_gradient_seed: bad arguments\n"); return -1; }
    hipLaunchKernelGGL(k_hit_seed, dim3(cdiv(rows, 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), logits, classes, rows, n_classes, value_kind, seed);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int tcvn_ig_scale(const float* values, float alpha, float* out, int64_t count, void* stream) {
    if (count <= 0) return 0;
    if (!values || !out) return -1;
    hipLaunchKernelGGL(k_ig_scale, dim3(cdiv(count, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), values, alpha, out, (long)count);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int tcvn_ig_accumulate(double* acc, const float* grad, double weight, int64_t count, void* stream) {
    if (count <= 0) return 0;
    if (!acc || !grad) return -1;
    hipLaunchKernelGGL(k_ig_accumulate, dim3(cdiv(count, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), acc, grad, weight, (long)count);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int tcvn_ig_finish(const double* acc, const float* values, float* attr, int64_t count, void* stream) {
    if (count <= 0) return 0;
    if (!acc || !values || !attr) return -1;
    hipLaunchKernelGGL(k_ig_finish, dim3(cdiv(count, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), acc, values, attr, (long)count);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
