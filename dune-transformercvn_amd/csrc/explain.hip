// Explanation kernels of the token path: export of the attention probabilities both encoder forwards leave in the head workspace,
// attention rollout (Abnar & Zuidema 2020) and the batches of a leave-one-prong-out scan -- forward only, exact fp32.
// The encoder has no positional encoding (every token gets the same position embedding), so "event b without prong p" is the same
// sequence with token 1+p zeroed and padded as a key: the scan re-runs the encoder stage that exists on B * P more sequences.
#include "../../include/tcvn_hip.h"
#include "tcvn_explain.h"

namespace tcvn {

namespace {

__global__ __launch_bounds__(256) void k_attn_export(const char* ws, long probs0, long layer_stride, const int* tok_row, float* out,
                                                     int H, int S, long per_layer) {
    const int l = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;          // element of [B][H][S][S]
    if (i >= per_layer) return;
    const float* src = reinterpret_cast<const float*>(ws + probs0 + l * layer_stride);
    const int q = (int)((i / S) % S), b = (int)(i / ((long)H * S * S));
    out[l * per_layer + i] = tok_row[b * S + q] >= 0 ? src[i] : 0.f;      // padded keys are exact zeros in the workspace already
}

// ---- rollout: one workgroup per event; R and the fused layer matrix in LDS ------------------------------------------------------
constexpr int RS = 64, RLD = RS + 1, RPT = RS * RS / 256;
__global__ __launch_bounds__(256) void k_attn_rollout(const float* w, const int* tok_row, float* out, int L, int B, int H, int S,
                                                      int fuse_max) {
    __shared__ float R[RS * RLD], A[RS * RLD];
    __shared__ float rsum[RS];
    __shared__ int valid[RS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = S * S;
    if (tid < RS) valid[tid] = tid < S ? tok_row[b * S + tid] >= 0 : 0;
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        const float* wl = w + ((long)l * B + b) * H * n;
        for (int e = tid; e < n; e += 256) {                      // head fusion + residual mix
            const int i = e / S, j = e - i * S;
            float f = wl[e];
            for (int h = 1; h < H; ++h) { const float v = wl[(long)h * n + e]; f = fuse_max ? fmaxf(f, v) : f + v; }
            if (!fuse_max) f /= (float)H;
            A[i * RLD + j] = 0.5f * f + ((i == j && valid[i]) ? 0.5f : 0.f);
        }
        __syncthreads();
        if (tid < S) {
            float s = 0.f;
            for (int j = 0; j < S; ++j) s += A[tid * RLD + j];
            rsum[tid] = s;
        }
        __syncthreads();
        for (int e = tid; e < n; e += 256) {                      // row normalisation; rows of padded tokens are zero and stay zero
            const int i = e / S, j = e - i * S;
            const float s = rsum[i];
            A[i * RLD + j] = s > 0.f ? A[i * RLD + j] / s : 0.f;
        }
        __syncthreads();
        float acc[RPT];
#pragma unroll
        for (int t = 0; t < RPT; ++t) {
            const int e = tid + 256 * t;
            acc[t] = 0.f;
            if (e < n) {
                const int i = e / S, j = e - i * S;
                if (l == 0) acc[t] = A[i * RLD + j];
                else {
                    float a = 0.f;
                    for (int k = 0; k < S; ++k) a = fmaf(A[i * RLD + k], R[k * RLD + j], a);
                    acc[t] = a;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < RPT; ++t) {
            const int e = tid + 256 * t;
            if (e < n) { const int i = e / S, j = e - i * S; R[i * RLD + j] = acc[t]; }
        }
        __syncthreads();
    }
    for (int e = tid; e < n; e += 256) { const int i = e / S, j = e - i * S; out[(long)b * n + e] = R[i * RLD + j]; }
}

// ---- leave-one-prong-out batches --------------------------------------------------------------------------------------------------
__global__ void k_loo_gather(const float* tokens, const int* tok_row, const int* jobs, float* X0, int* vrow, int n, int S, int D) {
    const int t = blockIdx.x;                       // t = s*n + j
    const int s = t / n, j = t - s * n;
    const int job = jobs[j];
    const int b = job / S, gone = job - b * S;      // gone = 0: the base sequence
    const bool keep = tok_row[b * S + s] >= 0 && !(gone > 0 && s == gone);
    const float* src = tokens + ((long)b * S + s) * D;
    for (int d = threadIdx.x; d < D; d += blockDim.x) X0[(long)t * D + d] = keep ? src[d] : 0.f;
    if (threadIdx.x == 0) vrow[j * S + s] = keep ? 0 : -1;
}
__global__ void k_loo_scatter(const float* logits, const int* src, float* ev, float* loo, int B, int S, int Ce) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * S * Ce) return;
    const int slot = (int)(i / Ce), c = (int)(i - (long)slot * Ce);
    const int b = slot / S, s = slot - b * S;
    const float v = logits[(long)src[slot] * Ce + c];
    if (s == 0) ev[(long)b * Ce + c] = v;
    else loo[((long)b * (S - 1) + (s - 1)) * Ce + c] = v;
}

}  // namespace

int attn_export(const char* ws, long probs0, long layer_stride, const int* tok_row, float* weights, int L, int B, int H, int S,
                hipStream_t st) {
    const long per_layer = (long)B * H * S * S;
    hipLaunchKernelGGL(k_attn_export, dim3(cdiv(per_layer, 256), L), dim3(256), 0, st, ws, probs0, layer_stride, tok_row, weights, H, S,
                       per_layer);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int attn_rollout(const float* weights, const int* tok_row, float* rollout, int L, int B, int H, int S, int fuse_max, hipStream_t st) {
    if (S > RS) return -1;
    hipLaunchKernelGGL(k_attn_rollout, dim3(B), dim3(256), 0, st, weights, tok_row, rollout, L, B, H, S, fuse_max);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int loo_gather(const float* tokens, const int* tok_row, const int* jobs, float* X0, int* vrow, int n, int S, int D, hipStream_t st) {
    hipLaunchKernelGGL(k_loo_gather, dim3(S * n), dim3(128), 0, st, tokens, tok_row, jobs, X0, vrow, n, S, D);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int loo_scatter(const float* logits, const int* src, float* event_logits, float* loo, int B, int S, int Ce, hipStream_t st) {
    hipLaunchKernelGGL(k_loo_scatter, dim3(cdiv((long)B * S * Ce, 256)), dim3(256), 0, st, logits, src, event_logits, loo, B, S, Ce);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace tcvn

extern "C" int tcvn_attention_rollout(const float* weights, const int32_t* tok_row, int layers, int batch, int heads, int seq,
                                      int head_fusion, float* rollout, void* stream) {
    if (!weights || !tok_row || !rollout || layers < 1 || batch < 1 || heads < 1 || seq < 1 || seq > 64 ||
        (head_fusion != TCVN_FUSE_MEAN && head_fusion != TCVN_FUSE_MAX)) {
        fprintf(stderr, "tcvn: attention_rollout: bad argument (NULL pointer, layers / batch / heads < 1, seq outside 1..64 or unknown head fusion)\n");
        return -1;
    }
    return tcvn::attn_rollout(weights, tok_row, rollout, layers, batch, heads, seq, head_fusion == TCVN_FUSE_MAX,
                              reinterpret_cast<hipStream_t>(stream));
}
