// Prong Shapley values of the event decoder's class scores: permutations, coalition batches for the encoder stage that exists, and the
// reductions of the coalition values -- forward only, wave64.  A coalition is event b's sequence with every absent prong token zeroed and
// padded as a key (no positional encoding: this IS the event with only those prongs, see explain.hip).  Values are fp64 and every sum is
// taken in a fixed order (lane stride, xor shuffles, one ordered pass over the waves' partials): no atomics, two runs agree bit for bit.
#include "../../include/tcvn_hip.h"
#include "tcvn_shapley.h"

namespace tcvn {

namespace {

constexpr uint32_t kShapStream = 0x53484150u;       // Philox stream constant of the permutation keys ("SHAP")
constexpr int CC = 8;                               // classes reduced together; more event classes take another sweep
constexpr int RED = 256, RW = RED / 64;             // threads and waves of a reduction workgroup

// ---- permutations: one wave per (event, permutation), lane = slot -------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_shap_perm(const int* tok_row, int32_t* perms, int32_t* pos, int M, int P, uint64_t seed) {
    const int m = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const bool valid = lane < P && tok_row[b * (1 + P) + 1 + lane] >= 0;
    const uint32_t key = philox4((uint32_t)lane, (uint32_t)m, (uint32_t)b, kShapStream, (uint32_t)seed, (uint32_t)(seed >> 32)).x;
    int rank = 0;                                   // valid lanes ahead of this one in (key, slot) order
    for (int l = 0; l < 64; ++l) {
        const uint32_t k = __shfl(key, l);
        const int v = __shfl((int)valid, l);
        rank += (v && (k < key || (k == key && l < lane))) ? 1 : 0;
    }
    const int n = __popcll(__ballot(valid));
    int32_t* out = perms + ((long)b * M + m) * P;
    if (valid) out[rank] = lane;                    // the ranks of the n valid lanes are 0 .. n-1, each once
    if (lane >= n && lane < P) out[lane] = -1;      // positions n .. P-1, whoever holds that lane
    if (lane < P) pos[((long)b * M + m) * P + lane] = valid ? rank : -1;      // the inverse, for k_shap_sampled
}

// ---- coalition batches ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int shap_event(const int64_t* offsets, int B, long job) {       // offsets[b] <= job < offsets[b + 1]
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= job) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int64_t shap_mask(const ShapTable& t, const int32_t* perms, int b, long k, int M, int P) {
    const int64_t vm = t.vmask[b];
    int64_t mask = 0;
    if (t.exact[b]) {                               // deposit the bits of k into the valid slots, lowest slot first (k < 2^n)
        int64_t v = vm;
        for (; k; k >>= 1, v &= v - 1)
            if (k & 1) mask |= v & -v;
        return mask;
    }
    if (k < 2) return k == 0 ? 0 : vm;
    const int n = t.n[b];                           // sampled events have n >= 2 here: n = 1 has the two jobs above only
    const long r = k - 2;
    const int m = (int)(r / (n - 1)), len = (int)(r - (long)m * (n - 1)) + 1;
    const int32_t* perm = perms + ((long)b * M + m) * P;
    for (int i = 0; i < len; ++i) mask |= (int64_t)1 << perm[i];
    return mask;
}
__global__ __launch_bounds__(128) void k_shap_gather(const float* tokens, const int* tok_row, ShapTable t, const int32_t* perms, long first,
                                                     int n, int B, int M, int S, int D, float* X0, int* vrow, int64_t* masks,
                                                     int32_t* event) {
    const int j = blockIdx.x;                       // one workgroup per job: the (event, mask) lookup is done once
    const long job = first + j;
    const int b = shap_event(t.offsets, B, job);
    const int64_t mask = shap_mask(t, perms, b, job - t.offsets[b], M, S - 1);
    for (int s = 0; s < S; ++s) {
        const bool keep = s == 0 ? tok_row[b * S] >= 0 : ((mask >> (s - 1)) & 1) != 0;
        const float* src = tokens + ((long)b * S + s) * D;
        float* dst = X0 + ((long)s * n + j) * D;    // sequence-major: token s of job j is row s*n + j
        for (int d = threadIdx.x; d < D; d += blockDim.x) dst[d] = keep ? src[d] : 0.f;
        if (threadIdx.x == 0) vrow[j * S + s] = keep ? 0 : -1;
    }
    if (threadIdx.x == 0) { masks[job] = mask; event[job] = b; }
}

// ---- logits -> values -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_shap_values(const float* logits, double* values, long J, int Ce, int prob) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= J) return;
    const float* lg = logits + j * Ce;
    double* v = values + j * Ce;
    if (!prob) { for (int c = 0; c < Ce; ++c) v[c] = (double)lg[c]; return; }
    double mx = (double)lg[0], sum = 0.0;
    for (int c = 1; c < Ce; ++c) mx = fmax(mx, (double)lg[c]);
    for (int c = 0; c < Ce; ++c) sum += exp((double)lg[c] - mx);
    for (int c = 0; c < Ce; ++c) v[c] = exp((double)lg[c] - mx) / sum;
}
__global__ __launch_bounds__(256) void k_shap_full_rows(const float* logits, ShapTable t, float* ev, int B, int Ce) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * Ce) return;
    const int b = i / Ce, c = i - b * Ce;
    const long full = t.exact[b] ? t.offsets[b + 1] - 1 : t.offsets[b] + 1;
    ev[i] = logits[full * Ce + c];
}

// ---- reductions ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long ins0(long r, int i) { return ((r >> i) << (i + 1)) | (r & (((long)1 << i) - 1)); }     // a zero bit at i
__device__ __forceinline__ int slot_index(int64_t vm, int p) { return __popcll((unsigned long long)(vm & (((int64_t)1 << p) - 1))); }
// 1 / (a C(a-1, c)): |C|! (n-|C|-1)! / n! with a = n, and the pair weight |C|! (n-|C|-2)! / (n-1)! with a = n-1
__device__ __forceinline__ double shap_weight(int a, int c) {
    double comb = 1.0;
    for (int j = 1; j <= c; ++j) comb = comb * (double)(a - 1 - c + j) / (double)j;         // an integer at every step
    return 1.0 / ((double)a * comb);
}
// sum of acc over the workgroup: xor shuffles inside a wave, then the waves' partials in wave order; the result is in threads < CC
__device__ __forceinline__ double block_sum(const double acc[CC], double (*part)[CC]) {
    const int tid = threadIdx.x, w = tid >> 6;
    __syncthreads();                                // the previous sweep's partials have been read
#pragma unroll
    for (int c = 0; c < CC; ++c) {
        const double s = wave_sum(acc[c]);
        if ((tid & 63) == 0) part[w][c] = s;
    }
    __syncthreads();
    double s = 0.0;
    if (tid < CC)
        for (int k = 0; k < RW; ++k) s += part[k][tid];
    return s;
}
// += sign * sum_{C without slot i} W1[|C|] (v(C + i) - v(C)) over this thread's share of the coalitions
__device__ __forceinline__ void acc_single(double acc[CC], const double* v, const double* W1, int n, int i, int Ce, int c0, int nc) {
    const long half = (long)1 << (n - 1), bi = (long)1 << i;
    for (long r = threadIdx.x; r < half; r += RED) {
        const long k = ins0(r, i);
        const double w = W1[__popcll((unsigned long long)k)];
        const double *a = v + (k | bi) * Ce + c0, *z = v + k * Ce + c0;
        for (int c = 0; c < nc; ++c) acc[c] += w * (a[c] - z[c]);
    }
}
// += scale * sum_{C without slots i < j} W2[|C|] (v(C + i + j) - v(C + i) - v(C + j) + v(C))
__device__ __forceinline__ void acc_pair(double acc[CC], const double* v, const double* W2, int n, int i, int j, double scale, int Ce, int c0,
                                         int nc) {
    const long quarter = (long)1 << (n - 2), bi = (long)1 << i, bj = (long)1 << j;
    for (long r = threadIdx.x; r < quarter; r += RED) {
        const long k = ins0(ins0(r, i), j);
        const double w = scale * W2[__popcll((unsigned long long)k)];
        const double *a = v + (k | bi | bj) * Ce + c0, *pi = v + (k | bi) * Ce + c0, *pj = v + (k | bj) * Ce + c0, *z = v + k * Ce + c0;
        for (int c = 0; c < nc; ++c) acc[c] += w * (a[c] - pi[c] - pj[c] + z[c]);
    }
}

// one workgroup per (event, prong slot)
__global__ __launch_bounds__(RED) void k_shap_exact(const double* values, ShapTable t, float* phi, float* se, int P, int Ce) {
    __shared__ double W1[16], part[RW][CC];
    const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t vm = t.vmask[b];
    const long base = ((long)b * P + p) * Ce;
    const bool valid = (vm >> p) & 1;
    if (!valid || t.exact[b])
        for (int c = tid; c < Ce; c += RED) { se[base + c] = 0.f; if (!valid) phi[base + c] = 0.f; }
    if (!valid || !t.exact[b]) return;
    const int n = t.n[b], i = slot_index(vm, p);
    if (tid < n) W1[tid] = shap_weight(n, tid);
    __syncthreads();
    const double* v = values + t.offsets[b] * Ce;
    for (int c0 = 0; c0 < Ce; c0 += CC) {
        const int nc = Ce - c0 < CC ? Ce - c0 : CC;
        double acc[CC] = {};
        acc_single(acc, v, W1, n, i, Ce, c0, nc);
        const double s = block_sum(acc, part);
        if (tid < nc) phi[base + c0 + tid] = (float)s;
    }
}

// one workgroup per (event, slot pair); the pair p < q writes [p][q] and [q][p], p = q the main effect phi_p - sum_{q != p} [p][q]
__global__ __launch_bounds__(RED) void k_shap_pairs(const double* values, ShapTable t, float* inter, int P, int Ce) {
    __shared__ double W1[16], W2[16], part[RW][CC];
    const int p = blockIdx.x / P, q = blockIdx.x - p * P, b = blockIdx.y, tid = threadIdx.x;
    const int64_t vm = t.vmask[b];
    const long base = (((long)b * P + p) * P + q) * Ce;
    if (!((vm >> p) & 1) || !((vm >> q) & 1) || !t.exact[b]) {
        const float fill = ((vm >> p) & 1) && ((vm >> q) & 1) ? __builtin_nanf("") : 0.f;
        for (int c = tid; c < Ce; c += RED) inter[base + c] = fill;
        return;
    }
    if (p > q) return;
    const int n = t.n[b], i = slot_index(vm, p), j = slot_index(vm, q);
    if (tid < n) W1[tid] = shap_weight(n, tid);
    if (n > 1 && tid < n - 1) W2[tid] = shap_weight(n - 1, tid);
    __syncthreads();
    const double* v = values + t.offsets[b] * Ce;
    const long mirror = (((long)b * P + q) * P + p) * Ce;
    for (int c0 = 0; c0 < Ce; c0 += CC) {
        const int nc = Ce - c0 < CC ? Ce - c0 : CC;
        double acc[CC] = {};
        if (p < q) acc_pair(acc, v, W2, n, i, j, 0.5, Ce, c0, nc);
        else {
            acc_single(acc, v, W1, n, i, Ce, c0, nc);
            for (int o = 0; o < n; ++o)
                if (o != i) acc_pair(acc, v, W2, n, o < i ? o : i, o < i ? i : o, -0.5, Ce, c0, nc);
        }
        const double s = block_sum(acc, part);
        if (tid < nc) { inter[base + c0 + tid] = (float)s; inter[mirror + c0 + tid] = (float)s; }
    }
}

// one workgroup per sampled event: wave w takes the slots w, w + RW, ...; its lanes stride over the permutations and read the slot's
// position from the inverse k_shap_perm stored
__device__ __forceinline__ void shap_marginal(double d[CC], const double* v, int pos, int m, int n, int Ce, int c0, int nc) {
    // the prefix of length len: 0 the empty coalition (job 0), n the full one (job 1), else job 2 + m (n-1) + len-1
    const long lo = pos == 0 ? 0 : 2 + (long)m * (n - 1) + pos - 1, hi = pos + 1 == n ? 1 : 2 + (long)m * (n - 1) + pos;
    for (int c = 0; c < nc; ++c) d[c] = v[hi * Ce + c0 + c] - v[lo * Ce + c0 + c];
}
__global__ __launch_bounds__(RED) void k_shap_sampled(const double* values, ShapTable t, const int32_t* pos, float* phi, float* se, int M,
                                                      int P, int Ce) {
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (t.exact[b]) return;
    const int64_t vm = t.vmask[b];
    const int n = t.n[b];
    const double* v = values + t.offsets[b] * Ce;
    const int32_t* pb = pos + (long)b * M * P;         // pb[m * P + p]: where slot p stands in permutation m
    for (int p = w; p < P; p += RW) {               // p is the same in every lane of the wave
        if (!((vm >> p) & 1)) continue;             // padded slots: zeroed by k_shap_exact
        for (int c0 = 0; c0 < Ce; c0 += CC) {
            const int nc = Ce - c0 < CC ? Ce - c0 : CC;
            double sum[CC] = {}, ss[CC] = {}, d[CC];
            for (int m = lane; m < M; m += 64) {
                shap_marginal(d, v, pb[(long)m * P + p], m, n, Ce, c0, nc);
                for (int c = 0; c < nc; ++c) sum[c] += d[c];
            }
#pragma unroll
            for (int c = 0; c < CC; ++c) sum[c] = wave_sum(sum[c]) / (double)M;
            for (int m = lane; m < M; m += 64) {
                shap_marginal(d, v, pb[(long)m * P + p], m, n, Ce, c0, nc);
                for (int c = 0; c < nc; ++c) ss[c] += (d[c] - sum[c]) * (d[c] - sum[c]);
            }
#pragma unroll
            for (int c = 0; c < CC; ++c) ss[c] = wave_sum(ss[c]);
            const long base = ((long)b * P + p) * Ce + c0;
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (lane == c && c < nc) {
                    phi[base + c] = (float)sum[c];
                    se[base + c] = M > 1 ? (float)sqrt(ss[c] / (double)(M - 1) / (double)M) : 0.f;
                }
        }
    }
}

}  // namespace

int shap_perm(const int* tok_row, int32_t* perms, int32_t* pos, int B, int M, int P, uint64_t seed, hipStream_t st) {
    if (P < 1) return 0;
    hipLaunchKernelGGL(k_shap_perm, dim3(M, B), dim3(64), 0, st, tok_row, perms, pos, M, P, seed);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int shap_gather(const float* tokens, const int* tok_row, const ShapTable& t, const int32_t* perms, long first, int n, int B, int M, int S,
                int D, float* X0, int* vrow, int64_t* masks, int32_t* event, hipStream_t st) {
    hipLaunchKernelGGL(k_shap_gather, dim3(n), dim3(128), 0, st, tokens, tok_row, t, perms, first, n, B, M, S, D, X0, vrow, masks, event);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int shap_values(const float* logits, double* values, long J, int Ce, int prob, hipStream_t st) {
    hipLaunchKernelGGL(k_shap_values, dim3(cdiv(J, 256)), dim3(256), 0, st, logits, values, J, Ce, prob);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int shap_full_rows(const float* logits, const ShapTable& t, float* event_logits, int B, int Ce, hipStream_t st) {
    hipLaunchKernelGGL(k_shap_full_rows, dim3(cdiv((long)B * Ce, 256)), dim3(256), 0, st, logits, t, event_logits, B, Ce);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int shap_exact(const double* values, const ShapTable& t, float* phi, float* stderr_, int B, int P, int Ce, hipStream_t st) {
    if (P < 1) return 0;
    hipLaunchKernelGGL(k_shap_exact, dim3(P, B), dim3(RED), 0, st, values, t, phi, stderr_, P, Ce);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int shap_pairs(const double* values, const ShapTable& t, float* inter, int B, int P, int Ce, hipStream_t st) {
    if (P < 1) return 0;
    hipLaunchKernelGGL(k_shap_pairs, dim3(P * P, B), dim3(RED), 0, st, values, t, inter, P, Ce);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int shap_sampled(const double* values, const ShapTable& t, const int32_t* pos, float* phi, float* stderr_, int B, int M, int P, int Ce,
                 hipStream_t st) {
    if (P < 1) return 0;
    hipLaunchKernelGGL(k_shap_sampled, dim3(B), dim3(RED), 0, st, values, t, pos, phi, stderr_, M, P, Ce);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace tcvn
