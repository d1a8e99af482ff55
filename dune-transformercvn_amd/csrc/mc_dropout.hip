// Monte-Carlo dropout statistics: T sampled logit rows per prediction -> mean and standard deviation of the class probabilities,
// predictive entropy, expected entropy, mutual information and arg-max votes.  Forward only, wave64.  Every softmax is formed in fp64
// (max-subtracted), every sum is taken in a fixed order (lane stride over the samples, xor shuffles): no atomics, no LDS, two runs agree
// bit for bit, and every output is rounded to fp32 once.
#include "../../include/tcvn_hip.h"
#include "tcvn_mc.h"

namespace tcvn {

namespace {

constexpr int CC = 8;                    // classes reduced together; more classes take another sweep (as shapley.hip)
constexpr int MCW = 4;                   // waves (= rows) of a workgroup

// max, arg max (ties: the lowest class) and sum_c exp(l_c - max) of one sample's logits; u = sum_c exp(l_c - max) (l_c - max)
__device__ __forceinline__ void mc_softmax(const float* lg, int C, double& mx, int& am, double& s, double& u) {
    mx = (double)lg[0]; am = 0;
    for (int c = 1; c < C; ++c) {
        const double l = (double)lg[c];
        if (l > mx) { mx = l; am = c; }
    }
    s = 0.0; u = 0.0;
    for (int c = 0; c < C; ++c) {
        const double d = (double)lg[c] - mx, e = exp(d);
        s += e;
        if (e > 0.0) u += e * d;         // 0 ln 0 = 0
    }
}

// one wave per row; its lanes stride over the T samples
__global__ __launch_bounds__(64 * MCW) void k_mc_stats(const McStatsArgs a) {
    const int r = blockIdx.x * MCW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.R) return;                // (no barrier below: whole waves leave)
    const int T = a.T, C = a.C;
    float *mean = a.mean + (long)r * C, *sd = a.std + (long)r * C, *votes = a.votes + (long)r * C;
    if (a.valid != nullptr && a.valid[r] < 0) {
        const float nan = __builtin_nanf("");
        for (int c = lane; c < C; c += 64) { mean[c] = nan; sd[c] = nan; votes[c] = nan; }
        if (lane == 0) { a.entropy[r] = nan; a.expected_entropy[r] = nan; a.mutual_info[r] = nan; }
        return;
    }
    const float* row = a.logits + (long)r * C;
    const long tstride = (long)a.R * C;
    double ent = 0.0, hexp = 0.0;        // -sum_c mean ln mean over the sweeps; (in the first sweep) sum_t H(p_t)
    for (int c0 = 0; c0 < C; c0 += CC) {
        const int nc = C - c0 < CC ? C - c0 : CC;
        double sum[CC] = {}, vote[CC] = {}, ss[CC] = {}, p0[CC] = {}, h = 0.0;
        {   // Sample 0's probabilities (every lane forms them): the sums below run over p_t - p_0, so that the mean of identical
            // samples is p_0 itself and their spread exactly 0 -- (p + p + p) / 3 is not always p
            double mx, s, u; int am;
            mc_softmax(row, C, mx, am, s, u);
            for (int c = 0; c < nc; ++c) p0[c] = exp((double)row[c0 + c] - mx) / s;
        }
        for (int t = lane; t < T; t += 64) {
            const float* lg = row + t * tstride;
            double mx, s, u; int am;
            mc_softmax(lg, C, mx, am, s, u);
            for (int c = 0; c < nc; ++c) {
                sum[c] += exp((double)lg[c0 + c] - mx) / s - p0[c];
                vote[c] += am == c0 + c ? 1.0 : 0.0;
            }
            if (c0 == 0) h += log(s) - u / s;      // H(p) = ln s - sum_c p_c (l_c - max)
        }
#pragma unroll
        for (int c = 0; c < CC; ++c) { sum[c] = p0[c] + wave_sum(sum[c]) / (double)T; vote[c] = wave_sum(vote[c]) / (double)T; }
        if (c0 == 0) hexp = wave_sum(h) / (double)T;
        for (int t = lane; t < T; t += 64) {       // second sweep: the centred sum of squares
            const float* lg = row + t * tstride;
            double mx, s, u; int am;
            mc_softmax(lg, C, mx, am, s, u);
            for (int c = 0; c < nc; ++c) {
                const double d = exp((double)lg[c0 + c] - mx) / s - sum[c];
                ss[c] += d * d;
            }
        }
#pragma unroll
        for (int c = 0; c < CC; ++c) ss[c] = wave_sum(ss[c]);
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            if (c < nc && sum[c] > 0.0) ent -= sum[c] * log(sum[c]);      // the same value in every lane
            if (lane == c && c < nc) {
                mean[c0 + c] = (float)sum[c];
                sd[c0 + c] = T > 1 ? (float)sqrt(ss[c] / (double)(T - 1)) : 0.f;
                votes[c0 + c] = (float)vote[c];
            }
        }
    }
    if (lane == 0) {
        const double mi = ent - hexp;
        a.entropy[r] = (float)ent; a.expected_entropy[r] = (float)hexp; a.mutual_info[r] = (float)(mi > 0.0 ? mi : 0.0);
    }
}

}  // namespace

int mc_stats(const McStatsArgs& a, hipStream_t st) {
    if (a.R <= 0) return 0;
    hipLaunchKernelGGL(k_mc_stats, dim3(cdiv(a.R, MCW)), dim3(64 * MCW), 0, st, a);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace tcvn

extern "C" int tcvn_mc_dropout_stats(const float* sample_logits, const int32_t* valid, int n_samples, int rows, int classes,
                                     float* mean_prob, float* std_prob, float* entropy, float* expected_entropy, float* mutual_info,
                                     float* votes, void* stream) {
    if (!sample_logits || !mean_prob || !std_prob || !entropy || !expected_entropy || !mutual_info || !votes) {
        fprintf(stderr, "tcvn: mc_dropout_stats: NULL argument\n");
        return -1;
    }
    if (n_samples < 1 || rows < 0 || classes < 1 || classes > tcvn::MC_MAX_CLASSES) {
        fprintf(stderr, "tcvn: mc_dropout_stats: %d samples, %d rows, %d classes (samples >= 1, classes 1..%d)\n", n_samples, rows, classes,
                tcvn::MC_MAX_CLASSES);
        return -1;
    }
    tcvn::McStatsArgs a{sample_logits, valid, n_samples, rows, classes, mean_prob, std_prob, entropy, expected_entropy, mutual_info, votes};
    return tcvn::mc_stats(a, reinterpret_cast<hipStream_t>(stream));
}
