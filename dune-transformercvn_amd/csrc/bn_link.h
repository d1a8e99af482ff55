// BatchNorm backward link: the arithmetic of k_bn_bwd_link as a device function, for the launches it rides in (k_slab_reduce_link,
// k_conv3x3_wgrad_bf16).
#pragma once
#include "tcvn_ops.h"

namespace tcvn {

// BatchNorm backward bookkeeping for one norm layer (train mode):
//   s1 = sum dU, t2 = sum dU*x, s3 = sum dA*min(u,0)   (partials from the dgrad epilogue / pooling backward kernels)
//   dbeta = s1 ; dgamma = sum dU*xhat = r*(t2 - mu*s1) ; dslope = s3
//   dx = sc*dU + Px*x + Qx  with  Px = -sc*dgamma*r/M ,  Qx = -sc*s1/M + sc*dgamma*r*mu/M      (sc = gamma*r)
// One wave per channel: workgroup `blk` of `nblk` takes channels blk * waves + wave, then every nblk * waves-th one, so any number of
// workgroups of any size covers all C channels with the same arithmetic per channel.
__device__ __forceinline__ void bn_bwd_link_body(const BnBwdLinkArgs& a, int blk, int nblk) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    for (int c = blk * waves + wave; c < a.C; c += nblk * waves) {
        // everything the closing arithmetic needs is requested up front, with the partial rows (one round trip instead of two: see k_bn_link)
        const double mu = a.bstat[c * 2], var = a.bstat[c * 2 + 1];
        const float gam = a.gamma[c];
        const float g_dg = a.dgamma[c], g_db = a.dbeta[c], g_ds = a.dslope[c];
        const float p_old = a.accumulate_pq ? a.P[c] : 0.f, q_old = a.accumulate_pq ? a.Q[c] : 0.f;
        double s1 = 0, t2 = 0, s3 = 0;
        int b = lane;
        // Eight partial rows per trip = every row of a launch with <= 512 workgroups (all of them) in ONE round trip: 24 loads in flight
        // per lane.  This kernel sits between two convolutions of the critical chain while the other embedder's kernels keep the memory system
        // busy: each dependent trip cost a full loaded-latency round trip (fp32 mode: 25 us per launch with two trips, 132 launches per step).
        for (; b < a.nblk; b += 512) {
            double v[8][3];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int bb = b + 64 * i;
                const double* p = a.part + ((long)(bb < a.nblk ? bb : b) * a.C + c) * 3;
                v[i][0] = p[0]; v[i][1] = p[1]; v[i][2] = p[2];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (b + 64 * i < a.nblk) { s1 += v[i][0]; t2 += v[i][1]; s3 += v[i][2]; }
        }
        s1 = wave_sum(s1); t2 = wave_sum(t2); s3 = wave_sum(s3);
        if (lane != 0) continue;
        const double r = 1.0 / sqrt(var + (double)a.eps);
        const double dgamma = r * (t2 - mu * s1);
        const double sc = (double)gam * r;
        const double M = (double)a.count;
        a.dgamma[c] = g_dg + (float)dgamma;
        a.dbeta[c] = g_db + (float)s1;
        a.dslope[c] = g_ds + (float)s3;
        const float Px = (float)(-sc * dgamma * r / M);
        const float Qx = (float)(-sc * s1 / M + sc * dgamma * r * mu / M);
        a.P[c] = p_old + Px; a.Q[c] = q_old + Qx;
    }
}

}  // namespace tcvn
