// bf16 3x3 convolution on padded LDS tiles (see tile3x3.h), data gradient.  The forward is conv3x3_fwd_tile.hip, the weight gradient
// conv3x3_wgrad_tile.hip.
// Reference call site: the autograd of Bottleneck.output_block (transformercvn/network/layers/dense_net.py:29-40).
#include <cstddef>
#include <cstdlib>
#include <type_traits>
#include "tile3x3.h"
#include "prof.h"
#include "bn_link.h"

namespace tcvn {

using namespace t3;

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Data gradient: dA[p][c] = sum_tap sum_n eff[p - shift(tap)][n] * W2[n][c][tap]  (128 channels out, K = 9 x 32), followed
// by the PReLU + BatchNorm backward of norm2 on the bottleneck tensor Y.  The 32-channel eff image (gradient of the layer's
// concat slice, dropout mask and BN mean-terms applied) is built once per tile in LDS; each wave owns 32 of the 128 output
// channels for all 128 positions, so its 18 weight fragments stay in registers.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void k_conv3x3_dgrad_bf16(const ConvDgradArgs g, int n_img, int ntiles, int swz) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const EffSrc& e = g.e;
    const PadGeom q(n_img, g.H, g.W);
    const int nrows4 = (q.rows() + 3) & ~3;
    int* tbl = reinterpret_cast<int*>(smem + nrows4 * 64);                 // [nrows4] pixel index per image row
    constexpr int CLD3 = 132;
    double* sred = reinterpret_cast<double*>(smem + nrows4 * 68);           // [128][3] per-channel sums of this workgroup
    float* Cs = reinterpret_cast<float*>(smem + nrows4 * 68 + 128 * 24);    // [64][CLD3] fp32 dA tile (one pass)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const float invWp = 1.0f / q.Wp, invHp = 1.0f / q.Hp;
    const bf16* __restrict__ G = reinterpret_cast<const bf16*>(e.G);
    const bf16* __restrict__ D = reinterpret_cast<const bf16*>(e.X);
    const bf16* __restrict__ Y = reinterpret_cast<const bf16*>(g.Xin);
    bf16* __restrict__ DU = reinterpret_cast<bf16*>(g.Gout);
    const int nb = gridDim.x;
    const int lb = swz ? (blockIdx.x & 7) * (nb >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const bool drop = e.drop_p > 0.f;
    const uint32_t dkey = drop_key(e.seed, e.stream_id);

    // weights of this wave's 32 output channels: fragment (row tile = wave, k-step) at ((wave*18 + ks)*64 + lane)*8
    const bf16* __restrict__ Wf = reinterpret_cast<const bf16*>(g.Wfrag) + ((long)wave * 18 * 64 + lane) * 8;
    bf16x8_t bw[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) bw[i] = *reinterpret_cast<const bf16x8_t*>(Wf + i * 512);
    const int e_c8 = tid & 15, e_r0 = tid >> 4;                            // epilogue role: 8-channel chunk, rows e_r0 + 16*i
    float esc[8], esh[8], esl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { esc[j] = g.sc[e_c8 * 8 + j]; esh[j] = g.sh[e_c8 * 8 + j]; esl[j] = g.sl[e_c8 * 8 + j]; }
    for (int i = tid; i < 128 * 3; i += 256) sred[i] = 0.0;

    const int ec = tid & 3, er0 = tid >> 2;                                // eff staging: chunk ec of rows er0, er0+64, ...
    float cP[8], cQ[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = ec * 8 + j;
        cP[j] = n < e.N ? e.P[n] : 0.f; cQ[j] = n < e.N ? e.Q[n] : 0.f;
    }
    for (int t = lb; t < ntiles; t += nb) {
        const int g0 = t * TP;
        __syncthreads();
        for (int rr = tid; rr < nrows4; rr += 256) tbl[rr] = pix_of(q, g0 - q.halo + rr, invWp, invHp);
        __syncthreads();
        // eff image: 16-B chunk ec of row rr at rr*64 + ((ec ^ ((rr>>2)&3)) << 4)
        for (int rr = er0; rr < nrows4; rr += 64) {
            const int m = tbl[rr];
            u16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
            if (m >= 0) {
                const u16x8 gv = *reinterpret_cast<const u16x8*>(G + (long)m * e.ldg + e.c_off + ec * 8);
                const u16x8 xv = *reinterpret_cast<const u16x8*>(D + (long)m * e.ldx + e.c_off + ec * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int n = ec * 8 + j;
                    float v = 0.f;
                    if (n < e.N) {
                        v = eff3(bf2f(gv[j]), cP[j], bf2f(xv[j]), cQ[j]);
                        if (drop) v *= drop_pick(drop_bits(dkey, m, n, e.N), m, e.drop_p);
                    }
                    o[j] = f2bf(v);
                }
            }
            *reinterpret_cast<u16x8*>(smem + off64(rr, ec)) = o;
        }
        __syncthreads();

        f32x16 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int base = q.halo - ((tap / 3 - 1) * q.Wp + (tap % 3 - 1)) + r;      // source position = p - shift(tap)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const int lr = base + mt * 32;
                    const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(smem + off64(lr, 2 * ks + h));
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bw[tap * 2 + ks], acc[mt], 0, 0, 0);
                }
            }
        }
        // epilogue through LDS (two passes of 64 rows): the fp32 dA tile is re-read as 8-channel chunks so that Y is loaded and
        // DU stored 16 B per lane; u = sc*y + sh ; dU = dA * prelu'(u) ; DU = sc*dU ; sums (dU, dU*y, dA*min(u,0)) per channel
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int mt = pass * 2 + half;
#pragma unroll
                for (int k = 0; k < 16; ++k) Cs[(half * 32 + (k & 3) + 8 * (k >> 2) + 4 * h) * CLD3 + wave * 32 + r] = acc[mt][k];
            }
            __syncthreads();
            float f1[8], f2[8], f3[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { f1[j] = 0.f; f2[j] = 0.f; f3[j] = 0.f; }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = e_r0 + 16 * i;
                const int m = tbl[q.halo + pass * 64 + rr];
                if (m >= 0) {
                    float cv[8];
                    ld8(Cs + rr * CLD3 + e_c8 * 8, cv);
                    const u16x8 yv = *reinterpret_cast<const u16x8*>(Y + (long)m * g.ldxin + e_c8 * 8);
                    u16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float y = bf2f(yv[j]);
                        const float u = fmaf(y, esc[j], esh[j]);
                        const float du = u > 0.f ? cv[j] : esl[j] * cv[j];
                        f1[j] += du; f2[j] += du * y; f3[j] += u > 0.f ? 0.f : cv[j] * u;
                        o[j] = f2bf(esc[j] * du);
                    }
                    *reinterpret_cast<u16x8*>(DU + (long)m * g.ldgo + e_c8 * 8) = o;
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                atomicAdd(&sred[(e_c8 * 8 + j) * 3], (double)f1[j]);
                atomicAdd(&sred[(e_c8 * 8 + j) * 3 + 1], (double)f2[j]);
                atomicAdd(&sred[(e_c8 * 8 + j) * 3 + 2], (double)f3[j]);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < 128) {
        double* p = g.part + ((long)blockIdx.x * g.N + tid) * 3;
        p[0] = sred[tid * 3]; p[1] = sred[tid * 3 + 1]; p[2] = sred[tid * 3 + 2];
    }
}

// Pipelined variant (concat slice 16-B aligned, 32 channels): the raw (G, x) slice rows of tile t+1 travel by LDS-DMA while
// tile t is multiplied and its epilogue runs; the epilogue's Y rows are requested one 32-row pass ahead; the per-channel sums
// stay in registers until the end of the launch.  Barriers inside the pipeline are lds_barrier (bare s_barrier + lgkmcnt(0)): a
// __syncthreads() would drain the DMA and the prefetched loads (its fence waits for vmcnt(0)).
__global__ __launch_bounds__(256, 2) void k_conv3x3_dgrad2_bf16(const ConvDgradArgs g, int n_img, int ntiles, int swz) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const EffSrc& e = g.e;
    const PadGeom q(n_img, g.H, g.W);
    const int nr = (q.rows() + 15) & ~15;                       // image rows, whole DMA row groups (16 rows x 64 B = 1 KiB)
    constexpr int CLD3 = 132;
    const int o_rg = nr * 64, o_rd = 2 * nr * 64, o_tbl = 3 * nr * 64, o_cs = o_tbl + 2 * nr * 4;     // eff image at 0
    const int o_km = o_cs + 32 * 132 * 4 + 448 * 4;             // [nr rounded up to 64] keep words of the tile's rows (when the forward stored them)
    int* tbl = reinterpret_cast<int*>(smem + o_tbl);            // [2][nr] pixel index per image row (this tile / next tile)
    float* Cs = reinterpret_cast<float*>(smem + o_cs);          // [32][CLD3] fp32 dA rows of one pass
    double* red = reinterpret_cast<double*>(smem + o_cs);       // [4][128][3] after the last tile
    float* tab = reinterpret_cast<float*>(smem + o_cs + 32 * CLD3 * 4);      // sc, sh, sl of norm2 [3][128]; P, Q of the slice [2][32]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const float invWp = 1.0f / q.Wp, invHp = 1.0f / q.Hp;
    const bf16* __restrict__ G = reinterpret_cast<const bf16*>(e.G);
    const bf16* __restrict__ D = reinterpret_cast<const bf16*>(e.X);
    const bf16* __restrict__ Y = reinterpret_cast<const bf16*>(g.Xin);
    const char* __restrict__ zeros = reinterpret_cast<const char*>(g.zeros);
    bf16* __restrict__ DU = reinterpret_cast<bf16*>(g.Gout);
    const int nb = gridDim.x;
    const int lb = swz ? (blockIdx.x & 7) * (nb >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const bool drop = e.drop_p > 0.f;
    const uint32_t dkey = drop_key(e.seed, e.stream_id);

    const bf16* __restrict__ Wf = reinterpret_cast<const bf16*>(g.Wfrag) + ((long)wave * 18 * 64 + lane) * 8;
    bf16x8_t bw[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) bw[i] = *reinterpret_cast<const bf16x8_t*>(Wf + i * 512);
    const int e_c8 = tid & 15, e_r0 = tid >> 4;                 // epilogue role: 8-channel chunk, rows e_r0 + 16*i of a pass
    if (tid < 128) { tab[tid] = g.sc[tid]; tab[128 + tid] = g.sh[tid]; tab[256 + tid] = g.sl[tid]; }
    if (tid < 32) { tab[384 + tid] = e.P[tid]; tab[416 + tid] = e.Q[tid]; }
    const int ec = tid & 3, er0 = tid >> 2;                     // eff role: chunk ec of rows er0 + 64*k
    float st1[8], st2[8], st3[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { st1[j] = 0.f; st2[j] = 0.f; st3[j] = 0.f; }

    auto fill_tbl = [&](int slot, int tile) {
        for (int rr = tid; rr < nr; rr += 256) tbl[slot * nr + rr] = pix_of(q, tile * TP - q.halo + rr, invWp, invHp);
    };
    const uint32_t* __restrict__ KM = e.keep;                    // keep words of the forward kernel (or nullptr: hash)
    const float dinv = 1.f / (1.f - e.drop_p);
    auto dma_raw = [&](int slot) {                              // both slices, this wave's row groups; padding rows <- zeros
        const int rsub = lane >> 2, chunk = lane & 3;
        if (KM != nullptr) {                                    // one word per row: 64 rows per instruction (lane = row), 4 B per lane
            for (int r64 = wave; r64 * 64 < nr; r64 += 4) {
                const int rr = r64 * 64 + lane;
                const int m = rr < nr ? tbl[slot * nr + rr] : -1;
                const char* sk = m >= 0 ? reinterpret_cast<const char*>(KM + m) : zeros;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)sk,
                                                 (__attribute__((address_space(3))) void*)(smem + o_km + r64 * 256), 4, 0, 0);
            }
        }
        for (int rg = wave; rg * 16 < nr; rg += 4) {
            const int m = tbl[slot * nr + rg * 16 + rsub];
            const char* sg = m >= 0 ? reinterpret_cast<const char*>(G + (long)m * e.ldg + e.c_off) + chunk * 16 : zeros + chunk * 16;
            const char* sd = m >= 0 ? reinterpret_cast<const char*>(D + (long)m * e.ldx + e.c_off) + chunk * 16 : zeros + chunk * 16;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)sg,
                                             (__attribute__((address_space(3))) void*)(smem + o_rg + rg * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)sd,
                                             (__attribute__((address_space(3))) void*)(smem + o_rd + rg * 1024), 16, 0, 0);
        }
    };
    auto load_y = [&](int slot, int pass, u16x8 (&yv)[2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = tbl[slot * nr + q.halo + pass * 32 + e_r0 + 16 * i];
            yv[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (m >= 0) yv[i] = *reinterpret_cast<const u16x8*>(Y + (long)m * g.ldxin + e_c8 * 8);
        }
    };

    int cur = 0;
    if (lb < ntiles) fill_tbl(0, lb);
    __syncthreads();
    if (lb < ntiles) dma_raw(0);
    // the epilogue's Y rows travel TWO passes ahead of their use, across tile boundaries: pass p of a tile lives in yq[p]; passes
    // 0/1 of the next tile are requested during passes 2/3 of this one (one pass ahead left a pass shorter than an HBM round trip)
    u16x8 yq[4][2];
    if (lb < ntiles) { load_y(0, 0, yq[0]); load_y(0, 1, yq[1]); }
    for (int t = lb; t < ntiles; t += nb, cur ^= 1) {
        if (t + nb < ntiles) fill_tbl(cur ^ 1, t + nb);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this wave's share of tile t's raw rows has landed
        __syncthreads();                                         // ... and everybody else's; next table visible
        // eff image: 16-B chunk ec of row rr at off64(rr, ec);  eff = (G + P*x + Q) * dropout, exactly 0 on padding rows
        float cP[8], cQ[8];
        ld8(tab + 384 + ec * 8, cP);
        ld8(tab + 416 + ec * 8, cQ);
        for (int rr = er0; rr < nr; rr += 64) {
            const int m = tbl[cur * nr + rr];
            u16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
            if (m >= 0) {
                const u16x8 gv = *reinterpret_cast<const u16x8*>(smem + o_rg + rr * 64 + ec * 16);
                const u16x8 xv = *reinterpret_cast<const u16x8*>(smem + o_rd + rr * 64 + ec * 16);
                const uint32_t kb = KM != nullptr ? *reinterpret_cast<const uint32_t*>(smem + o_km + rr * 4) >> (ec * 8) : 0u;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float v = eff3(bf2f(gv[j]), cP[j], bf2f(xv[j]), cQ[j]);
                    if (drop) v *= KM != nullptr ? (((kb >> j) & 1u) ? dinv : 0.f)
                                                 : drop_pick(drop_bits32(dkey, m, ec * 8 + j, e.N), m, e.drop_p);      // (pixels * N < 2^32: conv3x3_dgrad_tile_ok)
                    o[j] = f2bf(v);
                }
            }
            *reinterpret_cast<u16x8*>(smem + off64(rr, ec)) = o;
        }
        __syncthreads();                                         // image complete, raw buffers free again
        if (t + nb < ntiles) dma_raw(cur ^ 1);                   // next tile's slices travel under the MFMAs + epilogue

        // the 128 positions are multiplied in two halves of 64 (two accumulator tiles live instead of four: the kernel sits at
        // the 256-register limit of two workgroups per CU); each half is followed by its two 32-row epilogue passes
#pragma unroll
        for (int half = 0; half < 2; ++half) {
        f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int base = q.halo - ((tap / 3 - 1) * q.Wp + (tap % 3 - 1)) + r + half * 64;      // source position = p - shift(tap)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const int lr = base + mt * 32;
                    const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(smem + off64(lr, 2 * ks + h));
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bw[tap * 2 + ks], acc[mt], 0, 0, 0);
                }
            }
        }
        // epilogue, four passes of 32 rows through the fp32 C tile: u = sc*y + sh ; dU = dA * prelu'(u) ; DU = sc*dU ;
        // sums (dU, dU*y, dA*min(u,0)) per channel
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int pass = half * 2 + pp;
            u16x8 (&yc)[2] = yq[pass];
            if (pass < 2) load_y(cur, pass + 2, yq[pass + 2]);
            else if (t + nb < ntiles) load_y(cur ^ 1, pass - 2, yq[pass - 2]);      // next tile's table: filled at the top of this iteration
#pragma unroll
            for (int k = 0; k < 16; ++k) Cs[((k & 3) + 8 * (k >> 2) + 4 * h) * CLD3 + wave * 32 + r] = acc[pp][k];
            lds_barrier();
            float esc[8], esh[8], esl[8];
#pragma unroll
            for (int j4 = 0; j4 < 2; ++j4) {      // (not three ld8: the six reads leave in another order, and the kernel's schedule with them)
                const float4 a4 = *reinterpret_cast<const float4*>(tab + e_c8 * 8 + j4 * 4);
                const float4 b4 = *reinterpret_cast<const float4*>(tab + 128 + e_c8 * 8 + j4 * 4);
                const float4 c4 = *reinterpret_cast<const float4*>(tab + 256 + e_c8 * 8 + j4 * 4);
                esc[j4 * 4] = a4.x; esc[j4 * 4 + 1] = a4.y; esc[j4 * 4 + 2] = a4.z; esc[j4 * 4 + 3] = a4.w;
                esh[j4 * 4] = b4.x; esh[j4 * 4 + 1] = b4.y; esh[j4 * 4 + 2] = b4.z; esh[j4 * 4 + 3] = b4.w;
                esl[j4 * 4] = c4.x; esl[j4 * 4 + 1] = c4.y; esl[j4 * 4 + 2] = c4.z; esl[j4 * 4 + 3] = c4.w;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int rr = e_r0 + 16 * i;
                const int m = tbl[cur * nr + q.halo + pass * 32 + rr];
                if (m >= 0) {
                    float cv[8];
                    ld8(Cs + rr * CLD3 + e_c8 * 8, cv);
                    u16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float y = bf2f(yc[i][j]);
                        const float u = fmaf(y, esc[j], esh[j]);
                        const float du = u > 0.f ? cv[j] : esl[j] * cv[j];
                        st1[j] += du; st2[j] += du * y; st3[j] += u > 0.f ? 0.f : cv[j] * u;
                        o[j] = f2bf(esc[j] * du);
                    }
                    *reinterpret_cast<u16x8*>(DU + (long)m * g.ldgo + e_c8 * 8) = o;
                }
            }
            lds_barrier();
        }
        }   // half
    }
    // reduce the 16 row groups: 4 per wave by shuffles (lane bits 4, 5), then across waves through LDS
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double d1 = (double)st1[j], d2 = (double)st2[j], d3 = (double)st3[j];
        d1 += __shfl_xor(d1, 16); d1 += __shfl_xor(d1, 32);
        d2 += __shfl_xor(d2, 16); d2 += __shfl_xor(d2, 32);
        d3 += __shfl_xor(d3, 16); d3 += __shfl_xor(d3, 32);
        if (lane < 16) {
            double* p = red + ((wave * 128) + e_c8 * 8 + j) * 3;
            p[0] = d1; p[1] = d2; p[2] = d3;
        }
    }
    __syncthreads();
    if (tid < 128) {
        double a = 0, b = 0, c = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { a += red[(w * 128 + tid) * 3]; b += red[(w * 128 + tid) * 3 + 1]; c += red[(w * 128 + tid) * 3 + 2]; }
        double* p = g.part + ((long)blockIdx.x * g.N + tid) * 3;
        p[0] = a; p[1] = b; p[2] = c;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Third data-gradient kernel (the one the dense layers of blocks 1-3 run): consecutive tiles per workgroup, the eff image in a ring
// of 512 rows, one barrier per tile.  k_conv3x3_dgrad2_bf16 rebuilds the whole (128 + 2 halo)-row eff image per tile (2.1x the rows
// at W = 69, each with its dropout flags and BatchNorm mean terms) and walks ten barriers per tile -- fp32 C tile exchange between the
// four waves, pass by pass -- which its ablations put at half of its time ("other": 177 of 358 us).  Here:
//   * 512 threads = 8 waves: wave (cs, ph) owns output channels [32 cs, +32) for positions [64 ph, +64) of the tile; its 18 weight
//     fragments stay in registers; two waves per SIMD, so one wave's epilogue runs under the other's MFMAs;
//   * every eff row is built ONCE, as one of the 128 new rows of the next tile: thread -> (row, 16-B chunk), slice loads requested
//     two tiles ahead, keep bits or hash;
//   * the epilogue is wave-private: the wave's 32 x 32 fp32 tile goes through its own LDS patch (no workgroup barrier), a lane then
//     owns (row, 8 channels): Y load (requested before the MFMAs), PReLU / BatchNorm backward, 16-B store, fp32 running sums.
// Row space as in the weight-gradient kernel: row 0 = padded position t0 * TP - halo, ring slot = row & 511, table entry = row & 1023.
constexpr int DG_RING = 512, DG_TBL = 1024, DG_CP = 36;
__global__ __launch_bounds__(512, 1) void k_conv3x3_dgrad3_bf16(const ConvDgradArgs g, int n_img, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const EffSrc& e = g.e;
    const PadGeom q(n_img, g.H, g.W);
    const int nrows = q.rows();
    constexpr int o_tbl = DG_RING * 64, o_tab = o_tbl + DG_TBL * 4, o_cw = o_tab + 448 * 4, o_w = o_cw + 8 * 32 * DG_CP * 4;
    int* tbl = reinterpret_cast<int*>(smem + o_tbl);
    float* tab = reinterpret_cast<float*>(smem + o_tab);        // sc, sh, sl of norm2 [3][128]; P, Q of the slice [2][32]
    double* red = reinterpret_cast<double*>(smem + o_cw);       // [8][32][3] after the last tile (aliases the C patches)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cs = wave & 3, ph = wave >> 2;
    float* Cw = reinterpret_cast<float*>(smem + o_cw) + wave * 32 * DG_CP;      // this wave's [32][DG_CP] fp32 patch
    const int r = lane & 31, h = lane >> 5;
    const float invWp = 1.0f / q.Wp, invHp = 1.0f / q.Hp;
    const bf16* __restrict__ G = reinterpret_cast<const bf16*>(e.G);
    const bf16* __restrict__ D = reinterpret_cast<const bf16*>(e.X);
    const bf16* __restrict__ Y = reinterpret_cast<const bf16*>(g.Xin);
    const char* __restrict__ zeros = reinterpret_cast<const char*>(g.zeros);
    bf16* __restrict__ DU = reinterpret_cast<bf16*>(g.Gout);
    const uint32_t* __restrict__ KM = e.keep;
    bf16* __restrict__ EY = reinterpret_cast<bf16*>(g.ey_out);
    const int nb = gridDim.x, per = ntiles / nb, rem = ntiles % nb;           // (own copy of tile_span: see there)
    const int t0 = blockIdx.x * per + min((int)blockIdx.x, rem), ntl = per + ((int)blockIdx.x < rem ? 1 : 0);
    const int g_org = t0 * TP - q.halo;
    const bool drop = e.drop_p > 0.f;
    const uint32_t dkey = drop_key(e.seed, e.stream_id);
    const float dinv = 1.f / (1.f - e.drop_p);

    // the 4 x 18 weight fragments (72 KB) live in LDS: in registers (72 per lane) they push the kernel past the 256 registers two waves
    // per SIMD leave each, next to the accumulators, the Y rows in flight and the running sums
    {
        const u16x8* __restrict__ wsrc = reinterpret_cast<const u16x8*>(g.Wfrag);
        u16x8* wdst = reinterpret_cast<u16x8*>(smem + o_w);
        for (int i = tid; i < 4 * 18 * 64; i += 512) wdst[i] = wsrc[i];
    }
    const char* wl = smem + o_w + (cs * 18 * 64 + lane) * 16;
    if (tid < 128) { tab[tid] = g.sc[tid]; tab[128 + tid] = g.sh[tid]; tab[256 + tid] = g.sl[tid]; }
    if (tid < 32) { tab[384 + tid] = e.P[tid]; tab[416 + tid] = e.Q[tid]; }

    // eff role of a thread: chunk ec of one row per 128-row batch
    const int ec = tid & 3, er = tid >> 2;
    auto fill_rows = [&](int row0, int n) {
        ring_tbl_fill<DG_TBL>(tbl, q, g_org, row0, n, tid, 512, invWp, invHp);
    };
    auto eff_fetch = [&](int m, u16x8& gv, u16x8& xv, uint32_t& kw) {
        const long o = (long)(m >= 0 ? m : 0);
        gv = *reinterpret_cast<const u16x8*>(G + o * e.ldg + e.c_off + ec * 8);
        xv = *reinterpret_cast<const u16x8*>(D + o * e.ldx + e.c_off + ec * 8);
        kw = *(KM != nullptr ? KM + o : reinterpret_cast<const uint32_t*>(zeros));
    };
    auto eff_store = [&](int row, int m, const u16x8& gv, const u16x8& xv, uint32_t kw) {      // eff = (G + P*x + Q) * dropout; 0 on padding rows
        u16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
        if (m >= 0) {
            float cP[8], cQ[8];
            ld8(tab + 384 + ec * 8, cP);
            ld8(tab + 416 + ec * 8, cQ);
            const uint32_t kb = kw >> (ec * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = eff3(bf2f(gv[j]), cP[j], bf2f(xv[j]), cQ[j]);
                if (drop) v *= KM != nullptr ? (((kb >> j) & 1u) ? dinv : 0.f)
                                             : drop_pick(drop_bits32(dkey, m, ec * 8 + j, e.N), m, e.drop_p);      // (pixels * N < 2^32: launcher)
                o[j] = f2bf(v);
            }
        }
        *reinterpret_cast<u16x8*>(smem + off64(row & (DG_RING - 1), ec)) = o;
        if (EY != nullptr && m >= 0) *reinterpret_cast<u16x8*>(EY + (long)m * 32 + ec * 8) = o;      // the weight gradient's operand, built once
    };

    if (ntl > 0) fill_rows(0, nrows + min(ntl - 1, 2) * TP);                // tile 0's rows, the new rows of tiles 1 and 2
    __syncthreads();
    if (ntl > 0) {
        for (int row = er; row < nrows; row += 128) {                       // tile 0: all its rows
            u16x8 g0, x0; uint32_t k0;
            const int m = tbl[row & (DG_TBL - 1)];
            eff_fetch(m, g0, x0, k0);
            eff_store(row, m, g0, x0, k0);
        }
    }
    u16x8 gv, xv;
    uint32_t kw = 0;
    int mm = -1;
    if (ntl > 1) { mm = tbl[(nrows + er) & (DG_TBL - 1)]; eff_fetch(mm, gv, xv, kw); }       // tile 1's new rows
    else { gv = u16x8{0, 0, 0, 0, 0, 0, 0, 0}; xv = gv; }
    __syncthreads();

    // epilogue role of a lane in its wave's 32 x 32 patch: rows el and el + 16, channel chunk e4
    const int e4 = lane & 3, el = lane >> 2;
    float st1[8], st2[8], st3[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { st1[j] = 0.f; st2[j] = 0.f; st3[j] = 0.f; }
    // Y rows of the wave's two 32-position passes: slot mt is reloaded with the NEXT tile's rows as soon as this tile's pass mt has
    // consumed it, so a request has a whole tile to arrive (requested at the top of its own tile it had the MFMA phase only: ~1 us
    // against 2-4 us of HBM latency under load, and the first version of this kernel ran 45 % slower than the kernel it replaces)
    u16x8 yq[2][2];
    auto y_fetch = [&](int tile_row, int mt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = tbl[(tile_row + q.halo + ph * 64 + mt * 32 + el + 16 * i) & (DG_TBL - 1)];
            const long o = (long)(m >= 0 ? m : 0);
            yq[mt][i] = *reinterpret_cast<const u16x8*>(Y + o * g.ldxin + cs * 32 + e4 * 8);
        }
    };
    if (ntl > 0) { y_fetch(0, 0); y_fetch(0, 1); }

    for (int il = 0; il < ntl; ++il) {
        const int trow = il * TP;                                            // first image row of this tile
        // ---- next tiles: eff rows of tile il+1 into the ring, slice loads of tile il+2, table of tile il+3 ----
        if (il + 1 < ntl) eff_store(trow + nrows + er, mm, gv, xv, kw);
        if (il + 2 < ntl) { mm = tbl[(trow + TP + nrows + er) & (DG_TBL - 1)]; eff_fetch(mm, gv, xv, kw); }
        if (il + 3 < ntl) fill_rows(trow + 2 * TP + nrows, TP);
        f32x16 acc[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[mt][k] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int base = trow + q.halo - ((tap / 3 - 1) * q.Wp + (tap % 3 - 1)) + ph * 64 + r;      // source position = p - shift(tap)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(wl + (tap * 2 + ks) * 1024);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(smem + off64((base + mt * 32) & (DG_RING - 1), 2 * ks + h));
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[mt], 0, 0, 0);
                }
            }
        }
        // ---- epilogue: u = sc*y + sh ; dU = dA * prelu'(u) ; DU = sc*dU ; sums (dU, dU*y, dA*min(u,0)) per channel ----
        float esc[8], esh[8], esl[8];                                        // norm2's table of this lane's 8 channels (re-read per tile: 24 registers
        ld8(tab + cs * 32 + e4 * 8, esc);                                     // the MFMA phase needs more)
        ld8(tab + 128 + cs * 32 + e4 * 8, esh);
        ld8(tab + 256 + cs * 32 + e4 * 8, esl);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int k = 0; k < 16; ++k) Cw[((k & 3) + 8 * (k >> 2) + 4 * h) * DG_CP + r] = acc[mt][k];
            // (the same wave reads what it wrote: LDS operations of a wave execute in order, no barrier)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = tbl[(trow + q.halo + ph * 64 + mt * 32 + el + 16 * i) & (DG_TBL - 1)];
                float cv[8];
                ld8(Cw + (el + 16 * i) * DG_CP + e4 * 8, cv);
                u16x8 o;
                const bool ok = m >= 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float y = bf2f(yq[mt][i][j]);
                    const float u = fmaf(y, esc[j], esh[j]);
                    const float c = ok ? cv[j] : 0.f;
                    const float du = u > 0.f ? c : esl[j] * c;
                    st1[j] += du; st2[j] = fmaf(du, y, st2[j]); st3[j] += u > 0.f ? 0.f : c * u;
                    o[j] = f2bf(esc[j] * du);
                }
                if (ok) *reinterpret_cast<u16x8*>(DU + (long)m * g.ldgo + cs * 32 + e4 * 8) = o;
            }
            if (il + 1 < ntl) y_fetch(trow + TP, mt);                        // this slot's rows of the next tile
        }
        lds_barrier();      // tile il+1's rows and the table entries are in place
    }
    // per-channel sums: lanes with equal e4 hold the same 8 channels (fold lane bits 2..5), the two position halves through LDS
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double d1 = (double)st1[j], d2 = (double)st2[j], d3 = (double)st3[j];
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) { d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); d3 += __shfl_xor(d3, o); }
        if (lane < 4) {
            double* p = red + ((wave * 32) + e4 * 8 + j) * 3;
            p[0] = d1; p[1] = d2; p[2] = d3;
        }
    }
    __syncthreads();
    if (tid < 128) {
        const int c_cs = tid >> 5, c_in = tid & 31;
        double a = 0, b = 0, c = 0;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const double* p = red + (((hh * 4 + c_cs) * 32) + c_in) * 3;
            a += p[0]; b += p[1]; c += p[2];
        }
        double* p = g.part + ((long)blockIdx.x * g.N + tid) * 3;
        p[0] = a; p[1] = b; p[2] = c;
    }
}
static long cu_tiles() { return 256; }      // workgroups of a full persistent grid (one per CU)
constexpr size_t dgrad3_smem() { return size_t(DG_RING) * 64 + DG_TBL * 4 + 448 * 4 + 8 * 32 * DG_CP * 4 + 4 * 18 * 1024; }
constexpr size_t dgrad2_smem(const PadGeom& q) { const size_t nr = (q.rows() + 15) & ~15; return 3 * nr * 64 + 2 * nr * 4 + 32 * 132 * 4 + 448 * 4 + ((nr + 63) & ~size_t(63)) * 4; }
constexpr size_t dgrad_smem(const PadGeom& q) { const size_t r4 = (q.rows() + 3) & ~3; return r4 * 68 + 128 * 24 + 64 * 132 * 4; }

}  // namespace

bool conv3x3_dgrad_tile_ok(const ConvDgradArgs& a) {
    if (!conv3x3_tile_enabled() || a.mode != MODE_BF16 || a.dmode != DG_3X3 || a.N != 128 || a.e.N > 32 || a.Kp != 288) return false;
    if (a.Wfrag == nullptr || a.accumulate || a.ldxin != 128 || a.ldgo != 128) return false;
    if ((a.e.ldg & 7) || (a.e.ldx & 7) || (a.e.c_off & 1) || a.M % (a.H * a.W) != 0) return false;
    return geom_of(a.M, a.H, a.W).gtot < (1L << 24) && (long)a.M * a.e.N < (1L << 32);
}
// The ONE place that chooses the data-gradient kernel (as conv3x3_fwd_kernel for the forward)
Conv3x3Dgrad conv3x3_dgrad_kernel(const ConvDgradArgs& a) {
    if (!conv3x3_dgrad_tile_ok(a)) return CONV3X3_DGRAD_NONE;
    static const bool any_size = TCVN_KNOB_SET("TCVN_DGRAD3_ANY_SIZE");      // validation build: the consecutive-tile kernel at any size
    const PadGeom q = geom_of(a.M, a.H, a.W);
    // both LDS-DMA kernels need the concat slice 16-B aligned and all 32 channels present
    const bool dma = a.zeros != nullptr && a.e.N == 32 && (a.e.c_off & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(a.e.G) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.e.X) & 15) == 0;
    // consecutive tiles, eff ring, wave-private epilogue -- from 8 tiles per workgroup on: below that its prologue (72 KB of weights into LDS, the
    // whole first eff image) costs more than the ring saves (block 3, 816 tiles: 37 us against 32 us for the two-workgroup kernel; block 2,
    // 3 600 tiles: 94 against 102)
    if (dma && q.rows() + TP + 8 <= DG_RING && (q.tiles() >= 8 * cu_tiles() || any_size) &&
        (reinterpret_cast<uintptr_t>(a.Xin) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.Gout) & 15) == 0)
        return CONV3X3_DGRAD_CONSEC;
    return dma && dgrad2_smem(q) <= 80 * 1024 ? CONV3X3_DGRAD_PIPELINED : CONV3X3_DGRAD_TWO_WG;
}
int conv3x3_dgrad_tile_nblk(const ConvDgradArgs& a) {      // one 512-thread workgroup per CU, or two of 256
    const long ntiles = geom_of(a.M, a.H, a.W).tiles();
    return conv3x3_dgrad_kernel(a) == CONV3X3_DGRAD_CONSEC ? tile_grid(ntiles) : tile_grid2(ntiles);
}
int conv3x3_dgrad_tile(const ConvDgradArgs& a, hipStream_t st) {
    const PadGeom q = geom_of(a.M, a.H, a.W);
    const int n_img = a.M / (a.H * a.W), ntiles = (int)q.tiles(), nb = tile_grid2(ntiles), swz = (nb >= 8 && nb % 8 == 0) ? 1 : 0;
    static bool attr_consec = false, attr_pipe = false;
    ProfScope ps("k_conv3x3_dgrad_bf16", 2.0 * a.M * (double)a.N * 9 * a.e.N, (double)a.M * 2.0 * (2 * a.e.N + 2 * a.N), st);   // (G, x) slices in; Y in, DU out
    int rc;
    switch (conv3x3_dgrad_kernel(a)) {
        case CONV3X3_DGRAD_NONE: return -2;
        case CONV3X3_DGRAD_CONSEC:
            if ((rc = allow_lds(reinterpret_cast<const void*>(k_conv3x3_dgrad3_bf16), 160 * 1024, attr_consec))) return rc;
            hipLaunchKernelGGL(k_conv3x3_dgrad3_bf16, dim3(tile_grid(ntiles)), dim3(512), dgrad3_smem(), st, a, n_img, ntiles);
            break;
        case CONV3X3_DGRAD_PIPELINED:
            if ((rc = allow_lds(reinterpret_cast<const void*>(k_conv3x3_dgrad2_bf16), 80 * 1024, attr_pipe))) return rc;
            hipLaunchKernelGGL(k_conv3x3_dgrad2_bf16, dim3(nb), dim3(256), dgrad2_smem(q), st, a, n_img, ntiles, swz);
            break;
        case CONV3X3_DGRAD_TWO_WG:
            hipLaunchKernelGGL(k_conv3x3_dgrad_bf16, dim3(nb), dim3(256), dgrad_smem(q), st, a, n_img, ntiles, swz);
    }
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace tcvn
