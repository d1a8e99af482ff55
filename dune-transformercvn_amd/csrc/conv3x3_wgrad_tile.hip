// bf16 3x3 convolution on padded LDS tiles (see tile3x3.h), weight gradient.  The forward is conv3x3_fwd_tile.hip, the data gradient
// conv3x3_dgrad_tile.hip.
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

#ifdef TCVN_DEBUG_KNOBS
__device__ unsigned long long g_wg_ph[16];                   // phase counters (tile3x3.h), read by tcvn_debug_wgrad_phases
#endif

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient: dW[tap][c][n] = sum over padded positions p of Yact[p + shift(tap)][c] * eff[p][n].
// The contraction runs over pixels, i.e. over the ROW index of both row-major LDS images, so both MFMA operands are
// read transposed with ds_read_b64_tr_b16 (semantics checked by tools/micro/tr_read_test.hip): per 16-position k-step a
// wave reads the eff fragment once and nine shifted Yact fragments, and owns the 9 x (32 c x 32 n) accumulators of its
// 32-channel slice for the whole launch (144 accumulator registers); one atomic pass at the end.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int WG_RING = 512, WG_TBL = 1024;
// Round 5: the ring carries WG_MIRROR extra rows behind its end that MIRROR its first rows (whoever writes ring row r < WG_MIRROR also writes
// row WG_RING + r).  A transposed read takes the 16 consecutive rows of a k-step starting anywhere in the ring: with the mirror it never
// wraps inside an instruction, so its address is (per-lane part, fixed per tap) + (a SCALAR start, one s_and per tap and k-step) -- one VALU
// add per fragment instead of an add and a mask per read (the multiplying waves issued ~560 instructions per tile around their 72 MFMAs
// and shared the SIMD's issue slots with the helper wave: 4 800 cycles per tile for 2 300 of matrix work, tools/wgrad_phases.py).  The
// ring's swizzle moves only the 64-B quad (wswz: row & 3), so rows r and r + 4 -- the two halves of a fragment -- differ by exactly 1 KiB:
// the second read of a fragment is the first one's address with an immediate offset.
constexpr int WG_MIRROR = 16, WG_RING_BYTES = (WG_RING + WG_MIRROR) * 256;
__device__ __forceinline__ int wswz(int r) { return (r & 3) << 2; }
__device__ __forceinline__ void wg_kloop(f32x16 (&acc)[9], const char* smem, int base_row, const int (&arow0)[9], const int (&lp)[9], const char* ebase) {
    bf16x8_t fr[3][3], fb[2];
    auto issue = [&](int j) {                                       // j = 3 * ks + third
        const int ks = j / 3, third = j - 3 * ks;
        if (third == 0) fb[ks & 1] = tr_frag(ebase, ks * 1024, ks * 1024 + 256);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int tap = third * 3 + i;
            const int s0 = ((base_row + arow0[tap] + 16 * ks) & (WG_RING - 1)) << 8;      // uniform: scalar ALU
            fr[j % 3][i] = tr_frag(smem + s0, lp[tap], lp[tap] + 1024);
        }
    };
    constexpr int NG = 3 * (TP / 16);
    issue(0);
    issue(1);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        __builtin_amdgcn_sched_barrier(0);
        // group j complete <=> at most the reads of group j+1 outstanding (6, or 8 when it opens a k-step)
        if (j + 1 < NG) { if ((j + 1) % 3 == 0) __builtin_amdgcn_s_waitcnt(0xC07F | (8 << 8)); else __builtin_amdgcn_s_waitcnt(0xC07F | (6 << 8)); }
        else __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_sched_barrier(0);
        if (j + 2 < NG) issue(j + 2);
        __builtin_amdgcn_sched_barrier(0);
        const int ks = j / 3, third = j - 3 * ks;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            acc[third * 3 + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[j % 3][i], fb[ks & 1], acc[third * 3 + i], 0, 0, 0);
    }
}

// Two waves per SIMD with different roles (as in the forward pair kernel): 512 threads.  Waves 0-3 only multiply -- the pipelined
// fragment reads + 72 MFMAs of tile t.  Waves 4-7 prepare tile t+1 meanwhile: image rows by LDS-DMA, the eff tile (slice loads,
// BatchNorm mean terms, dropout keep bits), the pixel table of tile t+2.  One barrier per tile.
// A workgroup walks CONSECUTIVE tiles and keeps the image in a ring of WG_RING = 512 rows (128 KB): tile t+1 shares all but its last
// 128 rows with tile t, so only those are fetched -- 32 KB per tile instead of the whole 70 KB image (272 rows at W = 69).  The phase
// counters of the one-image-per-tile version showed the helper waves, not the MFMAs, bounding the tile: 6 700 cycles stalled in the DMA
// issue and 5 100 more until the slice loads queued behind it returned, i.e. the kernel moved its 2.1x redundant image traffic at
// the HBM rate (3.2 TB/s) while the multiplying waves waited 9 600 of 13 700 cycles at the barrier.
// Row space of a workgroup: row 0 = padded position t0 * TP - halo; ring slot = row & 511; table entry = row & 1023; the XOR
// swizzle of a row's 16-B chunks is wswz(row) = (row & 3) << 2 (TP and the ring are multiples of 16, so it equals the tile-relative
// value).  Every LDS read of the multiplying waves is a transposed read of four consecutive rows x 64 B: the forward kernels' `row & 15`
// swizzle put those four rows on the same 16 banks (two- to four-way conflicts on all 160 reads per wave and tile, rocprofv3 round 4:
// LDS_BANK_CONFLICT = 2.6 x the LDS-active cycles); with row & 3 selecting the 64-B quad they cover all 64 banks.
constexpr int WGRAD_ARGS_KERNARG_OFFSET = 0;      // ConvWgradArgs is the FIRST argument of k_conv3x3_wgrad_bf16 (its link rider reads it from the segment)
template <typename F> struct first_arg;
template <typename A, typename... R> struct first_arg<void (*)(A, R...)> { typedef A type; };
__global__ __launch_bounds__(512, 1) void k_conv3x3_wgrad_bf16(const ConvWgradArgs g, int n_img, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ConvFwdArgs& fa = g.fa;
    const EffSrc& e = g.e;
    const PadGeom q(n_img, fa.H, fa.W);
    const int nrows4 = (q.rows() + 3) & ~3;
    constexpr int eff_off = WG_RING_BYTES;                                // two [TP][32] bf16 tiles behind the ring (+ mirror rows), 64-B rows, unswizzled
    int* tbl = reinterpret_cast<int*>(smem + eff_off + 2 * TP * 64);      // [1024] pixel index of row (row & 1023)
    float* bred = reinterpret_cast<float*>(smem + eff_off);               // [64][32], aliases the eff tiles after the last barrier
    float* xtab = reinterpret_cast<float*>(smem + eff_off + 2 * TP * 64 + WG_TBL * 4);      // act_fused: [3][128] tables of the image's BatchNorm + PReLU
    const bool xf = fa.act_fused != 0;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w4 = wave & 3, htid = tid & 255;                             // wave / thread index inside the role
    int t0, t1;
    const int g_org = tile_span(q, ntiles, t0, t1);
#ifdef TCVN_DEBUG_KNOBS
    unsigned long long ph[16] = {0};
#endif

    if (wave >= 4) {
        // ---------------- helper role: tables, image DMA, eff tiles ----------------
        const float invWp = 1.0f / q.Wp, invHp = 1.0f / q.Hp;
        const bf16* __restrict__ YA = reinterpret_cast<const bf16*>(fa.Aact);
        const char* __restrict__ zeros = reinterpret_cast<const char*>(fa.zeros);
        const bf16* __restrict__ G = reinterpret_cast<const bf16*>(e.G);
        const bf16* __restrict__ D = reinterpret_cast<const bf16*>(e.X);
        const bool drop = e.drop_p > 0.f;
        const uint32_t dkey = drop_key(e.seed, e.stream_id);
        const int ec = htid & 3, ra = htid >> 2;                           // eff staging: rows ra and ra + 64, channel chunk ec
        float cP[8], cQ[8], bsum[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = ec * 8 + j;
            cP[j] = n < e.N ? e.P[n] : 0.f; cQ[j] = n < e.N ? e.Q[n] : 0.f; bsum[j] = 0.f;
        }
        const uint32_t* __restrict__ KM = e.keep;                          // keep words written by the forward kernel (or nullptr: hash)
        const float dinv = 1.f / (1.f - e.drop_p);
        auto eff_fetch = [&](int m, u16x8& gv, u16x8& xv, uint32_t& kw) {                     // slice rows + keep word of pixel m: three loads
            const long o = (long)(m >= 0 ? m : 0);
            gv = *reinterpret_cast<const u16x8*>(G + o * e.ldg + e.c_off + ec * 8);
            xv = *reinterpret_cast<const u16x8*>(D + o * e.ldx + e.c_off + ec * 8);
            kw = *(KM != nullptr ? KM + o : reinterpret_cast<const uint32_t*>(zeros));      // always three loads per row (the barrier counts them)
        };
        auto eff_load = [&](int row0, int i, u16x8& gv, u16x8& xv, uint32_t& kw) -> int {      // row0: first body row of the tile
            const int m = tbl[(row0 + ra + 64 * i) & (WG_TBL - 1)];
            eff_fetch(m, gv, xv, kw);
            return m;
        };
        auto eff_store = [&](int buf, int i, int m, const u16x8& gv, const u16x8& xv, uint32_t kw) {
            u16x8 o;
            const uint32_t kb = kw >> (ec * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float t = 0.f;
                const int n = ec * 8 + j;
                if (m >= 0 && n < e.N) {
                    t = eff3(bf2f(gv[j]), cP[j], bf2f(xv[j]), cQ[j]);
                    if (drop) t *= KM != nullptr ? (((kb >> j) & 1u) ? dinv : 0.f)
                                                 : drop_pick(drop_bits32(dkey, m, n, e.N), m, e.drop_p);      // (pixels * N < 2^32: conv3x3_wgrad_tile_ok)
                }
                o[j] = f2bf(t);
                bsum[j] += bf2f(o[j]);
            }
            *reinterpret_cast<u16x8*>(smem + eff_off + buf * TP * 64 + (ra + 64 * i) * 64 + ec * 16) = o;
        };
        auto fill_rows = [&](int row0, int n) {                            // table entries of rows [row0, row0 + n)
            ring_tbl_fill<WG_TBL>(tbl, q, g_org, row0, n, htid, 256, invWp, invHp);
        };
        // rows [row0, row0 + n) -> ring (n multiple of 4): 4 rows = 1 KiB per wave instruction; all table reads first, then the DMAs
        auto dma_rows = [&](int row0, int n) {
            const int rsub = lane >> 4, slot = lane & 15;
            constexpr int DMA_RG = 24;                                     // row groups per wave: up to 384 rows per call
            int mrow[DMA_RG];
#pragma unroll
            for (int i = 0; i < DMA_RG; ++i) {
                const int rg = w4 + 4 * i;
                mrow[i] = rg * 4 < n ? tbl[(row0 + rg * 4 + rsub) & (WG_TBL - 1)] : -1;
            }
#pragma unroll
            for (int i = 0; i < DMA_RG; ++i) {
                const int rg = w4 + 4 * i;
                if (rg * 4 < n) {
                    const int row = row0 + rg * 4, rr = row + rsub;       // row0 multiple of 4: the group stays inside the ring
                    const char* src = mrow[i] >= 0 ? reinterpret_cast<const char*>(YA + (long)mrow[i] * 128) + ((slot ^ wswz(rr)) << 4)
                                                   : zeros + (slot << 4);
                    // the DMA as inline assembly: behind the builtin the compiler orders every later LDS access of this wave (eff tile,
                    // table) behind vmcnt(0) -- it cannot know they touch other rows -- which would put the DMAs last in the iteration with
                    // their latency exposed at the barrier.  The waits that matter are placed by hand (vmcnt(6) in front of the barrier).
                    const unsigned lds = __builtin_amdgcn_readfirstlane(
                        (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)(smem + (row & (WG_RING - 1)) * 256)));
                    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds), "v"(src) : "memory");      // (m0 is not allocatable: nothing else in this kernel uses it)
                    if ((row & (WG_RING - 1)) < WG_MIRROR) {               // the ring's first rows also live behind its end (uniform: row is a multiple of 4)
                        const unsigned lds2 = lds + WG_RING * 256;
                        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds2), "v"(src) : "memory");
                    }
                }
            }
        };
        // act_fused: the image rows arrive RAW (the bottleneck map itself); the helper wave that requested a row group applies the
        // layer's BatchNorm + PReLU to it in LDS once its DMAs have landed, in front of the tile barrier (same row groups as dma_rows)
        // (phase counters, first version: 3 630 cycles per wave and tile for 8 chunks -- three dependent LDS round trips per group of four
        // chunks and the 24 table values re-read per call; now every LDS read of a call is requested before the first use and the
        // thread's table values stay in registers for the whole launch)
        Act8 xtb;
        auto xform_rows = [&](int row0, int n) {
            const int rsub = lane >> 4, cc = lane & 15;
            for (int i0 = 0; (w4 + 4 * i0) * 4 < n; i0 += 8) {
                int mr[8];
                u16x8 v[8];
                char* p[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int rg = w4 + 4 * (i0 + j);
                    const bool in = rg * 4 < n;
                    const int row = row0 + (in ? rg * 4 : 0) + rsub;
                    mr[j] = tbl[row & (WG_TBL - 1)];
                    if (!in) mr[j] = -1;
                    p[j] = smem + (row & (WG_RING - 1)) * 256 + ((cc ^ wswz(row)) << 4);
                    v[j] = *reinterpret_cast<const u16x8*>(p[j]);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (mr[j] >= 0) {
                        const u16x8 o = act8_apply(v[j], xtb);
                        *reinterpret_cast<u16x8*>(p[j]) = o;
                        if (p[j] < smem + WG_MIRROR * 256) *reinterpret_cast<u16x8*>(p[j] + WG_RING * 256) = o;      // mirror of the ring's first rows
                    }
            }
        };
        // With the eff rows materialised by the data-gradient kernel (e.ey): a tile's 128 rows x 64 B arrive by DMA like the image rows,
        // 16 rows per wave instruction (lane = 4 * row + chunk); the helper then only adds up the bias gradient from the landed tile.
        const bf16* __restrict__ EYs = reinterpret_cast<const bf16*>(e.ey);
        auto dma_eff = [&](int row0, int buf) {                            // row0: first body row of the tile
            const int rsub = lane >> 2, chunk = lane & 3;
            int mr[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) mr[i] = tbl[(row0 + (w4 + 4 * i) * 16 + rsub) & (WG_TBL - 1)];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const char* src = mr[i] >= 0 ? reinterpret_cast<const char*>(EYs + (long)mr[i] * 32 + chunk * 8) : zeros + chunk * 16;
                const unsigned lds = __builtin_amdgcn_readfirstlane(
                    (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)(smem + eff_off + buf * TP * 64 + (w4 + 4 * i) * 1024)));
                asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds), "v"(src) : "memory");
            }
        };
        auto bias_from_tile = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const u16x8 v = *reinterpret_cast<const u16x8*>(smem + eff_off + buf * TP * 64 + (ra + 64 * i) * 64 + ec * 16);
#pragma unroll
                for (int j = 0; j < 8; ++j) bsum[j] += bf2f(v[j]);
            }
        };
        // Pipeline of the helper role, iteration i (tile t0 + i is being multiplied): eff tile of tile i+1 from the slice rows requested
        // one iteration earlier (a tile time ago: they have arrived), DMA of tile i+1's new image rows, slice loads of tile i+2,
        // table entries of tile i+3's new rows.  The barrier waits for the DMAs only -- vmcnt(6): the six slice loads behind them stay in
        // flight (waiting for them there cost 5 300 cycles per tile, the whole memory latency under load).
        const int ntl = t1 - t0;
        if (ntl > 0) fill_rows(0, nrows4 + min(ntl - 1, 2) * TP);          // tile 0's image rows, the new rows of tiles 1 and 2
        if (xf) act_tab_fill(xtab, fa.sc, fa.sh, fa.sl, htid, 256);
        __syncthreads();                                                    // (1)
        if (xf) xtb = act8_load(xtab, lane & 15);
        u16x8 gv[2], xv[2];
        uint32_t kw[2];
        int mm[2] = {-1, -1};
        if (ntl > 0) {
            dma_rows(0, nrows4);
            if (EYs != nullptr) dma_eff(q.halo, 0);
            else {
#pragma unroll
                for (int i = 0; i < 2; ++i) { u16x8 g0, x0; uint32_t k0; const int m = eff_load(q.halo, i, g0, x0, k0); eff_store(0, i, m, g0, x0, k0); }
            }
        }
        if (ntl > 1 && EYs == nullptr) {
#pragma unroll
            for (int i = 0; i < 2; ++i) mm[i] = eff_load(TP + q.halo, i, gv[i], xv[i], kw[i]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (xf && ntl > 0) xform_rows(0, nrows4);
        __syncthreads();                                                    // (2)
        int cur = 0;
        TILE_PH_T0();
        if (EYs != nullptr && xf) {
            // Round 5 (the path the dense blocks 1-2 run).  Per tile the helper moves 128 image rows x 256 B (activated on the way) and 128 eff rows
            // x 64 B from HBM to LDS.  Requested one tile ahead and waited for in the same iteration (round 4), a helper wave spent ~1 500 of its
            // 6 100 cycles per tile waiting for those loads, and the multiplying waves waited for the helpers (tools/wgrad_phases.py: k loop 3 800
            // cycles, barrier 2 700).  Now BOTH travel HBM -> registers TWO tiles ahead (two register sets, the loop unrolled by two): a request has
            // a whole tile time to arrive, nothing in the loop waits on vmcnt for the current iteration's requests (the barrier needs lgkmcnt
            // only), the eff tile needs no DMA and its bias sums come from the registers.  32-bit byte offsets against a uniform base (the
            // launchers bound pixels * 256 B below 4 GB).
            const int rsub_x = lane >> 4, cc_x = lane & 15;
            const char* __restrict__ yab = reinterpret_cast<const char*>(YA);
            const char* __restrict__ eyb = reinterpret_cast<const char*>(EYs);
            u16x8 rva[10], rvb[10];                                           // [0..7] image chunks, [8..9] eff chunks (rows ra, ra + 64; chunk ec)
            int ma[10], mb[10];
            auto fetch = [&](int tl, u16x8 (&rv)[10], int (&rm)[10]) {      // tile tl's 128 new image rows and its 128 eff rows -> registers
                const int row0 = (tl - 1) * TP + nrows4, body = tl * TP + q.halo;
#pragma unroll
                for (int j = 0; j < 8; ++j) rm[j] = tbl[(row0 + (w4 + 4 * j) * 4 + rsub_x) & (WG_TBL - 1)];
#pragma unroll
                for (int i = 0; i < 2; ++i) rm[8 + i] = tbl[(body + ra + 64 * i) & (WG_TBL - 1)];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    rv[j] = *reinterpret_cast<const u16x8*>(yab + (size_t)((unsigned)(rm[j] >= 0 ? rm[j] : 0) * 256u + (unsigned)(cc_x * 16)));
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    rv[8 + i] = *reinterpret_cast<const u16x8*>(eyb + (size_t)((unsigned)(rm[8 + i] >= 0 ? rm[8 + i] : 0) * 64u + (unsigned)(ec * 16)));
            };
            auto commit = [&](int tl, const u16x8 (&rv)[10], const int (&rm)[10]) {      // ... -> the ring (activated) and eff buffer tl & 1
                const int row0 = (tl - 1) * TP + nrows4;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int row = row0 + (w4 + 4 * j) * 4 + rsub_x;
                    u16x8 o = act8_apply(rv[j], xtb);
                    if (rm[j] < 0) o = u16x8{0, 0, 0, 0, 0, 0, 0, 0};                      // padding position: a zero row
                    char* wp = smem + (row & (WG_RING - 1)) * 256 + ((cc_x ^ wswz(row)) << 4);
                    *reinterpret_cast<u16x8*>(wp) = o;
                    if ((row & (WG_RING - 1)) < WG_MIRROR) *reinterpret_cast<u16x8*>(wp + WG_RING * 256) = o;       // mirror of the ring's first rows
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    u16x8 o = rv[8 + i];
                    if (rm[8 + i] < 0) o = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
                    *reinterpret_cast<u16x8*>(smem + eff_off + (tl & 1) * TP * 64 + (ra + 64 * i) * 64 + ec * 16) = o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) bsum[j] += bf2f(o[j]);
                }
            };
            if (ntl > 0) bias_from_tile(0);                                 // tile 0's eff rows came by DMA above
            if (ntl > 1) fetch(1, rva, ma);
            for (int il = 0; il < ntl; il += 2) {
                // ---- even half: the multiplying waves work on tile il; set A holds tile il+1 (requested a tile ago) ----
                if (il + 2 < ntl) fetch(il + 2, rvb, mb);
                TILE_PH(8);
                if (il + 3 < ntl) fill_rows((il + 2) * TP + nrows4, TP);                     // new rows of tile il+3
                TILE_PH(10);
                if (il + 1 < ntl) commit(il + 1, rva, ma);
                TILE_PH(13);
                lds_barrier();            // (tile)
                TILE_PH(12);
                if (il + 1 >= ntl) break;
                // ---- odd half: tile il+1 is multiplied; set B holds tile il+2 ----
                if (il + 3 < ntl) fetch(il + 3, rva, ma);
                TILE_PH(8);
                if (il + 4 < ntl) fill_rows((il + 3) * TP + nrows4, TP);                     // new rows of tile il+4
                TILE_PH(10);
                if (il + 2 < ntl) commit(il + 2, rvb, mb);
                TILE_PH(13);
                lds_barrier();
                TILE_PH(12);
            }
        } else if (EYs != nullptr) {
            // act_fused: the 128 new image rows of tile il+1 travel HBM -> registers (8 x 16 B per lane) instead of HBM -> LDS, are activated in
            // registers and written to the ring once.  The DMA + in-place variant needed an LDS read and a second LDS write per chunk, queued
            // behind the multiplying waves' 160 transposed reads per tile on the one LDS pipe of the CU: 3 200-3 600 cycles per wave and tile
            // in the phase counters (the multiplying waves then waited 2 500 of 7 400 cycles at the barrier).
            u16x8 rv[8];
            int rm[8];
            const int rsub_x = lane >> 4, cc_x = lane & 15;
            for (int il = 0; il < ntl; ++il, cur ^= 1) {
                if (il + 1 < ntl) {
                    if (xf) {
                        const int row0 = il * TP + nrows4;
#pragma unroll
                        for (int j = 0; j < 8; ++j) rm[j] = tbl[(row0 + (w4 + 4 * j) * 4 + rsub_x) & (WG_TBL - 1)];
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            rv[j] = *reinterpret_cast<const u16x8*>(YA + (long)(rm[j] >= 0 ? rm[j] : 0) * 128 + cc_x * 8);
                    } else dma_rows(il * TP + nrows4, TP);                 // image: the 128 rows tile il+1 does not share with tile il
                    dma_eff((il + 1) * TP + q.halo, cur ^ 1);              // its eff rows
                }
                TILE_PH(8);
                bias_from_tile(cur);
                TILE_PH(9);
                if (il + 3 < ntl) fill_rows((il + 2) * TP + nrows4, TP);   // new rows of tile il+3
                TILE_PH(10);
                if (xf && il + 1 < ntl) {
                    const int row0 = il * TP + nrows4;
                    TILE_PH(11);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int row = row0 + (w4 + 4 * j) * 4 + rsub_x;
                        u16x8 o = act8_apply(rv[j], xtb);
                        if (rm[j] < 0) o = u16x8{0, 0, 0, 0, 0, 0, 0, 0};                  // padding position: a zero row
                        char* wp = smem + (row & (WG_RING - 1)) * 256 + ((cc_x ^ wswz(row)) << 4);
                        *reinterpret_cast<u16x8*>(wp) = o;
                        if ((row & (WG_RING - 1)) < WG_MIRROR) *reinterpret_cast<u16x8*>(wp + WG_RING * 256) = o;       // mirror of the ring's first rows
                    }
                    TILE_PH(13);
                }
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");      // (tile)
                TILE_PH(12);
            }
        } else
        for (int il = 0; il < ntl; ++il, cur ^= 1) {
            // the six slice loads of the previous iteration landed a tile ago: this wait is free, and it tells the compiler's scoreboard
            // that their registers are ready, so that nothing below waits on the vmcnt counter behind the DMAs
            __builtin_amdgcn_s_waitcnt(0x0F70);
            if (il + 1 < ntl) dma_rows(il * TP + nrows4, TP);              // the 128 rows tile il+1 does not share with tile il: requested first,
            TILE_PH(8);                                                    // they travel under the eff tile and the table work
            if (il + 1 < ntl) {
#pragma unroll
                for (int i = 0; i < 2; ++i) eff_store(cur ^ 1, i, mm[i], gv[i], xv[i], kw[i]);      // tile il+1 (loads of the previous iteration)
            }
            TILE_PH(9);
            const int body2 = il + 2 < ntl ? (il + 2) * TP + q.halo : q.halo;                     // (past the end: any rows -- keeps six loads behind the DMAs)
#pragma unroll
            for (int i = 0; i < 2; ++i) mm[i] = tbl[(body2 + ra + 64 * i) & (WG_TBL - 1)];
            if (il + 3 < ntl) fill_rows((il + 2) * TP + nrows4, TP);       // new rows of tile il+3
            TILE_PH(10);
            __builtin_amdgcn_sched_barrier(0);                             // program order = issue order: the six loads below stay BEHIND the DMAs
#pragma unroll
            for (int i = 0; i < 2; ++i) eff_fetch(mm[i], gv[i], xv[i], kw[i]);
            __builtin_amdgcn_sched_barrier(0);
            if (xf) {
                asm volatile("s_waitcnt vmcnt(6)" ::: "memory");           // the DMAs (in front of the six slice loads) have landed
                if (il + 1 < ntl) xform_rows(il * TP + nrows4, TP);
            }
            asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory");      // (tile) DMAs landed, eff tile and table written
            TILE_PH(12);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (g.dbias != nullptr) {
#pragma unroll
            for (int j = 0; j < 8; ++j) bred[ra * 32 + ec * 8 + j] = bsum[j];
        }
    } else {
        // ---------------- multiplying role ----------------
        f32x16 acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
        // tr-read lane roles: group gq = lane>>4 -> (k half = gq>>1, column half = gq&1); lane 4q+p supplies row q, cols 4p..4p+3
        const int gq = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
        const int khalf = gq >> 1, chalf = gq & 1;
        const int a_chunk = w4 * 4 + 2 * chalf + (tp >> 1), a_sub = (tp & 1) * 8;         // Yact: this wave's 32 channels
        const int b_colbyte = (16 * chalf + 4 * tp) * 2;                                  // eff: 32 channels
        // a fragment's address = scalar start of its 16-row k-step window (wg_kloop) + this lane's part: row 8*khalf + tq of the window, the
        // swizzled 16-B chunk (the swizzle takes row & 3: window starts differ from the tile's first row by multiples of 16 plus the tap's
        // constant shift, so it is fixed per tap) and the 8-B half; the second read of the fragment is 4 rows = 1 KiB further
        int arow0[9], lp[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            arow0[tap] = q.halo + (tap / 3 - 1) * q.Wp + (tap % 3 - 1);
            const int arow = arow0[tap] + 8 * khalf + tq;
            lp[tap] = (8 * khalf + tq) * 256 + ((a_chunk ^ wswz(arow)) << 4) + a_sub;
        }
        const int b_off0 = (8 * khalf + tq) * 64 + b_colbyte;
        __syncthreads();                                                    // (1)
        __syncthreads();                                                    // (2)
        int cur = 0;
        TILE_PH_T0();
        // 8 k-steps x (1 eff + 9 image fragments, two transposed LDS reads each) as a software pipeline over 24 groups of three image
        // fragments (the first group of a k-step also carries the eff fragment): group j+2 is requested while group j is multiplied, so
        // 12-14 LDS reads stay in flight (lgkmcnt holds 15) instead of every k-step waiting for its own 20 reads (7 200 cycles per wave and
        // tile in the phase counters against 2 300 of MFMA issue).  The waits are placed by hand in front of the new requests -- left to
        // itself the compiler sinks the requests behind the MFMAs or waits for all of them.
        for (int t = t0; t < t1; ++t, cur ^= 1) {
            const int base_row = ((t - t0) * TP) & (WG_RING - 1);
            const char* ebase = smem + eff_off + cur * TP * 64 + b_off0;
            wg_kloop(acc, smem, base_row, arow0, lp, ebase);
            TILE_PH(0);
            __syncthreads();                                                // (tile)
            TILE_PH(1);
        }
        // dW[tap*128 + c][n] ; rows of the C tile are this wave's channels, columns the 32 output channels
        const int n = lane & 31, hh = lane >> 5;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = w4 * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                g.slab[(long)blockIdx.x * (9 * 128 * 32) + ((long)tap * 128 + c) * 32 + n] = acc[tap][i];
            }
    }
#ifdef TCVN_DEBUG_KNOBS
    if (lane == 0 && (blockIdx.x & 15) == 0)
        for (int i = 0; i < 16; ++i)
            if (ph[i]) atomicAdd(&g_wg_ph[i], ph[i]);
#endif
    if (g.dbias != nullptr) {
        __syncthreads();
        if (tid < 32) {
            float sum = 0.f;
            for (int rr = 0; rr < 64; ++rr) sum += bred[rr * 32 + tid];
            g.slab[(long)gridDim.x * (9 * 128 * 32) + blockIdx.x * 32 + tid] = tid < e.N ? sum : 0.f;
        }
    }
    // A BatchNorm backward link rides at the end of the launch (the dense layers' norm2 link: this kernel reads neither its inputs nor its
    // outputs, the fused 1x1 backward behind it needs them): one wave per channel, exactly k_bn_bwd_link's arithmetic.  The channels go to
    // the workgroups from the END of the grid: the tile split gives the first ntiles % nb workgroups one tile more, so the last ones reach
    // this point a tile time before the others -- unless ntiles % nb == 0, when nobody has slack and the link lengthens the launch by its
    // own latency (measured: +1.3 us per launch on average, profiles/helper_launches.md).  A grid of 1..15 workgroups loops over the channels.
    // Its arguments are read HERE, from the kernel's argument segment behind an opaque copy of its address (WGRAD_ARGS_KERNARG_OFFSET: the
    // position of ConvWgradArgs among the kernel's arguments, checked below the kernel).  Read as g.link, the compiler loads the link's
    // twelve values at the top of the kernel and holds them through the tile loops: cross-compiled, 39 spilled SGPRs and 204 lane reads
    // in the kernel's code, against 21 and 64 without the link; read here, 14 and 21 (VGPRs 209 -> 211, no scratch, occupancy 2 in all three).
    {
        typedef const char __attribute__((address_space(4)))* kernarg_ptr;
        kernarg_ptr ka = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        BnBwdLinkArgs link;
        __builtin_memcpy(&link, ka + WGRAD_ARGS_KERNARG_OFFSET + offsetof(ConvWgradArgs, link), sizeof(link));
        if (link.part != nullptr) bn_bwd_link_body(link, gridDim.x - 1 - blockIdx.x, gridDim.x);
    }
}

static_assert(std::is_same<first_arg<decltype(&k_conv3x3_wgrad_bf16)>::type, ConvWgradArgs>::value && WGRAD_ARGS_KERNARG_OFFSET == 0,
              "the link rider of k_conv3x3_wgrad_bf16 reads ConvWgradArgs at WGRAD_ARGS_KERNARG_OFFSET of the argument segment");

// ring + two eff tiles + table; the ring must hold a tile's rows and the 128 rows being fetched for the next one
constexpr size_t wgrad_smem(const PadGeom& q) { const size_t r4 = (q.rows() + 3) & ~3; return r4 + TP + 8 <= 512 ? size_t(WG_RING_BYTES) + 2 * TP * 64 + 1024 * 4 + 3 * 128 * 4 : size_t(1) << 30; }

}  // namespace

bool conv3x3_act_fusable(const ConvFwdArgs& a) {
    static const bool off = TCVN_KNOB_SET("TCVN_NO_ACT_FUSE");      // validation build: keep the materialised activation (A/B and variant tests)
    // forward: only the pair kernel activates in LDS; backward: this file's kernel (same geometry conditions as conv3x3_wgrad_tile_ok)
    return !off && a.sc != nullptr && a.sh != nullptr && a.sl != nullptr && conv3x3_fwd_kernel(a) == CONV3X3_FWD_PAIR &&
           wgrad_smem(geom_of(a.M, a.H, a.W)) <= 160 * 1024;
}

bool conv3x3_wgrad_tile_ok(const ConvWgradArgs& a) {
    const ConvFwdArgs& fa = a.fa;
    if (!conv3x3_tile_enabled() || a.mode != MODE_BF16 || fa.amode != A_3X3 || fa.C != 128 || a.e.N > 32) return false;
    if (fa.Aact == nullptr || fa.zeros == nullptr || (a.e.ldg & 7) || (a.e.ldx & 7) || (a.e.c_off & 1)) return false;
    if (fa.M % (fa.H * fa.W) != 0) return false;
    const PadGeom q = geom_of(fa.M, fa.H, fa.W);
    return q.gtot < (1L << 24) && wgrad_smem(q) <= 160 * 1024 && (long)fa.M * a.e.N < (1L << 32);
}

int conv3x3_wgrad_tile(const ConvWgradArgs& a, hipStream_t st) {
    const PadGeom q = geom_of(a.fa.M, a.fa.H, a.fa.W);
    const int n_img = a.fa.M / (a.fa.H * a.fa.W), ntiles = (int)q.tiles(), nb = tile_grid(ntiles);
    static bool attr = false;
    int rc;
    if ((rc = allow_lds(reinterpret_cast<const void*>(k_conv3x3_wgrad_bf16), 160 * 1024, attr))) return rc;
    if (a.slab == nullptr || (long)nb * (9 * 128 * 32 + 32) * 4 > a.slab_bytes || a.dbias == nullptr) return -3;
    {
        ProfScope ps("k_conv3x3_wgrad_bf16", 2.0 * a.fa.M * (double)a.e.N * a.fa.K, (double)a.fa.M * 2.0 * (a.fa.C + 2 * a.e.N), st);   // YA + (G, x) slices
        hipLaunchKernelGGL(k_conv3x3_wgrad_bf16, dim3(nb), dim3(512), wgrad_smem(q), st, a, n_img, ntiles);
        TCVN_LAUNCH_CHECK();
    }
    // weight partials [nb][9*128*32] -> dWk and bias partials [nb][32] -> dbias[0:N) (32-wide rows, zero beyond N): one launch
    const SlabJob jw = slab_job(a.slab, nb, 9 * 128 * 32, a.dWk, 0), jb = slab_job(a.slab + (long)nb * (9 * 128 * 32), nb, a.e.N, a.dbias, 32);
    if (a.deferred != nullptr) { a.deferred[0] = jw; a.deferred[1] = jb; return 0; }
    return slab_reduce2(jw, jb, st);
}

}  // namespace tcvn

#ifdef TCVN_DEBUG_KNOBS
extern "C" void tcvn_debug_wgrad_phases(unsigned long long* out16, int reset) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(tcvn::g_wg_ph), 16 * 8);
    if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(tcvn::g_wg_ph), z, 16 * 8); }
}
#endif
