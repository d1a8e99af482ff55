// bf16 3x3 convolution on padded LDS tiles (see tile3x3.h), forward.  The weight gradient is conv3x3_wgrad_tile.hip, the data gradient
// conv3x3_dgrad_tile.hip.
// Reference call site: Bottleneck.output_block (transformercvn/network/layers/dense_net.py:29-40).
//
// One workgroup = 128 padded output positions x 32 output channels; the BatchNorm+PReLU-transformed bf16 input
// image (128 + 2*(W+3) rows x 128 channels) is staged ONCE in LDS, then 9 taps x 8 k-steps of v_mfma_f32_32x32x16_bf16
// read it with row offsets (ds_read_b128, XOR-swizzled, conflict free); weights stream from L2 in fragment order.
// Algorithmic work per launch: 2 * pixels * 32 * 1152 FLOP; HBM: read 128 ch + write 32 ch per pixel.
#include <cstddef>
#include <cstdlib>
#include <type_traits>
#include "tile3x3.h"
#include "prof.h"
#include "bn_link.h"

namespace tcvn {

using namespace t3;

namespace {

// The strip kernel: validation build only (TCVN_FWD_STRIP), an independent second implementation that the variant tests compare with the
// pair kernel.  No map that conv3x3_tile_ok admits needs it (see the static_asserts at conv3x3_fwd_kernel), and at 512 VGPRs + 244 B of
// scratch it is not one to ship.
#ifdef TCVN_DEBUG_KNOBS
// LDS-DMA one padded image (rows [g_first, g_first + nrows4)) of a pre-activated [pixels,128] bf16 tensor into `buf`:
// every wave-instruction writes 1 KiB = 4 image rows, lane -> (row = lane>>4, slot = lane&15); the XOR swizzle is applied
// on the SOURCE chunk (slot s of row r holds channel chunk s ^ (r & 15)), padding rows come from a page of zeros.
__device__ __forceinline__ void dma_image(char* smem_base, int buf_off, const bf16* __restrict__ XA, const char* __restrict__ zeros,
                                          const int* rowpix, int nrows4, int wave, int lane) {
    const int rsub = lane >> 4, slot = lane & 15;
    // all table entries first, then all DMA instructions: one table read per DMA was an exposed LDS round trip each (4 500 of the weight
    // gradient's 17 400 cycles per wave and tile in the phase counters).  Up to DMA_RG row groups per wave = 384 image rows.
    constexpr int DMA_RG = 24;
    int mrow[DMA_RG];
#pragma unroll
    for (int i = 0; i < DMA_RG; ++i) {
        const int rg = wave + 4 * i;
        mrow[i] = rg * 4 < nrows4 ? rowpix[rg * 4 + rsub] : -1;
    }
#pragma unroll
    for (int i = 0; i < DMA_RG; ++i) {
        const int rg = wave + 4 * i, r = rg * 4 + rsub;
        if (rg * 4 < nrows4) {
            const int m = mrow[i];                     // pixel index of this image row or -1 (table filled a tile ahead)
            const char* src = m >= 0 ? reinterpret_cast<const char*>(XA + (long)m * 128) + ((slot ^ (r & 15)) << 4)
                                     : zeros + (slot << 4);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(smem_base + buf_off + rg * 1024), 16, 0, 0);
        }
    }
}

// One workgroup per CU (persistent): weights live in registers for the whole launch (72 fragments = 288 VGPRs), two LDS
// images double-buffer the LDS-DMA of tile t+1 under the 72 MFMAs + epilogue of tile t.
__global__ __launch_bounds__(256, 1) void k_conv3x3_fwd_bf16(const ConvFwdArgs g, int n_img, int ntiles, int swz) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PadGeom q(n_img, g.H, g.W);
    const int nrows4 = (q.rows() + 3) & ~3;
    const int img_bytes = nrows4 * 256;      // images at byte offsets 0 and img_bytes (kept as offsets: LDS address space)
    int* tbl = reinterpret_cast<int*>(smem + 2 * nrows4 * 256);               // [3][nrows4] pixel index per image row
    double* red = reinterpret_cast<double*>(smem + 2 * nrows4 * 256 + 3 * nrows4 * 4);   // [4][32][2]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const float invWp = 1.0f / q.Wp, invHp = 1.0f / q.Hp;
    const bf16* __restrict__ YA = reinterpret_cast<const bf16*>(g.Aact);
    const char* __restrict__ zeros = reinterpret_cast<const char*>(g.zeros);
    const bf16* __restrict__ Wf = reinterpret_cast<const bf16*>(g.Wfrag) + lane * 8;   // fragment order: 1 KiB per wave load
    bf16* __restrict__ Out = reinterpret_cast<bf16*>(g.Out);
    const int nb = gridDim.x;
    const int lb = swz ? (blockIdx.x & 7) * (nb >> 3) + (blockIdx.x >> 3) : blockIdx.x;   // neighbours share an XCD's L2
    const bool nok = r < g.N;
    const float bias = nok ? g.bias[r] : 0.f;
    const bool drop = g.drop_p > 0.f;
    const uint32_t dkey = drop_key(g.seed, g.stream_id);

    bf16x8_t bw[72];
#pragma unroll
    for (int i = 0; i < 72; ++i) bw[i] = *reinterpret_cast<const bf16x8_t*>(Wf + i * 512);

    double s1 = 0, s2 = 0;
    auto fill_tbl = [&](int slot, int tile) {
        for (int rr = tid; rr < nrows4; rr += 256) tbl[slot * nrows4 + rr] = pix_of(q, tile * TP - q.halo + rr, invWp, invHp);
    };
    if (lb < ntiles) fill_tbl(0, lb);
    if (lb + nb < ntiles) fill_tbl(1, lb + nb);
    __syncthreads();
    if (lb < ntiles) dma_image(smem, 0, YA, zeros, tbl, nrows4, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0, ts = 0;                                         // image buffer / table slot of the current tile
    for (int t = lb; t < ntiles; t += nb, cur ^= 1, ts = ts == 2 ? 0 : ts + 1) {
        const int tn = ts == 2 ? 0 : ts + 1, tnn = tn == 2 ? 0 : tn + 1;
        if (t + nb < ntiles)                     // prefetch the next tile's image under this tile's MFMAs
            dma_image(smem, (cur ^ 1) * img_bytes, YA, zeros, tbl + tn * nrows4, nrows4, wave, lane);
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        asm volatile("s_nop 4" : "+a"(acc));          // accvgpr writes -> first MFMA (inside asm) needs its wait states
        const int lrow0 = wave * 32 + r + q.halo;
        const int image = cur * img_bytes;
        // A fragments of tap+1 are read from LDS while the 8 MFMAs of tap run; weights are consumed straight from AGPRs
        bf16x8_t af[2][8];
        {
            const int lr = lrow0 - q.Wp - 1;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks)
                af[0][ks] = *reinterpret_cast<const bf16x8_t*>(smem + image + lr * 256 + (((2 * ks + h) ^ (lr & 15)) << 4));
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap + 1 < 9) {
                const int lr = lrow0 + ((tap + 1) / 3 - 1) * q.Wp + ((tap + 1) % 3 - 1);
#pragma unroll
                for (int ks = 0; ks < 8; ++ks)
                    af[(tap + 1) & 1][ks] =
                        *reinterpret_cast<const bf16x8_t*>(smem + image + lr * 256 + (((2 * ks + h) ^ (lr & 15)) << 4));
            }
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                // taps 0-6 keep their weights in AGPRs (16 acc + 224), taps 7-8 in arch VGPRs.  hipcc's hazard recognizer does
                // not see inside asm: the leading s_nop 1 covers (a) the two wait states gfx950 needs between a VALU write of an
                // operand register (the allocator's v_accvgpr_read/v_mov copies land right in front of a statement) and the MFMA
                // reading it, and (b) the wait state between back-to-back MFMAs chained through the accumulator.  Without it a
                // wave occasionally (~1e-4 of tiles) computed a whole tile with one stale operand dword.  The nops are free:
                // they sit in the shadow of the previous MFMA's 8 passes.
                if (tap < 7) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(af[tap & 1][ks]), "a"(bw[tap * 8 + ks]));
                else asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(af[tap & 1][ks]), "v"(bw[tap * 8 + ks]));
            }
        }
        // the MFMAs sit inside asm statements: hipcc pads no hazard for them -- wait out the last MFMA's result latency
        asm volatile("s_nop 15\n\ts_nop 7" : "+a"(acc));
        // epilogue: bias, dropout (one Philox call per 4 consecutive pixels of a channel), store, statistics
        long cur_grp = -1;
        uint32_t bits = 0;
        const int* px = tbl + ts * nrows4 + q.halo;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int lp = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            const int m = px[lp];
            if (m >= 0 && nok) {
                float v = acc[e] + bias;
                if (drop) {
                    if ((m >> 1) != cur_grp) { cur_grp = m >> 1; bits = drop_bits(dkey, m, r, g.N); }
                    v *= drop_pick(bits, m, g.drop_p);
                }
                const bf16 o = f2bf(v);
                Out[(long)m * g.ldo + g.n_off + r] = o;
                const double x = (double)bf2f(o);
                s1 += x; s2 += x * x;
            }
        }
        if (t + 2 * nb < ntiles) fill_tbl(tnn, t + 2 * nb);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (g.part != nullptr) {
        double a = s1, b = s2;
        a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
        if (lane < 32) { red[(wave * 32 + lane) * 2] = a; red[(wave * 32 + lane) * 2 + 1] = b; }
        __syncthreads();
        if (tid < g.N) {
            double x = 0, y = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { x += red[(w * 32 + tid) * 2]; y += red[(w * 32 + tid) * 2 + 1]; }
            g.part[((long)blockIdx.x * g.N + tid) * 2] = x;
            g.part[((long)blockIdx.x * g.N + tid) * 2 + 1] = y;
        }
    }
}
#endif

// Pair kernel: a workgroup walks CONSECUTIVE tiles, so tile t+1's image shares its first rows() - 128 rows with tile t's: the LDS image is
// a ring (padded position g -> row (g - g_org) mod ring, g_org = first row of the workgroup's first tile) and per tile only the 128 new
// rows are fetched (32 KB instead of 128 + 2*(W+3) rows = 70 KB at W = 69; measured on the strip kernel: the LDS-DMA fill alone cost 173
// of the 335 us of a block-1 launch).  512 threads = two waves per SIMD.  The timing ablation of its one-wave-per-SIMD predecessor (the
// ring kernel, since removed: block 1, 277 us = 76 fixed + 47 DMA issue + 86 MFMA + 68 epilogue, nothing overlapping) says a single
// wave per SIMD serialises its phases; here the
// two waves of a SIMD split the NINE TAPS of the same 32 positions -- wave w (role A) owns taps 0-4 (40 weight fragments = 160 registers),
// wave w+4 (role B) taps 5-8 (32 fragments) -- which is what fits the 256 registers a wave has at two waves per SIMD, and they run
// skewed by half a tile: after the tile barrier, B first finishes tile t-1 (adds A's partial sums, exchanged through LDS, applies bias /
// dropout, stores, statistics) while A already multiplies tile t; then B multiplies its taps of tile t.  A also fills the pixel table.
// The matrix pipe of the SIMD sees the same 72 MFMAs per tile, but the epilogue, the table arithmetic, the LDS waits and the DMA issue of
// one wave now sit under the other wave's MFMAs.  Ring rows are sized from the map width (rows() + 128, multiple of 16) so that the LDS
// also holds the two exchange buffers: 100 KB + 32 KB at W = 69.
// phase counters of the pair kernel (validation build only): wave-cycles per phase, reported by every 16th workgroup
#ifdef TCVN_DEBUG_KNOBS
__device__ unsigned long long g_pair_ph[16];
#endif
constexpr int PAIR_TBL = 1024;       // table entries (power of two > 512 + halo: an entry lives two tiles longer than its image row)
__global__ __launch_bounds__(512, 2) void k_conv3x3_fwd_pair_bf16(const ConvFwdArgs g, int n_img, int ntiles, int ring) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PadGeom q(n_img, g.H, g.W);
    const int nrows4 = (q.rows() + 3) & ~3;
    int* tbl = reinterpret_cast<int*>(smem + ring * 256);                             // [1024] pixel index of row (row-space index & 1023): an entry
                                                                                      // outlives its image row (the deferred epilogue reads it a tile later)
    float* xchg = reinterpret_cast<float*>(smem + ring * 256 + PAIR_TBL * 4);         // [2][4 pairs][16][64] role A's partial sums
    bf16* ctile = reinterpret_cast<bf16*>(xchg + 2 * 4 * 16 * 64);                    // [4 pairs][32][32] bf16 output tiles of the epilogue
    double* red = reinterpret_cast<double*>(ctile + 4 * 32 * 32);                     // [4][32][2]
    float* xtab = reinterpret_cast<float*>(red + 4 * 32 * 2);                         // act_fused: [3][128] scale, shift, slope of the input BatchNorm + PReLU

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool roleB = wave >= 4;
    const bool xf = g.act_fused != 0;
    const int pw = wave & 3;                                                          // pair index = 32-position block of the tile
    const int r = lane & 31, h = lane >> 5;
    const float invWp = 1.0f / q.Wp, invHp = 1.0f / q.Hp;
    const bf16* __restrict__ YA = reinterpret_cast<const bf16*>(g.Aact);
    const char* __restrict__ zeros = reinterpret_cast<const char*>(g.zeros);
    bf16* __restrict__ Out = reinterpret_cast<bf16*>(g.Out);
    int t0, t1;
    const int g_org = tile_span(q, ntiles, t0, t1);
    const bool nok = r < g.N;
    const float bias = nok ? g.bias[r] : 0.f;
    const bool drop = g.drop_p > 0.f;
    const uint32_t dkey = drop_key(g.seed, g.stream_id);
    // all 32 channels present and the output slice 16-B aligned: the tile leaves in 16-B stores through LDS
    const bool vec_store = g.N == 32 && (g.n_off & 7) == 0 && (g.ldo & 7) == 0 && (reinterpret_cast<uintptr_t>(g.Out) & 15) == 0;
    auto wrap = [&](int x) { return x >= ring ? x - ring : x; };                      // x in [0, 2 * ring)

    // weight fragment (tap, ks) sits at ((tap*8 + ks)*64 + lane)*8; role A keeps taps 0..4 in registers, role B taps 5..8
    const bf16* __restrict__ Wf = reinterpret_cast<const bf16*>(g.Wfrag) + lane * 8;

    // rows [row0, row0 + n) of this workgroup's row space (row 0 = g_org); image row -> ring slot (row mod ring), table entry row & 1023
    auto fill_rows = [&](int row0, int n, int t, int nt) {                            // by threads [t, t + nt)
        ring_tbl_fill<PAIR_TBL>(tbl, q, g_org, row0, n, t, nt, invWp, invHp);
    };
    auto dma_rows = [&](int row0, int slot0, int n, int w0, int nw) {                 // n multiple of 4; 4 rows (1 KiB) per wave instruction, issued by
        const int rsub = lane >> 4, slot = lane & 15;                                 // wave w0 of nw
        // four instructions per trip with their table reads batched in front (one dependent LDS read per instruction: 1 200 cycles per
        // wave and tile in the phase counters, 750-900 batched)
        for (int rg0 = w0; rg0 * 4 < n; rg0 += 4 * nw) {
            int m4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) m4[j] = tbl[(row0 + (rg0 + nw * j) * 4 + rsub) & (PAIR_TBL - 1)];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rg = rg0 + nw * j;
                if (rg * 4 < n) {
                    const int ring_row = wrap(slot0 + rg * 4);                        // slot0, ring multiples of 4: a group never wraps
                    const int rr = ring_row + rsub;
                    const char* src = m4[j] >= 0 ? reinterpret_cast<const char*>(YA + (long)m4[j] * 128) + ((slot ^ (rr & 15)) << 4) : zeros + (slot << 4);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(smem + ring_row * 256), 16, 0, 0);
                }
            }
        }
    };
    // act_fused: the rows arrive RAW; the wave that requested a row group activates it in place once its own DMAs have landed (vmcnt(0) at the
    // top of the tile loop) and before the tile barrier that publishes the rows -- same (w0, nw) assignment as dma_rows.  The rows of the NEXT
    // tile are disjoint from every row the current tile's taps read, so no other wave touches them meanwhile.  A lane keeps one logical
    // 8-channel chunk (cc) for all rows: its 24 table values are read from LDS once per call.
    auto xform_rows = [&](int row0, int slot0, int n, int w0, int nw) {
        const int rsub = lane >> 4, cc = lane & 15;
        for (int rg0 = w0; rg0 * 4 < n; rg0 += 4 * nw) {
            int m4[4];
            u16x8 v[4];
            char* p[4];
            // every LDS read of the trip -- table entries, image chunks, the 24 table values -- is requested before the first use
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rg = rg0 + nw * j;
                const bool in = rg * 4 < n;
                m4[j] = tbl[(row0 + (in ? rg * 4 : 0) + rsub) & (PAIR_TBL - 1)];
                if (!in) m4[j] = -1;
                const int rr = wrap(slot0 + (in ? rg * 4 : 0)) + rsub;
                p[j] = smem + rr * 256 + ((cc ^ (rr & 15)) << 4);
                v[j] = *reinterpret_cast<const u16x8*>(p[j]);
            }
            const Act8 tb = act8_load(xtab, cc);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (m4[j] >= 0) *reinterpret_cast<u16x8*>(p[j]) = act8_apply(v[j], tb);      // padding rows stay the zeros the DMA wrote
        }
    };
    if (t0 < t1) fill_rows(0, nrows4, tid, 512);
    if (t0 + 1 < t1) fill_rows(nrows4, TP, tid, 512);
    if (xf && g.lf.isum != nullptr) {                                                  // link-free (round 5): norm2's table from the 1x1 kernel's sums (bn_lf.h)
        if (tid < 128) {
            float tsc, tsh;
            lf_table(g.lf, tid, blockIdx.x == 0, tsc, tsh);
            xtab[tid] = tsc; xtab[128 + tid] = tsh; xtab[256 + tid] = g.sl[tid];
        }
    } else if (xf) act_tab_fill(xtab, g.sc, g.sh, g.sl, tid, 512);
    __syncthreads();
    if (t0 < t1) dma_rows(0, 0, nrows4, wave, 8);

#ifdef TCVN_DEBUG_KNOBS
    unsigned long long ph[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    double s1 = 0, s2 = 0;
    f32x16 accp;                                                                      // role B: its partial sums of the previous tile
#pragma unroll
    for (int e = 0; e < 16; ++e) accp[e] = 0.f;
    int slot_tile = 0;                                                                // ring slot of the current tile's first image row
    int slot_new = wrap(nrows4);                                                      // ring slot of the NEXT tile's first new row
    // role B's deferred epilogue of tile `te`: partial sums of both waves, bias, dropout, store, statistics.  Branch-free: the first
    // version tested `m >= 0`, the dropout group and the store path per element -- ~100 taken branches per tile, 5 460 cycles per wave and
    // tile in the phase counters (4 000 now) -- so everything is computed for all 16 elements and selected.  With all 32 channels present the
    // tile leaves through a bf16 tile in LDS as 16-B stores (two per lane instead of sixteen 2-byte scattered stores).
    auto epilogue_impl = [&](auto dropc, auto vecc, int te, const f32x16& mine) {
        constexpr bool DROP = decltype(dropc)::value, VEC = decltype(vecc)::value;
        const float* xc = xchg + (((te - t0) & 1) * 4 + pw) * 16 * 64 + lane;
        float part[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) part[e] = xc[e * 64];
        int mrow[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) mrow[e] = tbl[((te - t0) * TP + q.halo + pw * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) & (PAIR_TBL - 1)];
        float f1 = 0.f, f2 = 0.f;
        bf16* ct = ctile + pw * 32 * 32;                                              // this pair's [32 positions][32 channels] bf16 tile (wave private)
        uint32_t kword = 0;                                                           // lane L < 32: keep flags of position pos(e = L >> 1, h = L & 1)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = mrow[e];
            const bool ok = m >= 0 && nok;
            float v = mine[e] + part[e] + bias;
            if (DROP) {
                const int mm = m < 0 ? 0 : m;
                const float dsc = drop_pick(drop_bits32(dkey, mm, r, g.N), mm, g.drop_p);   // (the launcher checks pixels * N < 2^32)
                v *= dsc;
                // the 32 channels of a position sit in the 32 lanes of a wave half: one ballot = the keep words of two positions
                const unsigned long long bal = __ballot(dsc != 0.f);
                kword = lane == 2 * e ? (uint32_t)bal : lane == 2 * e + 1 ? (uint32_t)(bal >> 32) : kword;
            }
            const bf16 o = ok ? f2bf(v) : (bf16)0;
            const float x = bf2f(o);                                                  // 0 for padding positions / absent channels
            f1 += x; f2 = fmaf(x, x, f2);
            if (VEC) ct[((e & 3) + 8 * (e >> 2) + 4 * h) * 32 + r] = o;
            else if (ok) Out[(long)m * g.ldo + g.n_off + r] = o;
        }
        s1 += (double)f1; s2 += (double)f2;
        if (DROP && g.keep_out != nullptr && lane < 32) {                                 // the backward kernels test these bits instead of hashing
            const int el = lane >> 1, pos = (el & 3) + 8 * (el >> 2) + 4 * (lane & 1);
            const int m = tbl[((te - t0) * TP + q.halo + pw * 32 + pos) & (PAIR_TBL - 1)];
            if (m >= 0) g.keep_out[m] = kword;
        }
        if (VEC) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {                                             // 32 positions x 64 B = 128 chunks of 16 B, two per lane
                const int c = lane + 64 * i, pos = c >> 2, chunk = c & 3;
                const int m = tbl[((te - t0) * TP + q.halo + pw * 32 + pos) & (PAIR_TBL - 1)];
                const u16x8 v8 = *reinterpret_cast<const u16x8*>(ct + pos * 32 + chunk * 8);
                if (m >= 0) *reinterpret_cast<u16x8*>(Out + (long)m * g.ldo + g.n_off + chunk * 8) = v8;
            }
        }
    };
    auto epilogue = [&](int te, const f32x16& mine) {                                  // uniform dispatch, once per tile
        if (drop) {
            if (vec_store) epilogue_impl(std::true_type{}, std::true_type{}, te, mine);
            else epilogue_impl(std::true_type{}, std::false_type{}, te, mine);
        } else {
            if (vec_store) epilogue_impl(std::false_type{}, std::true_type{}, te, mine);
            else epilogue_impl(std::false_type{}, std::false_type{}, te, mine);
        }
    };

    // one multiply pass: NT taps starting at tap `tap_first` over the 32 positions of this pair, image of the tile in ring slot `slot_t`.
    // The A fragments travel LDS -> registers four k-steps (half a tap) ahead of the MFMAs that consume them (two register groups of four
    // fragments); the lgkmcnt wait is placed by hand BEFORE the next group's reads are issued -- hipcc would sink the reads next to their
    // uses or put the wait behind the new reads.  (Two accumulator chains with two-fragment groups measured slower: 212 vs 197 us.)
    auto multiply = [&](auto& bwr, auto ntc, int tap_first, int slot_t, f32x16& acc) {
        constexpr int NT = decltype(ntc)::value, NG = NT * 2;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        const int lrow0 = slot_t + pw * 32 + r + q.halo;                               // < 2 * ring; tap shifts add at most Wp + 1 < ring more
        auto row_of = [&](int tp) {
            const int tap = tap_first + tp;
            int lr = lrow0 + (tap / 3 - 1) * q.Wp + (tap % 3 - 1);
            lr = lr >= ring ? lr - ring : lr;
            return lr >= ring ? lr - ring : lr;
        };
        bf16x8_t af[2][4];
        auto load_group = [&](int gI, bf16x8_t (&dst)[4]) {
            const int lr = row_of(gI >> 1), ks0 = (gI & 1) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                dst[i] = *reinterpret_cast<const bf16x8_t*>(smem + lr * 256 + (((2 * (ks0 + i) + h) ^ (lr & 15)) << 4));
        };
        load_group(0, af[0]);
#pragma unroll
        for (int gI = 0; gI < NG; ++gI) {
            __builtin_amdgcn_s_waitcnt(0xC07F);         // lgkmcnt(0): this group's fragments (read four MFMAs ago) are in
            __builtin_amdgcn_sched_barrier(0);
            if (gI + 1 < NG) load_group(gI + 1, af[(gI + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[gI & 1][i], bwr[gI * 4 + i], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // The two roles run the same barrier sequence (one __syncthreads per tile + one after the loop) on their own register sets.
    if (!roleB) {
        bf16x8_t bw[40];
#pragma unroll
        for (int i = 0; i < 40; ++i) bw[i] = *reinterpret_cast<const bf16x8_t*>(Wf + i * 512);
        TILE_PH_T0();
        int slot_dma = 0;                                                             // ring slot of the rows requested during the previous tile
        for (int t = t0; t < t1; ++t) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                          // this wave's share of tile t's rows has landed
            if (xf) {
                if (t == t0) xform_rows(0, 0, nrows4, wave, 8);
                else xform_rows(nrows4 + (t - 1 - t0) * TP, slot_dma, TP, wave, 8);
            }
            TILE_PH(0);
            __syncthreads();                                                          // ... everybody's; tile t-1's MFMAs are done; xchg / tbl of the last phase visible
            TILE_PH(1);
            slot_dma = slot_new;
            // the next tile's 128 new rows travel under this tile's work.  Materialised input: issued by role A alone, so that role B's stores do
            // not queue behind loads.  act_fused: every wave requests a sixteenth and activates exactly the rows it requested (both roles share
            // the in-LDS activation: role A alone carried +28 % on the launch, 2.17 -> 2.77 ms per step)
            if (t + 1 < t1) { if (xf) dma_rows(nrows4 + (t - t0) * TP, slot_new, TP, wave, 8); else dma_rows(nrows4 + (t - t0) * TP, slot_new, TP, pw, 4); }
            TILE_PH(2);
            f32x16 acc;
            multiply(bw, std::integral_constant<int, 5>{}, 0, slot_tile, acc);
            float* xc = xchg + (((t - t0) & 1) * 4 + pw) * 16 * 64 + lane;
#pragma unroll
            for (int e = 0; e < 16; ++e) xc[e * 64] = acc[e];
            TILE_PH(3);
            // table of the rows the NEXT iteration will fetch (tile t + 2's new rows), by the 256 role-A threads
            if (t + 2 < t1) fill_rows(nrows4 + (t - t0 + 1) * TP, TP, tid, 256);
            TILE_PH(4);
            slot_tile = wrap(slot_tile + TP);
            slot_new = wrap(slot_new + TP);
        }
    } else {
        bf16x8_t bw[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) bw[i] = *reinterpret_cast<const bf16x8_t*>(Wf + (40 + i) * 512);
        __builtin_amdgcn_s_setprio(1);     // the second-dispatched half loses every issue arbitration otherwise
        TILE_PH_T0();
        int slot_dma = 0;
        for (int t = t0; t < t1; ++t) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                          // DMA share landed, stores of the last epilogue left
            if (xf) {                                                                  // this wave's share of the tile's new rows (see role A)
                if (t == t0) xform_rows(0, 0, nrows4, wave, 8);
                else xform_rows(nrows4 + (t - 1 - t0) * TP, slot_dma, TP, wave, 8);
            }
            TILE_PH(8);
            __syncthreads();
            TILE_PH(9);
            slot_dma = slot_new;
            if (xf && t + 1 < t1) dma_rows(nrows4 + (t - t0) * TP, slot_new, TP, wave, 8);
            TILE_PH(10);
            if (t > t0) epilogue(t - 1, accp);                                         // finish tile t-1 while role A multiplies tile t
            TILE_PH(11);
            multiply(bw, std::integral_constant<int, 4>{}, 5, slot_tile, accp);
            TILE_PH(12);
            slot_tile = wrap(slot_tile + TP);
            slot_new = wrap(slot_new + TP);
        }
    }
#ifdef TCVN_DEBUG_KNOBS
    if (lane == 0 && (blockIdx.x & 15) == 0)                  // every 16th workgroup reports (the atomics of all of them cost ~70 us per launch)
        for (int i = 0; i < 16; ++i)
            if (ph[i]) atomicAdd(&g_pair_ph[i], ph[i]);
#endif
    __syncthreads();                                                                  // the last tile's exchange buffer is complete
    if (roleB && t1 > t0) epilogue(t1 - 1, accp);
    if (g.part != nullptr || g.isum_out != nullptr) {
        double a = s1, b = s2;
        a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
        if (roleB && lane < 32) { red[(pw * 32 + lane) * 2] = a; red[(pw * 32 + lane) * 2 + 1] = b; }
        __syncthreads();
        if (tid < g.N) {
            double x = 0, y = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { x += red[(w * 32 + tid) * 2]; y += red[(w * 32 + tid) * 2 + 1]; }
            if (g.isum_out != nullptr) lf_add(g.isum_out, g.isum_stride, tid, x, y);                   // link-free: the next consumer derives its table itself
            else {
                g.part[((long)blockIdx.x * g.N + tid) * 2] = x;
                g.part[((long)blockIdx.x * g.N + tid) * 2 + 1] = y;
            }
        }
    }
}
constexpr int fwd_pair_ring(const PadGeom& q) { return (int)((((q.rows() + 3) & ~3) + TP + 15) & ~15); }
constexpr size_t fwd_pair_smem(const PadGeom& q) { const size_t ring = fwd_pair_ring(q); return ring * 256 + PAIR_TBL * 4 + 2 * 4 * 16 * 64 * 4 + 4 * 32 * 32 * 2 + 4 * 32 * 16 + 3 * 128 * 4; }
// LDS of the strip kernel (two whole images).  It also sets the widest map conv3x3_tile_ok admits, in every build.
constexpr size_t fwd_smem(const PadGeom& q) { const size_t r4 = (q.rows() + 3) & ~3; return 2 * r4 * 256 + 3 * r4 * 4 + 4 * 32 * 16; }

}  // namespace

bool conv3x3_tile_enabled() {
    static const bool off = TCVN_KNOB_SET("TCVN_DISABLE_TILE");      // validation switch: force the generic kernels
    return !off;
}

bool conv3x3_tile_ok(const ConvFwdArgs& a) {
    if (!conv3x3_tile_enabled()) return false;
    if (a.Wfrag == nullptr || (reinterpret_cast<uintptr_t>(a.Wfrag) & 15) || a.Aact == nullptr || a.zeros == nullptr) return false;
    if (a.mode != MODE_BF16 || a.amode != A_3X3 || a.C != 128 || a.lda != 128 || a.N > 32 || a.Kp != 1152) return false;
    if ((reinterpret_cast<uintptr_t>(a.A) & 15) || (reinterpret_cast<uintptr_t>(a.Wk) & 15)) return false;
    if (a.M % (a.H * a.W) != 0) return false;
    const PadGeom q = geom_of(a.M, a.H, a.W);
    return q.gtot < (1L << 24) && fwd_smem(q) <= 160 * 1024;
}
int conv3x3_tile_nblk(const ConvFwdArgs& a) { return tile_grid(geom_of(a.M, a.H, a.W).tiles()); }

// Every map conv3x3_tile_ok admits runs the pair kernel.  All the LDS formulas depend on the map width alone and grow with it, so the
// widest admitted width decides: the strip formula in conv3x3_tile_ok admits W <= TILE_MAX_W (kept as the bound although the pair
// kernel alone would fit wider maps: widening it changes which maps take the tile path), and at that width the pair kernel's LDS
// and its table condition hold.  Its third condition, pixels * N < 2^32 (drop_bits32), follows from gtot < 2^24 and N <= 32.
constexpr int TILE_MAX_W = 87;
static_assert(fwd_smem(PadGeom(1, 1, TILE_MAX_W)) <= 160 * 1024 && fwd_smem(PadGeom(1, 1, TILE_MAX_W + 1)) > 160 * 1024,
              "conv3x3_tile_ok admits exactly the maps up to TILE_MAX_W columns");
static_assert(fwd_pair_smem(PadGeom(1, 1, TILE_MAX_W)) <= 160 * 1024, "the pair kernel's LDS fits at the widest admitted map");
static_assert(4 * TP + PadGeom(1, 1, TILE_MAX_W).halo + PadGeom(1, 1, TILE_MAX_W).Wp + 1 < PAIR_TBL,
              "the pair kernel's table outlives its entries' last readers at the widest admitted map");

// The ONE place that chooses the forward kernel: the launcher switches on it, the DenseNet driver asks it what the launch will do
Conv3x3Fwd conv3x3_fwd_kernel(const ConvFwdArgs& a) {
    if (!conv3x3_tile_ok(a)) return CONV3X3_FWD_NONE;
#ifdef TCVN_DEBUG_KNOBS
    static const bool strip_forced = TCVN_KNOB_SET("TCVN_FWD_STRIP");      // validation build: the strip kernel where the pair kernel would run
    if (strip_forced) return CONV3X3_FWD_STRIP;
#endif
    return CONV3X3_FWD_PAIR;                        // two waves per SIMD, taps split
}
int conv3x3_fwd_tile(const ConvFwdArgs& a, hipStream_t st) {
    const PadGeom q = geom_of(a.M, a.H, a.W);
    const int n_img = a.M / (a.H * a.W), ntiles = (int)q.tiles(), nb = tile_grid(ntiles);
    const Conv3x3Fwd k = conv3x3_fwd_kernel(a);
    // only the pair kernel derives / adds link-free statistics (lf, isum_out) and activates in LDS (conv3x3_act_fusable)
    if (k == CONV3X3_FWD_NONE || (k != CONV3X3_FWD_PAIR && (a.lf.isum != nullptr || a.isum_out != nullptr || a.act_fused))) return -2;
    static bool attr_pair = false;
    ProfScope ps("k_conv3x3_fwd_bf16", 2.0 * a.M * (double)a.N * a.K, (double)a.M * 2.0 * (a.C + a.N), st);   // read 128 ch, write N ch
    int rc;
#ifdef TCVN_DEBUG_KNOBS
    static bool attr_strip = false;
    if (k == CONV3X3_FWD_STRIP) {
        if ((rc = allow_lds(reinterpret_cast<const void*>(k_conv3x3_fwd_bf16), 160 * 1024, attr_strip))) return rc;
        hipLaunchKernelGGL(k_conv3x3_fwd_bf16, dim3(nb), dim3(256), fwd_smem(q), st, a, n_img, ntiles, (nb >= 8 && nb % 8 == 0) ? 1 : 0);
        TCVN_LAUNCH_CHECK();
        return 0;
    }
#endif
    if ((rc = allow_lds(reinterpret_cast<const void*>(k_conv3x3_fwd_pair_bf16), 160 * 1024, attr_pair))) return rc;
    hipLaunchKernelGGL(k_conv3x3_fwd_pair_bf16, dim3(nb), dim3(512), fwd_pair_smem(q), st, a, n_img, ntiles, fwd_pair_ring(q));
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace tcvn

#ifdef TCVN_DEBUG_KNOBS
extern "C" void tcvn_debug_pair_phases(unsigned long long* out16, int reset) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(tcvn::g_pair_ph), 16 * 8);
    if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(tcvn::g_pair_ph), z, 16 * 8); }
}
#endif
