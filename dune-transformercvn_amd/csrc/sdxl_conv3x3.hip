// bf16 3x3 / stride 1 / pad 1 convolutions with 64 input and 64 output channels on full-resolution NHWC maps: the layers of the
// first two stages of the SDXL-style embedder (diffusers ResnetBlock2D conv1 / conv2 at 400x280 and 200x140; reference call
// site transformercvn/network/layers/sdxl_net.py:27-34, block definitions restated in oracle/sdxl_oracle.py), forward and data
// gradient.  These maps are 40 % of the embedder's FLOPs and, in the generic implicit-GEMM kernels, re-read every input pixel
// nine times from L2 with one dependent load per 32-wide K chunk.
//
// Here a 512-thread workgroup owns an 8 x 32 pixel tile of one map: its 10 x 34 pixel halo patch (64 channels, 128 B per pixel,
// 144-B pitch so that the 16-B fragment reads of 16 lanes fall on 16 different bank groups) is staged ONCE in LDS, double
// buffered -- the loads of the next tile are in flight under the MFMAs of this one.  A wave owns two tile rows (2 x 32
// positions) and 32 of the 64 output channels; its 36 weight fragments (9 taps x 4 chunks of 16 input channels,
// v_mfma_f32_32x32x16_bf16) stay in registers for the whole launch, the nine taps are plain offsets into the patch.  The tile
// leaves through an fp32 C tile in LDS (two passes of 128 positions), so bias / residual are added in fp32 before the one rounding
// to bf16 -- the same arithmetic as the generic kernel -- and every lane stores 16 contiguous bytes of an NHWC row.
//
// The data gradient of such a layer is the same convolution over the output gradient with the taps flipped and the channel
// roles exchanged: the kernel reads the transposed weight pack ([Cin][tap*Cout + n]) at tap 8 - t.
// Algorithmic HBM bytes per map pixel: 128 B read + 128 B written (+ 128 B residual); MFMA work 2 * 576 * 64 flop.
//
// The five kernels of this file are built from one copy each of: the tile walk (first_tile, tile_pos), the patch loader (patch_dma),
// the weight loaders (load_w36, ring_load) and the ring's tap loop (ring_taps), the tap step (tap_step) and the C-tile epilogue
// (acc_to_cs, cs_store8, tile8x32_out).  A kernel differs in its tile shape, its source-pixel callback and its output offsets.
#include "prof.h"
#include "sdxl_ops.h"
#include "tcvn_ops.h"

namespace tcvn {

namespace {

constexpr int TH = 8, TW = 32;                        // output tile
constexpr int PW = TW + 2, PH = TH + 2;               // halo patch
constexpr int PS = 144;                               // bytes per patch pixel (128 + 16)
constexpr int patch_dma_bytes(int ph, int pw) { return ((ph * pw + 6) / 7) * 7 * PS; }      // what patch_dma<ph, pw> writes: whole groups of 7 pixels
constexpr int PATCH_BYTES = patch_dma_bytes(PH, PW);  // 49 392
constexpr int CP = 68;                                // fp32 C tile pitch (floats)
constexpr int CT_BYTES = 128 * CP * 4;                // 34 816

// ---------------------------------------------------------------------------------------------------------------------
// Tile walk.  Workgroups of one XCD (blockIdx % 8) walk neighbouring tiles, so the halo pixels two tiles share are served by one L2:
// a workgroup starts at first_tile() and advances by gridDim.x.  Tiles are numbered x fastest, then y, then image (or image group).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int first_tile() {
    const int nb = gridDim.x;
    return (nb % 8 == 0) ? (blockIdx.x & 7) * (nb >> 3) + (blockIdx.x >> 3) : blockIdx.x;
}
struct TilePos { int tx, ty, img; };
__device__ __forceinline__ TilePos tile_pos(int t, int tiles_x, int tiles_y) {
    const int tx = t % tiles_x, r = t / tiles_x;
    return {tx, r % tiles_y, r / tiles_y};
}

// Tile -> pixel mapping of the 8 x 32 stride-1 tile.  Large maps: tiles_x x tiles_y tiles per image.  Small maps would waste most
// of a tile (a 7 x 5 map fills 14 % of it) and re-read the weights once per image, so maps of width <= 15 are PACKED side by side
// (px images per tile row, one zero column between neighbours -- the padding both of them need) and maps of height <= 3 are stacked
// (py per tile).  A tile then carries px * py images.
struct TileMap {
    int n, H, W, tiles_x, tiles_y, px, py;
    __host__ __device__ int ntiles() const { return ((n + px * py - 1) / (px * py)) * tiles_x * tiles_y; }
    // pixel of tile t at tile-relative (ry, rx), ry in [-1, 8], rx in [-1, 32]; false = zero padding / outside / no such image
    __device__ __forceinline__ bool pixel(int t, int ry, int rx, int& img, int& y, int& x) const {
        const TilePos p = tile_pos(t, tiles_x, tiles_y);           // p.img: the image group
        int sx = 0, sy = 0;
        if (px > 1) { if (rx < 0) return false; sx = rx / (W + 1); x = rx - sx * (W + 1); if (sx >= px) return false; }
        else x = p.tx * TW + rx;
        if (py > 1) { if (ry < 0) return false; sy = ry / (H + 1); y = ry - sy * (H + 1); if (sy >= py) return false; }
        else y = p.ty * TH + ry;
        img = p.img * (px * py) + sy * px + sx;
        return x >= 0 && x < W && y >= 0 && y < H && img < n;
    }
};

// GroupNorm statistics of a tile's STORED values (sum, sum of squares over pixels x channels of one image), fused into the producing
// convolution's epilogue: wave partials through two LDS float atomics, one pair of fp64 atomics per tile by thread 0 afterwards.
__device__ __forceinline__ void stats_wave_add(float s, float ss, float* lacc) {
    s = wave_sum(s); ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&lacc[0], s); atomicAdd(&lacc[1], ss); }
}
__device__ __forceinline__ void stats_flush(float* lacc, double* stats, int img) {      // thread 0, after a barrier behind the adds
    atomicAdd(stats + 2 * img, (double)lacc[0]); atomicAdd(stats + 2 * img + 1, (double)lacc[1]);
    lacc[0] = 0.f; lacc[1] = 0.f;
}

__device__ __attribute__((aligned(16))) unsigned int g_zero_line[4];       // 16 B of zeros: LDS-DMA source of padding

// ---------------------------------------------------------------------------------------------------------------------
// Patch loader.  A PH_ x PW_ pixel patch (64 channels, PS bytes per pixel) into `dst` by LDS-DMA (global_load_lds, 16 B per lane, no
// registers), by NWAVES waves.  One wave instruction writes 1 KiB of consecutive LDS, so it carries 7 pixels of 144 B -- lanes
// 9q .. 9q+7 the eight chunks of pixel q, lane 9q+8 the pad slot (fed from zeros), lane 63 switched off.  src_of(py, px) gives the
// first of the pixel's 64 channels, or null for a pixel that reads as zero (padding, outside the map): those read the zero line as
// well.  The last group may run past PH_ * PW_ pixels: `dst` holds patch_dma_bytes(PH_, PW_).
// ---------------------------------------------------------------------------------------------------------------------
template <int PH_, int PW_, int NWAVES, typename SrcOf>
__device__ __forceinline__ void patch_dma(char* dst, int wave, int lane, SrcOf src_of) {
    const int dq = lane / 9, dslot = lane - dq * 9;
    for (int j = wave; j * 7 < PH_ * PW_; j += NWAVES) {
        const int pix = j * 7 + dq;
        const int py = pix / PW_, px = pix - py * PW_;
        const bf16* p = (dslot < 8 && pix < PH_ * PW_) ? src_of(py, px) : nullptr;
        const bf16* src = p ? p + dslot * 8 : reinterpret_cast<const bf16*>(g_zero_line);
        if (lane < 63)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(dst + j * 7 * PS), 16, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weights.  B[k][j = n]: lane (n = l31, k half = lh) holds W[n][tap'*cin + chunk*64 + kc*16 + lh*8 .. +8]; `wrow` points at
// W[n][lh*8], tap' = 8 - tap for the data gradient on the transposed pack (flip).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ring_load(bf16x8_t (&slot)[4], const bf16* wrow, int cin, int flip, int chunk, int tap) {
    const bf16* p = wrow + (flip ? 8 - tap : tap) * cin + chunk * 64;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) slot[kc] = *reinterpret_cast<const bf16x8_t*>(p + kc * 16);
}
// all 36 fragments of a 64-channel input, for the whole launch
__device__ __forceinline__ void load_w36(bf16x8_t (&bw)[9][4], const bf16* wrow, int flip) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) ring_load(bw[tap], wrow, 64, flip, 0, tap);
}

// Tap step: the four 16-channel fragments of ROWS patch rows (ROW_BYTES apart, first one at `pt`) against one tap's weight fragments
template <int ROWS, int ROW_BYTES>
__device__ __forceinline__ void tap_step(f32x16 (&acc)[ROWS], const char* pt, const bf16x8_t (&w)[4]) {
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
        bf16x8_t a[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) a[r] = *reinterpret_cast<const bf16x8_t*>(pt + r * ROW_BYTES + kc * 32);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[r], w[kc], acc[r], 0, 0, 0);
    }
}

template <int ROWS>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[ROWS]) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;
}

// The nine taps of one 64-channel chunk with the weight fragments streaming from L2 one tap ahead of the MFMAs in a ring of five slots
// (tap t lives in slot t % 5; the loads of tap t+2 are issued under tap t; on entry taps 0 and 1 of `chunk` are in slots 0 and 1).
// vmcnt retires in order, so next_patch() -- the LDS-DMA of the next chunk's patch -- is called only after the last fragment loads of
// this chunk and the first two taps of the next chunk are in flight: nothing the MFMAs wait for is queued behind an HBM access.
// `pb`: the lane's patch address at tap (0, 0); PITCH: patch pixels per row.
template <int ROWS, int PITCH, typename NextPatch>
__device__ __forceinline__ void ring_taps(f32x16 (&acc)[ROWS], bf16x8_t (&bq)[5][4], const char* pb, const bf16* wrow, int cin, int flip,
                                          int chunk, int nchunk, bool more, NextPatch next_patch) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if (tap <= 6) ring_load(bq[(tap + 2) % 5], wrow, cin, flip, chunk, tap + 2);
        if (tap == 6 && more) ring_load(bq[0], wrow, cin, flip, nchunk, 0);
        if (tap == 7 && more) {
            ring_load(bq[1], wrow, cin, flip, nchunk, 1);
            next_patch();
        }
        tap_step<ROWS, PITCH * PS>(acc, pb + ((tap / 3) * PITCH + (tap % 3)) * PS, bq[tap % 5]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// C-tile epilogue.  acc_to_cs: a wave's 32 positions x 32 channels (+ bias) into rows [row0, row0 + 32) of the fp32 C tile, column
// `col` = the lane's channel.  cs_store8: a thread's 8 channels of position `pos` out of the C tile, + the bf16 operand at add[o ..]
// (residual or the gradient so far; null = none), ONE rounding to bf16, the rounded values summed into (ts, tss) when `sum`
// (the statistics are those of the STORED values), 16-B store to out[o ..].
// ---------------------------------------------------------------------------------------------------------------------
template <bool BIAS>
__device__ __forceinline__ void acc_to_cs(float* Cs, const f32x16& acc, int row0, int col, int lh, float bias) {
#pragma unroll
    for (int e = 0; e < 16; ++e) Cs[(row0 + (e & 3) + 8 * (e >> 2) + 4 * lh) * CP + col] = BIAS ? acc[e] + bias : acc[e];
}
__device__ __forceinline__ void cs_store8(const float* Cs, int pos, int ch, const bf16* add, bf16* out, long o, bool sum, float& ts, float& tss) {
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(Cs + pos * CP + ch * 8);
    const f32x4 c1 = *reinterpret_cast<const f32x4*>(Cs + pos * CP + ch * 8 + 4);
    float v[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
    if (add) {
        const u16x8 rv = *reinterpret_cast<const u16x8*>(add + o);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += bf2f(rv[j]);
    }
    u16x8 ov;
#pragma unroll
    for (int j = 0; j < 8; ++j) ov[j] = f2bf(v[j]);
    if (sum) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = bf2f(ov[j]); ts += f; tss += f * f; }
    }
    *reinterpret_cast<u16x8*>(out + o) = ov;
}

// Epilogue of the 8 x 32 tile (512 threads; wave = tile rows 2wp, 2wp+1 x channels [32wn, +32)): two passes of 128 positions (tile
// rows 0-3, 4-7) through the C tile.  out_of(ry, rx, o): whether tile position (ry, rx) is a pixel of the map, and the offset of
// this workgroup's first channel of it in Out / Res.  Ends with the wave partials of the statistics added to lacc.
template <typename OutOf>
__device__ __forceinline__ void tile8x32_out(float* Cs, const f32x16 (&acc)[2], float bias, const bf16* Res, bf16* Out, bool stats, float* lacc,
                                             OutOf out_of) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5, wp = wave >> 1, wn = wave & 1;
    float ts = 0.f, tss = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if ((wp >> 1) == pass) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) acc_to_cs<true>(Cs, acc[rt], ((wp & 1) * 2 + rt) * 32, 32 * wn + l31, lh, bias);
        }
        lds_barrier();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * 512, pos = idx >> 3, ch = idx & 7;     // 128 positions x 8 chunks
            long o;
            if (out_of(pass * 4 + (pos >> 5), pos & 31, o)) cs_store8(Cs, pos, ch, Res, Out, o + ch * 8, stats, ts, tss);
        }
        if (pass == 0) lds_barrier();
    }
    if (stats) stats_wave_add(ts, tss, lacc);
}

struct C64Args {
    const bf16* In; const bf16* W; const float* bias; const bf16* Res; bf16* Out; double* stats;
    int n, H, W_, flip;
    int tiles_x, tiles_y, ntiles;
};

__global__ __launch_bounds__(512, 1) void k_sconv3_c64(const C64Args g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* patch = smem;                                            // [2][PATCH_BYTES]
    float* Cs = reinterpret_cast<float*>(smem + 2 * PATCH_BYTES);  // [128][CP]
    float* lacc = reinterpret_cast<float*>(smem + 2 * PATCH_BYTES + CT_BYTES);     // [2] statistics of the tile
    if (threadIdx.x == 0) { lacc[0] = 0.f; lacc[1] = 0.f; }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wp = wave >> 1, wn = wave & 1;                       // tile rows 2wp, 2wp+1; output channels [32wn, +32)

    bf16x8_t bw[9][4];
    load_w36(bw, g.W + (long)(32 * wn + l31) * 576 + lh * 8, g.flip);
    const float bias = g.bias ? g.bias[32 * wn + l31] : 0.f;

    auto stage = [&](int t, int buf) {
        const TilePos p = tile_pos(t, g.tiles_x, g.tiles_y);
        const int y0 = p.ty * TH - 1, x0 = p.tx * TW - 1;
        patch_dma<PH, PW, 8>(patch + buf * PATCH_BYTES, wave, lane, [&](int py, int px) -> const bf16* {
            const int y = y0 + py, x = x0 + px;
            return (y >= 0 && y < g.H && x >= 0 && x < g.W_) ? g.In + (((long)p.img * g.H + y) * g.W_ + x) * 64 : nullptr;
        });
    };

    const int nb = gridDim.x;
    int t = first_tile(), buf = 0;
    if (t < g.ntiles) stage(t, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (; t < g.ntiles; t += nb, buf ^= 1) {
        if (t + nb < g.ntiles) stage(t + nb, buf ^ 1);
        f32x16 acc[2];
        zero_acc(acc);
        const char* pb = patch + buf * PATCH_BYTES + ((2 * wp) * PW + l31) * PS + lh * 16;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) tap_step<2, PW * PS>(acc, pb + ((tap / 3) * PW + (tap % 3)) * PS, bw[tap]);
        // the next patch was requested before the MFMAs: collect it here, in front of the epilogue, so that the epilogue's global
        // stores (which retire through the same in-order vmcnt) drain under the next tile instead of being waited for
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const TilePos p = tile_pos(t, g.tiles_x, g.tiles_y);
        tile8x32_out(Cs, acc, bias, g.Res, g.Out, g.stats != nullptr, lacc, [&](int ry, int rx, long& o) {
            const int y = p.ty * TH + ry, x = p.tx * TW + rx;
            o = (((long)p.img * g.H + y) * g.W_ + x) * 64;
            return y < g.H && x < g.W_;
        });
        lds_barrier();                                             // C tile free again, next patch complete
        if (g.stats && threadIdx.x == 0) stats_flush(lacc, g.stats, p.img);
    }
}

TileMap make_map(int n, int H, int W) {
    TileMap m{};
    m.n = n; m.H = H; m.W = W;
    m.px = W <= 15 ? TW / (W + 1) : 1;
    m.py = (H <= 3 && m.px > 1) ? TH / (H + 1) : 1;                // stacking only together with side-by-side packing
    m.tiles_x = m.px > 1 ? 1 : (W + TW - 1) / TW;
    m.tiles_y = m.py > 1 ? 1 : (H + TH - 1) / TH;
    return m;
}

constexpr size_t C64_SMEM = 2 * PATCH_BYTES + CT_BYTES + 16;
static_assert(C64_SMEM == 133616, "dynamic LDS of k_sconv3_c64 / k_sconv3_g");

// ---------------------------------------------------------------------------------------------------------------------
// General width (input and output channels multiples of 64; the 128 / 256 / 512-channel stages): same tile, same patch, but the
// input channels pass through LDS in chunks of 64 and a workgroup produces one group of 64 output channels (blockIdx.y).
// The weight fragments no longer fit in registers: they stream through the ring of ring_taps.
// ---------------------------------------------------------------------------------------------------------------------
struct CGArgs {
    const bf16* In; const bf16* W; const float* bias; const bf16* Res; bf16* Out; double* stats;   // stats: unpacked maps only
    int n, H, W_, flip;
    int cin, cout, nc;                                  // channels of this pass' input / output, cin / 64
    TileMap map; int ntiles;
};

__global__ __launch_bounds__(512, 1) void k_sconv3_g(const CGArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* patch = smem;
    float* Cs = reinterpret_cast<float*>(smem + 2 * PATCH_BYTES);
    float* lacc = reinterpret_cast<float*>(smem + 2 * PATCH_BYTES + CT_BYTES);
    if (threadIdx.x == 0) { lacc[0] = 0.f; lacc[1] = 0.f; }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wp = wave >> 1, wn = wave & 1;
    const int n0 = 64 * blockIdx.y;                                // this workgroup's output channels [n0, n0 + 64)
    const bf16* wrow = g.W + (long)(n0 + 32 * wn + l31) * (9 * g.cin) + lh * 8;
    const float bias = g.bias ? g.bias[n0 + 32 * wn + l31] : 0.f;

    bf16x8_t bq[5][4];
    auto stage = [&](int t, int chunk, int buf) {
        patch_dma<PH, PW, 8>(patch + buf * PATCH_BYTES, wave, lane, [&](int py, int px) -> const bf16* {
            int img = 0, y = 0, x = 0;
            return g.map.pixel(t, py - 1, px - 1, img, y, x) ? g.In + (((long)img * g.H + y) * g.W_ + x) * g.cin + chunk * 64 : nullptr;
        });
    };

    const int nb = gridDim.x;
    int t = first_tile(), chunk = 0, buf = 0;
    if (t >= g.ntiles) return;
    stage(t, 0, 0);
    ring_load(bq[0], wrow, g.cin, g.flip, 0, 0);
    ring_load(bq[1], wrow, g.cin, g.flip, 0, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x16 acc[2];
    zero_acc(acc);
    while (true) {
        int nchunk = chunk + 1, nt = t;
        if (nchunk == g.nc) { nchunk = 0; nt = t + nb; }
        const bool more = nt < g.ntiles;
        ring_taps<2, PW>(acc, bq, patch + buf * PATCH_BYTES + ((2 * wp) * PW + l31) * PS + lh * 16, wrow, g.cin, g.flip, chunk, nchunk, more,
                         [&] { stage(nt, nchunk, buf ^ 1); });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // next patch + next fragments; in front of the epilogue's stores
        if (chunk == g.nc - 1) {
            tile8x32_out(Cs, acc, bias, g.Res, g.Out, g.stats != nullptr, lacc, [&](int ry, int rx, long& o) {
                int img = 0, y = 0, x = 0;
                const bool ok = g.map.pixel(t, ry, rx, img, y, x);
                o = (((long)img * g.H + y) * g.W_ + x) * g.cout + n0;
                return ok;
            });
            zero_acc(acc);
        }
        lds_barrier();
        if (g.stats && chunk == g.nc - 1 && threadIdx.x == 0) stats_flush(lacc, g.stats, tile_pos(t, g.map.tiles_x, g.map.tiles_y).img);
        if (!more) break;
        t = nt; chunk = nchunk; buf ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stride-2 down-sampler forward (3x3, pad 0, zeros beyond the map; channels multiples of 64): the general-width scheme on a
// 2 x 32 output tile -- its 5 x 65 input patch fits the stride-1 patch buffer -- with four waves (tile row x channel half),
// input pixel = 2 * output pixel + tap.  Input-bound: four input pixels are read per output pixel.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int S2_PH = 5, S2_PW = 65;                  // patch of a 2 x 32 output tile
static_assert(patch_dma_bytes(S2_PH, S2_PW) <= PATCH_BYTES, "the stride-2 forward stages its patch in a stride-1 patch buffer");
constexpr size_t S2_SMEM = 2 * PATCH_BYTES + 64 * CP * 4 + 16;
static_assert(S2_SMEM == 116208, "dynamic LDS of k_sconv3_s2_fwd");

struct S2Args {
    const bf16* In; const bf16* W; const float* bias; bf16* Out; double* stats;
    int n, Hi, Wi, Ho, Wo, cin, cout, nc;
    int tiles_x, tiles_y, ntiles;
};

__global__ __launch_bounds__(256, 1) void k_sconv3_s2_fwd(const S2Args g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* patch = smem;
    float* Cs = reinterpret_cast<float*>(smem + 2 * PATCH_BYTES);
    float* lacc = reinterpret_cast<float*>(smem + 2 * PATCH_BYTES + 64 * CP * 4);
    if (threadIdx.x == 0) { lacc[0] = 0.f; lacc[1] = 0.f; }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wr = wave >> 1, wn = wave & 1;                       // output tile row, channel half
    const int n0 = 64 * blockIdx.y;
    const bf16* wrow = g.W + (long)(n0 + 32 * wn + l31) * (9 * g.cin) + lh * 8;
    const float bias = g.bias ? g.bias[n0 + 32 * wn + l31] : 0.f;
    bf16x8_t bq[5][4];
    auto stage = [&](int t, int chunk, int buf) {
        const TilePos p = tile_pos(t, g.tiles_x, g.tiles_y);
        const int y0 = 2 * (p.ty * 2), x0 = 2 * (p.tx * TW);
        patch_dma<S2_PH, S2_PW, 4>(patch + buf * PATCH_BYTES, wave, lane, [&](int py, int px) -> const bf16* {
            const int y = y0 + py, x = x0 + px;
            return (y < g.Hi && x < g.Wi) ? g.In + (((long)p.img * g.Hi + y) * g.Wi + x) * g.cin + chunk * 64 : nullptr;
        });
    };
    const int nb = gridDim.x;
    int t = first_tile(), chunk = 0, buf = 0;
    if (t >= g.ntiles) return;
    stage(t, 0, 0);
    ring_load(bq[0], wrow, g.cin, 0, 0, 0);
    ring_load(bq[1], wrow, g.cin, 0, 0, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x16 acc[1];
    zero_acc(acc);
    while (true) {
        int nchunk = chunk + 1, nt = t;
        if (nchunk == g.nc) { nchunk = 0; nt = t + nb; }
        const bool more = nt < g.ntiles;
        ring_taps<1, S2_PW>(acc, bq, patch + buf * PATCH_BYTES + ((2 * wr) * S2_PW + 2 * l31) * PS + lh * 16, wrow, g.cin, 0, chunk, nchunk, more,
                            [&] { stage(nt, nchunk, buf ^ 1); });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (chunk == g.nc - 1) {
            const TilePos p = tile_pos(t, g.tiles_x, g.tiles_y);
            acc_to_cs<true>(Cs, acc[0], wr * 32, 32 * wn + l31, lh, bias);
            lds_barrier();
            float ts = 0.f, tss = 0.f;                             // summed whether or not g.stats asks for them; added only then
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + i * 256, pos = idx >> 3, ch = idx & 7;     // 64 positions x 8 chunks
                const int y = p.ty * 2 + (pos >> 5), x = p.tx * TW + (pos & 31);
                if (y < g.Ho && x < g.Wo)
                    cs_store8(Cs, pos, ch, nullptr, g.Out, (((long)p.img * g.Ho + y) * g.Wo + x) * g.cout + n0 + ch * 8, true, ts, tss);
            }
            if (g.stats) stats_wave_add(ts, tss, lacc);
            zero_acc(acc);
        }
        lds_barrier();
        if (g.stats && chunk == g.nc - 1 && threadIdx.x == 0) stats_flush(lacc, g.stats, tile_pos(t, g.tiles_x, g.tiles_y).img);
        if (!more) break;
        t = nt; chunk = nchunk; buf ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stride-2 down-sampler data gradient, 64 output-gradient channels (the two full-resolution down-samplers):
//   dIn[y][x][c] = sum over taps with (y - ky), (x - kx) even of dOut[(y - ky)/2][(x - kx)/2][n] * W[n][c][ky][kx].
// The input pixels fall into four parity classes (y & 1, x & 1) with 4 / 2 / 2 / 1 contributing taps; each class is a small
// stride-1 convolution over the half-resolution output gradient.  A workgroup owns 4 x 32 half-resolution positions (8 x 64 input
// pixels): the 5 x 33 dOut patch arrives by LDS-DMA (double buffered), the 36 weight fragments of the transposed pack stay in
// registers, and the four classes are multiplied one after the other through the fp32 C tile (16-B stores of every other pixel).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int D2_PH = 5, D2_PW = 33;
constexpr int D2_PATCH = patch_dma_bytes(D2_PH, D2_PW);               // 24 192
constexpr size_t D2_SMEM = 2 * D2_PATCH + CT_BYTES;
static_assert(D2_SMEM == 83200, "dynamic LDS of k_sconv3_s2_dgrad");

struct D2Args {
    const bf16* dOut; const bf16* Wt; bf16* dIn;
    int n, Hi, Wi, Ho, Wo, cin, accumulate;
    int tiles_x, tiles_y, ntiles;
};

__global__ __launch_bounds__(512, 1) void k_sconv3_s2_dgrad(const D2Args g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* patch = smem;
    float* Cs = reinterpret_cast<float*>(smem + 2 * D2_PATCH);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wy = wave >> 1, wn = wave & 1;
    const int n0 = 64 * blockIdx.y;                                // this workgroup's input channels [n0, n0 + 64)
    bf16x8_t bw[9][4];
    load_w36(bw, g.Wt + (long)(n0 + 32 * wn + l31) * 576 + lh * 8, 0);
    const bf16* so_far = g.accumulate ? g.dIn : nullptr;           // accumulation: the gradient so far is the operand added before the rounding
    auto stage = [&](int t, int buf) {
        const TilePos p = tile_pos(t, g.tiles_x, g.tiles_y);
        const int y0 = p.ty * 4 - 1, x0 = p.tx * TW - 1;
        patch_dma<D2_PH, D2_PW, 8>(patch + buf * D2_PATCH, wave, lane, [&](int py, int px) -> const bf16* {
            const int y = y0 + py, x = x0 + px;
            return (y >= 0 && y < g.Ho && x >= 0 && x < g.Wo) ? g.dOut + (((long)p.img * g.Ho + y) * g.Wo + x) * 64 : nullptr;
        });
    };
    const int nb = gridDim.x;
    int t = first_tile(), buf = 0;
    if (t < g.ntiles) stage(t, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (; t < g.ntiles; t += nb, buf ^= 1) {
        if (t + nb < g.ntiles) stage(t + nb, buf ^ 1);
        const TilePos p = tile_pos(t, g.tiles_x, g.tiles_y);
        const char* pb = patch + buf * D2_PATCH + lh * 16;
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int py = cls >> 1, px = cls & 1;
            f32x16 acc[1];
            zero_acc(acc);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                if ((ky & 1) != py) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    if ((kx & 1) != px) continue;
                    tap_step<1, 0>(acc, pb + ((wy + (ky == 2 ? 0 : 1)) * D2_PW + l31 + (kx == 2 ? 0 : 1)) * PS, bw[ky * 3 + kx]);
                }
            }
            acc_to_cs<false>(Cs, acc[0], wy * 32, 32 * wn + l31, lh, 0.f);
            lds_barrier();
            float ts = 0.f, tss = 0.f;                             // unused: no statistics of a gradient
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + i * 512, pos = idx >> 3, ch = idx & 7;     // 128 half-resolution positions x 8 chunks
                const int y = 2 * (p.ty * 4 + (pos >> 5)) + py, x = 2 * (p.tx * TW + (pos & 31)) + px;
                if (y < g.Hi && x < g.Wi)
                    cs_store8(Cs, pos, ch, so_far, g.dIn, (((long)p.img * g.Hi + y) * g.Wi + x) * g.cin + n0 + ch * 8, false, ts, tss);
            }
            lds_barrier();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // next patch (the stores of this tile with it: once per tile)
        lds_barrier();
    }
}

bool packed(const TileMap& m) { return m.px > 1 || m.py > 1; }
int grid256(int ntiles) { return ntiles < 256 ? ntiles : 256; }        // one persistent workgroup per CU

// Raise the dynamic-LDS limit once for kernel K, launch it, check the launch
template <auto K, typename Args>
int launch(dim3 grid, int threads, size_t smem, hipStream_t st, const Args& a) {
    static bool attr = false;                                      // one per kernel: K is a template argument
    int rc;
    if ((rc = allow_lds(reinterpret_cast<const void*>(K), (int)smem, attr))) return rc;
    hipLaunchKernelGGL(K, grid, dim3(threads), smem, st, a);
    TCVN_LAUNCH_CHECK();
    return 0;
}

// SCONV_G forward (flip = 0) and, on the transposed pack with the channel roles exchanged, data gradient (flip = 1)
int launch_g(const SConv& g, const void* In, int cin, const void* W, int cout, const float* bias, const void* Res, void* Out, int flip,
             hipStream_t st) {
    CGArgs a{};
    a.In = reinterpret_cast<const bf16*>(In); a.W = reinterpret_cast<const bf16*>(W); a.bias = bias;
    a.Res = reinterpret_cast<const bf16*>(Res); a.Out = reinterpret_cast<bf16*>(Out);
    a.n = g.n; a.H = g.Hin; a.W_ = g.Win; a.flip = flip; a.cin = cin; a.cout = cout; a.nc = cin / 64;
    a.map = make_map(g.n, g.Hin, g.Win); a.ntiles = a.map.ntiles();
    a.stats = (flip || packed(a.map)) ? nullptr : g.stats;
    return launch<k_sconv3_g>(dim3(grid256(a.ntiles), cout / 64), 512, C64_SMEM, st, a);
}

// SCONV_C64, same two roles
int launch_c64(const SConv& g, const void* In, const void* W, const float* bias, const void* Res, void* Out, int flip, hipStream_t st) {
    C64Args a{};
    a.stats = flip ? nullptr : g.stats;
    a.In = reinterpret_cast<const bf16*>(In); a.W = reinterpret_cast<const bf16*>(W); a.bias = bias;
    a.Res = reinterpret_cast<const bf16*>(Res); a.Out = reinterpret_cast<bf16*>(Out);
    a.n = g.n; a.H = g.Hin; a.W_ = g.Win; a.flip = flip;
    a.tiles_x = (g.Win + TW - 1) / TW; a.tiles_y = (g.Hin + TH - 1) / TH; a.ntiles = g.n * a.tiles_x * a.tiles_y;
    return launch<k_sconv3_c64>(dim3(grid256(a.ntiles)), 512, C64_SMEM, st, a);
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient: dW[n][tap*64 + c] = sum over positions p of In[p + shift(tap)][c] * dOut[p][n].
// The contraction runs over pixels, i.e. over the ROW index of both pixel-major LDS images, so both MFMA operands are read
// transposed with ds_read_b64_tr_b16 (tr_frag; lane roles as in conv3x3_wgrad_tile.hip, checked by tools/micro/tr_read_test.hip): per
// 16-position k-step (half a tile row) a wave reads one dOut fragment and nine shifted In fragments.  A wave owns one
// (32 c x 32 n) quarter of all nine taps for the whole launch (144 accumulator registers); the workgroup's partial
// gradient leaves as one slab in the kernel layout [n][576], summed by k_slab_reduce.  Pixel rows are 128 B, 16-B chunks
// XOR-swizzled with the pixel index so that the four rows of a transpose group fall on different banks.
// Two workgroups per CU (76 KB of LDS each): one stages while the other multiplies.
// ---------------------------------------------------------------------------------------------------------------------
// 128-B pixel rows: two rows per 256 B of banks.  A transposed read (half a wave) takes four consecutive pixels x one 64-B half row; with
// `chunk ^ (pix & 7)` pixels p and p + 2 of such a group landed on the same 16 banks (same row parity, same half) -- bit 1 of the pixel index
// now selects the half, so the four pixels of a group cover four different 64-B bank ranges whatever their alignment.
__device__ __forceinline__ int swz(int pix, int chunk, int sub) { return pix * 128 + ((chunk ^ ((((pix >> 1) & 1) << 2) | (pix & 3))) << 4) + sub; }

constexpr int WG_PATCH = PH * PW * 128;               // 43 520
constexpr int WG_DOUT = TH * TW * 128;                // 32 768
constexpr size_t WG_SMEM = WG_PATCH + WG_DOUT + PH * PW * 4;          // stride 1: patch, dOut tile, packed-map table
constexpr size_t WG2_SMEM = S2_PH * S2_PW * 128 + 2 * TW * 128;       // stride 2: 5 x 65 patch, 2 x 32 dOut tile
static_assert(WG_SMEM == 77648 && WG2_SMEM == 49792, "dynamic LDS of k_sconv3_c64_wgrad");

struct W64Args {
    const bf16* In; const bf16* dOut; float* slab; float* bslab;
    int n, H, W_;                         // output map (= the dOut tensor)
    int tiles_x, tiles_y, ntiles;
    int cin, cout;                        // row strides; blockIdx.y selects the (64 c) x (64 n) sub-block: c chunk fastest
    int Hi, Wi;                           // input map
    TileMap map;                          // stride 1: tile -> pixel mapping (small maps packed)
};

// Source of a staged pixel, for both operands: `base` = the thread's 8 channels of pixel 0 of a [.][Hm][Wm] map with `ld` channels per
// pixel; false = the pixel stages as zero (a flag, not a null pointer: the staging then branches once per load).  Unpacked: pixel (y, x) of
// image `img`.  PACK (stride 1: both maps have the tile's size): `img` is the tile's image group, e the table entry of the tile position --
// the pixel offset within the group's images when the map is stacked in y too, else (packed in x only: rows follow the y tile) the slot's column, row y.
template <bool PACK>
__device__ __forceinline__ bool wg_src(const bf16* base, int Hm, int Wm, int ld, int img, int y, int x, int e, const TileMap& map, const bf16*& src) {
    if (PACK) {
        const int gbase = img * (map.px * map.py), slot = e >> 24, off = e & 0xffffff;
        if (e < 0 || gbase + slot >= map.n) return false;
        if (map.py > 1) { src = base + ((long)gbase * Hm * Wm + off) * ld; return true; }
        src = base + (((long)(gbase + slot) * Hm + y) * Wm + (off - slot * Hm * Wm)) * ld;
        return y >= 0 && y < Hm;
    }
    src = base + (((long)img * Hm + y) * Wm + x) * ld;
    return y >= 0 && y < Hm && x >= 0 && x < Wm;
}

// S = 1: 3x3 / stride 1 / pad 1 (8 x 32 output tile, 10 x 34 patch); S = 2: 3x3 / stride 2 / pad 0 with zeros beyond the map
// (diffusers' F.pad(0,1,0,1) down-sampler: 2 x 32 output tile, 5 x 65 patch, input pixel = 2 * output pixel + tap)
template <int S, bool PACK>
__global__ __launch_bounds__(256, 2) void k_sconv3_c64_wgrad(const W64Args g) {
    constexpr int OTH = S == 1 ? 8 : 2;                            // output tile rows
    constexpr int PHs = S * OTH + (S == 1 ? 2 : 1), PWs = S * TW + (S == 1 ? 2 : 1), ORG = S == 1 ? 1 : 0;
    constexpr int NPC = PHs * PWs * 8, NPL = (NPC + 255) / 256;    // patch chunks, per thread
    constexpr int NDL = OTH * TW * 8 / 256;                        // dOut chunks per thread
    constexpr int PATCH_B = PHs * PWs * 128;
    static_assert(!PACK || S == 1, "packed maps are stride 1");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* patch = smem;                                            // [PH*PW][128 B] In halo patch
    char* dout = smem + PATCH_B;                                   // [TH*TW][128 B] output-gradient tile
    // packed small maps: tile-independent part of the tile -> pixel mapping, one entry per patch pixel:
    // (image slot within the group) << 24 | pixel offset within the group's images, -1 = padding
    int* ptab = reinterpret_cast<int*>(smem + PATCH_B + OTH * TW * 128);
    if (PACK) {
        for (int p = threadIdx.x; p < PHs * PWs; p += 256) {
            const int ry = p / PWs - 1, rx = p % PWs - 1;
            int e = -1;                                            // packing in y implies packing in x (make_map); x-only packing
            if (rx >= 0 && (g.map.py == 1 || ry >= 0)) {           // keeps y for the use site (rows follow the y tile)
                const int sx = rx / (g.map.W + 1), x = rx - sx * (g.map.W + 1);
                int sy = 0, y = 0;
                if (g.map.py > 1) { sy = ry / (g.map.H + 1); y = ry - sy * (g.map.H + 1); }
                if (sx < g.map.px && x < g.map.W && (g.map.py == 1 || (sy < g.map.py && y < g.map.H))) {
                    const int slot = sy * g.map.px + sx;
                    e = (slot << 24) | (slot * g.map.H * g.map.W + y * g.map.W + x);
                }
            }
            ptab[p] = e;
        }
        __syncthreads();
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wc = wave >> 1, wn = wave & 1;                       // input-channel half, output-channel half
    const int gq = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int khalf = gq >> 1, chalf = gq & 1;
    const int a_chunk = 4 * wc + 2 * chalf + (tp >> 1), b_chunk = 4 * wn + 2 * chalf + (tp >> 1), sub = (tp & 1) * 8;
    f32x16 acc[9];
    zero_acc(acc);
    float bsum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bsum[j] = 0.f;

    const int ncc = g.cin >> 6;
    const int c0 = 64 * (blockIdx.y % ncc), n0 = 64 * (blockIdx.y / ncc);
    const int nb = gridDim.x;
    for (int t = first_tile(); t < g.ntiles; t += nb) {
        const TilePos p = tile_pos(t, g.tiles_x, g.tiles_y);
        const int y0 = p.ty * OTH, x0 = p.tx * TW;
        __syncthreads();                                           // previous tile's readers are done
        {
            // two batches: the tile mapping of the packed small maps needs registers too, and this kernel sits at the 256-register
            // limit of two workgroups per CU
            constexpr int NBAT = PACK ? 2 : 1, NPH = (NPL + NBAT - 1) / NBAT;
#pragma unroll
            for (int hb = 0; hb < NBAT; ++hb) {
                u16x8 v[NPH];
#pragma unroll
                for (int i = 0; i < NPH; ++i) {
                    const int idx = tid + (hb * NPH + i) * 256, pix = idx >> 3, ch = idx & 7;
                    const int py = pix / PWs, px = pix - py * PWs;
                    const int e = PACK && idx < NPC ? ptab[pix] : -1;
                    const bf16* src;
                    v[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
                    if (idx < NPC && wg_src<PACK>(g.In + c0 + ch * 8, g.Hi, g.Wi, g.cin, p.img, S * y0 - ORG + py, S * x0 - ORG + px, e, g.map, src))
                        v[i] = *reinterpret_cast<const u16x8*>(src);
                }
#pragma unroll
                for (int i = 0; i < NPH; ++i) {
                    const int idx = tid + (hb * NPH + i) * 256, pix = idx >> 3, ch = idx & 7;
                    if (idx < NPC) *reinterpret_cast<u16x8*>(patch + swz(pix, ch, 0)) = v[i];
                }
            }
        }
        {
            u16x8 d[NDL];
#pragma unroll
            for (int i = 0; i < NDL; ++i) {
                const int idx = tid + i * 256, pos = idx >> 3, ch = idx & 7;
                const int e = PACK ? ptab[((pos >> 5) + 1) * PWs + (pos & 31) + 1] : -1;
                const bf16* src;
                d[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
                if (wg_src<PACK>(g.dOut + n0 + ch * 8, g.H, g.W_, g.cout, p.img, y0 + (pos >> 5), x0 + (pos & 31), e, g.map, src))
                    d[i] = *reinterpret_cast<const u16x8*>(src);
            }
#pragma unroll
            for (int i = 0; i < NDL; ++i) {
                const int idx = tid + i * 256, pos = idx >> 3, ch = idx & 7;
                *reinterpret_cast<u16x8*>(dout + swz(pos, ch, 0)) = d[i];
#pragma unroll
                for (int j = 0; j < 8; ++j) bsum[j] += bf2f(d[i][j]);
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int ks = 0; ks < OTH * TW / 16; ++ks) {
            const int ry = ks >> 1, xb = (ks & 1) * 16 + 8 * khalf + tq;           // this lane's row of the transpose group
            const int bp = ry * TW + xb;
            const bf16x8_t b = tr_frag(dout, swz(bp, b_chunk, sub), swz(bp + 4, b_chunk, sub));
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ap = (S * ry + tap / 3) * PWs + S * xb + tap % 3;
                const bf16x8_t a = tr_frag(patch, swz(ap, a_chunk, sub), swz(ap + 4 * S, a_chunk, sub));
                acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[tap], 0, 0, 0);
            }
        }
    }
    // slab[blockIdx][n][576]: accumulator row = input channel within the wave's half, column = output channel
    {
        const int l31 = lane & 31, lh = lane >> 5;
        float* out = g.slab + ((long)blockIdx.x * gridDim.y + blockIdx.y) * (64 * 576) + (long)(32 * wn + l31) * 576 + 32 * wc;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int e = 0; e < 16; ++e) out[tap * 64 + (e & 3) + 8 * (e >> 2) + 4 * lh] = acc[tap][e];
    }
    if (g.bslab == nullptr) return;                                // uniform
    // general width (2-D grid): the sub-blocks of one output-channel group saw the same dOut tiles; the first of them leaves the
    // group's column sums (uniform per workgroup)
    if ((int)blockIdx.y % ncc != 0) return;
    // bias gradient: threads with equal tid & 7 hold the same 8 channels
    __syncthreads();
    float* br = reinterpret_cast<float*>(smem);                    // [32][64]
#pragma unroll
    for (int j = 0; j < 8; ++j) br[(tid >> 3) * 64 + (tid & 7) * 8 + j] = bsum[j];
    __syncthreads();
    if (tid < 64) {
        float s = 0.f;
        for (int q = 0; q < 32; ++q) s += br[q * 64 + tid];
        g.bslab[((long)blockIdx.x * (g.cout / 64) + blockIdx.y / ncc) * 64 + tid] = s;
    }
}

// dWk[(n0 + n)*Kp + tap*Cin + c0 + c] += sum_x slab[x][sub][n][tap*64 + c]
__global__ __launch_bounds__(256) void k_sub_reduce(const float* __restrict__ slab, int nx, int nsub, int ncc, int cin, float* __restrict__ dWk) {
    const int sub = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;                  // element of the 64 x 576 sub-block
    if (i >= 64 * 576) return;
    float s0 = 0.f, s1 = 0.f;
    int x = 0;
    for (; x + 7 < nx; x += 8) {                                   // eight slabs requested together (two per trip was a memory round trip per pair:
        float v[8];                                                // up to 128 dependent trips per launch, 73 launches per step)
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = slab[((long)(x + q) * nsub + sub) * (64 * 576) + i];
        s0 += (v[0] + v[2]) + (v[4] + v[6]);
        s1 += (v[1] + v[3]) + (v[5] + v[7]);
    }
    for (; x + 1 < nx; x += 2) {
        s0 += slab[((long)x * nsub + sub) * (64 * 576) + i];
        s1 += slab[((long)(x + 1) * nsub + sub) * (64 * 576) + i];
    }
    if (x < nx) s0 += slab[((long)x * nsub + sub) * (64 * 576) + i];
    const int n = i / 576, k = i - n * 576, tap = k >> 6, c = k & 63;
    const int c0 = 64 * (sub % ncc), n0 = 64 * (sub / ncc);
    dWk[(long)(n0 + n) * (9 * cin) + tap * cin + c0 + c] += s0 + s1;
}

int launch_s2_fwd(const SConvFwd& c, hipStream_t st) {
    const SConv& g = c.g;
    S2Args a{};
    a.stats = g.stats;
    a.In = reinterpret_cast<const bf16*>(c.In); a.W = reinterpret_cast<const bf16*>(c.Wk); a.bias = c.bias; a.Out = reinterpret_cast<bf16*>(c.Out);
    a.n = g.n; a.Hi = g.Hin; a.Wi = g.Win; a.Ho = g.Ho; a.Wo = g.Wo; a.cin = g.Cin; a.cout = g.Cout; a.nc = g.Cin / 64;
    a.tiles_x = (g.Wo + TW - 1) / TW; a.tiles_y = (g.Ho + 1) / 2; a.ntiles = g.n * a.tiles_x * a.tiles_y;
    return launch<k_sconv3_s2_fwd>(dim3(grid256(a.ntiles), g.Cout / 64), 256, S2_SMEM, st, a);
}
int launch_s2_dgrad(const SConvDgrad& c, hipStream_t st) {
    const SConv& g = c.g;
    D2Args a{};
    a.dOut = reinterpret_cast<const bf16*>(c.dOut); a.Wt = reinterpret_cast<const bf16*>(c.Wt); a.dIn = reinterpret_cast<bf16*>(c.dIn);
    a.n = g.n; a.Hi = g.Hin; a.Wi = g.Win; a.Ho = g.Ho; a.Wo = g.Wo; a.cin = g.Cin; a.accumulate = c.accumulate;
    // half-resolution positions (Y, X) cover input pixels (2Y + py, 2X + px): Y up to ceil(Hi / 2) - 1
    const int hy = (g.Hin + 1) / 2, hx = (g.Win + 1) / 2;
    a.tiles_x = (hx + TW - 1) / TW; a.tiles_y = (hy + 3) / 4; a.ntiles = g.n * a.tiles_x * a.tiles_y;
    return launch<k_sconv3_s2_dgrad>(dim3(grid256(a.ntiles), g.Cin / 64), 512, D2_SMEM, st, a);
}

// The weight gradient of all three families is k_sconv3_c64_wgrad over 64 x 64 channel sub-blocks (blockIdx.y, c chunk fastest).  SCONV_G
// walks the packed TileMap; SCONV_C64 (always one sub-block) and SCONV_S2 tile every image on its own.
W64Args wgrad_args(SConvKernel k, const SConvWgrad& c) {
    const SConv& g = c.g;
    W64Args a{};
    a.In = reinterpret_cast<const bf16*>(c.In); a.dOut = reinterpret_cast<const bf16*>(c.dOut); a.slab = g.slab;
    a.n = g.n; a.H = g.Ho; a.W_ = g.Wo; a.Hi = g.Hin; a.Wi = g.Win; a.cin = g.Cin; a.cout = g.Cout;
    if (k == SCONV_G) {
        a.map = make_map(g.n, g.Hin, g.Win); a.tiles_x = a.map.tiles_x; a.tiles_y = a.map.tiles_y; a.ntiles = a.map.ntiles();
    } else {
        a.tiles_x = (g.Wo + TW - 1) / TW; a.tiles_y = k == SCONV_S2 ? (g.Ho + 1) / 2 : (g.Ho + TH - 1) / TH; a.ntiles = g.n * a.tiles_x * a.tiles_y;
    }
    return a;
}

}  // namespace

bool sconv3_packs(const SConv& g) { return packed(make_map(g.n, g.Hin, g.Win)); }

int sconv3_fwd(SConvKernel k, const SConvFwd& c, hipStream_t st) {
    const SConv& g = c.g;
    switch (k) {
    case SCONV_C64: return launch_c64(g, c.In, c.Wk, c.bias, c.Res, c.Out, 0, st);
    case SCONV_G: return launch_g(g, c.In, g.Cin, c.Wk, g.Cout, c.bias, c.Res, c.Out, 0, st);
    case SCONV_S2: return launch_s2_fwd(c, st);
    default: return -2;
    }
}
int sconv3_dgrad(SConvKernel k, const SConvDgrad& c, hipStream_t st) {
    const SConv& g = c.g;
    const void* acc = c.accumulate ? c.dIn : nullptr;              // accumulation = the gradient so far as the residual operand
    switch (k) {
    case SCONV_C64: return launch_c64(g, c.dOut, c.Wt, nullptr, acc, c.dIn, 1, st);
    case SCONV_G: return launch_g(g, c.dOut, g.Cout, c.Wt, g.Cin, nullptr, acc, c.dIn, 1, st);
    case SCONV_S2: return launch_s2_dgrad(c, st);
    default: return -2;
    }
}
int sconv3_wgrad(SConvKernel k, const SConvWgrad& c, hipStream_t st) {
    const SConv& g = c.g;
    W64Args a = wgrad_args(k, c);
    int rc;
    if (k == SCONV_C64) {
        // one slab per workgroup, two workgroups per CU; the bias rows sit behind the slabs in use
        const int grid = a.ntiles < 512 ? grid256(a.ntiles) : 512;
        a.bslab = g.slab + (long)grid * 64 * 576;
        if ((rc = launch<k_sconv3_c64_wgrad<1, false>>(dim3(grid), 256, WG_SMEM, st, a))) return rc;
        SlabJob none{};
        return slab_reduce2(slab_job(a.slab, grid, 64L * 576, c.dWk, 0), c.dbias ? slab_job(a.bslab, grid, 64, c.dbias, 0) : none, st);
    }
    const int ncc = g.Cin / 64, nsub = ncc * (g.Cout / 64);
    int gx = 512 / nsub;                                           // slab holds 512 sub-block partials; two workgroups per CU
    if (gx > a.ntiles) gx = a.ntiles;
    if (gx < 1) gx = 1;
    // bias gradient from the kernel's own dOut tiles: one row of cout sums per x-workgroup, behind the 512 weight sub-block slabs
    // (gx * cout <= 512 * 64 floats)
    a.bslab = c.dbias != nullptr ? g.slab + 512L * 64 * 576 : nullptr;
    const dim3 grid(gx, nsub);
    if (k == SCONV_S2) rc = launch<k_sconv3_c64_wgrad<2, false>>(grid, 256, WG2_SMEM, st, a);
    else if (packed(a.map)) rc = launch<k_sconv3_c64_wgrad<1, true>>(grid, 256, WG_SMEM, st, a);
    else rc = launch<k_sconv3_c64_wgrad<1, false>>(grid, 256, WG_SMEM, st, a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sub_reduce, dim3((64 * 576 + 255) / 256, nsub), dim3(256), 0, st, a.slab, gx, nsub, ncc, g.Cin, c.dWk);
    TCVN_LAUNCH_CHECK();
    return c.dbias != nullptr ? slab_reduce(a.bslab, gx, g.Cout, c.dbias, st) : 0;
}

}  // namespace tcvn
