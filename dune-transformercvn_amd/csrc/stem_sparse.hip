// Sparse-aware stem (bf16 throughput mode): conv0 7x7/2 + BatchNorm0 + PReLU0 + AvgPool 3/2 and their backward straight from
// the COO hit list (reference: trainers/neutrino_full_dense_trainer.py:15-24 `sparse_to_dense` + layers/dense_net.py:112-121).
//
// The pixel maps are mostly empty: a 400 x 280 prong map holds 20-800 hits, an event map 500-4000.  The dense path scatters them into
// a [n,400,280,3] map, runs a dense MFMA convolution over all 28 000 output positions of every map, writes the [n,200,140,64] conv0
// output (1 GB for 288 maps), reads it again for the pooling and twice more in backward.  Here neither the dense map nor the conv0
// output exists in HBM, and the work is proportional to the hits:
//   * index (once per forward): the hits are bucketed by (map, pixel row) -- count, prefix sum, fill -- as 16-byte records (HitRec);
//     duplicate coordinates keep the record with the highest list index (a valid outcome of the reference's non-accumulating indexed
//     write, and a deterministic one).
//   * every pass gives a workgroup one map (or a range of row bands of one map): for_each_band.  Per band it copies the band's records
//     -- one contiguous range of the index -- into LDS, lays out an occupancy bitmap and a pixel -> record map, and from then on works on
//     chip: a conv0 position whose 7x7 window holds no hit equals the bias exactly, so it is never evaluated; the non-empty positions are
//     collected in an ordered worklist and evaluated by eight threads each (8 channels per thread), one FMA chain per hit in window
//     order (for_each_hit).
//   k_stem_sparse_stats      sum / sum of squares of the conv0 output per channel (BatchNorm0's batch statistics)     [train only]
//   k_stem_sparse_pool       conv0 -> BN0 -> PReLU0 -> AvgPool(3, stride 2) -> first 64 channels of dense block 1 (+ their
//                            statistics); pooled pixels whose 11x11 input window is empty are one constant vector
//   k_stem_sparse_bwd_sums   pooling / PReLU0 / BN0 backward sums (sum dU, sum dU*x, sum dz*min(u,0)): the empty positions enter through
//                            the identity sum_p dz[p] = sum_q eff[q] (every pooled pixel spreads eff/9 over nine existing positions)
//   k_stem_sparse_bwd_wgrad  conv0 weight gradient: eff0 = sc*dU + P0*x + Q0 of the non-empty positions, contracted with the hits
// conv0's output stays fp32 on chip (the dense bf16 path rounds it to bf16 when it stores it).  Deterministic: integer atomics only,
// fixed summation orders.  HBM traffic per step: the index, the pooled map (written once, read in backward).
#include <cstdlib>
#include "tcvn_ops.h"
#include "prof.h"

namespace tcvn {

namespace {

constexpr int SS_N = 64;                        // conv0 output channels
constexpr int SS_K = 147;                       // 7*7*3
constexpr int SS_HCAP = 2048;                   // records of one band kept in LDS (longer bands read their records from the index)
constexpr int SS_CROWS = 8;                     // conv0 rows per band (21 input rows): stats and both backward passes
constexpr int SS_PROWS = 4;                     // pooled rows per band (23 input rows): pooled pass
constexpr int SS_BROWS = 23;                    // input rows of the tallest band (4 pooled rows: 4*4 + 7)
constexpr int SS_CHUNK = 64;                    // worklist positions per contraction round of the weight-gradient pass
constexpr int SS_WMAX = 384;                    // widest map stem_sparse_ok admits: what the LDS layouts are checked for
constexpr int SS_LDS_MAX = 160 * 1024;          // dynamic LDS the pass kernels are allowed

// 16-byte hit record of the index.  x: y << 16 | x (the pixel);  y: v0 | v1 << 16;  z: v2 | DEAD;  w: list index.  Values are bf16.
struct HitRec {
    static constexpr unsigned DEAD = 0x80000000u;   // flag: a later list entry has the same pixel
    uint4 r;
    __device__ static HitRec pack(int y, int x, const float (&v)[3], bool dead, long index) {
        return HitRec{make_uint4(((unsigned)y << 16) | (unsigned)x, (unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16),
                                 (unsigned)f2bf(v[2]) | (dead ? DEAD : 0u), (unsigned)index)};
    }
    __device__ bool dead() const { return (r.z & DEAD) != 0u; }
    __device__ HitRec killed() const { return HitRec{make_uint4(r.x, r.y, r.z | DEAD, r.w)}; }
    __device__ unsigned pixel() const { return r.x; }
    __device__ int y() const { return (int)(r.x >> 16); }
    __device__ int x() const { return (int)(r.x & 0xffffu); }
    __device__ unsigned index() const { return r.w; }
    __device__ void values(float (&v)[3]) const {
        v[0] = bf2f((bf16)(r.y & 0xffffu)); v[1] = bf2f((bf16)(r.y >> 16)); v[2] = bf2f((bf16)(r.z & 0xffffu));
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// index: row_start[map*H + y] .. row_start[map*H + y + 1] lists the hits of pixel row y of a map
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float preprocess_value(float v, int mode, float noise_std, uint64_t seed, long flat_index) {
    v = mode == 1 ? logf(v + 1.f) : mode == 0 ? v / 255.0f : v;        // same arithmetic as k_scatter (elementwise.hip)
    if (noise_std != 0.f) {
        const float u1 = fmaxf(rng_uniform(seed, 0x6e6f6973u, (uint64_t)flat_index * 2), 1e-7f);
        const float u2 = rng_uniform(seed, 0x6e6f6973u, (uint64_t)flat_index * 2 + 1);
        v *= 1.f + noise_std * sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
    }
    return v;                                                           // rounded to bf16 when the record is packed (= the dense bf16 map)
}

__global__ void k_stem_index_count(const StemSparseArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int img, y, x;
    if (i >= a.nnz || !hit_in_map(a.coords, i, a.n_img, a.H, a.W, img, y, x)) return;
    atomicAdd(&a.row_fill[(long)img * a.H + y], 1);
}

// exclusive prefix sum of the per-row counts (one workgroup); resets the counters to zero for the fill pass.  Each of the 16 waves owns a
// contiguous region and walks it in 64-element strips (lane = consecutive element: coalesced) with a shuffle scan per strip and a running
// carry -- two passes over the counts.  (Before: one contiguous chunk of ~110 counts per THREAD, i.e. 64 different lines per wave load:
// 110-210 us per launch at 288 maps, a quarter of the eval-mode stem.)
__global__ __launch_bounds__(1024) void k_stem_index_scan(const StemSparseArgs a, int nbins) {
    __shared__ int wsum[16];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int R = ((nbins + 15) / 16 + 63) & ~63;              // region per wave, whole strips
    const int lo = wave * R, hi = min(nbins, lo + R);
    int s = 0;
    for (int i = lo + lane; i < hi; i += 64) s += a.row_fill[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    int carry = 0;
    for (int w = 0; w < wave; ++w) carry += wsum[w];
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const int v = i < hi ? a.row_fill[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int n = __shfl_up(incl, o);
            if (lane >= o) incl += n;
        }
        if (i < hi) { a.row_start[i] = carry + incl - v; a.row_fill[i] = 0; }
        carry += __shfl(incl, 63);
    }
    if (t == 0) { int tot = 0; for (int w = 0; w < 16; ++w) tot += wsum[w]; a.row_start[nbins] = tot; }
}

__global__ void k_stem_index_fill(const StemSparseArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int img, y, x;
    if (i >= a.nnz || !hit_in_map(a.coords, i, a.n_img, a.H, a.W, img, y, x)) return;
    const long bin = (long)img * a.H + y;
    const int pos = atomicAdd(&a.row_fill[bin], 1);
    float v[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < a.Cpix && c < 3; ++c) v[c] = preprocess_value(a.values[i * a.Cpix + c], a.value_mode, a.noise_std, a.seed, i * a.Cpix + c);
    // a row listed more than 65535 times (possible only with > 200 duplicates per pixel) keeps its first 65535 entries in arrival order:
    // still one of the duplicates per pixel, like the reference's write
    a.rec[a.row_start[bin] + pos] = HitRec::pack(y, x, v, pos >= 65535, i).r;   // order inside a row is arbitrary: lookups go through the pixel map
}

// duplicates: of the records of one pixel only the one with the highest list index stays alive
__global__ void k_stem_index_dedup(const StemSparseArgs a, const int* total) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= *total) return;
    const HitRec r{a.rec[k]};
    const long bin = (long)a.coords[(long)r.index() * 3] * a.H + r.y();
    const int k0 = a.row_start[bin], k1 = a.row_start[bin + 1];
    bool dead = false;
    for (int j = k0; j < k1 && !dead; ++j) {
        const HitRec o{a.rec[j]};
        dead = o.pixel() == r.pixel() && o.index() > r.index() && j - k0 < 65535;
    }
    if (dead) a.rec[k].z = r.killed().r.z;
}

// ---------------------------------------------------------------------------------------------------------------------
// dynamic LDS of a pass: ONE record of byte offsets (multiples of 16) and their total.  The kernel takes its pointers from it, the
// launcher its byte count.  An array the pass does not have takes no bytes.
// ---------------------------------------------------------------------------------------------------------------------
struct PassLds {
    int recs;               // [SS_HCAP] records of the band (when they fit)
    int bits, bw;           // [SS_BROWS][bw] occupancy bitmap, one zero word in front of and two behind every row; bw words per row
    int map;                // [SS_BROWS][W] u16: position of the pixel's record inside its row (valid where the bit is set)
    int rowbase;            // [SS_BROWS + 1] first record of each band row, relative to the band's first record
    int wl, bias;           // conv0 weights [147][64] bf16 (k = (ky*7 + kx)*3 + c), bias [64]
    int tab;                // per-channel tables [3][64] (pooled pass) or [7][64] (backward; the sums pass reads five)
    int cvec;               // [64] bf16 pooled value of an all-empty window
    int wlist, flag, cnt;   // ordered worklist [rows][width] u16, its per-candidate flags (pooled pass), wave counts
    int red;                // channel_fold scratch
    int eff0, wsum;         // weight-gradient pass: eff0 rows of a chunk [SS_CHUNK][64], accumulator [147][64]
    int total;
};
constexpr int align16(int n) { return (n + 15) & ~15; }
constexpr int SUMS_NS = 5;                      // running sums of the sums pass
__host__ __device__ constexpr PassLds pass_lds(StemPass pass, int W, int Wc, int Wo) {
    const bool pool = pass == StemPass::Pool, sums = pass == StemPass::BwdSums, wgrad = pass == StemPass::BwdWgrad;
    const int cells = pool ? SS_PROWS * Wo : SS_CROWS * Wc;
    PassLds l{};
    int p = 0;
    l.recs = p; p += SS_HCAP * 16;
    l.bw = (W + 31) / 32 + 3;
    l.bits = p; p += align16(SS_BROWS * l.bw * 4);
    l.map = p; p += align16(SS_BROWS * W * 2);
    l.rowbase = p; p += 128;
    l.wl = p; p += SS_K * SS_N * 2;
    l.bias = p; p += SS_N * 4;
    l.tab = p; p += (pool ? 3 : sums || wgrad ? 7 : 0) * SS_N * 4;
    l.cvec = p; p += pool ? SS_N * 2 : 0;
    l.wlist = p; p += align16(cells * 2);
    l.flag = p; p += pool ? align16(cells) : 0;
    l.cnt = p; p += 32;
    // the forward passes own their fold scratch; the sums pass folds after its last band, over the record buffer
    l.red = sums ? l.recs : p; p += sums || wgrad ? 0 : channel_fold_bytes(2);
    l.eff0 = p; p += wgrad ? SS_CHUNK * SS_N * 4 : 0;
    l.wsum = p; p += wgrad ? SS_K * SS_N * 4 : 0;
    l.total = p;
    return l;
}
static_assert(channel_fold_bytes(SUMS_NS) <= SS_HCAP * 16, "the sums pass folds over the record buffer");
constexpr int lds_at_limit(StemPass pass) { return pass_lds(pass, SS_WMAX, (SS_WMAX - 1) / 2 + 1, ((SS_WMAX - 1) / 2 + 1 - 3) / 2 + 1).total; }
static_assert(lds_at_limit(StemPass::Stats) <= SS_LDS_MAX && lds_at_limit(StemPass::Pool) <= SS_LDS_MAX &&
              lds_at_limit(StemPass::BwdSums) <= SS_LDS_MAX && lds_at_limit(StemPass::BwdWgrad) <= SS_LDS_MAX,
              "every pass fits its LDS at the widest admitted map (every term grows with W)");

// ---------------------------------------------------------------------------------------------------------------------
// band machinery shared by the passes
// ---------------------------------------------------------------------------------------------------------------------
struct BandLds {            // what every pass has: the band structures, the worklist, the conv0 weights and bias
    uint4* recs; int* rowbase; unsigned* bits; unsigned short* map; int bw, W;
    unsigned short* wlist; unsigned char* flag; int* cnt;
    bf16* wl; float* bias;
};
struct Band { int in_lo, in_hi, nrec; const uint4* rec; bool in_lds; };    // rec: the band's records in the index

template <typename T>
__device__ __forceinline__ T* lds_at(char* smem, int off) { return reinterpret_cast<T*>(smem + off); }
__device__ __forceinline__ BandLds band_lds(char* smem, const PassLds& l, int W) {
    return BandLds{lds_at<uint4>(smem, l.recs), lds_at<int>(smem, l.rowbase), lds_at<unsigned>(smem, l.bits), lds_at<unsigned short>(smem, l.map),
                   l.bw, W, lds_at<unsigned short>(smem, l.wlist), lds_at<unsigned char>(smem, l.flag), lds_at<int>(smem, l.cnt),
                   lds_at<bf16>(smem, l.wl), lds_at<float>(smem, l.bias)};
}

// input rows [in_lo, in_hi] of map img (clipped to the map by the caller; in_hi - in_lo < SS_BROWS)
__device__ __forceinline__ Band load_band(const StemSparseArgs& a, const BandLds& L, int img, int in_lo, int in_hi, int tid) {
    Band b;
    b.in_lo = in_lo; b.in_hi = in_hi;
    const int* rs = a.row_start + (long)img * a.H;
    const int k0 = rs[in_lo];
    b.rec = a.rec + k0;
    b.nrec = rs[in_hi + 1] - k0;
    b.in_lds = b.nrec <= SS_HCAP;
    const int nrows = in_hi - in_lo + 1;
    __syncthreads();                                          // the previous band's readers are done
    for (int i = tid; i < nrows * L.bw; i += 256) L.bits[i] = 0u;
    if (tid <= nrows) L.rowbase[tid] = rs[in_lo + tid] - k0;
    __syncthreads();
    for (int k = tid; k < b.nrec; k += 256) {
        const HitRec r{b.rec[k]};
        if (b.in_lds) L.recs[k] = r.r;
        if (!r.dead()) {
            const int yr = r.y() - in_lo, x = r.x();
            atomicOr(&L.bits[yr * L.bw + 1 + (x >> 5)], 1u << (x & 31));
            L.map[yr * L.W + x] = (unsigned short)(k - L.rowbase[yr]);
        }
    }
    __syncthreads();
    return b;
}

// bits [x0, x0 + n) (n <= 16) of pixel row y; rows outside the band and columns outside the map read as zero
__device__ __forceinline__ unsigned rowbits(const BandLds& L, const Band& b, int y, int x0, int n) {
    if (y < b.in_lo || y > b.in_hi) return 0u;
    const unsigned* row = L.bits + (y - b.in_lo) * L.bw + 1;
    const int w = x0 >> 5, sh = x0 & 31;                      // x0 >= -3: w >= -1 (the zero word in front)
    const unsigned long long v = (unsigned long long)row[w] | ((unsigned long long)row[w + 1] << 32);
    return (unsigned)(v >> sh) & ((1u << n) - 1u);
}

// The window walk.  for_each_row_hit: the hits of pixel row y in the columns [x0, x0 + cols) (cols <= 16), f(wx, v[3]) per hit at
// (y, x0 + wx), columns ascending.  for_each_hit: the window rows [y0, y0 + rows) in ascending order, f(wy, wx, v[3]).  This is the
// order every FMA chain and LDS accumulation of the passes is defined by.
template <typename F>
__device__ __forceinline__ void for_each_row_hit(const BandLds& L, const Band& b, int y, int x0, int cols, F f) {
    unsigned m = rowbits(L, b, y, x0, cols);
    while (m) {
        const int wx = __ffs(m) - 1;
        m &= m - 1;
        const int yr = y - b.in_lo;
        const int k = L.rowbase[yr] + (int)L.map[yr * L.W + x0 + wx];
        const HitRec r{b.in_lds ? L.recs[k] : b.rec[k]};
        float v[3];
        r.values(v);
        f(wx, v);
    }
}
template <typename F>
__device__ __forceinline__ void for_each_hit(const BandLds& L, const Band& b, int y0, int x0, int rows, int cols, F f) {
#pragma unroll 1
    for (int wy = 0; wy < rows; ++wy) for_each_row_hit(L, b, y0 + wy, x0, cols, [&](int wx, const float (&v)[3]) { f(wy, wx, v); });
}

// ordered worklist of the candidates [0, n) for which `test(i)` holds: wlist[.] = i ascending; returns the count (uniform)
template <typename F>
__device__ __forceinline__ int build_worklist(unsigned short* wlist, int* cnt, int n, int tid, F test) {
    const int lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int r0 = 0; r0 < n; r0 += 256) {
        const int i = r0 + tid;
        const bool has = i < n && test(i);
        const unsigned long long m = __ballot(has);
        if (lane == 0) cnt[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += cnt[w];
        if (has) wlist[off + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)i;
        base += cnt[0] + cnt[1] + cnt[2] + cnt[3];
        __syncthreads();
    }
    return base;
}

// The pass driver.  The `extent` x `width` output cells of a map -- conv0 positions or pooled pixels; the window of cell (r, c) is
// WIN x WIN input pixels from (STRIDE*r - 3, STRIDE*c - 3) -- are cut into bands of ROWS rows; a work unit is (map, split) = one of
// nsplit ranges of a map's bands, and the workgroups share the nunits units.  Per band: load it, collect the cells whose window holds
// a hit in L.wlist (ascending; with FLAGS, L.flag[cell] says the same per cell), then body(img, band, row0, nrows, nw) with nw the
// length of the worklist.  All threads of the workgroup run every body call.
struct Conv0Cells { static constexpr int ROWS = SS_CROWS, WIN = 7, STRIDE = 2; static constexpr bool FLAGS = false; };
struct PoolCells { static constexpr int ROWS = SS_PROWS, WIN = 11, STRIDE = 4; static constexpr bool FLAGS = true; };
template <typename Cells, typename Body>
__device__ __forceinline__ void for_each_band(const StemSparseArgs& a, const BandLds& L, int extent, int width, int nsplit, int nunits, int tid,
                                              Body body) {
    constexpr int ROWS = Cells::ROWS, WIN = Cells::WIN, STRIDE = Cells::STRIDE;
    const int nb = (extent + ROWS - 1) / ROWS;
    for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const int img = unit / nsplit, s = unit - img * nsplit;
        const int b0 = (int)((long)s * nb / nsplit), b1 = (int)((long)(s + 1) * nb / nsplit);
        for (int bi = b0; bi < b1; ++bi) {
            const int r0 = bi * ROWS, nr = min(ROWS, extent - r0);
            const Band b = load_band(a, L, img, max(0, STRIDE * r0 - 3), min(a.H - 1, STRIDE * (r0 + nr - 1) + WIN - 4), tid);
            const int nw = build_worklist(L.wlist, L.cnt, nr * width, tid, [&](int i) {
                const int r = r0 + i / width, c = i % width;
                unsigned any = 0;
#pragma unroll
                for (int wy = 0; wy < WIN; ++wy) any |= rowbits(L, b, STRIDE * r - 3 + wy, STRIDE * c - 3, WIN);
                if (Cells::FLAGS) L.flag[i] = any != 0u;
                return any != 0u;
            });
            body(img, b, r0, nr, nw);
        }
    }
}

// conv0 weights -> LDS [147][64] bf16 (k = (ky*7 + kx)*3 + c; packed as k = (ky*7 + kx)*Cpix + c: zero for c >= Cpix), bias
__device__ __forceinline__ void load_weights(const StemSparseArgs& a, const BandLds& L, int tid) {
    const bf16* Wk = reinterpret_cast<const bf16*>(a.Wk);
    for (int i = tid; i < SS_K * SS_N; i += 256) {
        const int k = i >> 6, n = i & 63, tap = k / 3, c = k - tap * 3;
        L.wl[i] = c < a.Cpix ? Wk[(long)n * a.Kp + tap * a.Cpix + c] : (bf16)0;
    }
    if (tid < SS_N) L.bias[tid] = a.bias[tid];
}

// this thread's eight channels [c8*8, c8*8 + 8) of a per-channel table
__device__ __forceinline__ void take8(const float* tab, int c8, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tab[c8 * 8 + j];
}

// acc[j] += v[c] * w[tap*3 + c][c8*8 + j]
__device__ __forceinline__ void fma_tap(const bf16* wl, int tap, int c8, const float (&v)[3], float (&acc)[8]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const u16x8 w = *reinterpret_cast<const u16x8*>(wl + (tap * 3 + c) * SS_N + c8 * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(v[c], bf2f(w[j]), acc[j]);
    }
}

// conv0 output of position (h, w) of the map, channels [c8*8, c8*8 + 8): bias + the hits of its 7x7 window in window order
__device__ __forceinline__ void conv0_at(const BandLds& L, const Band& b, int h, int w, int c8, float (&acc)[8]) {
    take8(L.bias, c8, acc);
    for_each_hit(L, b, 2 * h - 3, 2 * w - 3, 7, 7, [&](int ky, int kx, const float (&v)[3]) { fma_tap(L.wl, ky * 7 + kx, c8, v, acc); });
}

// statistics row of a forward pass: the workgroup's per-channel sum and sum of squares over the cells it evaluated (s) and over its
// n_empty other cells (thread 0's count), which all hold `ev` (thread c < 64: the value of channel c)
__device__ __forceinline__ void store_stats_part(const StemSparseArgs& a, const BandLds& L, double* red, double (&s)[2][8], long n_empty, double ev,
                                                 int tid) {
    __syncthreads();
    if (tid == 0) reinterpret_cast<long*>(L.cnt)[1] = n_empty;
    double tot[2];
    channel_fold(s, red, tid, tot);
    if (tid < SS_N) {
        const double ne = (double)reinterpret_cast<long*>(L.cnt)[1];
        a.part[((long)blockIdx.x * SS_N + tid) * 2] = tot[0] + ne * ev;
        a.part[((long)blockIdx.x * SS_N + tid) * 2 + 1] = tot[1] + ne * ev * ev;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// pass 1 (train): per-channel sum and sum of squares of the conv0 output over all Hc x Wc positions of every map
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void k_stem_sparse_stats(const StemSparseArgs a, int nsplit, int nunits) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PassLds lay = pass_lds(StemPass::Stats, a.W, a.Wc, a.Wo);
    const BandLds L = band_lds(smem, lay, a.W);
    const int tid = threadIdx.x, c8 = tid & 7;
    load_weights(a, L, tid);
    double s[2][8] = {};                                     // sum, sum of squares over the non-empty positions
    long n_empty = 0;                                        // counted by thread 0 only
    for_each_band<Conv0Cells>(a, L, a.Hc, a.Wc, nsplit, nunits, tid, [&](int img, const Band& b, int h0, int nh, int nw) {
        if (tid == 0) n_empty += nh * a.Wc - nw;
        for (int t = tid; t < nw * 8; t += 256) {
            const int i = L.wlist[t >> 3];
            float acc[8];
            conv0_at(L, b, h0 + i / a.Wc, i % a.Wc, c8, acc);
#pragma unroll
            for (int j = 0; j < 8; ++j) { s[0][j] += acc[j]; s[1][j] += (double)acc[j] * acc[j]; }
        }
    });
    store_stats_part(a, L, lds_at<double>(smem, lay.red), s, n_empty, (double)L.bias[tid & 63], tid);   // empty positions hold the bias exactly
}

// ---------------------------------------------------------------------------------------------------------------------
// pass 2: pooled, activated map.  Band = 4 pooled rows (23 input rows).  A pooled pixel covers conv0 rows 2q..2q+2 = input rows
// 4q-3 .. 4q+7; if that 11 x 11 window holds no hit its value is avgpool of nine copies of prelu(bn(bias)).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void k_stem_sparse_pool(const StemSparseArgs a, int nsplit, int nunits) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PassLds lay = pass_lds(StemPass::Pool, a.W, a.Wc, a.Wo);
    const BandLds L = band_lds(smem, lay, a.W);
    float* tab = lds_at<float>(smem, lay.tab);                             // BatchNorm0 scale, shift; PReLU0 slope
    bf16* cvec = lds_at<bf16>(smem, lay.cvec);
    const int tid = threadIdx.x, c8 = tid & 7;
    load_weights(a, L, tid);
    if (tid < SS_N) { tab[tid] = a.sc[tid]; tab[64 + tid] = a.sh[tid]; tab[128 + tid] = a.sl[tid]; }
    __syncthreads();
    if (tid < SS_N) {
        const float ae = prelu(fmaf(L.bias[tid], tab[tid], tab[64 + tid]), tab[128 + tid]);
        float s = 0.f;
        for (int i = 0; i < 9; ++i) s += ae;                              // the same nine additions the general path makes
        cvec[tid] = f2bf(s * (1.0f / 9.0f));
    }
    float sc[8], sh[8], sl[8];
    __syncthreads();
    take8(tab, c8, sc); take8(tab + 64, c8, sh); take8(tab + 128, c8, sl);
    bf16* __restrict__ Out = reinterpret_cast<bf16*>(a.Out);
    double s[2][8] = {};                                                  // sum, sum of squares of the stored non-constant pixels
    long n_empty = 0;
    for_each_band<PoolCells>(a, L, a.Ho, a.Wo, nsplit, nunits, tid, [&](int img, const Band& b, int q0, int nq, int nw) {
        const int npix = nq * a.Wo;
        if (tid == 0) n_empty += npix - nw;
        // non-empty pooled pixels: the nine conv0 positions from the hits of the 11 x 11 window, window order
        for (int t = tid; t < nw * 8; t += 256) {
            const int i = L.wlist[t >> 3];
            const int qy = q0 + i / a.Wo, qx = i % a.Wo;
            float acc[9][8];
#pragma unroll
            for (int ps = 0; ps < 9; ++ps) take8(L.bias, c8, acc[ps]);
            for_each_hit(L, b, 4 * qy - 3, 4 * qx - 3, 11, 11, [&](int wy, int wx, const float (&v)[3]) {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int ky = wy - 2 * dy;
                    if (ky < 0 || ky > 6) continue;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int kx = wx - 2 * dx;
                        if (kx < 0 || kx > 6) continue;
                        fma_tap(L.wl, ky * 7 + kx, c8, v, acc[dy * 3 + dx]);
                    }
                }
            });
            float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int ps = 0; ps < 9; ++ps)
#pragma unroll
                for (int j = 0; j < 8; ++j) p[j] += prelu(fmaf(acc[ps][j], sc[j], sh[j]), sl[j]);
            u16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                o[j] = f2bf(p[j] * (1.0f / 9.0f));
                const double x = (double)bf2f(o[j]);
                s[0][j] += x; s[1][j] += x * x;
            }
            *reinterpret_cast<u16x8*>(Out + (((long)img * a.Ho + qy) * a.Wo + qx) * a.ldo + c8 * 8) = o;
        }
        // empty pooled pixels: the constant vector
        const u16x8 cv = *reinterpret_cast<const u16x8*>(cvec + c8 * 8);
        for (int t = tid; t < npix * 8; t += 256) {
            const int i = t >> 3;
            if (!L.flag[i]) *reinterpret_cast<u16x8*>(Out + (((long)img * a.Ho + q0 + i / a.Wo) * a.Wo + i % a.Wo) * a.ldo + c8 * 8) = cv;
        }
    });
    if (a.part != nullptr) store_stats_part(a, L, lds_at<double>(smem, lay.red), s, n_empty, (double)bf2f(cvec[tid & 63]), tid);
}

// ---------------------------------------------------------------------------------------------------------------------
// backward.  dz[p] = 1/9 sum over the <= 4 pooled pixels q whose 3x3/2 window holds position p of eff[q] = G[q] + P*D[q] + Q.
// sums:  (dU, dU*x, dz*min(u,0)) per channel: explicit over the non-empty positions; over the empty ones (x = bias, u = u_e)
//        they are slope_e * S, bias * slope_e * S and min(u_e, 0) * S with S = sum over empty positions of dz = sum_q eff[q] - sum over
//        non-empty positions of dz (every pooled pixel spreads eff/9 over nine existing positions).
// wgrad: eff0 = sc*dU + P0*x + Q0 of the non-empty positions (chunks of 64 in LDS), contracted with the hits of their windows:
//        dW0[n][ky][kx][c] += v[hit][c] * eff0[p][n]; wave w owns the kernel rows ky = 2w, 2w + 1 of an LDS accumulator [147][64].
// ---------------------------------------------------------------------------------------------------------------------
struct BwdTab { float sc[8], sh[8], sl[8], P[8], Q[8]; };    // a thread's eight channels of BN0 (scale, shift), PReLU0 slope, the pooled map's (P, Q)

// stages the five tables in LDS ([5][64] from ctab) and hands every thread its channels; the caller's own LDS writes ride on the barrier
__device__ __forceinline__ void load_bwd_tab(const StemSparseArgs& a, float* ctab, int tid, BwdTab& T) {
    if (tid < SS_N) {
        ctab[tid] = a.sc[tid]; ctab[64 + tid] = a.sh[tid]; ctab[128 + tid] = a.sl[tid];
        ctab[192 + tid] = a.e.P[tid]; ctab[256 + tid] = a.e.Q[tid];
    }
    __syncthreads();
    const int c8 = tid & 7;
    take8(ctab, c8, T.sc); take8(ctab + 64, c8, T.sh); take8(ctab + 128, c8, T.sl); take8(ctab + 192, c8, T.P); take8(ctab + 256, c8, T.Q);
}

// gradient of pooled pixel (qy, qx), this thread's 8 channels
__device__ __forceinline__ void eff_at(const StemSparseArgs& a, const BwdTab& T, int img, int qy, int qx, int c8, float (&e8)[8]) {
    const long mo = ((long)img * a.Ho + qy) * a.Wo + qx;
    float gv[8], dv[8];
    load8<bf16>(reinterpret_cast<const bf16*>(a.e.G) + mo * a.e.ldg + c8 * 8, gv);
    load8<bf16>(reinterpret_cast<const bf16*>(a.e.X) + mo * a.e.ldx + c8 * 8, dv);
#pragma unroll
    for (int j = 0; j < 8; ++j) e8[j] = gv[j] + T.P[j] * dv[j] + T.Q[j];
}

// dz of conv0 position (h, w): windows containing row h are ho = h/2 and, when h is even, h/2 - 1 (rows 2ho .. 2ho + 2)
__device__ __forceinline__ void dz_at(const StemSparseArgs& a, const BwdTab& T, int img, int h, int w, int c8, float (&dz)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) dz[j] = 0.f;
#pragma unroll 1
    for (int d = 0; d < 4; ++d) {
        const int dy = d >> 1, dx = d & 1;
        const int qy = h / 2 - dy, qx = w / 2 - dx;
        if ((dy == 1 && (h & 1)) || qy < 0 || qy >= a.Ho || (dx == 1 && (w & 1)) || qx < 0 || qx >= a.Wo) continue;
        float e8[8];
        eff_at(a, T, img, qy, qx, c8, e8);
#pragma unroll
        for (int j = 0; j < 8; ++j) dz[j] += e8[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) dz[j] *= (1.0f / 9.0f);
}

// what both backward passes need of conv0 position (h, w): its output x, the gradient dz that pooling hands it, u = BN0(x), du = dU
__device__ __forceinline__ void conv0_bwd_at(const StemSparseArgs& a, const BandLds& L, const Band& b, const BwdTab& T, int img, int h, int w,
                                             int c8, float (&x)[8], float (&dz)[8], float (&u)[8], float (&du)[8]) {
    conv0_at(L, b, h, w, c8, x);
    dz_at(a, T, img, h, w, c8, dz);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        u[j] = fmaf(x[j], T.sc[j], T.sh[j]);
        du[j] = u[j] > 0.f ? dz[j] : T.sl[j] * dz[j];
    }
}

__global__ __launch_bounds__(256, 2) void k_stem_sparse_bwd_sums(const StemSparseArgs a, int nsplit, int nunits) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PassLds lay = pass_lds(StemPass::BwdSums, a.W, a.Wc, a.Wo);
    const BandLds L = band_lds(smem, lay, a.W);
    float* ctab = lds_at<float>(smem, lay.tab);
    const int tid = threadIdx.x, c8 = tid & 7;
    load_weights(a, L, tid);
    BwdTab T;
    load_bwd_tab(a, ctab, tid, T);
    double s[SUMS_NS][8] = {};      // non-empty positions: sums dU, dU*x, dz*min(u,0), dz;  pooled pixels: eff
    // sum_q eff[q] over every unit's share of the pooled rows (same split fractions as the bands)
    for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const int img = unit / nsplit, sp = unit - img * nsplit;
        const int qa = (int)((long)sp * a.Ho / nsplit), qb = (int)((long)(sp + 1) * a.Ho / nsplit);
#pragma unroll 1
        for (int t = tid; t < (qb - qa) * a.Wo * 8; t += 256) {
            const int i = t >> 3;
            float e8[8];
            eff_at(a, T, img, qa + i / a.Wo, i % a.Wo, c8, e8);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[4][j] += e8[j];
        }
    }
    for_each_band<Conv0Cells>(a, L, a.Hc, a.Wc, nsplit, nunits, tid, [&](int img, const Band& b, int h0, int nh, int nw) {
#pragma unroll 1
        for (int t = tid; t < nw * 8; t += 256) {
            const int i = L.wlist[t >> 3];
            float x[8], dz[8], u[8], du[8];
            conv0_bwd_at(a, L, b, T, img, h0 + i / a.Wc, i % a.Wc, c8, x, dz, u, du);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s[0][j] += du[j]; s[1][j] += (double)du[j] * x[j]; s[2][j] += u[j] > 0.f ? 0.f : dz[j] * u[j]; s[3][j] += dz[j];
            }
        }
    });
    __syncthreads();                                                       // the last band's records are read: the fold may overwrite them
    double tot[SUMS_NS];
    channel_fold(s, lds_at<double>(smem, lay.red), tid, tot);
    if (tid < SS_N) {
        const double bb = (double)L.bias[tid], ue = (double)fmaf(L.bias[tid], ctab[tid], ctab[64 + tid]);
        const double slope_e = ue > 0.0 ? 1.0 : (double)ctab[128 + tid];
        const double S = tot[4] - tot[3];                                  // sum of dz over the empty positions
        double* o = a.part + ((long)blockIdx.x * SS_N + tid) * 3;
        o[0] = tot[0] + slope_e * S;
        o[1] = tot[1] + bb * slope_e * S;
        o[2] = tot[2] + (ue > 0.0 ? 0.0 : ue * S);
    }
}

__global__ __launch_bounds__(256, 2) void k_stem_sparse_bwd_wgrad(const StemSparseArgs a, int nsplit, int nunits) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PassLds lay = pass_lds(StemPass::BwdWgrad, a.W, a.Wc, a.Wo);
    const BandLds L = band_lds(smem, lay, a.W);
    float* ctab = lds_at<float>(smem, lay.tab);
    float* eff0 = lds_at<float>(smem, lay.eff0);
    float* wsum = lds_at<float>(smem, lay.wsum);
    const int tid = threadIdx.x, c8 = tid & 7, lane = tid & 63, wave = tid >> 6;
    load_weights(a, L, tid);
    if (tid < SS_N) { ctab[320 + tid] = a.P0[tid]; ctab[384 + tid] = a.Q0[tid]; }      // BatchNorm0's (P, Q)
    for (int i = tid; i < SS_K * SS_N; i += 256) wsum[i] = 0.f;
    BwdTab T;
    load_bwd_tab(a, ctab, tid, T);
    float p0[8], q0[8];
    take8(ctab + 320, c8, p0); take8(ctab + 384, c8, q0);
    for_each_band<Conv0Cells>(a, L, a.Hc, a.Wc, nsplit, nunits, tid, [&](int img, const Band& b, int h0, int nh, int nw) {
        for (int c0 = 0; c0 < nw; c0 += SS_CHUNK) {
            const int cn = min(SS_CHUNK, nw - c0);
#pragma unroll 1
            for (int t = tid; t < cn * 8; t += 256) {
                const int i = L.wlist[c0 + (t >> 3)];
                float x[8], dz[8], u[8], du[8], ef[8];
                conv0_bwd_at(a, L, b, T, img, h0 + i / a.Wc, i % a.Wc, c8, x, dz, u, du);
#pragma unroll
                for (int j = 0; j < 8; ++j) ef[j] = fmaf(T.sc[j], du[j], fmaf(p0[j], x[j], q0[j]));
                float4* o = reinterpret_cast<float4*>(eff0 + (t >> 3) * SS_N + c8 * 8);
                o[0] = make_float4(ef[0], ef[1], ef[2], ef[3]); o[1] = make_float4(ef[4], ef[5], ef[6], ef[7]);
            }
            __syncthreads();
            // every wave walks the chunk's (position, hit) pairs in the same order and adds the pairs of its own kernel rows
            for (int s = 0; s < cn; ++s) {
                const int i = L.wlist[c0 + s];
                const int h = h0 + i / a.Wc, w = i % a.Wc;
                const float ef = eff0[s * SS_N + lane];
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int ky = 2 * wave + kk;
                    if (ky > 6) continue;
                    for_each_row_hit(L, b, 2 * h - 3 + ky, 2 * w - 3, 7, [&](int kx, const float (&v)[3]) {
                        float* d = wsum + ((ky * 7 + kx) * 3) * SS_N + lane;
                        d[0] = fmaf(v[0], ef, d[0]); d[SS_N] = fmaf(v[1], ef, d[SS_N]); d[2 * SS_N] = fmaf(v[2], ef, d[2 * SS_N]);
                    });
                }
            }
            __syncthreads();
        }
    });
    __syncthreads();
    float* out = a.slab + (long)blockIdx.x * SS_N * a.Kp;                  // slab[block][n][Kp], k = (ky*7 + kx)*Cpix + c
    for (int i = tid; i < SS_N * a.Kp; i += 256) {
        const int nn = i / a.Kp, k = i - nn * a.Kp, tap = k / a.Cpix, c = k - tap * a.Cpix;
        out[i] = tap < 49 ? wsum[(tap * 3 + c) * SS_N + nn] : 0.f;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
long stem_sparse_hit_capacity(int n_img) { return (long)n_img * 8192; }                 // average occupancy up to 7 % of a 400 x 280 map
long stem_sparse_index_bytes(int n_img, int H, int W) {
    const long nbins = (long)n_img * H;
    return round_up((nbins + 1) * 4, 256) + round_up(nbins * 4, 256) + round_up(stem_sparse_hit_capacity(n_img) * 16, 256);
}
void stem_sparse_carve(StemSparseArgs& a, char* base) {
    const long nbins = (long)a.n_img * a.H;
    a.row_start = reinterpret_cast<int*>(base); base += round_up((nbins + 1) * 4, 256);
    a.row_fill = reinterpret_cast<int*>(base); base += round_up(nbins * 4, 256);
    a.rec = reinterpret_cast<uint4*>(base);
}
bool stem_sparse_ok(int mode, int in_ch, int init_ch, int H, int W, int value_mode, long nnz, int n_img, long ldo) {
    return conv3x3_tile_enabled() && mode == MODE_BF16 && in_ch >= 1 && in_ch <= 3 && init_ch == SS_N && value_mode >= 0 && value_mode <= 2 &&
           nnz <= stem_sparse_hit_capacity(n_img) && H >= 11 && W >= 11 && H <= 32767 && W <= SS_WMAX && (ldo & 7) == 0 &&
           (long)n_img * H < (1L << 30);
}
StemPassPlan stem_sparse_plan(const StemSparseArgs& a, StemPass pass) {
    StemPassPlan p;
    p.rows = pass == StemPass::Pool ? SS_PROWS : SS_CROWS;
    p.nbands = cdiv(pass == StemPass::Pool ? a.Ho : a.Hc, p.rows);
    const int ns = (512 + a.n_img - 1) / a.n_img;             // enough units to fill the chip twice, never more splits than bands
    p.nsplit = ns < 1 ? 1 : ns > p.nbands ? p.nbands : ns;
    p.nunits = a.n_img * p.nsplit;
    p.grid = p.nunits < 1024 ? p.nunits : 1024;
    return p;
}

int stem_sparse_index(const StemSparseArgs& a, hipStream_t st) {
    const long nbins = (long)a.n_img * a.H;
    TCVN_CHECK(hipMemsetAsync(a.row_fill, 0, (size_t)nbins * 4, st));
    if (a.nnz > 0) {
        hipLaunchKernelGGL(k_stem_index_count, dim3(cdiv(a.nnz, 256)), dim3(256), 0, st, a);
        TCVN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_stem_index_scan, dim3(1), dim3(1024), 0, st, a, (int)nbins);
    TCVN_LAUNCH_CHECK();
    if (a.nnz > 0) {
        hipLaunchKernelGGL(k_stem_index_fill, dim3(cdiv(a.nnz, 256)), dim3(256), 0, st, a);
        TCVN_LAUNCH_CHECK();
        // the number of records (hits inside the maps) is row_start[nbins]: the kernel reads it on the device
        hipLaunchKernelGGL(k_stem_index_dedup, dim3(cdiv(a.nnz, 256)), dim3(256), 0, st, a, a.row_start + nbins);
        TCVN_LAUNCH_CHECK();
    }
    return 0;
}
// one pass: its grid from the plan, its LDS from the layout record
static int launch_pass(void (*kernel)(const StemSparseArgs, int, int), StemPass pass, const char* label, double flops, double bytes,
                       const StemSparseArgs& a, hipStream_t st) {
    const StemPassPlan p = stem_sparse_plan(a, pass);
    const int smem = pass_lds(pass, a.W, a.Wc, a.Wo).total;
    if (smem > SS_LDS_MAX) return -2;
    TCVN_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SS_LDS_MAX));
    ProfScope ps(label, flops, bytes, st);
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(256), smem, st, a, p.nsplit, p.nunits);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int stem_sparse_stats(const StemSparseArgs& a, hipStream_t st) {
    return launch_pass(k_stem_sparse_stats, StemPass::Stats, "k_stem_sparse_stats", 2.0 * a.nnz * 12.25 * a.Cpix * SS_N, (double)a.nnz * 16.0, a, st);
}
int stem_sparse_pool(const StemSparseArgs& a, hipStream_t st) {
    return launch_pass(k_stem_sparse_pool, StemPass::Pool, "k_stem_sparse_pool", 2.0 * a.nnz * 12.25 * a.Cpix * SS_N * 2.25,
                       (double)a.n_img * a.Ho * a.Wo * SS_N * 2.0 + (double)a.nnz * 16.0, a, st);
}
int stem_sparse_bwd(const StemSparseArgs& a, StemPass pass, hipStream_t st) {
    const double bytes = (double)a.n_img * a.Ho * a.Wo * SS_N * 2.0 * 2.0 + (double)a.nnz * 16.0;      // (G, x) of the pooled map + the index
    if (pass == StemPass::BwdSums) return launch_pass(k_stem_sparse_bwd_sums, pass, "k_stem_sparse_bwd<sums>", 2.0 * a.nnz * 12.25 * a.Cpix * SS_N, bytes, a, st);
    if (pass != StemPass::BwdWgrad) return -1;
    const int nb = stem_sparse_plan(a, pass).grid;
    if (a.slab == nullptr || (long)nb * SS_N * a.Kp * 4 > a.slab_bytes || a.Kp < 49 * a.Cpix) return -3;
    int rc;
    if ((rc = launch_pass(k_stem_sparse_bwd_wgrad, pass, "k_stem_sparse_bwd<wgrad>", 4.0 * a.nnz * 12.25 * a.Cpix * SS_N, bytes, a, st))) return rc;
    return slab_reduce(a.slab, nb, (long)SS_N * a.Kp, a.dWk, st);
}

}  // namespace tcvn
