// Padded-tile machinery of the bf16 3x3 kernels (forward, dgrad, wgrad).
//
// Pixels are addressed in a zero-padded index space: image n, padded row hp in [0,H+2), padded column wp in [0,W+2);
//   g = (n*(H+2) + hp)*(W+2) + wp ;  real pixel <=> 1<=hp<=H && 1<=wp<=W ;  m = (n*H + hp-1)*W + wp-1.
// In that space a 3x3 tap is the constant shift (ky-1)*(W+2) + (kx-1) and every out-of-image neighbour is an explicit
// zero row, so a workgroup stages ONE transformed (BatchNorm+PReLU applied, bf16) image of 128 + 2*(W+3) consecutive
// padded positions in LDS and all nine taps read it with plain row offsets: the transform runs once per element instead
// of once per tap, and no per-tap validity masks exist.  Useful fraction of the padded space: H*W/((H+2)*(W+2)) (95 % at
// 99x69).  LDS rows are 128 channels = 256 B (or 32 channels = 64 B for gradient images), 16-B chunks XOR-swizzled so
// that the 16 lanes of a ds_read_b128 group (consecutive rows, same chunk) hit 16 different bank slots.
#pragma once
#include "tcvn_ops.h"

namespace tcvn {
namespace t3 {

constexpr int TP = 128;                       // padded positions per tile (4 waves x 32 rows)

struct PadGeom {
    int n, H, W, Hp, Wp, halo;                // halo = Wp + 1 rows on each side
    long gtot;                                // n*Hp*Wp
    __host__ __device__ constexpr PadGeom(int n_, int H_, int W_) : n(n_), H(H_), W(W_), Hp(H_ + 2), Wp(W_ + 2), halo(W_ + 3),
                                                                     gtot((long)n_ * (H_ + 2) * (W_ + 2)) {}
    __host__ __device__ constexpr int rows() const { return TP + 2 * halo; }
    __host__ __device__ constexpr long tiles() const { return (gtot + TP - 1) / TP; }
};

struct Pos { int img, hp, wp; };

__device__ __forceinline__ Pos decode(const PadGeom& q, long g) {
    Pos p;
    const long row = g / q.Wp;
    p.wp = (int)(g - row * q.Wp);
    p.img = (int)(row / q.Hp);
    p.hp = (int)(row - (long)p.img * q.Hp);
    return p;
}
__device__ __forceinline__ void advance(const PadGeom& q, Pos& p, int d) {    // d >= 0, any size
    p.wp += d;
    while (p.wp >= q.Wp) { p.wp -= q.Wp; ++p.hp; }
    while (p.hp >= q.Hp) { p.hp -= q.Hp; ++p.img; }
}
// pixel index of a padded position or -1
__device__ __forceinline__ long pixel(const PadGeom& q, const Pos& p, long g) {
    if (g < 0 || g >= q.gtot || p.hp < 1 || p.hp > q.H || p.wp < 1 || p.wp > q.W) return -1;
    return ((long)p.img * q.H + (p.hp - 1)) * q.W + (p.wp - 1);
}

// byte offset of 16-B chunk `c` of LDS row `r`: 256-B rows (128 ch) and 64-B rows (32 ch)
__device__ __forceinline__ int off256(int r, int c) { return r * 256 + ((c ^ (r & 15)) << 4); }
__device__ __forceinline__ int off64(int r, int c) { return r * 64 + ((c ^ ((r >> 2) & 3)) << 4); }

__device__ __forceinline__ u16x8 pack8(const float v[8]) {
    u16x8 p;
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = f2bf(v[j]);
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// Shared by the three bf16 tile files (conv3x3_fwd_tile.hip, conv3x3_wgrad_tile.hip, conv3x3_dgrad_tile.hip).  Only text that compiles
// to the same instructions as the copies it replaced lives here; where a kernel keeps a copy of its own, a comment there says why.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fdiv(int a, int d, float inv, int& rem) {     // a in [0, 2^24)
    int q = (int)((float)a * inv);
    rem = a - q * d;
    if (rem < 0) { --q; rem += d; }
    else if (rem >= d) { ++q; rem -= d; }
    return q;
}
// pixel index of padded position g (or -1)
__device__ __forceinline__ int pix_of(const PadGeom& q, int g, float invWp, float invHp) {
    if (g < 0 || g >= (int)q.gtot) return -1;
    int wp, hp;
    const int row = fdiv(g, q.Wp, invWp, wp);
    const int img = fdiv(row, q.Hp, invHp, hp);
    if (hp < 1 || hp > q.H || wp < 1 || wp > q.W) return -1;
    return (img * q.H + (hp - 1)) * q.W + (wp - 1);
}

// eight consecutive floats from LDS as two 16-B reads
__device__ __forceinline__ void ld8(const float* __restrict__ p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// Consecutive-tile partition of a persistent grid: this workgroup owns tiles [t0, t1), the first ntiles % gridDim.x workgroups one more
// than the others.  Returns g_org, the padded position of row 0 of the workgroup's row space (first image row of its first tile).
// (k_conv3x3_dgrad3_bf16 keeps its own copy, which yields the tile COUNT: derived from t1 - t0, or t1 from the count, the sums associate
// differently and the register allocation of the whole kernel follows.)
__device__ __forceinline__ int tile_span(const PadGeom& q, int ntiles, int& t0, int& t1) {
    const int nb = gridDim.x, per = ntiles / nb, rem = ntiles % nb;
    t0 = blockIdx.x * per + min((int)blockIdx.x, rem);
    t1 = t0 + per + ((int)blockIdx.x < rem ? 1 : 0);
    return t0 * TP - q.halo;
}
// Pixel-table entries of rows [row0, row0 + n) of that row space, by thread t of nt: entry of a row = row & (TBL - 1).  g_org comes by
// reference, as the kernels' fill_rows lambdas captured it before this loop was shared: by value the loop is hoisted differently and the
// kernels' instruction streams change.
template <int TBL>
__device__ __forceinline__ void ring_tbl_fill(int* tbl, const PadGeom& q, const int& g_org, int row0, int n, int t, int nt, float invWp, float invHp) {
    for (int i = t; i < n; i += nt) tbl[(row0 + i) & (TBL - 1)] = pix_of(q, g_org + row0 + i, invWp, invHp);
}

// In-LDS activation of one landed 16-B chunk (ConvFwdArgs::act_fused): the same arithmetic as k_act_bf16 (fp32 fma, PReLU, one
// rounding to bf16), so a fused launch and a materialised one stage bit-identical images.
struct Act8 { float sc[8], sh[8], sl[8]; };
__device__ __forceinline__ Act8 act8_load(const float* __restrict__ xtab, int cc) {      // xtab: [3][128] floats in LDS
    Act8 t;
    ld8(xtab + cc * 8, t.sc);
    ld8(xtab + 128 + cc * 8, t.sh);
    ld8(xtab + 256 + cc * 8, t.sl);
    return t;
}
__device__ __forceinline__ u16x8 act8_apply(const u16x8 v, const Act8& t) {
    u16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(prelu(fmaf(bf2f(v[j]), t.sc[j], t.sh[j]), t.sl[j]));
    return o;
}
__device__ __forceinline__ void act_tab_fill(float* __restrict__ xtab, const float* __restrict__ sc, const float* __restrict__ sh,
                                             const float* __restrict__ sl, int tid, int nthreads) {
    for (int i = tid; i < 128; i += nthreads) { xtab[i] = sc[i]; xtab[128 + i] = sh[i]; xtab[256 + i] = sl[i]; }
}

// Phase counters of the role-split kernels (validation build only): wave-cycles per phase into the kernel's local `ph[16]`, which every
// 16th workgroup adds to the kernel's global counters (tcvn_debug_pair_phases / tcvn_debug_wgrad_phases read them)
#ifdef TCVN_DEBUG_KNOBS
#define TILE_PH_T0() unsigned long long ph_t = clock64()
#define TILE_PH(i) do { const unsigned long long n_ = clock64(); ph[i] += n_ - ph_t; ph_t = n_; } while (0)
#else
#define TILE_PH_T0() do {} while (0)
#define TILE_PH(i) do {} while (0)
#endif

inline int tile_grid(long ntiles) {            // one persistent workgroup per CU
    static_assert(256 <= LF_MAX_ADDERS, "bn_lf.h: more workgroups would add to one channel than its range guard allows for (the forward pair kernel's grid)");
    if (ntiles >= 256) return 256;
    if (ntiles >= 8) return (int)(ntiles / 8 * 8);
    return (int)ntiles;
}
inline int tile_grid2(long ntiles) {           // two workgroups per CU
    if (ntiles >= 512) return 512;
    if (ntiles >= 8) return (int)(ntiles / 8 * 8);
    return (int)ntiles;
}

inline PadGeom geom_of(int M, int H, int W) { return PadGeom(M / (H * W), H, W); }      // n_img is recovered from M = n*H*W

}  // namespace t3
}  // namespace tcvn
