// HBM-bound helper kernels of the DenseNet backward path.
#include "tcvn_ops.h"
#include "bn_link.h"

namespace tcvn {

namespace {

__global__ __launch_bounds__(256) void k_bn_bwd_link(const BnBwdLinkArgs a) { bn_bwd_link_body(a, blockIdx.x, gridDim.x); }

// global-average head backward: dz = dF/HW on every pixel, then PReLU+BN backward bookkeeping of final_norm
constexpr int HP_CJ = 4;     // up to 1024 channels with 256 threads
template <typename T>
__global__ __launch_bounds__(256) void k_head_pool_bwd(const HeadPoolBwdArgs a) {
    const T* X = reinterpret_cast<const T*>(a.X);
    T* Gout = reinterpret_cast<T*>(a.Gout);
    double s1[HP_CJ], s2[HP_CJ], s3[HP_CJ];
#pragma unroll
    for (int j = 0; j < HP_CJ; ++j) { s1[j] = 0; s2[j] = 0; s3[j] = 0; }
    const float inv = 1.0f / (float)a.HW;
    for (int img = blockIdx.x; img < a.n_img; img += gridDim.x) {
#pragma unroll
        for (int j = 0; j < HP_CJ; ++j) {
            const int c = threadIdx.x + 256 * j;
            if (c >= a.C) continue;
            const float sc = a.sc[c], sh = a.sh[c], sl = a.sl[c];
            const float dz = a.dF[(long)img * a.C + c] * inv;
            for (int p = 0; p < a.HW; ++p) {
                const long m = (long)img * a.HW + p;
                const float x = to_f<T>(X[m * a.ldx + c]);
                const float u = fmaf(x, sc, sh);
                const float du = u > 0.f ? dz : sl * dz;
                s1[j] += du; s2[j] += (double)du * x; s3[j] += u > 0.f ? 0.f : dz * u;
                Gout[m * a.ldgo + c] = from_f<T>(sc * du);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < HP_CJ; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c < a.C) {
            double* p = a.part + ((long)blockIdx.x * a.C + c) * 3;
            p[0] = s1[j]; p[1] = s2[j]; p[2] = s3[j];
        }
    }
}

// stem tail backward: AvgPool(3, s2) -> PReLU -> BN0, over the conv0 output pixels
constexpr int PB_CJ = 4;
template <typename T>
__global__ __launch_bounds__(256) void k_pool0_bwd(const Pool0BwdArgs a) {
    __shared__ double red[4][64 * PB_CJ][3];
    const int cl = threadIdx.x & 63, pg = threadIdx.x >> 6;
    const T* X = reinterpret_cast<const T*>(a.X);
    const T* G = reinterpret_cast<const T*>(a.e.G);
    const T* D = reinterpret_cast<const T*>(a.e.X);
    T* DU = reinterpret_cast<T*>(a.DU);
    double s1[PB_CJ], s2[PB_CJ], s3[PB_CJ];
#pragma unroll
    for (int j = 0; j < PB_CJ; ++j) { s1[j] = 0; s2[j] = 0; s3[j] = 0; }
    const long npix = (long)a.n_img * a.Hin * a.Win;
    for (long p = (long)blockIdx.x * 4 + pg; p < npix; p += (long)gridDim.x * 4) {
        const int w = (int)(p % a.Win);
        const int h = (int)((p / a.Win) % a.Hin);
        const long img = p / ((long)a.Win * a.Hin);
        const int ho_lo = max(0, (h - 1) / 2), ho_hi = min(a.Ho - 1, h / 2);     // windows 2*ho <= h <= 2*ho+2
        const int wo_lo = max(0, (w - 1) / 2), wo_hi = min(a.Wo - 1, w / 2);
#pragma unroll
        for (int j = 0; j < PB_CJ; ++j) {
            const int c = cl + 64 * j;
            if (c >= a.C) continue;
            float dz = 0.f;
            for (int ho = ho_lo; ho <= ho_hi; ++ho)
                for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                    if (2 * ho > h || 2 * ho + 2 < h || 2 * wo > w || 2 * wo + 2 < w) continue;
                    const long mo = (img * a.Ho + ho) * a.Wo + wo;
                    dz += to_f<T>(G[mo * a.e.ldg + c]) + a.e.P[c] * to_f<T>(D[mo * a.e.ldx + c]) + a.e.Q[c];
                }
            dz *= (1.0f / 9.0f);
            const float x = to_f<T>(X[p * a.C + c]);
            const float sc = a.sc[c];
            const float u = fmaf(x, sc, a.sh[c]);
            const float du = u > 0.f ? dz : a.sl[c] * dz;
            s1[j] += du; s2[j] += (double)du * x; s3[j] += u > 0.f ? 0.f : dz * u;
            DU[p * a.C + c] = from_f<T>(sc * du);
        }
    }
#pragma unroll
    for (int j = 0; j < PB_CJ; ++j) {
        red[pg][cl + 64 * j][0] = s1[j]; red[pg][cl + 64 * j][1] = s2[j]; red[pg][cl + 64 * j][2] = s3[j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < a.C; c += blockDim.x) {
        double x = 0, y = 0, z = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { x += red[q][c][0]; y += red[q][c][1]; z += red[q][c][2]; }
        double* o = a.part + ((long)blockIdx.x * a.C + c) * 3;
        o[0] = x; o[1] = y; o[2] = z;
    }
}

// materialised effective gradient (see EffMatArgs); block = W chunk-lanes (W = pow2 >= N/8) x 256/W rows, 16 B per thread
__global__ __launch_bounds__(256) void k_eff_mat(const EffMatArgs a, int wlog) {
    __shared__ float red[256][8];
    const EffSrc& e = a.e;
    const int W = 1 << wlog, rpb = 256 >> wlog;
    const int tx = threadIdx.x & (W - 1), ty = threadIdx.x >> wlog;
    const int cpr = (e.N + 7) >> 3;                        // the tail chunk is zero padded in Out
    const bf16* G = reinterpret_cast<const bf16*>(e.G);
    const bf16* X = reinterpret_cast<const bf16*>(e.X);
    bf16* O = reinterpret_cast<bf16*>(a.Out);
    float cs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (tx < cpr) {
        float cP[8], cQ[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const bool ok = tx * 8 + j < e.N; cP[j] = ok ? e.P[tx * 8 + j] : 0.f; cQ[j] = ok ? e.Q[tx * 8 + j] : 0.f; }
        const uint32_t dkey = drop_key(e.seed, e.stream_id);
        for (long m = (long)blockIdx.x * rpb + ty; m < a.M; m += (long)gridDim.x * rpb) {
            const u16x8 gv = *reinterpret_cast<const u16x8*>(G + m * e.ldg + e.c_off + tx * 8);
            const u16x8 xv = *reinterpret_cast<const u16x8*>(X + m * e.ldx + e.c_off + tx * 8);
            u16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float t = tx * 8 + j < e.N ? eff3(bf2f(gv[j]), cP[j], bf2f(xv[j]), cQ[j]) : 0.f;
                if (e.drop_p > 0.f) t *= drop_pick(drop_bits(dkey, m, tx * 8 + j, e.N), m, e.drop_p);
                o[j] = f2bf(t);
                cs[j] += bf2f(o[j]);
            }
            *reinterpret_cast<u16x8*>(O + m * a.ldo + tx * 8) = o;
        }
    }
    if (a.colsum == nullptr) return;
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = cs[j];
    __syncthreads();
    if (ty == 0 && tx < cpr) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float sum = 0.f;
            for (int q = 0; q < rpb; ++q) sum += red[q * W + tx][j];
            if (tx * 8 + j < e.N) a.slab[(long)blockIdx.x * e.N + tx * 8 + j] = sum;       // reduced by k_slab_reduce (same-line atomics serialise)
        }
    }
}

// dst[i] += sum_s slab[s*stride + i], up to four independent jobs (and one BatchNorm backward link) in one launch.
//
// Grid: 1-D.  Each job owns a contiguous range of workgroups (SlabFirst = the prefix offsets), the link the range behind the
// last job: every workgroup of the launch has work.  The split is by bytes, not by columns: a workgroup owns SR_COLS = 32 columns (one
// 128-B line of every slab row) and SR_LANES = 32 slab lanes -- thread = (lane sl = tid / 8, 16-B column group cg = tid % 8).  Lane sl
// sums the slabs sl, sl + 32, sl + 64, ... eight at a time (eight 16-B loads in flight per thread; 512 slabs = two trips), so a full-size
// job of the DenseNet plan is 512 (1x1, ldc = 128) to 1 152 (3x3) workgroups on 256 CUs where the column-major split had 128 to 288.
//
// Summation order of every output element, a function of nslab alone (not of count, stride, alignment or the other jobs of the launch):
//   lane partial   p[sl] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)),  a[q] = slabs sl + 32 * (8 * t + q) in ascending t
//   wave           the eight lanes of a wave by three exchange steps: lane distance 1, 2, 4
//   workgroup      the four wave sums through LDS: (w0 + w1) + (w2 + w3)
//   dst            one read-add-write by the thread that holds the sum
// No job ends in an atomic.  Slab rows that are not 16-B aligned, counts that are no multiple of 4 and unaligned dst take scalar accesses
// in the same order; columns in [count, stride) and rows >= nslab are never read.
// The shape follows from: at most two trips at 512 slabs, at least 2 x 256 workgroups for the smallest full-size job, 128 B contiguous per
// row access, 256 threads.  Measured: 71 MB in 19.7 us (3.6 TB/s; 23.0 us before); no alternative shape has been timed
// (profiles/helper_launches.md).
constexpr int SR_COLS = 32, SR_LANES = 32, SR_THREADS = SR_COLS / 4 * SR_LANES;
struct SlabFirst { int f1, f2, f3, f4; };      // job i = workgroups [f(i), f(i+1)), f0 = 0; the link from f4 on
struct SlabLaunch { SlabJob j[4]; SlabFirst F; };      // host side
typedef __attribute__((ext_vector_type(4))) float sr_f4;

// columns [0, nv) of a row chunk, zeros behind them; VEC: one 16-B load, else nv scalar loads (a column past nv re-reads column 0: no
// branch between the loads, nothing outside the job's columns is touched)
template <bool VEC>
__device__ __forceinline__ sr_f4 slab_row4(const float* p, int nv) {
    if constexpr (VEC) return *reinterpret_cast<const sr_f4*>(p);
    const sr_f4 v{p[0], p[nv > 1 ? 1 : 0], p[nv > 2 ? 2 : 0], p[nv > 3 ? 3 : 0]};
    return sr_f4{v.x, nv > 1 ? v.y : 0.f, nv > 2 ? v.z : 0.f, nv > 3 ? v.w : 0.f};
}
// lane sl's slabs sl, sl + SR_LANES, ... -> eight partial sums, eight loads in flight per trip
template <bool VEC>
__device__ __forceinline__ void slab_lane_sums(const SlabJob& j, const float* __restrict__ base, int sl, int nv, sr_f4 (&acc)[8]) {
    for (int k = sl; k < j.nslab; k += 8 * SR_LANES) {
        sr_f4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {                          // a row past the end is replaced by this lane's row k and not added
            const int kk = k + q * SR_LANES;
            v[q] = slab_row4<VEC>(base + (long)(kk < j.nslab ? kk : k) * j.stride, nv);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (k + q * SR_LANES < j.nslab) acc[q] += v[q];
    }
}
__device__ __forceinline__ void slab_reduce_body(const SlabJob& j, int wg, sr_f4 (*red)[SR_COLS / 4]) {
    constexpr int CG = SR_COLS / 4;
    static_assert(SR_THREADS == 256 && CG == 8, "the wave exchange and the four-wave tree below are written for 32 columns x 32 lanes");
    const int cg = threadIdx.x % CG, sl = threadIdx.x / CG;
    const long i = ((long)wg * CG + cg) * 4;
    const long left = j.count - i;
    const int nv = left >= 4 ? 4 : (int)left;                   // columns of this thread (<= 0: none)
    sr_f4 acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = sr_f4{0.f, 0.f, 0.f, 0.f};
    if (nv > 0) {
        if (j.v4 && nv == 4) slab_lane_sums<true>(j, j.slab + i, sl, nv, acc);
        else slab_lane_sums<false>(j, j.slab + i, sl, nv, acc);
    }
    sr_f4 s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
    for (int d = CG; d < 64; d <<= 1) {                         // the lanes of a wave (32 x 32: thread distance 8, 16, 32)
        s.x += __shfl_xor(s.x, d); s.y += __shfl_xor(s.y, d); s.z += __shfl_xor(s.z, d); s.w += __shfl_xor(s.w, d);
    }
    if ((threadIdx.x & 63) < CG) red[threadIdx.x >> 6][cg] = s;
    __syncthreads();
    if (threadIdx.x < CG && nv > 0) {
        const sr_f4 v = (red[0][cg] + red[1][cg]) + (red[2][cg] + red[3][cg]);
        float* d = j.dst + i;
        if (j.dv4 && nv == 4) { sr_f4* d4 = reinterpret_cast<sr_f4*>(d); *d4 = *d4 + v; }
        else {
            d[0] += v.x;
            if (nv > 1) d[1] += v.y;
            if (nv > 2) d[2] += v.z;
            if (nv > 3) d[3] += v.w;
        }
    }
}
// (the jobs are separate kernel arguments and every field is picked by a select: as one record, or picked by reference, the compiler
// indexes a private copy of the arguments -- 216 B of scratch per lane)
#define SR_JOBS const SlabJob j0, const SlabJob j1, const SlabJob j2, const SlabJob j3
__device__ __forceinline__ void slab_reduce_pick(const SlabJob& j0, const SlabJob& j1, const SlabJob& j2, const SlabJob& j3, const SlabFirst& F, int b) {
    __shared__ sr_f4 red[SR_THREADS / 64][SR_COLS / 4];
    const int z = (b >= F.f1) + (b >= F.f2) + (b >= F.f3);
    const int f = z == 0 ? 0 : z == 1 ? F.f1 : z == 2 ? F.f2 : F.f3;
#define SR_PICK(m) (z == 0 ? j0.m : z == 1 ? j1.m : z == 2 ? j2.m : j3.m)
    const SlabJob j{SR_PICK(slab), SR_PICK(dst), SR_PICK(nslab), SR_PICK(count), SR_PICK(stride), SR_PICK(v4), SR_PICK(dv4)};
#undef SR_PICK
    slab_reduce_body(j, b - f, red);
}
__global__ __launch_bounds__(SR_THREADS) void k_slab_reduce(SR_JOBS, const SlabFirst F) { slab_reduce_pick(j0, j1, j2, j3, F, blockIdx.x); }
// The same launch with a BatchNorm backward link behind the last job (round 5): after the fused 1x1 backward kernel both its slab
// reduction and the norm1 link are latency-floor launches on the critical chain, independent of each other (different inputs, different
// outputs) -- one launch instead of two per dense layer.  The link takes the last cdiv(C, 4) workgroups.
__global__ __launch_bounds__(SR_THREADS) void k_slab_reduce_link(SR_JOBS, const SlabFirst F, const BnBwdLinkArgs link) {
    const int b = blockIdx.x;
    if (b >= F.f4) { bn_bwd_link_body(link, b - F.f4, gridDim.x - F.f4); return; }
    slab_reduce_pick(j0, j1, j2, j3, F, b);
}

__global__ void k_unpack(const UnpackDesc* descs) {
    const UnpackDesc d = descs[blockIdx.y];
    const long total = (long)d.N * d.Cin * d.taps;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % d.taps);
        const int c = (int)((i / d.taps) % d.Cin);
        const int n = (int)(i / ((long)d.taps * d.Cin));
        d.dst[i] += d.nfast ? d.src[((long)tap * d.Cin + c) * 32 + n] : d.src[(long)n * d.Kp + tap * d.Cin + c];
    }
}

}  // namespace

#ifdef TCVN_DEBUG_KNOBS
static long g_link_launches = 0;      // validation build: k_bn_bwd_link launches so far (tests assert which links ride in other launches)
extern "C" long tcvn_debug_link_launches(void) { return g_link_launches; }
#endif
int bn_bwd_link(const BnBwdLinkArgs& a, hipStream_t st) {
#ifdef TCVN_DEBUG_KNOBS
    ++g_link_launches;
#endif
    hipLaunchKernelGGL(k_bn_bwd_link, dim3(cdiv(a.C, 4)), dim3(256), 0, st, a);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int head_pool_bwd_grid(int n_img) { return n_img < 256 ? n_img : 256; }
int head_pool_bwd(const HeadPoolBwdArgs& a, hipStream_t st) {
    if (a.C > 256 * HP_CJ) return -2;
    if (a.nblk != head_pool_bwd_grid(a.n_img)) return -3;
    if (a.mode == MODE_F32) hipLaunchKernelGGL(k_head_pool_bwd<float>, dim3(a.nblk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_head_pool_bwd<bf16>, dim3(a.nblk), dim3(256), 0, st, a);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int pool0_bwd_grid(int n_img, int Hin, int Win) {
    const long g = ((long)n_img * Hin * Win + 3) / 4;
    return (int)(g < 2048 ? g : 2048);
}
int pool0_bwd(const Pool0BwdArgs& a, hipStream_t st) {
    if (a.C > 64 * PB_CJ) return -2;
    if (a.nblk != pool0_bwd_grid(a.n_img, a.Hin, a.Win)) return -3;
    if (a.mode == MODE_F32) hipLaunchKernelGGL(k_pool0_bwd<float>, dim3(a.nblk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pool0_bwd<bf16>, dim3(a.nblk), dim3(256), 0, st, a);
    TCVN_LAUNCH_CHECK();
    return 0;
}

int eff_materialize_bf16(const EffMatArgs& a, hipStream_t st) {
    if (a.M <= 0) return 0;
    const EffSrc& e = a.e;
    if (e.N > 512 || (e.ldg & 7) || (e.ldx & 7) || (e.c_off & 7) || (a.ldo & 7) || a.ldo < ((e.N + 7) & ~7)) return -2;
    int wlog = 0;
    while ((1 << wlog) < ((e.N + 7) >> 3)) ++wlog;
    const int rpb = 256 >> wlog;
    const long g = (a.M + rpb - 1) / rpb;
    const int nb = (int)(g < 1024 ? g : 1024);
    if (a.colsum != nullptr && a.slab == nullptr) return -3;
    hipLaunchKernelGGL(k_eff_mat, dim3(nb), dim3(256), 0, st, a, wlog);
    TCVN_LAUNCH_CHECK();
    if (a.colsum != nullptr) {
        if (a.deferred != nullptr) *a.deferred = slab_job(a.slab, nb, e.N, a.colsum, 0);      // folded into the caller's next reduction
        else return slab_reduce(a.slab, nb, e.N, a.colsum, st);
    }
    return 0;
}

SlabJob slab_job(const float* slab, int nslab, long count, float* dst, long stride) {
    SlabJob j{slab, dst, nslab, count, stride > 0 ? stride : count, 0, 0};
    if (count <= 0 || nslab <= 0) { j.count = 0; return j; }
    j.v4 = ((nslab == 1 || j.stride % 4 == 0) && (reinterpret_cast<uintptr_t>(slab) & 15) == 0) ? 1 : 0;
    j.dv4 = (reinterpret_cast<uintptr_t>(dst) & 15) == 0 ? 1 : 0;
    return j;
}
namespace {
// workgroup ranges of up to four jobs; empty jobs (count == 0) get an empty range.  Returns the number of workgroups, -1 when it exceeds the grid limit.
long slab_launch(const SlabJob* jobs, int n, SlabLaunch& L) {
    L = SlabLaunch{};
    int* const first[5] = {nullptr, &L.F.f1, &L.F.f2, &L.F.f3, &L.F.f4};
    long total = 0;
    for (int i = 0; i < 4; ++i) {
        if (i < n && jobs[i].count > 0) { L.j[i] = jobs[i]; total += cdiv(jobs[i].count, (long)SR_COLS); }
        if (total > (1L << 30)) return -1;
        *first[i + 1] = (int)total;
    }
    return total;
}
}  // namespace
// up to four independent jobs in one launch; empty jobs (count == 0) are skipped
int slab_reduce4(const SlabJob* jobs, int n, hipStream_t st) {
    SlabLaunch L;
    const long total = slab_launch(jobs, n, L);
    if (total < 0) return -2;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_slab_reduce, dim3((unsigned)total), dim3(SR_THREADS), 0, st, L.j[0], L.j[1], L.j[2], L.j[3], L.F);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int slab_reduce4_link(const SlabJob* jobs, int n, const BnBwdLinkArgs& link, hipStream_t st) {
    SlabLaunch L;
    const long total = slab_launch(jobs, n, L);
    if (total < 0) return -2;
    if (total == 0) return bn_bwd_link(link, st);
    hipLaunchKernelGGL(k_slab_reduce_link, dim3((unsigned)(total + cdiv(link.C, SR_THREADS / 64))), dim3(SR_THREADS), 0, st, L.j[0], L.j[1], L.j[2], L.j[3], L.F, link);
    TCVN_LAUNCH_CHECK();
    return 0;
}
int slab_reduce2(const SlabJob& a, const SlabJob& b, hipStream_t st) {
    const SlabJob jobs[2] = {a, b};
    return slab_reduce4(jobs, 2, st);
}
int slab_reduce(const float* slab, int nslab, long count, float* dst, hipStream_t st, long stride) {
    SlabJob none{};
    return slab_reduce2(slab_job(slab, nslab, count, dst, stride), none, st);
}

int unpack_wgrads(const UnpackDesc* d_descs, int n, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_unpack, dim3(32, n), dim3(256), 0, st, d_descs);
    TCVN_LAUNCH_CHECK();
    return 0;
}

}  // namespace tcvn

#ifdef TCVN_DEBUG_KNOBS
// Validation build: the slab reducer alone, on the caller's device buffers (tests/test_slab_reduce_gpu.py).  n <= 4 jobs; link_C > 0
// adds a BatchNorm backward link to the launch.
extern "C" int tcvn_debug_slab_reduce(int n, const float* const* slab, const int* nslab, const long long* count, const long long* stride,
                                      float* const* dst, int link_C, int link_nblk, const double* part, const double* bstat,
                                      long long link_count, float eps, const float* gamma, float* dgamma, float* dbeta, float* dslope, float* P,
                                      float* Q, int accumulate_pq, void* stream) {
    using namespace tcvn;
    if (n < 0 || n > 4) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    SlabJob jobs[4] = {};
    for (int i = 0; i < n; ++i) jobs[i] = slab_job(slab[i], nslab[i], count[i], dst[i], stride[i]);
    if (link_C <= 0) return slab_reduce4(jobs, n, st);
    const BnBwdLinkArgs la{part, link_nblk, link_C, bstat, (long)link_count, eps, gamma, dgamma, dbeta, dslope, P, Q, accumulate_pq};
    return slab_reduce4_link(jobs, n, la, st);
}
#endif
