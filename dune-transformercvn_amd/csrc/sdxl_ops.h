// Launch interface of the SDXL-style embedder kernels: general NHWC convolutions (any kernel size / stride / top-left padding;
// forward, data gradient, weight gradient) and GroupNorm(1 group) + SiLU.
// Reference call sites: transformercvn/network/layers/sdxl_net.py:27-34,41-42 (diffusers.models.vae.Encoder, see
// oracle/sdxl_oracle.py for the restated block definitions).
//
// A convolution is ONE call record per direction (SConvFwd / SConvDgrad / SConvWgrad: the geometry plus that direction's operands
// and row strides) and runs on one of five kernel families, chosen by sconv_{fwd,dgrad,wgrad}_kernel and nowhere else:
//   SCONV_GENERIC  implicit GEMM, any geometry, fp32 and bf16                                          (sdxl_kernels.hip)
//   SCONV_C64      bf16 3x3 / stride 1 / pad 1, 64 -> 64: halo patch in LDS, weights in registers      (sdxl_conv3x3.hip)
//   SCONV_G        bf16 3x3 / stride 1 / pad 1, channels multiples of 64 up to 512: chunked patch      (sdxl_conv3x3.hip)
//   SCONV_S2       bf16 3x3 / stride 2 / pad 0 down-samplers, channels multiples of 64                 (sdxl_conv3x3.hip)
//   SCONV_IN       bf16 conv_in 3 -> 64: gather-MFMA forward, weight gradient from the hit list        (sdxl_stem.hip)
// sconv_fwd / sconv_dgrad / sconv_wgrad are a switch over that answer.
#pragma once
#include "tcvn_common.h"

namespace tcvn {

// One convolution: Out[(img,ho,wo)][n] = bias[n] + sum_{ky,kx,c} In[img][ho*stride + ky - pad][wo*stride + kx - pad][c] * W[n][c][ky][kx]
// (+ Res[(img,ho,wo)][n]).  Taps that fall outside [0,Hin) x [0,Win) read zero, which also realises diffusers' asymmetric
// F.pad(0,1,0,1) in front of its stride-2 downsampling convolution (pad = 0 here, the bottom/right row is the range check).
struct SConv {
    int mode;                               // MODE_F32 / MODE_BF16: element type of In, Out, Res, dOut, dIn and the packed weights
    int n, Hin, Win, Cin; long lda;         // input NHWC with row stride lda
    int Ho, Wo, Cout, ks, stride, pad;
    int Kp, Kpt;                            // padded K of the forward ([Cout][Kp], k = tap*Cin + c) and transposed ([Cin][Kpt], k = tap*Cout + n) packs
    float* slab; long slab_bytes;           // optional scratch for per-workgroup partial weight gradients (sconv_wgrad fast path)
    const int* hits; long nnz;              // optional: COO list (image, y, x) of the non-zero input pixels (conv_in weight gradient)
    double* stats;                          // optional (forward): [n][2] per-image (sum, sum of squares) of the stored output, pre-zeroed --
                                            // the GroupNorm statistics of the consumer, accumulated by the convolution's epilogue
};
constexpr long kSconvSlabBytes = 512L * (64 * 576 + 64) * 4;     // what the 64 -> 64 weight-gradient kernel asks for

struct SConvFwd { SConv g; const void* In; const void* Wk; const float* bias; const void* Res; long ldres; void* Out; long ldo; int out_f32; };
// dIn[(img,y,x)][c] (+)= sum_{ky,kx,n} dOut[img][(y+pad-ky)/stride][(x+pad-kx)/stride][n] * W[n][c][ky][kx]  (exact divisions only)
struct SConvDgrad { SConv g; const void* dOut; long lddo; const void* Wt; void* dIn; long lddi; int accumulate; };
// dWk[n][k] += sum_m dOut[m][n] * a(m, k) (fp32, kernel layout [Cout][Kp]);  dbias[n] += sum_m dOut[m][n]
struct SConvWgrad { SConv g; const void* In; const void* dOut; long lddo; float* dWk; float* dbias; };

enum SConvKernel { SCONV_GENERIC, SCONV_C64, SCONV_G, SCONV_S2, SCONV_IN };
// The ONE place per direction that chooses the kernel (every tile family goes through conv3x3_tile_enabled()).  fuses_stats: whether
// the chosen kernel accumulates g.stats in its epilogue; after any other kernel sconv_fwd runs the stand-alone statistics pass.
SConvKernel sconv_fwd_kernel(const SConvFwd& c, bool* fuses_stats = nullptr);
SConvKernel sconv_dgrad_kernel(const SConvDgrad& c);
SConvKernel sconv_wgrad_kernel(const SConvWgrad& c);

int sconv_fwd(const SConvFwd& c, hipStream_t st);
int sconv_dgrad(const SConvDgrad& c, hipStream_t st);
int sconv_wgrad(const SConvWgrad& c, hipStream_t st);

// behind the switch: the tile families of sdxl_conv3x3.hip (k = SCONV_C64 / SCONV_G / SCONV_S2) and of sdxl_stem.hip (SCONV_IN)
int sconv3_fwd(SConvKernel k, const SConvFwd& c, hipStream_t st);
int sconv3_dgrad(SConvKernel k, const SConvDgrad& c, hipStream_t st);
int sconv3_wgrad(SConvKernel k, const SConvWgrad& c, hipStream_t st);
int sconv_in_fwd(const SConvFwd& c, hipStream_t st);
int sconv_in_wgrad(const SConvWgrad& c, hipStream_t st);
// whether SCONV_G packs several maps of this size into one tile (TileMap); a packed tile cannot accumulate per-image statistics
bool sconv3_packs(const SConv& g);

// GroupNorm with ONE group (statistics over C*H*W of each image) followed by SiLU (act = 1) or nothing (act = 0).
// stats: [n][2] doubles (sum, sum of squares), zeroed by the caller before gn_stats.
struct GnArgs {
    int mode; const void* X; long ldx; int n, HW, C;
    const float *gamma, *beta; float eps; int act;
    double* stats;
};
int gn_stats(const GnArgs& a, hipStream_t st);
int gn_act(const GnArgs& a, void* Out, long ldo, hipStream_t st);
// Backward: dA = gradient w.r.t. the activated output.  bsum: [n][2] doubles (sum gamma*dU, sum gamma*dU*xhat), zeroed by the
// caller before gn_bwd_reduce, which also accumulates dgamma / dbeta.  gn_bwd_apply then writes / accumulates dX.
int gn_bwd_reduce(const GnArgs& a, const void* dA, long ldda, double* bsum, float* dgamma, float* dbeta, hipStream_t st);
int gn_bwd_apply(const GnArgs& a, const void* dA, long ldda, const double* bsum, void* dX, long lddx, int accumulate, hipStream_t st);

// elementwise helpers
int cast_f32_to(int mode, const float* src, long lds, void* dst, long ldd, long rows, int cols, hipStream_t st);
int add_into(int mode, void* dst, long ldd, const void* src, long lds, long rows, int cols, hipStream_t st);    // dst += src

}  // namespace tcvn
