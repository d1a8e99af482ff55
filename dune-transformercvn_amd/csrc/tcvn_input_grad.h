// Launch interface of the hit-gradient kernels (input_grad.hip): the data gradient of conv0 gathered at the hits of a COO list, the
// running-statistics form of the rows BatchNorm + PReLU backward, and the integrated-gradients accumulation.
#pragma once
#include "tcvn_ops.h"

namespace tcvn {

// d_values[h][c] = pre'(values[h][c]) * sum over the <= 4x4 conv0 outputs (oy, ox) that read pixel (y, x) of hit h, and over the N output
// channels, of E0[img, oy, ox, co] * W0[co][c][ky][kx]   (7x7, stride 2, pad 3: 2*oy - 3 + ky = y, x likewise).
// A hit outside the maps and an entry that does not own its pixel (PixelOwners: the highest list index owns it) get exactly 0.
struct HitGradArgs {
    int mode;                                   // element type of E0 (MODE_F32 or MODE_BF16)
    const int* coords; const float* values; long nnz; int n_img, H, W, Cpix;
    int value_mode;                             // 0: v/255, 1: log(v+1), 2: values are final (3, one-hot, has no gradient: refused)
    const void* E0; long lde; int Hc, Wc, N;    // effective gradient of the conv0 output [n,Hc,Wc,N], row pitch lde
    const float* W0;                            // conv0 weights as bound: OIHW fp32 [N][Cpix][7][7]
    PixelOwners o;                              // scatter_pixels' record (base == nullptr: the list has no duplicates)
    float* d_values;                            // [nnz][Cpix] fp32, every element written exactly once
};
int hit_gradient(const HitGradArgs& a, hipStream_t st);

// BatchNorm1d on running statistics + PReLU, backward for the data alone: u = (x - running_mean) * rstd * gamma + beta,
// dX = dY * prelu'(u) * gamma * rstd, rstd = 1 / sqrt(running_var + eps).  No batch terms, no parameter gradients, no dropout.
struct RowsBnFrozenBwdArgs {
    const float* X; long ldx; const float* dY; long lddy; int R, C;
    const float *gamma, *beta, *slope;          // slope == nullptr: ReLU; gamma / beta == nullptr: 1 / 0
    const float *running_mean, *running_var; float eps;
    float* dX; long lddx;
    int no_norm;                                // no BatchNorm1d in the block: dX = dY * act'(x)
};
int rows_bn_bwd_frozen(const RowsBnFrozenBwdArgs& a, hipStream_t st);

}  // namespace tcvn
