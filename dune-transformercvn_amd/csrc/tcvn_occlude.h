// Launch interface of the occlusion-map kernels (occlude.hip) that the token path calls: variant rows and variant sequences.
#pragma once
#include "tcvn_common.h"

namespace tcvn {

// vrows [n][in_dim]: variant j takes row row_base + vimg[j] of `rows` with columns [col0, col0 + width) replaced by emb[j] (row stride
// emb_ld; `rows` has n_rows rows); ident[j] = j (the token table of n one-token sequences).
int occ_rows(const float* rows, const int* vimg, int row_base, const float* emb, long emb_ld, int col0, int width, float* vrows,
             int* ident, int n, int in_dim, int n_rows, hipStream_t st);
// Variant batch of n sequences for the encoder: index[j] = (b, s, ty, tx) names event b with token s REPLACED by vtok[j].
// X0 [S*n][D] sequence-major tokens (padded rows zero), vrow [n][S] (0 valid, -1 padded).
int occ_gather(const float* tokens, const int* tok_row, const int* index, const float* vtok, float* X0, int* vrow, int n, int B, int S,
               int D, hipStream_t st);

}  // namespace tcvn
