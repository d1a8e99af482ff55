// Launch interface of the explanation kernels (explain.hip): attention export, attention rollout, leave-one-prong-out batches.
#pragma once
#include "tcvn_common.h"

namespace tcvn {

// weights [L][B][H][S][S] <- the per-layer probability buffers of a head workspace (layer l at ws + probs0 + l * layer_stride bytes,
// each [B][H][S][S]); rows of padded queries are written as zero.  Reads the workspace, never writes it.
int attn_export(const char* ws, long probs0, long layer_stride, const int* tok_row, float* weights, int L, int B, int H, int S,
                hipStream_t st);
// rollout [B][S][S] = A^_{L-1} ... A^_0,  A^_l = rownorm(0.5 fuse_h(weights[l]) + 0.5 I_valid); fuse_max: max over heads, else mean
int attn_rollout(const float* weights, const int* tok_row, float* rollout, int L, int B, int H, int S, int fuse_max, hipStream_t st);
// Variant batch of n sequences for the encoder: jobs[j] = b * S + s names event b with token s masked out (s = 0: nothing masked, the
// base sequence).  X0 [S*n][D] sequence-major tokens (masked and padded rows zero), vrow [n][S] (0 valid, -1 padded / masked).
int loo_gather(const float* tokens, const int* tok_row, const int* jobs, float* X0, int* vrow, int n, int S, int D, hipStream_t st);
// logits [J][Ce] of all jobs -> event_logits [B][Ce] (slot s = 0) and loo [B][S-1][Ce]: slot (b, s) takes row src[b*S+s] (padded
// slots name the base row b)
int loo_scatter(const float* logits, const int* src, float* event_logits, float* loo, int B, int S, int Ce, hipStream_t st);

}  // namespace tcvn
