// Launch interface of the prong Shapley kernels (shapley.hip): permutations, coalition batches, values and the three reductions.
// A coalition is an int64 mask over prong slots (bit p = slot p present); event b owns the jobs offsets[b] .. offsets[b+1]-1.
//   exact event (n valid slots, 2^n jobs)       job k: bit i of k stands for the i-th valid slot in ascending slot order
//   sampled event (2 + M (n-1) jobs)            job 0: empty, job 1: full, job 2 + m (n-1) + (len-1): the first len slots of permutation m
#pragma once
#include "tcvn_common.h"

namespace tcvn {

// The per-event table the host builds from tok_row: first job, number of valid slots, their mask, and the mode (1 exact, 0 sampled).
struct ShapTable { const int64_t* offsets; const int32_t* n; const int64_t* vmask; const int32_t* exact; };

// permutations [B][M][P]: permutation m of event b = its valid slots sorted by (Philox key(seed; b, m, slot), slot), then -1;
// pos [B][M][P] its inverse: the position of slot p in permutation m, -1 for padded slots
int shap_perm(const int* tok_row, int32_t* perms, int32_t* pos, int B, int M, int P, uint64_t seed, hipStream_t st);
// One pass of n jobs (first .. first+n-1) for the encoder: X0 [S*n][D] sequence-major tokens (absent and padded rows zero), vrow [n][S]
// (0 present, -1 absent / padded), and once per job masks[job], event[job].
int shap_gather(const float* tokens, const int* tok_row, const ShapTable& t, const int32_t* perms, long first, int n, int B, int M, int S,
                int D, float* X0, int* vrow, int64_t* masks, int32_t* event, hipStream_t st);
// values [J][Ce] (fp64) = logits (prob = 0) or their softmax formed in fp64 (prob = 1)
int shap_values(const float* logits, double* values, long J, int Ce, int prob, hipStream_t st);
// event_logits [B][Ce] <- the full coalition's row of coalition_logits
int shap_full_rows(const float* logits, const ShapTable& t, float* event_logits, int B, int Ce, hipStream_t st);
// exact events: phi [B][P][Ce] and stderr (0); rows of padded slots of EVERY event are zeroed here too
int shap_exact(const double* values, const ShapTable& t, float* phi, float* stderr_, int B, int P, int Ce, hipStream_t st);
// interaction [B][P][P][Ce]: exact events by the SHAP convention, sampled events NaN; padded rows and columns 0
int shap_pairs(const double* values, const ShapTable& t, float* inter, int B, int P, int Ce, hipStream_t st);
// sampled events: phi = mean and stderr = sample standard deviation / sqrt(M) of the marginal contributions over the M permutations
int shap_sampled(const double* values, const ShapTable& t, const int32_t* pos, float* phi, float* stderr_, int B, int M, int P, int Ce,
                 hipStream_t st);

}  // namespace tcvn
