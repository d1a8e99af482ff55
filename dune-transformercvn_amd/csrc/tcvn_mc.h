// Monte-Carlo dropout: the statistics of T sampled logit rows (mc_dropout.hip).  The sampling itself is a run mode of the plans
// (DenseNetPlan::Step::draw, HeadStep::draw), not a kernel of its own.
#pragma once
#include "tcvn_common.h"

namespace tcvn {

constexpr int MC_MAX_CLASSES = 256;      // TCVN_MC_MAX_CLASSES

struct McStatsArgs {
    const float* logits;       // [T][R][C]
    const int32_t* valid;      // [R] or null: rows with valid[r] < 0 are NaN in every output
    int T, R, C;
    float *mean, *std;         // [R][C]
    float *entropy, *expected_entropy, *mutual_info;      // [R]
    float* votes;              // [R][C]
};
int mc_stats(const McStatsArgs& a, hipStream_t st);

}  // namespace tcvn
