// gfpl_lm_plan.hpp — the host planner of the landmark descriptor store (gfpl_lm_plan.cpp): the
// check of an op list against the landmarks' counts, the stable grouping of the ops by landmark and
// the lane-group bucket of every touched landmark.  No HIP API and no device type: a plain host
// program can compile the planner (tests/lm_plan_main.cpp does, under ASan + UBSan).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/gfpl.h"
#include "gfpl_layout.hpp"

namespace gfpl {

struct LmPlan {
    std::vector<int32_t> order;    // op indices grouped by landmark, array order kept within a landmark
    std::vector<LmWork> work;      // the touched landmarks, bucket 0 (G = 2) first; first-touch order within a bucket
    int bucket_start[LM_BUCKETS + 1] = {};   // work items of bucket b: [bucket_start[b], bucket_start[b + 1])
};

// (lm_bucket_lanes / lm_bucket_of: gfpl_layout.hpp, shared with the device planner)

// Checks the ops in array order against counts [lm_cap] (the first op that fails decides the code)
// and, when all pass, leaves the final counts there; a refused list leaves counts as they were.
// plan (may be null) receives the grouping and the buckets.  slot: scratch of lm_cap entries, all
// -1 on entry and on return (the store keeps one; null: allocated here).
int lm_plan(const gfpl_lm_op* ops, int n, int32_t* counts, int lm_cap, int obs_cap, const int32_t* src_rows,
            int n_srcs, int min_g, LmPlan* plan, int32_t* slot);

}  // namespace gfpl
