// gfpl_lm_fuse_plan.hpp — the host planner of gfpl_lmstore_fuse (gfpl_lm_fuse_plan.cpp): the check
// of an op list that may append one landmark's list to another (GFPL_LM_APPEND_LM), run over the
// whole list in array order, and the resolution of every element a list gains to its origin.  No
// HIP API and no device type: tests/lm_fuse_plan_main.cpp compiles it under ASan + UBSan.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/gfpl.h"
#include "gfpl_lm_plan.hpp"

namespace gfpl {

// where a row of a final list comes from
struct LmOrigin {
    int32_t src;   // >= 0: row `row` of srcs[src];  < 0: the store's row (landmark -1 - src, position row) as it
    int32_t row;   // stood before the call (row < that landmark's count before the call)
};

// one landmark an op names as `lm`
struct LmFuseTouch {
    int32_t lm, count0;
    bool freed;                     // a FREE emptied it: no later op names it
    std::vector<LmOrigin> gained;   // positions count0, count0 + 1, ... of its list, in order (none once freed)
};

struct LmFusePlan {
    std::vector<LmFuseTouch> touch;   // in first-touch order
    // what k_lm_apply<G> runs: per work item its gained rows as ADDs, or one FREE; bucket by the final length
    std::vector<LmWork> work;
    std::vector<int32_t> work_touch;   // work item -> index into touch
    int bucket_start[LM_BUCKETS + 1] = {};
    int64_t n_dev_ops = 0;   // ops of all work items (<= n_rows)
};

// Checks the ops one after another (the first that fails decides the code) against counts [lm_cap]
// and, when all pass, leaves the final counts there; a refused list leaves counts as they were.
// n_rows (may be null): 1 per ADD or FREE and the source's length per append, 0 for a refused list.
// plan (may be null) receives the origins and the work items.  slot: scratch of lm_cap entries, all
// -1 on entry and on return (null: allocated here).
int lm_fuse_plan(const gfpl_lm_op* ops, int n, int32_t* counts, int lm_cap, int obs_cap, const int32_t* src_rows,
                 int n_srcs, int min_g, int64_t* n_rows, LmFusePlan* plan, int32_t* slot);

}  // namespace gfpl
