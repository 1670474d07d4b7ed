// gfpl_gba_plan.hpp — the host planner of the global bundle adjustment (gfpl_gba_plan.cpp): the
// checks of a problem's index arrays and the lists the kernels of k_gba.hip sum by, every one in an
// order that is a function of the problem alone.  No HIP API and no device type: a plain host
// program can compile the planner (tests/gba_plan_main.cpp does, under ASan + UBSan).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/gfpl.h"
#include "gfpl_layout.hpp"

namespace gfpl {

struct GbaPlan {
    gfpl_gba_counts n{};
    std::vector<int32_t> lm_start;     // [n_lm + 1] first observation of each landmark (points first)
    std::vector<int32_t> obs_lm;       // [n_obs] landmark in the unified numbering
    std::vector<int32_t> obs_kf;       // [n_obs] keyframe slot
    std::vector<int32_t> obs_pair;     // [n_obs] pair of the observation, -1 for a fixed pose
    std::vector<int32_t> pair_start;   // [n_lm + 1]
    std::vector<int32_t> pair_kf;      // [n_pairs] distinct local keyframes of each landmark, ascending
    std::vector<int32_t> kf_start;     // [n_kf + 1]
    std::vector<int32_t> kf_obs;       // observations of each local keyframe in list order
    std::vector<int32_t> blk_start;    // [n_kf (n_kf + 1) / 2 + 1]
    std::vector<int32_t> terms;        // [n_terms][3]: landmark, pair of a, pair of b; landmarks ascending per block
};

// Checks the problem (include/gfpl.h, gfpl_gba_check) and builds the lists; plan may be null.
int gba_plan(const gfpl_lba_problem* p, GbaPlan* plan);

}  // namespace gfpl
