// gfpl_pgo_plan.hpp — the host graph builder of the loop-closure pose graph (gfpl_pgo_plan.cpp):
// the index work of MapHandler::loopClosureOptimizationCovGraphG2O / EssGraphG2O
// (src/mapHandler.cpp:4209-4304, :3973-4066) and the structure the kernel accumulates and
// factorises by.  No HIP API and no device type: a plain host program can compile the builder
// (tests/pgo_plan_main.cpp does, under ASan + UBSan).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/gfpl.h"
#include "gfpl_layout.hpp"

namespace gfpl {

struct PgoPlan {
    int first = 0, kf_curr = -1;
    std::vector<int32_t> vert;        // [n_vert][4]: keyframe, flags (PGO_VERT_*), lc_id or -1, free index or -1
    std::vector<int32_t> free_vert;   // [n_free] vertex of free index r
    std::vector<int32_t> edge;        // [n_edge][4]: vertex i, vertex j, loop entry or -1, 0
    std::vector<int32_t> inc_start;   // [n_free + 1]
    std::vector<int32_t> inc;         // incident edges of every free vertex, edge-list order
    std::vector<int32_t> env_first;   // [n_free] f(r)
    std::vector<int32_t> env_off;     // [n_free + 1]
    std::vector<int32_t> reach;       // [n_free] the last row r with f(r) <= c
    std::vector<int32_t> jobs;        // [n_pt + n_ls][4]: landmark, keyframe, first dir row, dir rows
    gfpl_pgo_counts n{};
};

// Checks the problem's host arrays (include/gfpl.h, gfpl_pgo_check) and builds the graph; plan may
// be null.  GFPL_E_CAPACITY when the envelope or a list does not fit 32-bit counts.
int pgo_plan(const gfpl_pgo_problem* p, const gfpl_pgo_graph_params* prm, PgoPlan* plan);

}  // namespace gfpl
