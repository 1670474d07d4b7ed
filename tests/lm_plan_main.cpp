// lm_plan_main.cpp — a stand-alone caller of the landmark store's planner (gfpl_lm_plan.cpp), built
// by tests/test_lm_store_cpu.py with -fsanitize=address,undefined.  Reads op lists from a text file
//   lm_cap obs_cap min_g n_srcs rows... n_lists, then per list: n, n x (lm kind arg src)
// and runs each from zeroed counts through gfpl_lm_ops_check and through lm_plan with a plan.
// Prints per list: the return code; the counts after; the plan's op order; per work item
// lm n_ops count0 and its bucket.  Exit 1 when the two entry points disagree, a refused list
// changed the counts, or the planner's scratch is not all -1 again.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gf-pl-slam_amd/csrc/gfpl_lm_plan.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int lm_cap, obs_cap, min_g, n_srcs, n_lists;
    if (std::fscanf(f, "%d %d %d %d", &lm_cap, &obs_cap, &min_g, &n_srcs) != 4) return 2;
    std::vector<int32_t> src_rows((size_t)n_srcs);
    for (int& r : src_rows)
        if (std::fscanf(f, "%d", &r) != 1) return 2;
    if (std::fscanf(f, "%d", &n_lists) != 1) return 2;
    std::vector<int32_t> slot((size_t)lm_cap, -1);
    for (int l = 0; l < n_lists; ++l) {
        int n;
        if (std::fscanf(f, "%d", &n) != 1) return 2;
        // exactly n ops on the heap, so a read past the list is a report
        gfpl_lm_op* ops = n > 0 ? (gfpl_lm_op*)std::malloc((size_t)n * sizeof(gfpl_lm_op)) : nullptr;
        for (int i = 0; i < n; ++i)
            if (std::fscanf(f, "%d %d %d %d", &ops[i].lm, &ops[i].kind, &ops[i].arg, &ops[i].src) != 4) return 2;
        std::vector<int32_t> c1((size_t)lm_cap, 0), c2((size_t)lm_cap, 0);
        gfpl::LmPlan plan;
        const int r1 = gfpl_lm_ops_check(ops, n, c1.data(), lm_cap, obs_cap, src_rows.data(), n_srcs);
        const int r2 = gfpl::lm_plan(ops, n, c2.data(), lm_cap, obs_cap, src_rows.data(), n_srcs, min_g, &plan, slot.data());
        bool bad = r1 != r2 || c1 != c2;
        for (int32_t s : slot) bad = bad || s != -1;
        if (r1 != GFPL_OK)
            for (int32_t c : c1) bad = bad || c != 0;
        std::printf("rc %d\ncounts", r1);
        for (int32_t c : c1) std::printf(" %d", c);
        std::printf("\norder");
        for (int32_t o : plan.order) std::printf(" %d", o);
        std::printf("\nwork");
        for (size_t w = 0; w < plan.work.size(); ++w) {
            int b = 0;
            while (b < gfpl::LM_BUCKETS && (int)w >= plan.bucket_start[b + 1]) ++b;
            std::printf(" %d %d %d %d %d", plan.work[w].lm, plan.work[w].op0, plan.work[w].n_ops, plan.work[w].count0, b);
        }
        std::printf("\n");
        std::free(ops);
        if (bad) {
            std::fprintf(stderr, "list %d: the entry points disagree or a refused list left a trace\n", l);
            return 1;
        }
    }
    std::fclose(f);
    return 0;
}
