// lm_fuse_plan_main.cpp — a stand-alone caller of gfpl_lmstore_fuse's planner (gfpl_lm_fuse_plan.cpp),
// built by tests/test_lm_fuse_cpu.py with -fsanitize=address,undefined.  Reads op lists from a text file
//   lm_cap obs_cap min_g n_srcs rows... n_lists, then per list: lm_cap starting counts, n, n x (lm kind arg src)
// and runs each through gfpl_lm_fuse_check and through lm_fuse_plan with a plan.  Prints per list
//   rc <code> <n_rows>
//   counts <lm_cap counts after>
//   origins <per work item, in work order: lm bucket count0 freed n_gained, then n_gained x (src row)>
// Exit 1 when the two entry points disagree, a refused list changed the counts, the planner's
// scratch is not all -1 again, or the work items do not tile the device ops.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gf-pl-slam_amd/csrc/gfpl_lm_fuse_plan.hpp"

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
    gfpl::LmFusePlan plan;   // one plan over all lists, as the store keeps one over all calls
    for (int l = 0; l < n_lists; ++l) {
        std::vector<int32_t> c0((size_t)lm_cap);
        for (int32_t& c : c0)
            if (std::fscanf(f, "%d", &c) != 1) return 2;
        int n;
        if (std::fscanf(f, "%d", &n) != 1) return 2;
        // exactly n ops on the heap, so a read past the list is a report
        gfpl_lm_op* ops = n > 0 ? (gfpl_lm_op*)std::malloc((size_t)n * sizeof(gfpl_lm_op)) : nullptr;
        for (int i = 0; i < n; ++i)
            if (std::fscanf(f, "%d %d %d %d", &ops[i].lm, &ops[i].kind, &ops[i].arg, &ops[i].src) != 4) return 2;
        std::vector<int32_t> c1 = c0, c2 = c0;
        int64_t rows1 = -1, rows2 = -1;
        const int r1 = gfpl_lm_fuse_check(ops, n, c1.data(), lm_cap, obs_cap, src_rows.data(), n_srcs, &rows1);
        const int r2 = gfpl::lm_fuse_plan(ops, n, c2.data(), lm_cap, obs_cap, src_rows.data(), n_srcs, min_g, &rows2, &plan,
                                          slot.data());
        bool bad = r1 != r2 || c1 != c2 || rows1 != rows2;
        for (int32_t s : slot) bad = bad || s != -1;
        if (r1 != GFPL_OK) bad = bad || c1 != c0 || rows1 != 0 || !plan.work.empty();
        std::printf("rc %d %lld\ncounts", r1, (long long)rows1);
        for (int32_t c : c1) std::printf(" %d", c);
        std::printf("\norigins");
        int64_t op0 = 0;
        for (size_t w = 0; w < plan.work.size(); ++w) {
            int b = 0;
            while (b < gfpl::LM_BUCKETS && (int)w >= plan.bucket_start[b + 1]) ++b;
            const gfpl::LmFuseTouch& u = plan.touch[(size_t)plan.work_touch[w]];
            const gfpl::LmWork& k = plan.work[w];
            bad = bad || k.lm != u.lm || k.count0 != u.count0 || k.op0 != op0 ||
                  k.n_ops != (u.freed ? 1 : (int32_t)u.gained.size()) || k.n_ops < 1;
            op0 += k.n_ops;
            std::printf(" %d %d %d %d %zu", u.lm, b, u.count0, (int)u.freed, u.gained.size());
            for (const gfpl::LmOrigin& g : u.gained) std::printf(" %d %d", g.src, g.row);
        }
        bad = bad || op0 != plan.n_dev_ops || op0 > rows2;
        std::printf("\n");
        std::free(ops);
        if (bad) {
            std::fprintf(stderr, "list %d: the entry points disagree, a refused list left a trace or the work items do not tile\n", l);
            return 1;
        }
    }
    std::fclose(f);
    return 0;
}
