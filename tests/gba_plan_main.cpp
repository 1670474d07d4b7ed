// gba_plan_main.cpp — a stand-alone caller of the global bundle adjustment's planner
// (gfpl_gba_plan.cpp), built by tests/test_gba_cpu.py with -fsanitize=address,undefined.  Reads
// problems from a text file
//   n_problems, then per problem: n_kf n_fix n_pt n_ls n_pt_obs n_ls_obs, pt_obs_lm [n_pt_obs],
//   pt_obs_kf [n_pt_obs], ls_obs_lm [n_ls_obs], ls_obs_kf [n_ls_obs]
// and runs each through gba_plan twice (without and with a plan).  Prints per problem: rc; the
// counts; every list.  Exit 1 when the two calls disagree.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gf-pl-slam_amd/csrc/gfpl_gba_plan.hpp"

namespace {

// exactly n entries on the heap, so a read past the array is a report
int32_t* read_array(FILE* f, size_t n) {
    int32_t* a = (int32_t*)std::malloc(n ? n * sizeof(int32_t) : 1);
    for (size_t i = 0; i < n; ++i) {
        int v;
        if (std::fscanf(f, "%d", &v) != 1) std::exit(2);
        a[i] = (int32_t)v;
    }
    return a;
}

void line(const char* name, const std::vector<int32_t>& v) {
    std::printf("%s", name);
    for (int32_t x : v) std::printf(" %d", x);
    std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n_problems;
    if (std::fscanf(f, "%d", &n_problems) != 1) return 2;
    for (int k = 0; k < n_problems; ++k) {
        gfpl_lba_problem p = {};
        if (std::fscanf(f, "%d %d %d %d %d %d", &p.n.n_kf, &p.n.n_fix, &p.n.n_pt, &p.n.n_ls, &p.n.n_pt_obs, &p.n.n_ls_obs) != 6)
            return 2;
        const size_t npo = p.n.n_pt_obs > 0 ? (size_t)p.n.n_pt_obs : 0, nlo = p.n.n_ls_obs > 0 ? (size_t)p.n.n_ls_obs : 0;
        int32_t* plm = read_array(f, npo);
        int32_t* pkf = read_array(f, npo);
        int32_t* llm = read_array(f, nlo);
        int32_t* lkf = read_array(f, nlo);
        p.pt_obs_lm = plm; p.pt_obs_kf = pkf; p.ls_obs_lm = llm; p.ls_obs_kf = lkf;
        gfpl::GbaPlan plan;
        const int r1 = gfpl::gba_plan(&p, nullptr);
        const int r2 = gfpl::gba_plan(&p, &plan);
        std::printf("rc %d\n", r1);
        if (r2 == GFPL_OK) {
            std::printf("counts %d %d %d\n", plan.n.n_pt_pairs, plan.n.n_ls_pairs, plan.n.n_terms);
            line("lm_start", plan.lm_start);
            line("obs_lm", plan.obs_lm);
            line("obs_kf", plan.obs_kf);
            line("obs_pair", plan.obs_pair);
            line("pair_start", plan.pair_start);
            line("pair_kf", plan.pair_kf);
            line("kf_start", plan.kf_start);
            line("kf_obs", plan.kf_obs);
            line("blk_start", plan.blk_start);
            line("terms", plan.terms);
        }
        std::free(plm); std::free(pkf); std::free(llm); std::free(lkf);
        if (r1 != r2) {
            std::fprintf(stderr, "problem %d: the two calls disagree\n", k);
            return 1;
        }
    }
    std::fclose(f);
    return 0;
}
