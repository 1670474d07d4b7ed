// pgo_plan_main.cpp — a stand-alone caller of the pose graph's builder (gfpl_pgo_plan.cpp), built by
// tests/test_pgo_cpu.py with -fsanitize=address,undefined.  Reads problems from a text file
//   n_problems, then per problem: variant ess cov n_kf n_lc n_pt n_ls, alive [n_kf], full_graph
//   [n_kf][n_kf], lc [n_lc][3], then for points and for lines: start [n_kf + 1], idx [start[n_kf]]
// and runs each through gfpl_pgo_check and pgo_plan.  Prints per problem: rc; the counts; first and
// kf_curr; the vertex list; the edge list; inc_start; inc; env_first; env_off; reach; jobs.  Exit 1
// when the two entry points disagree.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gf-pl-slam_amd/csrc/gfpl_pgo_plan.hpp"

namespace {

// exactly n entries on the heap, so a read past the array is a report
template <typename T>
T* read_array(FILE* f, size_t n) {
    T* a = (T*)std::malloc(n ? n * sizeof(T) : 1);
    for (size_t i = 0; i < n; ++i) {
        int v;
        if (std::fscanf(f, "%d", &v) != 1) std::exit(2);
        a[i] = (T)v;
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
        gfpl_pgo_graph_params prm;
        gfpl_default_pgo_params(&prm);
        gfpl_pgo_problem p = {};
        if (std::fscanf(f, "%d %d %d %d %d %d %d", &prm.variant, &prm.min_lm_ess_graph, &prm.min_lm_cov_graph, &p.n_kf, &p.n_lc,
                        &p.n_pt, &p.n_ls) != 7)
            return 2;
        const size_t nkf = p.n_kf > 0 ? (size_t)p.n_kf : 0, nlc = p.n_lc > 0 ? (size_t)p.n_lc : 0;
        uint8_t* alive = read_array<uint8_t>(f, nkf);
        int32_t* fg = read_array<int32_t>(f, nkf * nkf);
        int32_t* lc = read_array<int32_t>(f, nlc * 3);
        double* pose = (double*)std::calloc(nlc * 6 + 1, sizeof(double));
        int32_t* ps = read_array<int32_t>(f, nkf + 1);
        int32_t* pi = read_array<int32_t>(f, nkf ? (size_t)ps[nkf] : 0);
        int32_t* ls = read_array<int32_t>(f, nkf + 1);
        int32_t* li = read_array<int32_t>(f, nkf ? (size_t)ls[nkf] : 0);
        p.alive = alive; p.full_graph = fg; p.lc = lc; p.lc_pose = pose;
        p.pt_kf_start = ps; p.pt_kf_idx = pi; p.ls_kf_start = ls; p.ls_kf_idx = li;
        gfpl_pgo_counts c1 = {};
        gfpl::PgoPlan plan;
        const int r1 = gfpl_pgo_check(&p, &prm, &c1);
        const int r2 = gfpl::pgo_plan(&p, &prm, &plan);
        std::printf("rc %d\n", r1);
        if (r1 == GFPL_OK) {
            const gfpl_pgo_counts& c = plan.n;
            std::printf("counts %d %d %d %d %d %d %d %d\n", c.n_kf, c.n_lc, c.n_vert, c.n_free, c.n_edge, c.env_blocks, c.n_pt, c.n_ls);
            std::printf("range %d %d\n", plan.first, plan.kf_curr);
            line("vert", plan.vert);
            line("edge", plan.edge);
            line("inc_start", plan.inc_start);
            line("inc", plan.inc);
            line("env_first", plan.env_first);
            line("env_off", plan.env_off);
            line("reach", plan.reach);
            line("jobs", plan.jobs);
        }
        bool bad = r1 != r2;
        if (r1 == GFPL_OK)
            bad = bad || c1.n_vert != plan.n.n_vert || c1.n_free != plan.n.n_free || c1.n_edge != plan.n.n_edge ||
                  c1.env_blocks != plan.n.env_blocks || c1.n_pt != plan.n.n_pt || c1.n_ls != plan.n.n_ls;
        std::free(alive); std::free(fg); std::free(lc); std::free(pose); std::free(ps); std::free(pi); std::free(ls); std::free(li);
        if (bad) {
            std::fprintf(stderr, "problem %d: the entry points disagree\n", k);
            return 1;
        }
    }
    std::fclose(f);
    return 0;
}
