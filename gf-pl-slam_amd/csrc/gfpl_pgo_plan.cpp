// gfpl_pgo_plan.cpp — host graph builder of the loop-closure pose graph (gfpl_pgo_plan.hpp,
// DESIGN.md §4j): the vertex list, the flags from the loop over the loop list WITH ITS BREAK, the
// edge list in the reference's order, and per free vertex its incident edges and the first column
// of its envelope row.  gfpl_pgo_check is the public face of it.  Host only.
#include "gfpl_pgo_plan.hpp"

#include <algorithm>

namespace gfpl {

namespace {

// one ownership list (map_points_kf_idx / map_lines_kf_idx) into jobs
int plan_jobs(const int32_t* start, const int32_t* idx, int n_kf, int n_lm, const uint8_t* freed, bool dirs,
              const int32_t* dir_off, std::vector<int32_t>* jobs, int* n_jobs) {
    *n_jobs = 0;
    if (n_lm < 0) return GFPL_E_INVALID;
    if (dirs) {
        if (!dir_off || dir_off[0] != 0) return GFPL_E_INVALID;
        for (int j = 0; j < n_lm; ++j)
            if (dir_off[j + 1] < dir_off[j]) return GFPL_E_INVALID;
    }
    if (!start) return n_lm == 0 ? GFPL_OK : GFPL_E_INVALID;
    if (start[0] != 0) return GFPL_E_INVALID;
    for (int i = 0; i < n_kf; ++i)
        if (start[i + 1] < start[i]) return GFPL_E_INVALID;
    if (start[n_kf] > 0 && !idx) return GFPL_E_INVALID;
    std::vector<uint8_t> seen((size_t)n_lm, 0);
    for (int i = 0; i < n_kf; ++i)
        for (int o = start[i]; o < start[i + 1]; ++o) {
            const int32_t j = idx[o];
            if (j < 0) continue;   // a freed landmark
            if (j >= n_lm || seen[(size_t)j]) return GFPL_E_INVALID;
            seen[(size_t)j] = 1;
            if (freed && freed[j]) continue;
            ++*n_jobs;
            if (jobs) {
                jobs->push_back(j);
                jobs->push_back(i);
                jobs->push_back(dirs ? dir_off[j] : 0);
                jobs->push_back(dirs ? dir_off[j + 1] - dir_off[j] : 0);
            }
        }
    return GFPL_OK;
}

}  // namespace

int pgo_plan(const gfpl_pgo_problem* p, const gfpl_pgo_graph_params* prm, PgoPlan* plan) {
    if (!p || !prm) return GFPL_E_INVALID;
    if (p->n_kf < 1 || p->n_lc < 1 || !p->alive || !p->full_graph || !p->lc || !p->lc_pose) return GFPL_E_INVALID;
    if (prm->min_lm_ess_graph < 0 || prm->min_lm_cov_graph < 0) return GFPL_E_INVALID;
    if (prm->variant != GFPL_PGO_COV && prm->variant != GFPL_PGO_ESS) return GFPL_E_INVALID;
    const int n_kf = p->n_kf, n_lc = p->n_lc;
    const bool cov = prm->variant == GFPL_PGO_COV;
    int kf_prev = 0x7fffffff, kf_curr = -1;
    for (int l = 0; l < n_lc; ++l) {
        const int a = p->lc[3 * l], b = p->lc[3 * l + 1];
        if (a < 0 || b >= n_kf || a >= b) return GFPL_E_INVALID;
        if (!p->alive[a] || !p->alive[b]) return GFPL_E_INVALID;
        kf_prev = std::min(kf_prev, a);
        kf_curr = std::max(kf_curr, b);
    }
    if (cov) {
        kf_prev = 0;   // :4219
        if (!p->alive[0]) return GFPL_E_INVALID;
    }
    PgoPlan local;
    PgoPlan& g = plan ? *plan : local;
    g = PgoPlan();
    g.first = kf_prev;
    g.kf_curr = kf_curr;

    // vertices (:4223-4264)
    std::vector<int32_t> vertex_of((size_t)n_kf, -1);
    int n_vert = 0, n_free = 0;
    for (int i = kf_prev; i <= kf_curr; ++i) {
        if (!p->alive[i]) continue;
        bool is_lc_i = false, is_lc_j = false;
        int id = 0;
        for (; id < n_lc; ++id) {
            if (p->lc[3 * id] == i) { is_lc_i = true; break; }
            if (p->lc[3 * id + 1] == i) { is_lc_j = true; break; }
        }
        bool fixed;
        if (is_lc_j) fixed = !cov;
        else fixed = cov ? i == 0 : (is_lc_i || i == 0);
        const int flags = (fixed ? PGO_VERT_FIXED : 0) | (is_lc_j ? PGO_VERT_LC_J : 0) | (is_lc_i ? PGO_VERT_LC_I : 0);
        vertex_of[(size_t)i] = n_vert++;
        g.vert.push_back(i);
        g.vert.push_back(flags);
        g.vert.push_back(is_lc_i || is_lc_j ? id : -1);
        g.vert.push_back(fixed ? -1 : n_free);
        if (!fixed) {
            g.free_vert.push_back(n_vert - 1);
            ++n_free;
        }
    }

    // edges (:4267-4304)
    for (int i = kf_prev; i <= kf_curr; ++i) {
        if (!p->alive[i]) continue;
        for (int j = i + 1; j <= kf_curr; ++j) {
            if (!p->alive[j]) continue;
            const int32_t c = p->full_graph[(size_t)i * n_kf + j];
            if (c >= prm->min_lm_ess_graph || (cov && c >= prm->min_lm_cov_graph) || j - i == 1) {
                g.edge.push_back(vertex_of[(size_t)i]);
                g.edge.push_back(vertex_of[(size_t)j]);
                g.edge.push_back(-1);
                g.edge.push_back(0);
            }
        }
    }
    for (int l = 0; l < n_lc; ++l) {
        g.edge.push_back(vertex_of[(size_t)p->lc[3 * l]]);
        g.edge.push_back(vertex_of[(size_t)p->lc[3 * l + 1]]);
        g.edge.push_back(l);
        g.edge.push_back(0);
    }
    if (g.edge.size() / 4 > (size_t)0x3fffffff) return GFPL_E_CAPACITY;
    const int n_edge = (int)(g.edge.size() / 4);

    // incident edges and envelope
    g.inc_start.assign((size_t)n_free + 1, 0);
    g.env_first.resize((size_t)n_free);
    for (int r = 0; r < n_free; ++r) g.env_first[(size_t)r] = r;
    auto free_of = [&](int v) { return g.vert[4 * (size_t)v + 3]; };
    for (int e = 0; e < n_edge; ++e) {
        const int ri = free_of(g.edge[4 * (size_t)e]), rj = free_of(g.edge[4 * (size_t)e + 1]);
        if (ri >= 0) ++g.inc_start[(size_t)ri + 1];
        if (rj >= 0) ++g.inc_start[(size_t)rj + 1];
        if (ri >= 0 && rj >= 0) g.env_first[(size_t)rj] = std::min(g.env_first[(size_t)rj], ri);   // ri < rj always
    }
    for (int r = 0; r < n_free; ++r) g.inc_start[(size_t)r + 1] += g.inc_start[(size_t)r];
    g.inc.resize((size_t)g.inc_start[(size_t)n_free]);
    {
        std::vector<int32_t> fill(g.inc_start.begin(), g.inc_start.end() - 1);
        for (int e = 0; e < n_edge; ++e) {
            const int ri = free_of(g.edge[4 * (size_t)e]), rj = free_of(g.edge[4 * (size_t)e + 1]);
            if (ri >= 0) g.inc[(size_t)fill[(size_t)ri]++] = e;
            if (rj >= 0) g.inc[(size_t)fill[(size_t)rj]++] = e;
        }
    }
    g.env_off.assign((size_t)n_free + 1, 0);
    int64_t off = 0;
    for (int r = 0; r < n_free; ++r) {
        g.env_off[(size_t)r] = (int32_t)off;
        off += r - g.env_first[(size_t)r] + 1;
        if (off > (int64_t)0x7fffffff / 64) return GFPL_E_CAPACITY;
    }
    g.env_off[(size_t)n_free] = (int32_t)off;
    g.reach.assign((size_t)n_free, 0);
    for (int r = 0; r < n_free; ++r) {
        int32_t& at = g.reach[(size_t)g.env_first[(size_t)r]];
        at = std::max(at, (int32_t)r);
    }
    for (int c = 1; c < n_free; ++c) g.reach[(size_t)c] = std::max(g.reach[(size_t)c], g.reach[(size_t)c - 1]);

    // ownership lists (:4327-4364)
    int n_pt = 0, n_ls = 0;
    int rc = plan_jobs(p->pt_kf_start, p->pt_kf_idx, n_kf, p->n_pt, p->pt_freed, p->pt_dir != nullptr, p->pt_dir_off, &g.jobs, &n_pt);
    if (rc != GFPL_OK) return rc;
    rc = plan_jobs(p->ls_kf_start, p->ls_kf_idx, n_kf, p->n_ls, p->ls_freed, p->ls_dir != nullptr, p->ls_dir_off, &g.jobs, &n_ls);
    if (rc != GFPL_OK) return rc;

    g.n.n_kf = n_kf; g.n.n_lc = n_lc; g.n.n_vert = n_vert; g.n.n_free = n_free; g.n.n_edge = n_edge;
    g.n.env_blocks = (int32_t)off; g.n.n_pt = n_pt; g.n.n_ls = n_ls;
    return GFPL_OK;
}

}  // namespace gfpl

extern "C" {

void gfpl_default_pgo_params(gfpl_pgo_graph_params* prm) {
    if (!prm) return;
    prm->min_lm_ess_graph = 100;
    prm->min_lm_cov_graph = 30;
    prm->variant = GFPL_PGO_COV;
    prm->max_iters = 100;
    prm->max_rejects = 10;
    prm->pad = 0;
    prm->lambda_init = 1e-10;
}

int gfpl_pgo_check(const gfpl_pgo_problem* p, const gfpl_pgo_graph_params* prm, gfpl_pgo_counts* counts) {
    gfpl::PgoPlan plan;
    const int rc = gfpl::pgo_plan(p, prm, &plan);
    if (rc == GFPL_OK && counts) *counts = plan.n;
    return rc;
}

}  // extern "C"
