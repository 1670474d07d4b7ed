// gfpl_gba_plan.cpp — host planner of the global bundle adjustment (gfpl_gba_plan.hpp).  Host only.
#include "gfpl_gba_plan.hpp"

#include <algorithm>

namespace gfpl {

namespace {

// landmark ids 0 .. n - 1, contiguous, each at least once; slots in [-n_fix, n_kf) (as gfpl_lba_check)
int check_list(const int32_t* lm, const int32_t* kf, int n_obs, int n_lm, int n_kf, int n_fix) {
    if (n_obs == 0) return n_lm == 0 ? GFPL_OK : GFPL_E_INVALID;
    if (!lm || !kf || n_lm < 1) return GFPL_E_INVALID;
    if (lm[0] != 0 || lm[n_obs - 1] != n_lm - 1) return GFPL_E_INVALID;
    for (int o = 0; o < n_obs; ++o) {
        if (o > 0 && lm[o] != lm[o - 1] && lm[o] != lm[o - 1] + 1) return GFPL_E_INVALID;
        if (kf[o] >= n_kf || kf[o] < -n_fix) return GFPL_E_INVALID;
    }
    return GFPL_OK;
}

}  // namespace

int gba_plan(const gfpl_lba_problem* p, GbaPlan* plan) {
    if (!p) return GFPL_E_INVALID;
    const gfpl_lba_counts& n = p->n;
    if (n.n_kf < 1 || n.n_fix < 0 || n.n_pt < 0 || n.n_ls < 0 || n.n_pt_obs < 0 || n.n_ls_obs < 0) return GFPL_E_INVALID;
    if (n.n_kf > GFPL_GBA_MAX_KFS) return GFPL_E_CAPACITY;
    const int64_t nobs64 = (int64_t)n.n_pt_obs + n.n_ls_obs, nlm64 = (int64_t)n.n_pt + n.n_ls;
    if (nobs64 == 0) return GFPL_E_INVALID;
    if (nobs64 > 0x7fffffff || nlm64 > 0x7ffffffe) return GFPL_E_CAPACITY;
    int rc = check_list(p->pt_obs_lm, p->pt_obs_kf, n.n_pt_obs, n.n_pt, n.n_kf, n.n_fix);
    if (rc != GFPL_OK) return rc;
    rc = check_list(p->ls_obs_lm, p->ls_obs_kf, n.n_ls_obs, n.n_ls, n.n_kf, n.n_fix);
    if (rc != GFPL_OK) return rc;

    GbaPlan local;
    GbaPlan& g = plan ? *plan : local;
    g = GbaPlan{};
    g.n.n = n;
    const int nobs = (int)nobs64, nlm = (int)nlm64, nkf = n.n_kf;
    g.lm_start.assign((size_t)nlm + 1, 0);
    g.obs_lm.resize((size_t)nobs);
    g.obs_kf.resize((size_t)nobs);
    g.obs_pair.assign((size_t)nobs, -1);
    int j = 0;
    for (int o = 0; o < n.n_pt_obs; ++o) {
        if (o == 0 || p->pt_obs_lm[o] != p->pt_obs_lm[o - 1]) g.lm_start[(size_t)j++] = o;
        g.obs_lm[(size_t)o] = p->pt_obs_lm[o];
        g.obs_kf[(size_t)o] = p->pt_obs_kf[o];
    }
    for (int o = 0; o < n.n_ls_obs; ++o) {
        if (o == 0 || p->ls_obs_lm[o] != p->ls_obs_lm[o - 1]) g.lm_start[(size_t)j++] = n.n_pt_obs + o;
        g.obs_lm[(size_t)n.n_pt_obs + o] = n.n_pt + p->ls_obs_lm[o];
        g.obs_kf[(size_t)n.n_pt_obs + o] = p->ls_obs_kf[o];
    }
    g.lm_start[(size_t)nlm] = nobs;

    // pairs: the distinct local keyframes of each landmark, ascending
    g.pair_start.assign((size_t)nlm + 1, 0);
    std::vector<int32_t> seen;
    int64_t n_terms = 0, n_pairs = 0, n_pt_pairs = 0;
    for (int l = 0; l < nlm; ++l) {
        seen.clear();
        for (int o = g.lm_start[(size_t)l]; o < g.lm_start[(size_t)l + 1]; ++o)
            if (g.obs_kf[(size_t)o] >= 0) seen.push_back(g.obs_kf[(size_t)o]);
        std::sort(seen.begin(), seen.end());
        seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
        g.pair_start[(size_t)l] = (int32_t)n_pairs;
        for (int o = g.lm_start[(size_t)l]; o < g.lm_start[(size_t)l + 1]; ++o) {
            const int s = g.obs_kf[(size_t)o];
            if (s >= 0)
                g.obs_pair[(size_t)o] = (int32_t)(n_pairs + (std::lower_bound(seen.begin(), seen.end(), s) - seen.begin()));
        }
        g.pair_kf.insert(g.pair_kf.end(), seen.begin(), seen.end());
        const int64_t m = (int64_t)seen.size();
        n_pairs += m;
        n_terms += m * (m + 1) / 2;
        if (l < n.n_pt) n_pt_pairs = n_pairs;
        if (n_pairs > 0x7fffffff / 36 || n_terms > 0x7fffffff / 3) return GFPL_E_CAPACITY;
    }
    g.pair_start[(size_t)nlm] = (int32_t)n_pairs;
    g.n.n_pt_pairs = (int32_t)n_pt_pairs;
    g.n.n_ls_pairs = (int32_t)(n_pairs - n_pt_pairs);
    g.n.n_terms = (int32_t)n_terms;

    // per local keyframe, its observations in list order (points, then lines)
    g.kf_start.assign((size_t)nkf + 1, 0);
    for (int o = 0; o < nobs; ++o)
        if (g.obs_kf[(size_t)o] >= 0) ++g.kf_start[(size_t)g.obs_kf[(size_t)o] + 1];
    for (int s = 0; s < nkf; ++s) g.kf_start[(size_t)s + 1] += g.kf_start[(size_t)s];
    g.kf_obs.assign((size_t)g.kf_start[(size_t)nkf], 0);
    {
        std::vector<int32_t> at(g.kf_start.begin(), g.kf_start.end() - 1);
        for (int o = 0; o < nobs; ++o)
            if (g.obs_kf[(size_t)o] >= 0) g.kf_obs[(size_t)at[(size_t)g.obs_kf[(size_t)o]]++] = o;
    }

    // per lower block (a >= b) of S, the landmarks seen by both, ascending, with the two pairs
    const size_t nblk = (size_t)nkf * ((size_t)nkf + 1) / 2;
    g.blk_start.assign(nblk + 1, 0);
    for (int l = 0; l < nlm; ++l)
        for (int ia = g.pair_start[(size_t)l]; ia < g.pair_start[(size_t)l + 1]; ++ia)
            for (int ib = g.pair_start[(size_t)l]; ib <= ia; ++ib) {
                const size_t a = (size_t)g.pair_kf[(size_t)ia], b = (size_t)g.pair_kf[(size_t)ib];
                ++g.blk_start[a * (a + 1) / 2 + b + 1];
            }
    for (size_t k = 0; k < nblk; ++k) g.blk_start[k + 1] += g.blk_start[k];
    g.terms.assign((size_t)n_terms * 3, 0);
    {
        std::vector<int32_t> at(g.blk_start.begin(), g.blk_start.end() - 1);
        for (int l = 0; l < nlm; ++l)
            for (int ia = g.pair_start[(size_t)l]; ia < g.pair_start[(size_t)l + 1]; ++ia)
                for (int ib = g.pair_start[(size_t)l]; ib <= ia; ++ib) {
                    const size_t a = (size_t)g.pair_kf[(size_t)ia], b = (size_t)g.pair_kf[(size_t)ib];
                    const size_t t = (size_t)at[a * (a + 1) / 2 + b]++;
                    g.terms[3 * t] = l;
                    g.terms[3 * t + 1] = ia;
                    g.terms[3 * t + 2] = ib;
                }
    }
    return GFPL_OK;
}

}  // namespace gfpl
