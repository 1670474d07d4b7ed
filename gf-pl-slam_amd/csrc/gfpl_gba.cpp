// gfpl_gba.cpp — host side of the global bundle adjustment (include/gfpl.h): the
// object that owns the device workspace of up to max_problems problems, the solve around k_gba.hip
// (every problem is checked and planned on the host first; one upload of the planner's index arrays
// per problem, every launch of every iteration enqueued, one copy of the results, one
// synchronisation) and the test hook that reads a problem's last evaluated system back.
#include "gfpl_gba_plan.hpp"
#include "gfpl_host.hpp"

using namespace gfpl;

static_assert(GBA_MAX_KFS == GFPL_GBA_MAX_KFS, "the layouts and the public cap are one number");

struct gfpl_gba {
    gfpl_ctx* ctx = nullptr;
    gfpl_gba_counts caps{};
    int max_problems = 0;
    size_t mem_stride = 0, idx_stride = 0;   // workspace / index bytes per problem at caps
    char* base = nullptr;                    // [max_problems][mem_stride + idx_stride], then the results
    gfpl_lba_result* d_res = nullptr;
    char* stage = nullptr;                   // pinned [max_problems][idx_stride]
    GbaGrid grid;
    bool poisoned = false;                   // a HIP error inside a solve: only destroy is left
    std::vector<GbaProb> last;               // the last solve's records (device pointers), for the test hook
    std::vector<GbaPlan> plans;              // and its plans (the pair list)
};

namespace {

int check_counts(const gfpl_gba_counts& c) {
    const gfpl_lba_counts& n = c.n;
    if (n.n_kf < 1 || n.n_fix < 0 || n.n_pt < 0 || n.n_ls < 0 || n.n_pt_obs < 0 || n.n_ls_obs < 0 || c.n_pt_pairs < 0 ||
        c.n_ls_pairs < 0 || c.n_terms < 0)
        return GFPL_E_INVALID;
    if (n.n_kf > GFPL_GBA_MAX_KFS) return GFPL_E_CAPACITY;
    if ((int64_t)n.n_pt_obs + n.n_ls_obs > 0x7fffffff || (int64_t)n.n_pt + n.n_ls > 0x7ffffffe ||
        (int64_t)c.n_pt_pairs + c.n_ls_pairs > 0x7fffffff / 36 || c.n_terms > 0x7fffffff / 3)
        return GFPL_E_CAPACITY;
    return GFPL_OK;
}

GbaMem mem_of(char* base, const gfpl_gba_counts& c) {
    return GbaMem(base, c.n.n_kf, c.n.n_pt, c.n.n_ls, c.n.n_pt_obs + c.n.n_ls_obs, c.n_pt_pairs, c.n_ls_pairs);
}
GbaIdx idx_of(char* base, const gfpl_gba_counts& c) {
    return GbaIdx(base, c.n.n_kf, c.n.n_pt + c.n.n_ls, c.n.n_pt_obs + c.n.n_ls_obs, c.n_pt_pairs + c.n_ls_pairs, c.n_terms);
}

bool within(const gfpl_gba_counts& c, const gfpl_gba_counts& caps) {
    return c.n.n_kf <= caps.n.n_kf && c.n.n_pt <= caps.n.n_pt && c.n.n_ls <= caps.n.n_ls && c.n.n_pt_obs <= caps.n.n_pt_obs &&
           c.n.n_ls_obs <= caps.n.n_ls_obs && c.n_pt_pairs <= caps.n_pt_pairs && c.n_ls_pairs <= caps.n_ls_pairs &&
           c.n_terms <= caps.n_terms;
}

}  // namespace

extern "C" {

void gfpl_default_gba_params(gfpl_gba_params* prm) { gfpl_default_lba_params(prm); }

int gfpl_gba_check(const gfpl_lba_problem* p, gfpl_gba_counts* counts) {
    GbaPlan plan;
    const int rc = gba_plan(p, &plan);
    if (rc == GFPL_OK && counts) *counts = plan.n;
    return rc;
}

int gfpl_gba_workspace(const gfpl_gba_counts* n, int64_t* hbm_bytes, int32_t* lds_bytes) {
    if (!n) return GFPL_E_INVALID;
    const int rc = check_counts(*n);
    if (rc != GFPL_OK) return rc;
    if (hbm_bytes) *hbm_bytes = (int64_t)(mem_of(nullptr, *n).bytes + idx_of(nullptr, *n).bytes);
    if (lds_bytes) *lds_bytes = gba_max_lds_bytes(n->n.n_kf);
    return GFPL_OK;
}

int gfpl_gba_create(gfpl_ctx* c, const gfpl_gba_counts* caps, int max_problems, gfpl_gba** out) {
    if (!c || !caps || !out || max_problems < 1) return GFPL_E_INVALID;
    const int rc = check_counts(*caps);
    if (rc != GFPL_OK) return rc;
    if (!gfpl_ctx_camera(c)) return GFPL_E_STATE;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(c)));
    gfpl_gba* l = new gfpl_gba();
    l->ctx = c;
    l->caps = *caps;
    l->max_problems = max_problems;
    l->mem_stride = mem_of(nullptr, *caps).bytes;
    l->idx_stride = idx_of(nullptr, *caps).bytes;
    // test-only overrides of how the wide phases are cut into workgroups, read once here
    {
        const int b = env_int("GFPL_GBA_BLOCK", GBA_BLOCK), r = env_int("GFPL_GBA_LDLT_KFS", GBA_LDLT_KFS);
        l->grid.block = (b == 64 || b == 128 || b == 256) ? b : GBA_BLOCK;
        l->grid.ldlt_kfs = (r >= 1 && r <= GBA_MAX_LDLT_ROWS) ? r : GBA_LDLT_KFS;
    }
    const size_t b_res = up256((size_t)max_problems * sizeof(gfpl_lba_result));
    if (hipMalloc(&l->base, (l->mem_stride + l->idx_stride) * max_problems + b_res) != hipSuccess) {
        (void)hipGetLastError();
        delete l;
        return GFPL_E_NOMEM;
    }
    l->d_res = reinterpret_cast<gfpl_lba_result*>(l->base + (l->mem_stride + l->idx_stride) * max_problems);
    if (hipHostMalloc((void**)&l->stage, l->idx_stride * max_problems, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(l->base);
        delete l;
        return GFPL_E_NOMEM;
    }
    gfpl_ctx_attach(c);
    *out = l;
    return GFPL_OK;
}

int gfpl_gba_destroy(gfpl_gba* l) {
    if (!l) return GFPL_E_INVALID;
    (void)hipSetDevice(gfpl_ctx_device(l->ctx));
    (void)hipStreamSynchronize(stream_of(l->ctx));
    (void)hipHostFree(l->stage);
    (void)hipFree(l->base);
    gfpl_ctx_detach(l->ctx);
    delete l;
    return GFPL_OK;
}

int gfpl_gba_solve(gfpl_gba* l, const gfpl_lba_problem* problems, int n, const gfpl_gba_params* prm,
                   gfpl_gba_result* results) {
    if (!l || n < 0 || (n > 0 && (!problems || !results)) || !prm) return GFPL_E_INVALID;
    if (l->poisoned) return GFPL_E_STATE;
    if (!(prm->lambda_k != 0.0)) return GFPL_E_INVALID;
    std::vector<GbaPlan> plans((size_t)n);
    for (int i = 0; i < n; ++i) {
        const gfpl_lba_problem& p = problems[i];
        const int rc = gba_plan(&p, &plans[(size_t)i]);
        if (rc != GFPL_OK) return rc;
        if (!ba_problem_pointers_ok(p)) return GFPL_E_INVALID;
    }
    if (n > l->max_problems) return GFPL_E_CAPACITY;
    for (int i = 0; i < n; ++i)
        if (!within(plans[(size_t)i].n, l->caps)) return GFPL_E_CAPACITY;
    if (n == 0) return GFPL_OK;
    const gfpl_camera* cam = gfpl_ctx_camera(l->ctx);
    if (!cam) return GFPL_E_STATE;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(l->ctx)));
    hipStream_t s = stream_of(l->ctx);

    l->last.assign((size_t)n, GbaProb{});
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        const gfpl_lba_problem& p = problems[i];
        const GbaPlan& g = plans[(size_t)i];
        char* dev = l->base + (l->mem_stride + l->idx_stride) * (size_t)i;
        const GbaMem m = mem_of(dev, g.n);
        const GbaIdx di = idx_of(dev + l->mem_stride, g.n);
        const GbaIdx hi = idx_of(l->stage + l->idx_stride * (size_t)i, g.n);
        put(hi.lm_start, g.lm_start); put(hi.obs_lm, g.obs_lm); put(hi.obs_kf, g.obs_kf); put(hi.obs_pair, g.obs_pair);
        put(hi.pair_start, g.pair_start); put(hi.pair_kf, g.pair_kf); put(hi.kf_start, g.kf_start); put(hi.kf_obs, g.kf_obs);
        put(hi.blk_start, g.blk_start); put(hi.terms, g.terms);
        e = hipMemcpyAsync(dev + l->mem_stride, l->stage + l->idx_stride * (size_t)i, hi.bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) break;
        GbaArgs a;
        std::memset(&a, 0, sizeof a);
        a.cam = dev_cam(cam);
        a.homog_th = gfpl_ctx_config(l->ctx)->homog_th;
        a.prm = *prm;
        a.rules = GBA_RULES_REFERENCE;
        a.out = l->d_res + i;
        GbaProb& q = a.pr;
        q.n = g.n;
        ba_fill_prob(q, p);
        q.lm_start = di.lm_start; q.obs_lm = di.obs_lm; q.obs_kf = di.obs_kf; q.obs_pair = di.obs_pair;
        q.pair_start = di.pair_start; q.pair_kf = di.pair_kf; q.kf_start = di.kf_start; q.kf_obs = di.kf_obs;
        q.blk_start = di.blk_start; q.terms = di.terms;
        q.m = m.p;
        l->last[(size_t)i] = q;
        e = enqueue_gba(a, l->grid, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(results, l->d_res, (size_t)n * sizeof(gfpl_lba_result), hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);   // also on an error path: the staging is still in use
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: gba_solve failed: %s\n", hipGetErrorString(e != hipSuccess ? e : es));
        l->last.clear();
        l->plans.clear();
        l->poisoned = true;
        return GFPL_E_HIP;
    }
    l->plans.swap(plans);
    return GFPL_OK;
}

int gfpl_gba_debug_system(gfpl_gba* l, int i, int iteration, double* U, double* g, double* V_pt, double* V_ls,
                          double* W_pt, double* W_ls, int32_t* pairs, double* err) {
    if (!l || i < 0 || iteration < 0) return GFPL_E_INVALID;
    if (l->poisoned || (size_t)i >= l->last.size()) return GFPL_E_STATE;
    const GbaProb& q = l->last[(size_t)i];
    const GbaPlan& plan = l->plans[(size_t)i];
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(l->ctx)));
    GFPL_HIPCHK(hipStreamSynchronize(stream_of(l->ctx)));
    int32_t si[16];
    GFPL_HIPCHK(hipMemcpy(si, q.m.si, sizeof si, hipMemcpyDeviceToHost));
    if (si[GBA_SI_LAST_IT] != iteration) return GFPL_E_STATE;
    const size_t npt = (size_t)q.n.n.n_pt, nls = (size_t)q.n.n.n_ls;
    const int rc = ba_read_system(q.m, q.n.n, l->d_res + i, U, g, V_pt, V_ls, err);
    if (rc != GFPL_OK) return rc;
    GFPL_HIPCHK(get_doubles(W_pt, q.m.W, 18 * (size_t)q.n.n_pt_pairs));
    GFPL_HIPCHK(get_doubles(W_ls, q.m.W + 18 * (size_t)q.n.n_pt_pairs, 36 * (size_t)q.n.n_ls_pairs));
    if (pairs) {
        size_t k = 0;
        for (size_t j = 0; j < npt + nls; ++j)
            for (int p = plan.pair_start[j]; p < plan.pair_start[j + 1]; ++p, ++k) {
                pairs[2 * k] = (int32_t)j;
                pairs[2 * k + 1] = plan.pair_kf[(size_t)p];
            }
    }
    return GFPL_OK;
}

}  // extern "C"
