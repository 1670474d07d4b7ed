// gfpl_pgo.cpp — host side of the loop-closure pose graph (include/gfpl.h): the
// workspace sizes, the object that owns the device workspace of up to max_problems problems, the
// batched solve around k_pgo.hip (the planner's lists of every problem staged once and uploaded,
// two launches, one copy of the results, one synchronisation) and the test hooks.
#include "gfpl_host.hpp"
#include "gfpl_pgo_plan.hpp"

using namespace gfpl;

struct gfpl_pgo {
    gfpl_ctx* ctx = nullptr;
    gfpl_pgo_counts caps{};
    int max_problems = 0;
    size_t ws_stride = 0, idx_stride = 0;   // bytes per problem at caps: workspace, uploaded lists
    char* base = nullptr;                   // [max_problems][ws_stride], [max_problems][idx_stride], records, results
    char* d_idx = nullptr;
    PgoProb* d_probs = nullptr;
    gfpl_pgo_result* d_res = nullptr;
    char* stage = nullptr;                  // pinned: [max_problems][idx_stride], then the records
    hipEvent_t ev[3] = {};
    bool timed = false, poisoned = false;
    int last_max_iters = 0;
    std::vector<PgoProb> last;              // the last solve's records (device pointers), for the test hook
};

namespace {

int check_counts(const gfpl_pgo_counts& n) {
    if (n.n_kf < 1 || n.n_lc < 1 || n.n_edge < 1 || n.env_blocks < 0 || n.n_pt < 0 || n.n_ls < 0) return GFPL_E_INVALID;
    if ((int64_t)n.n_pt + n.n_ls > 0x3fffffff || n.env_blocks > 0x7fffffff / 64 || n.n_edge > 0x3fffffff) return GFPL_E_CAPACITY;
    return GFPL_OK;
}

bool fits(const gfpl_pgo_counts& n, const gfpl_pgo_counts& caps) {
    return n.n_kf <= caps.n_kf && n.n_lc <= caps.n_lc && n.n_edge <= caps.n_edge && n.env_blocks <= caps.env_blocks &&
           n.n_pt <= caps.n_pt && n.n_ls <= caps.n_ls;
}

}  // namespace

extern "C" {

int gfpl_pgo_workspace(const gfpl_pgo_counts* n, int64_t* hbm_bytes, int32_t* lds_bytes) {
    if (!n) return GFPL_E_INVALID;
    const int rc = check_counts(*n);
    if (rc != GFPL_OK) return rc;
    if (n->n_vert < 0 || n->n_vert > n->n_kf || n->n_free < 0 || n->n_free > n->n_vert) return GFPL_E_INVALID;
    if (hbm_bytes)
        *hbm_bytes = (int64_t)(PgoMem(nullptr, n->n_kf, n->n_vert, n->n_free, n->n_edge, n->env_blocks).bytes +
                               PgoIdx(nullptr, n->n_kf, n->n_lc, n->n_vert, n->n_free, n->n_edge, n->n_pt + n->n_ls).bytes);
    if (lds_bytes) *lds_bytes = PgoLds(nullptr).bytes;
    return GFPL_OK;
}

int gfpl_pgo_create(gfpl_ctx* c, const gfpl_pgo_counts* caps, int max_problems, gfpl_pgo** out) {
    if (!c || !caps || !out || max_problems < 1) return GFPL_E_INVALID;
    const int rc = check_counts(*caps);
    if (rc != GFPL_OK) return rc;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(c)));
    gfpl_pgo* g = new gfpl_pgo();
    g->ctx = c;
    g->caps = *caps;
    g->caps.n_vert = g->caps.n_free = caps->n_kf;
    g->max_problems = max_problems;
    g->ws_stride = PgoMem(nullptr, caps->n_kf, caps->n_kf, caps->n_kf, caps->n_edge, caps->env_blocks).bytes;
    g->idx_stride = PgoIdx(nullptr, caps->n_kf, caps->n_lc, caps->n_kf, caps->n_kf, caps->n_edge, caps->n_pt + caps->n_ls).bytes;
    const size_t b_probs = up256((size_t)max_problems * sizeof(PgoProb));
    const size_t b_res = up256((size_t)max_problems * sizeof(gfpl_pgo_result));
    const size_t total = (g->ws_stride + g->idx_stride) * max_problems + b_probs + b_res;
    bool ok = hipMalloc(&g->base, total) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&g->stage, g->idx_stride * max_problems + b_probs, hipHostMallocDefault) == hipSuccess;
    for (int i = 0; i < 3 && ok; ++i) ok = hipEventCreate(&g->ev[i]) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        for (hipEvent_t e : g->ev)
            if (e) (void)hipEventDestroy(e);
        if (g->stage) (void)hipHostFree(g->stage);
        if (g->base) (void)hipFree(g->base);
        delete g;
        return GFPL_E_NOMEM;
    }
    g->d_idx = g->base + g->ws_stride * max_problems;
    g->d_probs = reinterpret_cast<PgoProb*>(g->d_idx + g->idx_stride * max_problems);
    g->d_res = reinterpret_cast<gfpl_pgo_result*>(reinterpret_cast<char*>(g->d_probs) + b_probs);
    gfpl_ctx_attach(c);
    *out = g;
    return GFPL_OK;
}

int gfpl_pgo_destroy(gfpl_pgo* g) {
    if (!g) return GFPL_E_INVALID;
    (void)hipSetDevice(gfpl_ctx_device(g->ctx));
    (void)hipStreamSynchronize(stream_of(g->ctx));
    for (hipEvent_t e : g->ev) (void)hipEventDestroy(e);
    (void)hipHostFree(g->stage);
    (void)hipFree(g->base);
    gfpl_ctx_detach(g->ctx);
    delete g;
    return GFPL_OK;
}

int gfpl_pgo_solve(gfpl_pgo* g, const gfpl_pgo_problem* problems, int n, const gfpl_pgo_graph_params* prm,
                   gfpl_pgo_result* results) {
    if (!g || n < 0 || (n > 0 && (!problems || !results)) || !prm) return GFPL_E_INVALID;
    if (g->poisoned) return GFPL_E_STATE;
    if (prm->max_iters < 0 || prm->max_rejects < 1 || !(prm->lambda_init > 0.0)) return GFPL_E_INVALID;
    std::vector<PgoPlan> plans((size_t)n);
    for (int i = 0; i < n; ++i) {
        const gfpl_pgo_problem& p = problems[i];
        const int rc = pgo_plan(&p, prm, &plans[(size_t)i]);
        if (rc != GFPL_OK) return rc;
        const gfpl_pgo_counts& c = plans[(size_t)i].n;
        if (!p.T_kf || !p.x_kf || (c.n_pt > 0 && !p.pt) || (c.n_ls > 0 && !p.ls)) return GFPL_E_INVALID;
    }
    if (n > g->max_problems) return GFPL_E_CAPACITY;
    for (int i = 0; i < n; ++i)
        if (!fits(plans[(size_t)i].n, g->caps)) return GFPL_E_CAPACITY;
    if (n == 0) return GFPL_OK;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(g->ctx)));
    hipStream_t s = stream_of(g->ctx);

    PgoProb* hp = reinterpret_cast<PgoProb*>(g->stage + g->idx_stride * (size_t)g->max_problems);
    g->last.assign((size_t)n, PgoProb{});
    g->timed = false;
    int max_jobs = 0;
    std::vector<size_t> idx_bytes((size_t)n);
    for (int i = 0; i < n; ++i) {
        const gfpl_pgo_problem& p = problems[i];
        const PgoPlan& pl = plans[(size_t)i];
        const gfpl_pgo_counts& c = pl.n;
        const int njobs = c.n_pt + c.n_ls;
        const PgoIdx h(g->stage + g->idx_stride * (size_t)i, c.n_kf, c.n_lc, c.n_vert, c.n_free, c.n_edge, njobs);
        const PgoIdx d(g->d_idx + g->idx_stride * (size_t)i, c.n_kf, c.n_lc, c.n_vert, c.n_free, c.n_edge, njobs);
        const PgoMem m(g->base + g->ws_stride * (size_t)i, c.n_kf, c.n_vert, c.n_free, c.n_edge, c.env_blocks);
        idx_bytes[(size_t)i] = h.bytes;
        put(h.vert, pl.vert); put(h.free_vert, pl.free_vert); put(h.edge, pl.edge); put(h.inc_start, pl.inc_start);
        put(h.inc, pl.inc); put(h.env_first, pl.env_first); put(h.env_off, pl.env_off); put(h.reach, pl.reach);
        put(h.jobs, pl.jobs);
        std::memcpy(h.lc, p.lc, (size_t)c.n_lc * 3 * sizeof(int32_t));
        std::memcpy(h.lc_pose, p.lc_pose, (size_t)c.n_lc * 6 * sizeof(double));
        for (int k = 0; k < c.n_kf; ++k) h.alive[k] = p.alive[k] ? 1 : 0;
        PgoProb& q = hp[i];
        std::memset(&q, 0, sizeof q);
        q.n = c;
        q.kf_curr = pl.kf_curr;
        q.T_kf = p.T_kf; q.x_kf = p.x_kf; q.pt = p.pt; q.ls = p.ls; q.pt_dir = p.pt_dir; q.ls_dir = p.ls_dir;
        q.vert = d.vert; q.free_vert = d.free_vert; q.edge = d.edge; q.inc_start = d.inc_start; q.inc = d.inc;
        q.env_first = d.env_first; q.env_off = d.env_off; q.reach = d.reach; q.lc = d.lc; q.alive = d.alive; q.jobs = d.jobs;
        q.lc_pose = d.lc_pose;
        q.m = m.p;
        g->last[(size_t)i] = q;
        if (njobs > max_jobs) max_jobs = njobs;
    }
    hipError_t e = hipMemcpyAsync(g->d_probs, hp, (size_t)n * sizeof(PgoProb), hipMemcpyHostToDevice, s);
    for (int i = 0; i < n && e == hipSuccess; ++i)
        e = hipMemcpyAsync(g->d_idx + g->idx_stride * (size_t)i, g->stage + g->idx_stride * (size_t)i, idx_bytes[(size_t)i],
                           hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(g->ev[0], s);
    if (e == hipSuccess) {
        PgoArgs a;
        std::memset(&a, 0, sizeof a);
        a.prm = *prm;
        a.probs = g->d_probs;
        a.out = g->d_res;
        e = launch_pgo(a, n, s);
    }
    if (e == hipSuccess) e = hipEventRecord(g->ev[1], s);
    if (e == hipSuccess && max_jobs > 0) e = launch_pgo_correct(g->d_probs, n, max_jobs, s);
    if (e == hipSuccess) e = hipEventRecord(g->ev[2], s);
    if (e == hipSuccess) e = hipMemcpyAsync(results, g->d_res, (size_t)n * sizeof(gfpl_pgo_result), hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);   // also on an error path: the staging is still in use
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: gfpl_pgo_solve failed: %s\n", hipGetErrorString(e != hipSuccess ? e : es));
        g->last.clear();
        g->poisoned = true;
        return GFPL_E_HIP;
    }
    g->timed = true;
    g->last_max_iters = prm->max_iters;
    return GFPL_OK;
}

int gfpl_pgo_debug_system(gfpl_pgo* g, int i, double* chi2, double* b, double* diag, double* env, int32_t* env_first,
                          int32_t* vert, int32_t* edge, double* Z, double* X0) {
    if (!g || i < 0) return GFPL_E_INVALID;
    if (g->poisoned || (size_t)i >= g->last.size() || g->last_max_iters != 1) return GFPL_E_STATE;
    const PgoProb& q = g->last[(size_t)i];
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(g->ctx)));
    GFPL_HIPCHK(hipStreamSynchronize(stream_of(g->ctx)));
    auto get = [](void* dst, const void* src, size_t bytes) {
        if (!dst || bytes == 0) return hipSuccess;
        return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    };
    const size_t nf = (size_t)q.n.n_free, nv = (size_t)q.n.n_vert, ne = (size_t)q.n.n_edge;
    if (chi2) {
        gfpl_pgo_result r;
        GFPL_HIPCHK(hipMemcpy(&r, g->d_res + i, sizeof r, hipMemcpyDeviceToHost));
        *chi2 = r.chi2_0;
    }
    GFPL_HIPCHK(get(b, q.m.b, nf * 6 * sizeof(double)));
    GFPL_HIPCHK(get(diag, q.m.diag, nf * 36 * sizeof(double)));
    if (nf > 0) GFPL_HIPCHK(get(env, q.m.H, (size_t)q.n.env_blocks * 36 * sizeof(double)));
    GFPL_HIPCHK(get(env_first, q.env_first, nf * sizeof(int32_t)));
    GFPL_HIPCHK(get(vert, q.vert, nv * 4 * sizeof(int32_t)));
    GFPL_HIPCHK(get(edge, q.edge, ne * 4 * sizeof(int32_t)));
    GFPL_HIPCHK(get(Z, q.m.Z, ne * 16 * sizeof(double)));
    GFPL_HIPCHK(get(X0, q.m.X0, nv * 16 * sizeof(double)));
    return GFPL_OK;
}

int gfpl_pgo_debug_ms(gfpl_pgo* g, float* ms_solve, float* ms_correct) {
    if (!g) return GFPL_E_INVALID;
    if (g->poisoned || !g->timed) return GFPL_E_STATE;
    if (ms_solve) GFPL_HIPCHK(hipEventElapsedTime(ms_solve, g->ev[0], g->ev[1]));
    if (ms_correct) GFPL_HIPCHK(hipEventElapsedTime(ms_correct, g->ev[1], g->ev[2]));
    return GFPL_OK;
}

}  // extern "C"
