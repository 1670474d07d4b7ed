// gfpl_lba.cpp — host side of the local bundle adjustment (include/gfpl.h): the
// checks of a problem's index arrays, the workspace sizes, the object that owns the device
// workspace of up to max_problems problems, the batched solve around k_lba.hip (one upload of the
// problem records and index arrays, one launch, one copy of the results, one synchronisation) and
// the test hook that reads a problem's last evaluated system back.
#include "gfpl_host.hpp"

using namespace gfpl;

static_assert(LBA_MAX_KFS == GFPL_LBA_MAX_KFS, "the LDS layout and the public cap are one number");

struct gfpl_lba {
    gfpl_ctx* ctx = nullptr;
    gfpl_lba_counts caps{};
    int max_problems = 0;
    size_t stride = 0;             // workspace bytes per problem at caps
    char* base = nullptr;          // [max_problems][stride], then the problem records and the results
    LbaProb* d_probs = nullptr;
    gfpl_lba_result* d_res = nullptr;
    char* stage = nullptr;         // pinned: the records and every problem's index arrays
    size_t stage_bytes = 0;
    std::vector<LbaProb> last;     // the last solve's records (device pointers), for the test hook
};

namespace {

int check_counts(const gfpl_lba_counts& n) {
    if (n.n_kf < 1 || n.n_fix < 0 || n.n_pt < 0 || n.n_ls < 0 || n.n_pt_obs < 0 || n.n_ls_obs < 0) return GFPL_E_INVALID;
    if (n.n_kf > GFPL_LBA_MAX_KFS) return GFPL_E_CAPACITY;
    return GFPL_OK;
}

// landmark ids 0 .. n - 1, contiguous, each at least once; slots in [-n_fix, n_kf)
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

namespace gfpl {

gfpl_ctx* lba_ctx(const gfpl_lba* l) { return l->ctx; }

int lba_stage_device(gfpl_lba* l, const gfpl_lba_problem& p, LbaProb* q) {
    const gfpl_lba_counts& c = p.n;
    if (c.n_kf > l->caps.n_kf || c.n_pt > l->caps.n_pt || c.n_ls > l->caps.n_ls || c.n_pt_obs > l->caps.n_pt_obs ||
        c.n_ls_obs > l->caps.n_ls_obs)
        return GFPL_E_CAPACITY;
    const LbaMem m(l->base, c.n_kf, c.n_pt, c.n_ls, c.n_pt_obs + c.n_ls_obs);
    LbaProb& h = *reinterpret_cast<LbaProb*>(l->stage);
    std::memset(&h, 0, sizeof h);
    h.n = c;
    ba_fill_prob(h, p);
    h.lm_start = m.lm_start; h.obs_lm = m.obs_lm; h.obs_kf = m.obs_kf;
    h.m = m.p;
    l->last.assign(1, h);
    *q = h;
    return GFPL_OK;
}

// the staged records to the device, the launch, the results to the host
hipError_t lba_enqueue(gfpl_lba* l, int n, int lds_kfs, const gfpl_lba_params* prm, gfpl_lba_result* results, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(l->d_probs, l->stage, (size_t)n * sizeof(LbaProb), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    LbaArgs a;
    std::memset(&a, 0, sizeof a);
    a.cam = dev_cam(gfpl_ctx_camera(l->ctx));
    a.homog_th = gfpl_ctx_config(l->ctx)->homog_th;
    a.prm = *prm;
    a.probs = l->d_probs;
    a.out = l->d_res;
    a.lds_kfs = lds_kfs;
    e = launch_lba(a, n, s);
    if (e == hipSuccess) e = hipMemcpyAsync(results, l->d_res, (size_t)n * sizeof(gfpl_lba_result), hipMemcpyDeviceToHost, s);
    return e;
}

}  // namespace gfpl

extern "C" {

void gfpl_default_lba_params(gfpl_lba_params* prm) {
    if (!prm) return;
    prm->lambda_lm = 0.001;
    prm->lambda_k = 10.0;
    prm->max_iters = 20;
    prm->pad = 0;
}

int gfpl_lba_check(const gfpl_lba_problem* p) {
    if (!p) return GFPL_E_INVALID;
    const int rc = check_counts(p->n);
    if (rc != GFPL_OK) return rc;
    if (p->n.n_pt_obs + p->n.n_ls_obs == 0) return GFPL_E_INVALID;
    const int rp = check_list(p->pt_obs_lm, p->pt_obs_kf, p->n.n_pt_obs, p->n.n_pt, p->n.n_kf, p->n.n_fix);
    if (rp != GFPL_OK) return rp;
    return check_list(p->ls_obs_lm, p->ls_obs_kf, p->n.n_ls_obs, p->n.n_ls, p->n.n_kf, p->n.n_fix);
}

int gfpl_lba_workspace(const gfpl_lba_counts* n, int64_t* hbm_bytes, int32_t* lds_bytes) {
    if (!n) return GFPL_E_INVALID;
    const int rc = check_counts(*n);
    if (rc != GFPL_OK) return rc;
    if (hbm_bytes) *hbm_bytes = (int64_t)LbaMem(nullptr, n->n_kf, n->n_pt, n->n_ls, n->n_pt_obs + n->n_ls_obs).bytes;
    if (lds_bytes) *lds_bytes = LbaLds(nullptr, n->n_kf).bytes;
    return GFPL_OK;
}

int gfpl_lba_create(gfpl_ctx* c, const gfpl_lba_counts* caps, int max_problems, gfpl_lba** out) {
    if (!c || !caps || !out || max_problems < 1) return GFPL_E_INVALID;
    const int rc = check_counts(*caps);
    if (rc != GFPL_OK) return rc;
    if (!gfpl_ctx_camera(c)) return GFPL_E_STATE;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(c)));
    gfpl_lba* l = new gfpl_lba();
    l->ctx = c;
    l->caps = *caps;
    l->max_problems = max_problems;
    const int nobs = caps->n_pt_obs + caps->n_ls_obs;
    l->stride = LbaMem(nullptr, caps->n_kf, caps->n_pt, caps->n_ls, nobs).bytes;
    const size_t b_probs = up256((size_t)max_problems * sizeof(LbaProb));
    const size_t b_res = up256((size_t)max_problems * sizeof(gfpl_lba_result));
    // a problem's three index arrays are staged at LbaMem's distances (each field 256-B aligned)
    const size_t b_idx = up256(up256(((size_t)caps->n_pt + caps->n_ls + 1) * sizeof(int32_t)) +
                               2 * up256((size_t)nobs * sizeof(int32_t)));
    if (hipMalloc(&l->base, l->stride * max_problems + b_probs + b_res) != hipSuccess) {
        (void)hipGetLastError();
        delete l;
        return GFPL_E_NOMEM;
    }
    l->d_probs = reinterpret_cast<LbaProb*>(l->base + l->stride * max_problems);
    l->d_res = reinterpret_cast<gfpl_lba_result*>(l->base + l->stride * max_problems + b_probs);
    l->stage_bytes = b_probs + b_idx * max_problems;
    if (hipHostMalloc((void**)&l->stage, l->stage_bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(l->base);
        delete l;
        return GFPL_E_NOMEM;
    }
    gfpl_ctx_attach(c);
    *out = l;
    return GFPL_OK;
}

int gfpl_lba_destroy(gfpl_lba* l) {
    if (!l) return GFPL_E_INVALID;
    (void)hipSetDevice(gfpl_ctx_device(l->ctx));
    (void)hipStreamSynchronize(stream_of(l->ctx));
    (void)hipHostFree(l->stage);
    (void)hipFree(l->base);
    gfpl_ctx_detach(l->ctx);
    delete l;
    return GFPL_OK;
}

int gfpl_lba_solve(gfpl_lba* l, const gfpl_lba_problem* problems, int n, const gfpl_lba_params* prm,
                   gfpl_lba_result* results) {
    if (!l || n < 0 || (n > 0 && (!problems || !results)) || !prm) return GFPL_E_INVALID;
    if (!(prm->lambda_k != 0.0)) return GFPL_E_INVALID;
    for (int i = 0; i < n; ++i) {
        const gfpl_lba_problem& p = problems[i];
        const int rc = gfpl_lba_check(&p);
        if (rc != GFPL_OK) return rc;
        if (!ba_problem_pointers_ok(p)) return GFPL_E_INVALID;
    }
    if (n > l->max_problems) return GFPL_E_CAPACITY;
    for (int i = 0; i < n; ++i) {
        const gfpl_lba_counts& c = problems[i].n;
        if (c.n_kf > l->caps.n_kf || c.n_pt > l->caps.n_pt || c.n_ls > l->caps.n_ls || c.n_pt_obs > l->caps.n_pt_obs ||
            c.n_ls_obs > l->caps.n_ls_obs)
            return GFPL_E_CAPACITY;
    }
    if (n == 0) return GFPL_OK;
    const gfpl_camera* cam = gfpl_ctx_camera(l->ctx);
    if (!cam) return GFPL_E_STATE;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(l->ctx)));
    hipStream_t s = stream_of(l->ctx);

    // the records and the index arrays, staged once.  A problem's indices travel to its own workspace.
    LbaProb* hp = reinterpret_cast<LbaProb*>(l->stage);
    int lds_kfs = 1;
    l->last.assign((size_t)n, LbaProb{});
    std::vector<int32_t*> hidx((size_t)n);
    int32_t* cursor = reinterpret_cast<int32_t*>(l->stage + up256((size_t)l->max_problems * sizeof(LbaProb)));
    for (int i = 0; i < n; ++i) {
        const gfpl_lba_problem& p = problems[i];
        const int nobs = p.n.n_pt_obs + p.n.n_ls_obs, nlm = p.n.n_pt + p.n.n_ls;
        const LbaMem m(l->base + l->stride * (size_t)i, p.n.n_kf, p.n.n_pt, p.n.n_ls, nobs);
        LbaProb& q = hp[i];
        std::memset(&q, 0, sizeof q);
        q.n = p.n;
        ba_fill_prob(q, p);
        q.lm_start = m.lm_start; q.obs_lm = m.obs_lm; q.obs_kf = m.obs_kf;
        q.m = m.p;
        l->last[(size_t)i] = q;
        if (p.n.n_kf > lds_kfs) lds_kfs = p.n.n_kf;
        // lm_start [nlm + 1], obs_lm [nobs], obs_kf [nobs] over the unified numbering (points first).
        // LbaMem lays the three out apart (256-B fields), so they are staged at the same distances.
        int32_t* h = cursor;
        hidx[(size_t)i] = h;
        const size_t o_lm = (size_t)((char*)m.obs_lm - (char*)m.lm_start) / sizeof(int32_t);
        const size_t o_kf = (size_t)((char*)m.obs_kf - (char*)m.lm_start) / sizeof(int32_t);
        int32_t *start = h, *olm = h + o_lm, *okf = h + o_kf;
        int j = 0;
        for (int o = 0; o < p.n.n_pt_obs; ++o) {
            if (o == 0 || p.pt_obs_lm[o] != p.pt_obs_lm[o - 1]) start[j++] = o;
            olm[o] = p.pt_obs_lm[o];
            okf[o] = p.pt_obs_kf[o];
        }
        for (int o = 0; o < p.n.n_ls_obs; ++o) {
            if (o == 0 || p.ls_obs_lm[o] != p.ls_obs_lm[o - 1]) start[j++] = p.n.n_pt_obs + o;
            olm[p.n.n_pt_obs + o] = p.n.n_pt + p.ls_obs_lm[o];
            okf[p.n.n_pt_obs + o] = p.ls_obs_kf[o];
        }
        start[nlm] = nobs;
        cursor += (o_kf + (size_t)nobs + 63) & ~(size_t)63;
    }
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        const LbaProb& q = l->last[(size_t)i];
        const size_t cnt = (size_t)(q.obs_kf - q.lm_start) + (size_t)(q.n.n_pt_obs + q.n.n_ls_obs);
        e = hipMemcpyAsync(const_cast<int32_t*>(q.lm_start), hidx[(size_t)i], cnt * sizeof(int32_t), hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) e = lba_enqueue(l, n, lds_kfs, prm, results, s);
    const hipError_t es = hipStreamSynchronize(s);   // also on an error path: the staging is still in use
    if (e != hipSuccess || es != hipSuccess) {
        l->last.clear();
        return GFPL_E_HIP;
    }
    return GFPL_OK;
}

int gfpl_lba_debug_system(gfpl_lba* l, int i, int iteration, double* U, double* g, double* V_pt, double* V_ls,
                          double* W_pt, double* W_ls, double* err) {
    if (!l || i < 0 || iteration < 0) return GFPL_E_INVALID;
    if ((size_t)i >= l->last.size()) return GFPL_E_STATE;
    const LbaProb& q = l->last[(size_t)i];
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(l->ctx)));
    GFPL_HIPCHK(hipStreamSynchronize(stream_of(l->ctx)));
    int32_t state[8];
    GFPL_HIPCHK(hipMemcpy(state, q.m.state, sizeof state, hipMemcpyDeviceToHost));
    if (state[0] != iteration) return GFPL_E_STATE;
    const size_t nkf = (size_t)q.n.n_kf, npt = (size_t)q.n.n_pt, nls = (size_t)q.n.n_ls;
    const int rc = ba_read_system(q.m, q.n, l->d_res + i, U, g, V_pt, V_ls, err);
    if (rc != GFPL_OK) return rc;
    // the blocks of keyframes that do not observe a landmark are never written on the device: they are zero
    std::vector<int32_t> mask(npt + nls);
    if (npt + nls) GFPL_HIPCHK(hipMemcpy(mask.data(), q.m.mask, (npt + nls) * sizeof(int32_t), hipMemcpyDeviceToHost));
    GFPL_HIPCHK(get_doubles(W_pt, q.m.W, nkf * 18 * npt));
    GFPL_HIPCHK(get_doubles(W_ls, q.m.W + nkf * 18 * npt, nkf * 36 * nls));
    for (size_t j = 0; j < npt + nls; ++j)
        for (size_t s = 0; s < nkf; ++s) {
            if ((mask[j] >> s) & 1) continue;
            if (j < npt) { if (W_pt) std::memset(W_pt + (j * nkf + s) * 18, 0, 18 * sizeof(double)); }
            else if (W_ls) std::memset(W_ls + ((j - npt) * nkf + s) * 36, 0, 36 * sizeof(double));
        }
    return GFPL_OK;
}

}  // extern "C"
