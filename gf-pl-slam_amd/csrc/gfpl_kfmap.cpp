// gfpl_kfmap.cpp — host side of the map's index half (include/gfpl.h): the object that
// owns the one device allocation (KfMapMem), a host copy of the few words every argument check needs
// (n_kf, the next ids, each keyframe's alive flag and row counts), and per call: the argument checks,
// the call's launches in stream order, one copy of the header and one synchronisation.
#include <algorithm>

#include "gfpl_host.hpp"

using namespace gfpl;

struct gfpl_kfmap {
    gfpl_ctx* ctx = nullptr;
    gfpl_kfmap_caps caps{};
    char* base = nullptr;
    size_t bytes = 0;
    int32_t* h_hdr = nullptr;            // pinned [2 * KFMAP_HDR]: the header's copy, then staging for a header write
    int n_kf = 0, next[2] = {0, 0};      // the header's words as the last call left them
    std::vector<uint8_t> kf_alive;
    std::vector<int32_t> kf_n[2];
    int epoch = 0;                       // observe calls so far (KfMapMem::seen0 / seen1)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool failed = false;
};

namespace {

bool caps_ok(const gfpl_kfmap_caps* c) {
    const int32_t lim = 1 << 30;
    return c && c->kf_cap >= 1 && c->kf_cap <= 65535 && c->pt_rows >= 1 && c->ls_rows >= 1 && c->pt_lm_cap >= 1 &&
           c->ls_lm_cap >= 1 && c->pt_rows <= lim && c->ls_rows <= lim && c->pt_lm_cap <= lim && c->ls_lm_cap <= lim &&
           c->obs_cap >= 2 && c->obs_cap <= GFPL_LM_MAX_OBS;
}

KfMapMem mem_of(char* base, const gfpl_kfmap_caps& c) {
    return KfMapMem(base, c.kf_cap, c.pt_rows, c.ls_rows, c.pt_lm_cap, c.ls_lm_cap, c.obs_cap);
}

KfMapCore core_of(const gfpl_kfmap* m) {
    const KfMapMem k = mem_of(m->base, m->caps);
    return KfMapCore{k.hdr, k.kf_alive, k.kf_local, k.graph, k.tile, k.seen0, k.seen1, k.pend, k.first_row,
                     k.pair_n0, k.pair_slot, k.kf_cap, k.obs_cap, m->n_kf};
}

KfMapLm lm_of(const gfpl_kfmap* m, int kind) {
    const KfMapMem k = mem_of(m->base, m->caps);
    return KfMapLm{k.lm_alive[kind], k.lm_local[kind], k.lm_inlier[kind], k.lm_nobs[kind], k.lm_owner[kind], k.lm_obs[kind],
                   k.kf_idx[kind], k.kf_n[kind], k.rows[kind], k.lm_cap[kind], m->next[kind]};
}

bool kf_ok(const gfpl_kfmap* m, int kf) { return kf >= 0 && kf < m->n_kf && m->kf_alive[(size_t)kf]; }

// a call's start: the device, the call's header words zeroed, the first event
hipError_t begin(gfpl_kfmap* m, hipStream_t* s) {
    *s = stream_of(m->ctx);
    m->timed = false;
    hipError_t e = hipSetDevice(gfpl_ctx_device(m->ctx));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(core_of(m).hdr, 0, KFMAP_H_CALL * sizeof(int32_t), *s);
    if (e == hipSuccess) e = hipEventRecord(m->ev0, *s);
    return e;
}

// a call's end: the second event, the header to the host, the call's one synchronisation.  Returns the
// call's code: the device's refusal when there is one.
int finish(gfpl_kfmap* m, hipStream_t s, hipError_t e, const char* what) {
    if (e == hipSuccess) e = hipEventRecord(m->ev1, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->h_hdr, core_of(m).hdr, KFMAP_HDR * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: kfmap_%s failed: %s\n", what, hipGetErrorString(e != hipSuccess ? e : es));
        (void)hipGetLastError();
        m->failed = true;   // some launches may have run: the state is not known any more
        return GFPL_E_HIP;
    }
    m->timed = true;
    m->n_kf = m->h_hdr[KFMAP_H_NKF];
    m->next[0] = m->h_hdr[KFMAP_H_NEXT_PT];
    m->next[1] = m->h_hdr[KFMAP_H_NEXT_LS];
    const int err = m->h_hdr[KFMAP_H_ERR];
    if (err & KFMAP_ERR_INVALID) return GFPL_E_INVALID;
    if (err & KFMAP_ERR_CAPACITY) return GFPL_E_CAPACITY;
    return GFPL_OK;
}

#define KFMAP_ENTER(m)                    \
    do {                                  \
        if (!(m)) return GFPL_E_INVALID;  \
        if ((m)->failed) return GFPL_E_STATE; \
    } while (0)

// synchronous copies of the read / patch calls
int copy_sync(gfpl_kfmap* m, hipError_t e, const char* what) {
    const hipError_t es = hipStreamSynchronize(stream_of(m->ctx));
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: kfmap_%s failed: %s\n", what, hipGetErrorString(e != hipSuccess ? e : es));
        (void)hipGetLastError();
        return GFPL_E_HIP;
    }
    return GFPL_OK;
}

template <typename T>
hipError_t get(hipError_t e, T* dst, const T* src, size_t n, hipStream_t s) {
    if (e != hipSuccess || !dst || n == 0) return e;
    return hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, s);
}
template <typename T>
hipError_t put_dev(hipError_t e, T* dst, const T* src, size_t n, hipStream_t s) {
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, s);
}

}  // namespace

namespace gfpl {
KfMapDevice kfmap_device(const gfpl_kfmap* m) { return KfMapDevice{m->ctx, m->caps, core_of(m), {lm_of(m, 0), lm_of(m, 1)}, m->failed}; }
}  // namespace gfpl

extern "C" {

void gfpl_default_kfmap_params(gfpl_kfmap_params* prm) {
    if (!prm) return;
    prm->min_lm_cov_graph = 30;
    prm->min_kf_local_map = 3;
    prm->min_lm_obs = 2;
    prm->cull_age = 10;
}

int64_t gfpl_kfmap_bytes(const gfpl_kfmap_caps* caps) {
    if (!caps_ok(caps)) return -1;
    return (int64_t)mem_of(nullptr, *caps).bytes;
}

int gfpl_kfmap_create(gfpl_ctx* c, const gfpl_kfmap_caps* caps, gfpl_kfmap** out) {
    if (!c || !out || !caps_ok(caps)) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(c)));
    gfpl_kfmap* m = new gfpl_kfmap();
    m->ctx = c;
    m->caps = *caps;
    m->bytes = mem_of(nullptr, *caps).bytes;
    hipStream_t s = stream_of(c);
    auto drop = [&](int code) {
        (void)hipGetLastError();
        if (m->ev0) (void)hipEventDestroy(m->ev0);
        if (m->ev1) (void)hipEventDestroy(m->ev1);
        if (m->h_hdr) (void)hipHostFree(m->h_hdr);
        if (m->base) (void)hipFree(m->base);
        delete m;
        return code;
    };
    if (hipMalloc(&m->base, m->bytes) != hipSuccess ||
        hipHostMalloc((void**)&m->h_hdr, 2 * KFMAP_HDR * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
        return drop(GFPL_E_NOMEM);
    // initialize's resets (:42-58), and every byte a kernel may read: all zero, then remove_bad's rows
    const KfMapMem k = mem_of(m->base, *caps);
    bool ok = hipMemsetAsync(m->base, 0, m->bytes, s) == hipSuccess &&
              hipMemsetD32Async((hipDeviceptr_t)k.first_row, 0x7fffffff, k.max_lm, s) == hipSuccess &&
              hipStreamSynchronize(s) == hipSuccess;
    ok = ok && hipEventCreate(&m->ev0) == hipSuccess && hipEventCreate(&m->ev1) == hipSuccess;
    if (!ok) return drop(GFPL_E_HIP);
    m->kf_alive.assign((size_t)caps->kf_cap, 0);
    m->kf_n[0].assign((size_t)caps->kf_cap, 0);
    m->kf_n[1].assign((size_t)caps->kf_cap, 0);
    gfpl_ctx_attach(c);
    *out = m;
    return GFPL_OK;
}

int gfpl_kfmap_destroy(gfpl_kfmap* m) {
    if (!m) return GFPL_E_INVALID;
    (void)hipSetDevice(gfpl_ctx_device(m->ctx));
    (void)hipStreamSynchronize(stream_of(m->ctx));
    (void)hipEventDestroy(m->ev0);
    (void)hipEventDestroy(m->ev1);
    (void)hipHostFree(m->h_hdr);
    (void)hipFree(m->base);
    gfpl_ctx_detach(m->ctx);
    delete m;
    return GFPL_OK;
}

int gfpl_kfmap_counts(const gfpl_kfmap* m, int32_t* n_kf, int32_t* next_pt, int32_t* next_ls) {
    if (!m) return GFPL_E_INVALID;
    if (m->failed) return GFPL_E_STATE;
    if (n_kf) *n_kf = m->n_kf;
    if (next_pt) *next_pt = m->next[0];
    if (next_ls) *next_ls = m->next[1];
    return GFPL_OK;
}

int gfpl_kfmap_add_keyframe(gfpl_kfmap* m, int n_pt, int n_ls, int32_t* kf_idx) {
    KFMAP_ENTER(m);
    if (!kf_idx || n_pt < 0 || n_ls < 0) return GFPL_E_INVALID;
    if (m->n_kf >= m->caps.kf_cap || n_pt > m->caps.pt_rows || n_ls > m->caps.ls_rows) return GFPL_E_CAPACITY;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    const int kf = m->n_kf;
    if (e == hipSuccess) e = enqueue_kfmap_add_keyframe(core_of(m), lm_of(m, 0), lm_of(m, 1), n_pt, n_ls, s);
    const int rc = finish(m, s, e, "add_keyframe");
    if (rc != GFPL_OK) return rc;
    m->kf_alive[(size_t)kf] = 1;
    m->kf_n[0][(size_t)kf] = n_pt;
    m->kf_n[1][(size_t)kf] = n_ls;
    *kf_idx = kf;
    return GFPL_OK;
}

int gfpl_kfmap_observe_pairs(gfpl_kfmap* m, int kind, int kf0, int kf1, const int32_t* pairs, int n, int32_t* lm_out,
                             int32_t* first_new, int32_t* n_new) {
    KFMAP_ENTER(m);
    if (!first_new || !n_new || n < 0 || (n > 0 && (!pairs || !lm_out)) || kind < 0 || kind > 1) return GFPL_E_INVALID;
    if (!kf_ok(m, kf0) || !kf_ok(m, kf1) || kf0 == kf1) return GFPL_E_INVALID;
    // more pairs than rows: a column holds a value twice or a row is out of range
    if (n > std::min(m->kf_n[kind][(size_t)kf0], m->kf_n[kind][(size_t)kf1])) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    const KfMapObserve a{kind, kf0, kf1, n, 0, 0, ++m->epoch, pairs, nullptr, nullptr, lm_out};
    if (e == hipSuccess) e = enqueue_kfmap_observe(core_of(m), lm_of(m, kind), a, s);
    const int rc = finish(m, s, e, "observe_pairs");
    if (rc != GFPL_OK) return rc;
    *first_new = m->h_hdr[KFMAP_H_FIRST_NEW];
    *n_new = m->h_hdr[KFMAP_H_COUNT0];
    return GFPL_OK;
}

int gfpl_kfmap_observe_local(gfpl_kfmap* m, int kind, int kf1, const int32_t* pairs, int n, const int32_t* sel_ids, int n_sel,
                             const int32_t* unm_rows, int n_unm, int32_t* lm_out) {
    KFMAP_ENTER(m);
    if (n < 0 || n_sel < 0 || n_unm < 0 || (n > 0 && (!pairs || !lm_out || !sel_ids || !unm_rows)) || kind < 0 || kind > 1)
        return GFPL_E_INVALID;
    if (!kf_ok(m, kf1)) return GFPL_E_INVALID;
    if (n_sel > m->next[kind] || n_unm > m->kf_n[kind][(size_t)kf1] || n > std::min(n_sel, n_unm)) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    const KfMapObserve a{kind, -1, kf1, n, n_sel, n_unm, ++m->epoch, pairs, sel_ids, unm_rows, lm_out};
    if (e == hipSuccess) e = enqueue_kfmap_observe(core_of(m), lm_of(m, kind), a, s);
    return finish(m, s, e, "observe_local");
}

int gfpl_kfmap_form_local_map(gfpl_kfmap* m, const gfpl_kfmap_params* prm) {
    KFMAP_ENTER(m);
    if (!prm) return GFPL_E_INVALID;
    if (m->n_kf < 1 || !m->kf_alive[(size_t)m->n_kf - 1]) return GFPL_E_STATE;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    if (e == hipSuccess)
        e = enqueue_kfmap_form_local_map(core_of(m), lm_of(m, 0), lm_of(m, 1), prm->min_lm_cov_graph, prm->min_kf_local_map, s);
    return finish(m, s, e, "form_local_map");
}

int gfpl_kfmap_select(gfpl_kfmap* m, int kind, int which, int kf1, int32_t* ids, int32_t* n) {
    KFMAP_ENTER(m);
    if (!n || kind < 0 || kind > 1 || which < GFPL_KFMAP_LOCAL || which > GFPL_KFMAP_ALIVE) return GFPL_E_INVALID;
    if (which == GFPL_KFMAP_LOCAL_UNSEEN && !kf_ok(m, kf1)) return GFPL_E_INVALID;
    if (m->next[kind] > 0 && !ids) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    const KfMapSelect a{which, kf1, m->next[kind], KFMAP_H_COUNT0, 0, 0, ids};
    if (e == hipSuccess) e = enqueue_kfmap_select(core_of(m), lm_of(m, kind), a, s);
    const int rc = finish(m, s, e, "select");
    if (rc == GFPL_OK) *n = m->h_hdr[KFMAP_H_COUNT0];
    return rc;
}

int gfpl_kfmap_unmatched(gfpl_kfmap* m, int kind, int kf, int32_t* rows, int32_t* n) {
    KFMAP_ENTER(m);
    if (!n || kind < 0 || kind > 1 || !kf_ok(m, kf)) return GFPL_E_INVALID;
    const int n_rows = m->kf_n[kind][(size_t)kf];
    if (n_rows > 0 && !rows) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    const KfMapSelect a{KFMAP_SEL_UNMATCHED, kf, n_rows, KFMAP_H_COUNT0, 0, 0, rows};
    if (e == hipSuccess) e = enqueue_kfmap_select(core_of(m), lm_of(m, kind), a, s);
    const int rc = finish(m, s, e, "unmatched");
    if (rc == GFPL_OK) *n = m->h_hdr[KFMAP_H_COUNT0];
    return rc;
}

int gfpl_kfmap_local_keyframes(gfpl_kfmap* m, int32_t* kf_list, int32_t* n) {
    KFMAP_ENTER(m);
    if (!kf_list || !n) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(m->ctx)));
    std::vector<uint8_t> local((size_t)m->n_kf);
    const int rc = copy_sync(m, get(hipSuccess, local.data(), core_of(m).kf_local, local.size(), stream_of(m->ctx)), "local_keyframes");
    if (rc != GFPL_OK) return rc;
    int cnt = 0;
    for (int k = 1; k < m->n_kf; ++k)   // kf_idx != 0 (:1119)
        if (m->kf_alive[(size_t)k] && local[(size_t)k]) kf_list[cnt++] = k;
    *n = cnt;
    return GFPL_OK;
}

int gfpl_kfmap_remove_bad(gfpl_kfmap* m, const gfpl_kfmap_params* prm, int32_t* pt_removed, int32_t* n_pt, int32_t* ls_removed,
                          int32_t* n_ls) {
    KFMAP_ENTER(m);
    if (!prm || !n_pt || !n_ls || (m->next[0] > 0 && !pt_removed) || (m->next[1] > 0 && !ls_removed)) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    int32_t* out[2] = {pt_removed, ls_removed};
    for (int kind = 0; kind < 2 && e == hipSuccess; ++kind) {
        const KfMapSelect a{KFMAP_SEL_BAD, 0, m->next[kind], kind ? KFMAP_H_COUNT1 : KFMAP_H_COUNT0, prm->min_lm_obs,
                            prm->cull_age, out[kind]};
        e = enqueue_kfmap_remove_bad(core_of(m), lm_of(m, kind), a, s);
    }
    const int rc = finish(m, s, e, "remove_bad");
    if (rc != GFPL_OK) return rc;
    *n_pt = m->h_hdr[KFMAP_H_COUNT0];
    *n_ls = m->h_hdr[KFMAP_H_COUNT1];
    return GFPL_OK;
}

int gfpl_kfmap_set_inlier(gfpl_kfmap* m, int kind, const int32_t* ids, int n, int value) {
    KFMAP_ENTER(m);
    if (n < 0 || (n > 0 && !ids) || kind < 0 || kind > 1 || value < 0 || value > 1) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    if (e == hipSuccess) e = enqueue_kfmap_set_inlier(core_of(m), lm_of(m, kind), ids, n, value, s);
    return finish(m, s, e, "set_inlier");
}

int gfpl_kfmap_erase_keyframe(gfpl_kfmap* m, int kf) {
    KFMAP_ENTER(m);
    if (!kf_ok(m, kf)) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(m, &s);
    if (e == hipSuccess) e = enqueue_kfmap_erase_keyframe(core_of(m), kf, s);
    const int rc = finish(m, s, e, "erase_keyframe");
    if (rc == GFPL_OK) m->kf_alive[(size_t)kf] = 0;
    return rc;
}

int gfpl_kfmap_read_keyframe(gfpl_kfmap* m, int kf, gfpl_kfmap_kf* rec, int32_t* pt_idx, int32_t* ls_idx) {
    KFMAP_ENTER(m);
    if (kf < 0 || kf >= m->n_kf) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(m->ctx)));
    hipStream_t s = stream_of(m->ctx);
    const KfMapMem k = mem_of(m->base, m->caps);
    uint8_t local = 0;
    hipError_t e = get(hipSuccess, &local, k.kf_local + kf, 1, s);
    e = get(e, pt_idx, k.kf_idx[0] + (size_t)kf * k.rows[0], (size_t)k.rows[0], s);
    e = get(e, ls_idx, k.kf_idx[1] + (size_t)kf * k.rows[1], (size_t)k.rows[1], s);
    const int rc = copy_sync(m, e, "read_keyframe");
    if (rc != GFPL_OK) return rc;
    if (rec) *rec = gfpl_kfmap_kf{m->kf_alive[(size_t)kf], local, m->kf_n[0][(size_t)kf], m->kf_n[1][(size_t)kf]};
    return GFPL_OK;
}

int gfpl_kfmap_write_keyframe_idx(gfpl_kfmap* m, int kind, int kf, int row0, int n, const int32_t* idx) {
    KFMAP_ENTER(m);
    if (kind < 0 || kind > 1 || !kf_ok(m, kf) || n < 0 || (n > 0 && !idx) || row0 < 0) return GFPL_E_INVALID;
    if (n > m->kf_n[kind][(size_t)kf] - row0) return GFPL_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (idx[i] < -1 || idx[i] >= m->next[kind]) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(m->ctx)));
    const KfMapMem k = mem_of(m->base, m->caps);
    return copy_sync(m, put_dev(hipSuccess, k.kf_idx[kind] + (size_t)kf * k.rows[kind] + row0, idx, (size_t)n, stream_of(m->ctx)),
                     "write_keyframe_idx");
}

int gfpl_kfmap_read_landmarks(gfpl_kfmap* m, int kind, int id0, int n, uint8_t* alive, uint8_t* local, uint8_t* inlier,
                              int32_t* n_obs, int32_t* owner, int32_t* kf_obs) {
    KFMAP_ENTER(m);
    const KfMapMem k = mem_of(m->base, m->caps);
    if (kind < 0 || kind > 1 || id0 < 0 || n < 0 || n > k.lm_cap[kind] - id0) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(m->ctx)));
    hipStream_t s = stream_of(m->ctx);
    hipError_t e = get(hipSuccess, alive, k.lm_alive[kind] + id0, (size_t)n, s);
    e = get(e, local, k.lm_local[kind] + id0, (size_t)n, s);
    e = get(e, inlier, k.lm_inlier[kind] + id0, (size_t)n, s);
    e = get(e, n_obs, k.lm_nobs[kind] + id0, (size_t)n, s);
    e = get(e, owner, k.lm_owner[kind] + id0, (size_t)n, s);
    e = get(e, kf_obs, k.lm_obs[kind] + (size_t)id0 * k.obs_cap, (size_t)n * k.obs_cap, s);
    return copy_sync(m, e, "read_landmarks");
}

int gfpl_kfmap_write_landmarks(gfpl_kfmap* m, int kind, int id0, int n, const uint8_t* alive, const uint8_t* local,
                               const uint8_t* inlier, const int32_t* n_obs, const int32_t* owner, const int32_t* kf_obs) {
    KFMAP_ENTER(m);
    const KfMapMem k = mem_of(m->base, m->caps);
    if (kind < 0 || kind > 1 || id0 < 0 || n < 0 || n > k.lm_cap[kind] - id0) return GFPL_E_INVALID;
    if (n == 0) return GFPL_OK;
    if (!alive || !local || !inlier || !n_obs || !owner || !kf_obs) return GFPL_E_INVALID;
    for (int i = 0; i < n; ++i) {
        if (alive[i] > 1 || local[i] > 1 || inlier[i] > 1) return GFPL_E_INVALID;
        if (n_obs[i] < (alive[i] ? 1 : 0) || n_obs[i] > k.obs_cap) return GFPL_E_INVALID;
        if (owner[i] < -1 || owner[i] >= m->n_kf) return GFPL_E_INVALID;
        for (int e = 0; e < n_obs[i]; ++e) {
            const int32_t kf = kf_obs[(size_t)i * k.obs_cap + e];
            if (kf < 0 || kf >= m->n_kf) return GFPL_E_INVALID;
        }
    }
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(m->ctx)));
    hipStream_t s = stream_of(m->ctx);
    hipError_t e = put_dev(hipSuccess, k.lm_alive[kind] + id0, alive, (size_t)n, s);
    e = put_dev(e, k.lm_local[kind] + id0, local, (size_t)n, s);
    e = put_dev(e, k.lm_inlier[kind] + id0, inlier, (size_t)n, s);
    e = put_dev(e, k.lm_nobs[kind] + id0, n_obs, (size_t)n, s);
    e = put_dev(e, k.lm_owner[kind] + id0, owner, (size_t)n, s);
    e = put_dev(e, k.lm_obs[kind] + (size_t)id0 * k.obs_cap, kf_obs, (size_t)n * k.obs_cap, s);
    const int next = std::max(m->next[kind], id0 + n);
    int32_t* stage = m->h_hdr + KFMAP_HDR;
    *stage = next;
    e = put_dev(e, k.hdr + (kind ? KFMAP_H_NEXT_LS : KFMAP_H_NEXT_PT), (const int32_t*)stage, 1, s);
    const int rc = copy_sync(m, e, "write_landmarks");
    if (rc != GFPL_OK) {
        m->failed = true;   // some of the arrays may have been written
        return rc;
    }
    m->next[kind] = next;
    return GFPL_OK;
}

int gfpl_kfmap_export_graph(gfpl_kfmap* m, uint8_t* alive, int32_t* full_graph, int32_t* pt_kf_start, int32_t* pt_kf_idx,
                            uint8_t* pt_freed, int32_t* ls_kf_start, int32_t* ls_kf_idx, uint8_t* ls_freed) {
    KFMAP_ENTER(m);
    if (!alive || !full_graph) return GFPL_E_INVALID;
    int32_t* start[2] = {pt_kf_start, ls_kf_start};
    int32_t* idx[2] = {pt_kf_idx, ls_kf_idx};
    uint8_t* freed[2] = {pt_freed, ls_freed};
    for (int kind = 0; kind < 2; ++kind) {
        const int given = (start[kind] != nullptr) + (idx[kind] != nullptr) + (freed[kind] != nullptr);
        if (given != 0 && given != 3) return GFPL_E_INVALID;
    }
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(m->ctx)));
    hipStream_t s = stream_of(m->ctx);
    const KfMapMem k = mem_of(m->base, m->caps);
    const size_t nkf = (size_t)m->n_kf;
    hipError_t e = hipSuccess;
    if (nkf > 0)
        e = hipMemcpy2DAsync(full_graph, nkf * sizeof(int32_t), k.graph, (size_t)k.kf_cap * sizeof(int32_t), nkf * sizeof(int32_t),
                             nkf, hipMemcpyDeviceToHost, s);
    std::vector<int32_t> owner[2];
    for (int kind = 0; kind < 2; ++kind) {
        if (!start[kind]) continue;
        owner[kind].resize((size_t)m->next[kind]);
        e = get(e, owner[kind].data(), k.lm_owner[kind], owner[kind].size(), s);
        e = get(e, freed[kind], k.lm_alive[kind], owner[kind].size(), s);
    }
    const int rc = copy_sync(m, e, "export_graph");
    if (rc != GFPL_OK) return rc;
    for (size_t i = 0; i < nkf; ++i) alive[i] = m->kf_alive[i];
    for (int kind = 0; kind < 2; ++kind) {
        if (!start[kind]) continue;
        // keyframe k's list: the landmarks it owns in ascending id (KM3), a counting sort by owner
        const std::vector<int32_t>& own = owner[kind];
        for (size_t i = 0; i <= nkf; ++i) start[kind][i] = 0;
        for (size_t j = 0; j < own.size(); ++j) {
            freed[kind][j] = !freed[kind][j];
            if (own[j] >= 0 && (size_t)own[j] < nkf) ++start[kind][(size_t)own[j] + 1];
        }
        for (size_t i = 0; i < nkf; ++i) start[kind][i + 1] += start[kind][i];
        std::vector<int32_t> at(start[kind], start[kind] + nkf);
        for (size_t j = 0; j < own.size(); ++j)
            if (own[j] >= 0 && (size_t)own[j] < nkf) idx[kind][at[(size_t)own[j]]++] = (int32_t)j;
    }
    return GFPL_OK;
}

int gfpl_kfmap_debug_ms(gfpl_kfmap* m, float* ms) {
    if (!m || !ms) return GFPL_E_INVALID;
    if (!m->timed) return GFPL_E_STATE;
    GFPL_HIPCHK(hipEventElapsedTime(ms, m->ev0, m->ev1));
    return GFPL_OK;
}

}  // extern "C"
