// gfpl_mapgeo.cpp — host side of the map's geometry half (include/gfpl.h): the object
// that owns the one device allocation (MapGeoMem) and a host note of which keyframes have a pose, and
// per call: the argument checks, the call's launches in stream order, one copy of the header and one
// synchronisation.  gfpl_mapgeo_assemble reads a gfpl_kfmap's device arrays (kfmap_device) and
// gfpl_mapgeo_lba hands the assembled problem to a gfpl_lba through lba_stage_device / lba_enqueue
// (gfpl_host.hpp), so the index lists never visit the host.
#include <algorithm>

#include "gfpl_host.hpp"

using namespace gfpl;

struct gfpl_mapgeo {
    gfpl_ctx* ctx = nullptr;
    gfpl_kfmap_caps caps{};
    char* base = nullptr;
    size_t bytes = 0;
    int32_t* h_hdr = nullptr;            // pinned [MAPGEO_HDR]: the header's copy
    double* h_kf = nullptr;              // pinned [22]: staging of set_keyframe
    std::vector<uint8_t> kf_set;         // set_keyframe has stored a pose
    gfpl_lba_counts last{};              // the last assembly's counts
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool failed = false;
};

namespace {

bool caps_ok(const gfpl_kfmap_caps* c) { return gfpl_kfmap_bytes(c) >= 0; }

MapGeoMem mem_of(char* base, const gfpl_kfmap_caps& c) {
    return MapGeoMem(base, c.kf_cap, c.pt_rows, c.ls_rows, c.pt_lm_cap, c.ls_lm_cap, c.obs_cap);
}

MapGeoCore core_of(const gfpl_mapgeo* g) {
    const MapGeoMem k = mem_of(g->base, g->caps);
    return MapGeoCore{k.hdr, k.T_kf, k.x_kf, k.pend, k.pair_n0, k.kf_cap, k.obs_cap};
}

MapGeoLm lm_of(const gfpl_mapgeo* g, int kind) {
    const MapGeoMem k = mem_of(g->base, g->caps);
    return MapGeoLm{k.lm3d[kind], k.obs[kind], k.sigma[kind], k.nobs[kind], MAPGEO_LM_W[kind], MAPGEO_OBS_W[kind], k.lm_cap[kind]};
}

MapGeoAsm asm_of(const gfpl_mapgeo* g, const KfMapDevice& d, int which) {
    const MapGeoMem k = mem_of(g->base, g->caps);
    MapGeoAsm a;
    a.which = which;
    a.n_kf = d.core.n_kf;
    a.kf_alive = d.core.kf_alive;
    a.kf_local = d.core.kf_local;
    a.kf_slot = k.kf_slot; a.kf_mark = k.kf_mark; a.kf_list = k.kf_list; a.fix_list = k.fix_list;
    a.a_x_kf = k.a_x_kf; a.a_T_kf = k.a_T_kf; a.a_T_fix = k.a_T_fix;
    for (int kind = 0; kind < 2; ++kind) {
        a.next[kind] = d.lm[kind].next;
        a.lm_alive[kind] = d.lm[kind].alive;
        a.lm_local[kind] = d.lm[kind].local;
        a.k_nobs[kind] = d.lm[kind].nobs;
        a.k_obs[kind] = d.lm[kind].obs;
        a.lm_cnt[kind] = k.lm_cnt[kind]; a.tile_lm[kind] = k.tile_lm[kind]; a.tile_obs[kind] = k.tile_obs[kind];
        a.lm_list[kind] = k.lm_list[kind]; a.lm_off[kind] = k.lm_off[kind];
        a.a_lm3d[kind] = k.a_lm3d[kind]; a.a_obs[kind] = k.a_obs[kind]; a.a_sigma[kind] = k.a_sigma[kind];
        a.a_obs_lm[kind] = k.a_obs_lm[kind]; a.a_obs_kf[kind] = k.a_obs_kf[kind];
    }
    return a;
}

bool same_caps(const gfpl_kfmap_caps& a, const gfpl_kfmap_caps& b) {
    return a.kf_cap == b.kf_cap && a.pt_rows == b.pt_rows && a.ls_rows == b.ls_rows && a.pt_lm_cap == b.pt_lm_cap &&
           a.ls_lm_cap == b.ls_lm_cap && a.obs_cap == b.obs_cap;
}

bool doubles_ok(const double* p) { return p && (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// a call's start: the device, the header zeroed, the first event
hipError_t begin(gfpl_mapgeo* g, hipStream_t* s) {
    *s = stream_of(g->ctx);
    g->timed = false;
    hipError_t e = hipSetDevice(gfpl_ctx_device(g->ctx));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(core_of(g).hdr, 0, MAPGEO_HDR * sizeof(int32_t), *s);
    if (e == hipSuccess) e = hipEventRecord(g->ev0, *s);
    return e;
}

// a call's end: the second event, the header to the host, the call's synchronisation.  Returns the
// call's code: the device's refusal when there is one.
int finish(gfpl_mapgeo* g, hipStream_t s, hipError_t e, const char* what) {
    if (e == hipSuccess) e = hipEventRecord(g->ev1, s);
    if (e == hipSuccess) e = hipMemcpyAsync(g->h_hdr, core_of(g).hdr, MAPGEO_HDR * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: mapgeo_%s failed: %s\n", what, hipGetErrorString(e != hipSuccess ? e : es));
        (void)hipGetLastError();
        g->failed = true;   // some launches may have run: the state is not known any more
        return GFPL_E_HIP;
    }
    g->timed = true;
    const int err = g->h_hdr[MAPGEO_H_ERR];
    if (err & KFMAP_ERR_INVALID) return GFPL_E_INVALID;
    if (err & KFMAP_ERR_CAPACITY) return GFPL_E_CAPACITY;
    return GFPL_OK;
}

#define MAPGEO_ENTER(g)                       \
    do {                                      \
        if (!(g)) return GFPL_E_INVALID;      \
        if ((g)->failed) return GFPL_E_STATE; \
    } while (0)

// synchronous copies of the read / patch calls
int copy_sync(gfpl_mapgeo* g, hipError_t e, const char* what) {
    const hipError_t es = hipStreamSynchronize(stream_of(g->ctx));
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: mapgeo_%s failed: %s\n", what, hipGetErrorString(e != hipSuccess ? e : es));
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

bool kf_in(const gfpl_mapgeo* g, int kf) { return kf >= 0 && kf < g->caps.kf_cap; }

// the assembly of `which`: the checks, the launches, the counts in the call's one synchronisation
int assemble_run(gfpl_mapgeo* g, const gfpl_kfmap* kfmap, int which, gfpl_lba_counts* n, MapGeoAsm* a) {
    if (!kfmap || (which != GFPL_KFMAP_LOCAL && which != GFPL_KFMAP_ALIVE)) return GFPL_E_INVALID;
    const KfMapDevice d = kfmap_device(kfmap);
    if (d.failed) return GFPL_E_STATE;
    if (d.ctx != g->ctx || !same_caps(d.caps, g->caps)) return GFPL_E_INVALID;
    *a = asm_of(g, d, which);
    hipStream_t s;
    hipError_t e = begin(g, &s);
    if (e == hipSuccess) e = enqueue_mapgeo_assemble(core_of(g), lm_of(g, 0), lm_of(g, 1), *a, s);
    const int rc = finish(g, s, e, "assemble");
    if (rc == GFPL_E_HIP) return rc;
    const int32_t* h = g->h_hdr;
    *n = gfpl_lba_counts{h[MAPGEO_H_NKF], h[MAPGEO_H_NFIX], h[MAPGEO_H_NPT], h[MAPGEO_H_NLS], h[MAPGEO_H_NPTOBS], h[MAPGEO_H_NLSOBS]};
    g->last = *n;
    return rc;
}

void fill_problem(const gfpl_mapgeo* g, const gfpl_lba_counts& n, gfpl_lba_problem* p) {
    const MapGeoMem k = mem_of(g->base, g->caps);
    std::memset(p, 0, sizeof *p);
    p->n = n;
    p->x_kf = k.a_x_kf; p->T_kf = k.a_T_kf; p->T_fix = k.a_T_fix; p->x_out = k.a_x_out;
    p->pt = k.a_lm3d[0]; p->pt_obs = k.a_obs[0]; p->pt_sigma = k.a_sigma[0];
    p->ls = k.a_lm3d[1]; p->ls_obs = k.a_obs[1]; p->ls_sigma = k.a_sigma[1];
}

}  // namespace

extern "C" {

int64_t gfpl_mapgeo_bytes(const gfpl_kfmap_caps* caps) {
    if (!caps_ok(caps)) return -1;
    return (int64_t)mem_of(nullptr, *caps).bytes;
}

int gfpl_mapgeo_create(gfpl_ctx* c, const gfpl_kfmap_caps* caps, gfpl_mapgeo** out) {
    if (!c || !out || !caps_ok(caps)) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(c)));
    gfpl_mapgeo* g = new gfpl_mapgeo();
    g->ctx = c;
    g->caps = *caps;
    g->bytes = mem_of(nullptr, *caps).bytes;
    hipStream_t s = stream_of(c);
    auto drop = [&](int code) {
        (void)hipGetLastError();
        if (g->ev0) (void)hipEventDestroy(g->ev0);
        if (g->ev1) (void)hipEventDestroy(g->ev1);
        if (g->h_hdr) (void)hipHostFree(g->h_hdr);
        if (g->h_kf) (void)hipHostFree(g->h_kf);
        if (g->base) (void)hipFree(g->base);
        delete g;
        return code;
    };
    if (hipMalloc(&g->base, g->bytes) != hipSuccess ||
        hipHostMalloc((void**)&g->h_hdr, MAPGEO_HDR * sizeof(int32_t), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&g->h_kf, 22 * sizeof(double), hipHostMallocDefault) != hipSuccess)
        return drop(GFPL_E_NOMEM);
    // every byte a kernel may read: all zero
    bool ok = hipMemsetAsync(g->base, 0, g->bytes, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    ok = ok && hipEventCreate(&g->ev0) == hipSuccess && hipEventCreate(&g->ev1) == hipSuccess;
    if (!ok) return drop(GFPL_E_HIP);
    g->kf_set.assign((size_t)caps->kf_cap, 0);
    gfpl_ctx_attach(c);
    *out = g;
    return GFPL_OK;
}

int gfpl_mapgeo_destroy(gfpl_mapgeo* g) {
    if (!g) return GFPL_E_INVALID;
    (void)hipSetDevice(gfpl_ctx_device(g->ctx));
    (void)hipStreamSynchronize(stream_of(g->ctx));
    (void)hipEventDestroy(g->ev0);
    (void)hipEventDestroy(g->ev1);
    (void)hipHostFree(g->h_hdr);
    (void)hipHostFree(g->h_kf);
    (void)hipFree(g->base);
    gfpl_ctx_detach(g->ctx);
    delete g;
    return GFPL_OK;
}

int gfpl_mapgeo_set_keyframe(gfpl_mapgeo* g, int kf, const double* T_kf_w, const double* x_kf_w) {
    MAPGEO_ENTER(g);
    if (!T_kf_w || !x_kf_w || !kf_in(g, kf)) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(g->ctx)));
    hipStream_t s = stream_of(g->ctx);
    const MapGeoCore c = core_of(g);
    std::memcpy(g->h_kf, T_kf_w, 16 * sizeof(double));
    std::memcpy(g->h_kf + 16, x_kf_w, 6 * sizeof(double));
    hipError_t e = put_dev(hipSuccess, c.T_kf + (size_t)kf * 16, (const double*)g->h_kf, 16, s);
    e = put_dev(e, c.x_kf + (size_t)kf * 6, (const double*)g->h_kf + 16, 6, s);
    const int rc = copy_sync(g, e, "set_keyframe");
    if (rc != GFPL_OK) {
        g->failed = true;   // one of the two may have been written
        return rc;
    }
    g->kf_set[(size_t)kf] = 1;
    return GFPL_OK;
}

int gfpl_mapgeo_read_keyframe(gfpl_mapgeo* g, int kf, double* T_kf_w, double* x_kf_w) {
    MAPGEO_ENTER(g);
    if (!kf_in(g, kf)) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(g->ctx)));
    hipStream_t s = stream_of(g->ctx);
    const MapGeoCore c = core_of(g);
    hipError_t e = get(hipSuccess, T_kf_w, (const double*)c.T_kf + (size_t)kf * 16, 16, s);
    e = get(e, x_kf_w, (const double*)c.x_kf + (size_t)kf * 6, 6, s);
    return copy_sync(g, e, "read_keyframe");
}

int gfpl_mapgeo_arrays(gfpl_mapgeo* g, double** T_kf, double** x_kf, double** point3D, double** line3D) {
    MAPGEO_ENTER(g);
    const MapGeoMem k = mem_of(g->base, g->caps);
    if (T_kf) *T_kf = k.T_kf;
    if (x_kf) *x_kf = k.x_kf;
    if (point3D) *point3D = k.lm3d[0];
    if (line3D) *line3D = k.lm3d[1];
    return GFPL_OK;
}

int gfpl_mapgeo_observe_pairs(gfpl_mapgeo* g, int kind, int kf0, int kf1, const gfpl_kf_view* v0, const gfpl_kf_view* v1,
                              const int32_t* pairs, const int32_t* lm_out, int n, int first_new) {
    MAPGEO_ENTER(g);
    if (!v0 || !v1 || kind < 0 || kind > 1 || n < 0 || (n > 0 && (!pairs || !lm_out))) return GFPL_E_INVALID;
    if (!kf_in(g, kf0) || !kf_in(g, kf1) || kf0 == kf1 || !g->kf_set[(size_t)kf0]) return GFPL_E_INVALID;
    const MapGeoLm L = lm_of(g, kind);
    if (first_new < 0 || first_new > L.cap) return GFPL_E_INVALID;
    const int n0 = kind ? v0->n_ls : v0->n_pt, n1 = kind ? v1->n_ls : v1->n_pt;
    if (n0 < 0 || n1 < 0 || n > std::min(n0, n1) || n > (kind ? g->caps.ls_rows : g->caps.pt_rows)) return GFPL_E_INVALID;
    MapGeoObserve a{kf0, n, 0, first_new, n0, n1, pairs, nullptr, lm_out, kind ? v0->sP : v0->P, kind ? v0->eP : nullptr,
                    kind ? v0->le : v0->pl, kind ? v1->le : v1->pl};
    if (n > 0 && (!doubles_ok(a.P0) || (kind && !doubles_ok(a.Q0)) || !doubles_ok(a.o0) || !doubles_ok(a.o1))) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(g, &s);
    if (e == hipSuccess) e = enqueue_mapgeo_observe(core_of(g), L, a, s);
    return finish(g, s, e, "observe_pairs");
}

int gfpl_mapgeo_observe_local(gfpl_mapgeo* g, int kind, int kf1, const gfpl_kf_view* v1, const int32_t* pairs, int n,
                              const int32_t* unm_rows, int n_unm, const int32_t* lm_out) {
    MAPGEO_ENTER(g);
    if (!v1 || kind < 0 || kind > 1 || n < 0 || n_unm < 0 || (n > 0 && (!pairs || !lm_out || !unm_rows))) return GFPL_E_INVALID;
    if (!kf_in(g, kf1)) return GFPL_E_INVALID;
    const int n1 = kind ? v1->n_ls : v1->n_pt;
    if (n1 < 0 || n_unm > n1 || n > n_unm || n > (kind ? g->caps.ls_rows : g->caps.pt_rows)) return GFPL_E_INVALID;
    MapGeoObserve a{-1, n, n_unm, 0, 0, n1, pairs, unm_rows, lm_out, nullptr, nullptr, nullptr, kind ? v1->le : v1->pl};
    if (n > 0 && !doubles_ok(a.o1)) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(g, &s);
    if (e == hipSuccess) e = enqueue_mapgeo_observe(core_of(g), lm_of(g, kind), a, s);
    return finish(g, s, e, "observe_local");
}

int gfpl_mapgeo_free(gfpl_mapgeo* g, int kind, const int32_t* ids, int n) {
    MAPGEO_ENTER(g);
    if (kind < 0 || kind > 1 || n < 0 || (n > 0 && !ids)) return GFPL_E_INVALID;
    const MapGeoLm L = lm_of(g, kind);
    if (n > L.cap) return GFPL_E_INVALID;
    hipStream_t s;
    hipError_t e = begin(g, &s);
    if (e == hipSuccess) e = enqueue_mapgeo_free(core_of(g), L, ids, n, s);
    return finish(g, s, e, "free");
}

int gfpl_mapgeo_read_landmarks(gfpl_mapgeo* g, int kind, int id0, int n, double* lm3d, int32_t* n_obs, double* obs, double* sigma) {
    MAPGEO_ENTER(g);
    if (kind < 0 || kind > 1 || id0 < 0 || n < 0) return GFPL_E_INVALID;
    const MapGeoLm L = lm_of(g, kind);
    if (n > L.cap - id0) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(g->ctx)));
    hipStream_t s = stream_of(g->ctx);
    const size_t oc = (size_t)g->caps.obs_cap;
    hipError_t e = get(hipSuccess, lm3d, (const double*)L.lm3d + (size_t)id0 * L.lw, (size_t)n * L.lw, s);
    e = get(e, n_obs, (const int32_t*)L.nobs + id0, (size_t)n, s);
    e = get(e, obs, (const double*)L.obs + (size_t)id0 * oc * L.ow, (size_t)n * oc * L.ow, s);
    e = get(e, sigma, (const double*)L.sigma + (size_t)id0 * oc, (size_t)n * oc, s);
    return copy_sync(g, e, "read_landmarks");
}

int gfpl_mapgeo_write_landmarks(gfpl_mapgeo* g, int kind, int id0, int n, const double* lm3d, const int32_t* n_obs,
                                const double* obs, const double* sigma) {
    MAPGEO_ENTER(g);
    if (kind < 0 || kind > 1 || id0 < 0 || n < 0) return GFPL_E_INVALID;
    const MapGeoLm L = lm_of(g, kind);
    if (n > L.cap - id0) return GFPL_E_INVALID;
    if (n == 0) return GFPL_OK;
    if (!lm3d || !n_obs || !obs || !sigma) return GFPL_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (n_obs[i] < 0 || n_obs[i] > g->caps.obs_cap) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(g->ctx)));
    hipStream_t s = stream_of(g->ctx);
    const size_t oc = (size_t)g->caps.obs_cap;
    hipError_t e = put_dev(hipSuccess, L.lm3d + (size_t)id0 * L.lw, lm3d, (size_t)n * L.lw, s);
    e = put_dev(e, L.nobs + id0, n_obs, (size_t)n, s);
    e = put_dev(e, L.obs + (size_t)id0 * oc * L.ow, obs, (size_t)n * oc * L.ow, s);
    e = put_dev(e, L.sigma + (size_t)id0 * oc, sigma, (size_t)n * oc, s);
    const int rc = copy_sync(g, e, "write_landmarks");
    if (rc != GFPL_OK) g->failed = true;   // some of the arrays may have been written
    return rc;
}

int gfpl_mapgeo_assemble(gfpl_mapgeo* g, const gfpl_kfmap* kfmap, int which, gfpl_lba_problem* problem,
                         const gfpl_mapgeo_lists* lists) {
    MAPGEO_ENTER(g);
    if (!problem) return GFPL_E_INVALID;
    if (lists && (lists->cap_pt_obs < 0 || lists->cap_ls_obs < 0 || !lists->pt_obs_lm || !lists->pt_obs_kf || !lists->ls_obs_lm ||
                  !lists->ls_obs_kf))
        return GFPL_E_INVALID;
    gfpl_lba_counts n{};
    MapGeoAsm a;
    const int rc = assemble_run(g, kfmap, which, &n, &a);
    if (rc != GFPL_OK) return rc;
    fill_problem(g, n, problem);
    if (!lists) return GFPL_OK;
    if (n.n_pt_obs > lists->cap_pt_obs || n.n_ls_obs > lists->cap_ls_obs) return GFPL_E_CAPACITY;
    hipStream_t s = stream_of(g->ctx);
    hipError_t e = get(hipSuccess, lists->pt_obs_lm, (const int32_t*)a.a_obs_lm[0], (size_t)n.n_pt_obs, s);
    e = get(e, lists->pt_obs_kf, (const int32_t*)a.a_obs_kf[0], (size_t)n.n_pt_obs, s);
    e = get(e, lists->ls_obs_lm, (const int32_t*)a.a_obs_lm[1], (size_t)n.n_ls_obs, s);
    e = get(e, lists->ls_obs_kf, (const int32_t*)a.a_obs_kf[1], (size_t)n.n_ls_obs, s);
    const int rcc = copy_sync(g, e, "assemble");
    if (rcc != GFPL_OK) return rcc;
    problem->pt_obs_lm = lists->pt_obs_lm; problem->pt_obs_kf = lists->pt_obs_kf;
    problem->ls_obs_lm = lists->ls_obs_lm; problem->ls_obs_kf = lists->ls_obs_kf;
    return GFPL_OK;
}

int gfpl_mapgeo_assembled_ids(gfpl_mapgeo* g, const int32_t** kf_list, const int32_t** fix_list, const int32_t** pt_list,
                              const int32_t** ls_list) {
    MAPGEO_ENTER(g);
    const MapGeoMem k = mem_of(g->base, g->caps);
    if (kf_list) *kf_list = k.kf_list;
    if (fix_list) *fix_list = k.fix_list;
    if (pt_list) *pt_list = k.lm_list[0];
    if (ls_list) *ls_list = k.lm_list[1];
    return GFPL_OK;
}

int gfpl_mapgeo_read_assembled(gfpl_mapgeo* g, const gfpl_lba_problem* host, int32_t* kf_list, int32_t* fix_list, int32_t* pt_list,
                               int32_t* ls_list) {
    MAPGEO_ENTER(g);
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(g->ctx)));
    hipStream_t s = stream_of(g->ctx);
    const MapGeoMem k = mem_of(g->base, g->caps);
    const gfpl_lba_counts& n = g->last;
    hipError_t e = get(hipSuccess, kf_list, (const int32_t*)k.kf_list, (size_t)n.n_kf, s);
    e = get(e, fix_list, (const int32_t*)k.fix_list, (size_t)n.n_fix, s);
    e = get(e, pt_list, (const int32_t*)k.lm_list[0], (size_t)n.n_pt, s);
    e = get(e, ls_list, (const int32_t*)k.lm_list[1], (size_t)n.n_ls, s);
    if (host) {
        e = get(e, const_cast<double*>(host->x_kf), (const double*)k.a_x_kf, (size_t)n.n_kf * 6, s);
        e = get(e, host->T_kf, (const double*)k.a_T_kf, (size_t)n.n_kf * 16, s);
        e = get(e, const_cast<double*>(host->T_fix), (const double*)k.a_T_fix, (size_t)n.n_fix * 16, s);
        e = get(e, host->pt, (const double*)k.a_lm3d[0], (size_t)n.n_pt * 3, s);
        e = get(e, host->ls, (const double*)k.a_lm3d[1], (size_t)n.n_ls * 6, s);
        e = get(e, const_cast<double*>(host->pt_obs), (const double*)k.a_obs[0], (size_t)n.n_pt_obs * 2, s);
        e = get(e, const_cast<double*>(host->pt_sigma), (const double*)k.a_sigma[0], (size_t)n.n_pt_obs, s);
        e = get(e, const_cast<double*>(host->ls_obs), (const double*)k.a_obs[1], (size_t)n.n_ls_obs * 3, s);
        e = get(e, const_cast<double*>(host->ls_sigma), (const double*)k.a_sigma[1], (size_t)n.n_ls_obs, s);
    }
    return copy_sync(g, e, "read_assembled");
}

int gfpl_mapgeo_lba(gfpl_mapgeo* g, const gfpl_kfmap* kfmap, gfpl_lba* lba, const gfpl_lba_params* prm, gfpl_lba_result* result,
                    gfpl_lba_counts* counts) {
    MAPGEO_ENTER(g);
    if (!kfmap || !lba || !prm || !result) return GFPL_E_INVALID;
    if (!(prm->lambda_k != 0.0) || lba_ctx(lba) != g->ctx) return GFPL_E_INVALID;
    if (!gfpl_ctx_camera(g->ctx)) return GFPL_E_STATE;
    std::memset(result, 0, sizeof *result);
    gfpl_lba_counts n{};
    MapGeoAsm a;
    int rc = assemble_run(g, kfmap, GFPL_KFMAP_LOCAL, &n, &a);
    if (counts && rc != GFPL_E_HIP && rc != GFPL_E_STATE) *counts = n;
    if (rc != GFPL_OK) return rc;
    if (n.n_pt_obs + n.n_ls_obs == 0) return GFPL_OK;   // :1212
    if (n.n_kf < 1) return GFPL_E_INVALID;              // MG6
    if (n.n_kf > GFPL_LBA_MAX_KFS) return GFPL_E_CAPACITY;
    gfpl_lba_problem p;
    fill_problem(g, n, &p);
    LbaProb q;
    rc = lba_stage_device(lba, p, &q);
    if (rc != GFPL_OK) return rc;
    hipStream_t s = stream_of(g->ctx);
    hipError_t e = enqueue_mapgeo_lba_index(a, n, const_cast<int32_t*>(q.lm_start), const_cast<int32_t*>(q.obs_lm),
                                            const_cast<int32_t*>(q.obs_kf), s);
    if (e == hipSuccess) e = lba_enqueue(lba, 1, n.n_kf, prm, result, s);
    if (e == hipSuccess) e = enqueue_mapgeo_write_back(core_of(g), lm_of(g, 0), lm_of(g, 1), a, n, s);
    const int rcs = copy_sync(g, e, "lba");
    if (rcs != GFPL_OK) g->failed = true;   // the write-back may have run in part
    return rcs;
}

int gfpl_mapgeo_debug_ms(gfpl_mapgeo* g, float* ms) {
    if (!g || !ms) return GFPL_E_INVALID;
    if (!g->timed) return GFPL_E_STATE;
    GFPL_HIPCHK(hipEventElapsedTime(ms, g->ev0, g->ev1));
    return GFPL_OK;
}

}  // extern "C"
