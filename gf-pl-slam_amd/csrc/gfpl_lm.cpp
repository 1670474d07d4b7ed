// gfpl_lm.cpp — host side of the landmark descriptor store (include/gfpl.h): the
// object that owns the store's device memory and the host mirror of the counts, apply (the planner,
// one upload of the work items and ops, one launch per lane-group bucket that has work, one
// synchronisation), fuse (the same with the planner of gfpl_lm_fuse_plan.cpp), gather and read; and
// the device-id calls (observe_pairs, observe_local, free_ids, gather_ids), whose planner and refusals
// run on the device (k_lm_plan.hip): the argument checks, the call's launches in stream order, one
// copy of the header and one synchronisation.
#include "gfpl_host.hpp"
#include "gfpl_lm_fuse_plan.hpp"
#include "gfpl_lm_plan.hpp"

using namespace gfpl;

struct gfpl_lmstore {
    gfpl_ctx* ctx = nullptr;
    int lm_cap = 0, obs_cap = 0, max_ops = 0;
    char* base = nullptr;          // LmStoreMem, then LmWorkMem
    size_t store_bytes = 0, work_bytes = 0;
    char* stage = nullptr;         // pinned LmWorkMem
    int32_t* d_ids = nullptr;      // gather's id list (grown on demand) and its pinned staging
    int32_t* h_ids = nullptr;
    int ids_cap = 0;
    std::vector<int32_t> counts;   // the mirror every check runs against
    std::vector<int32_t> slot;     // the planner's scratch, all -1 between calls
    LmPlan plan;
    LmFusePlan fuse_plan;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the last apply's or gather's kernels (gfpl_lmstore_debug_ms)
    bool timed = false;
    int min_g = 0;                 // GFPL_LM_MIN_LANES as it stood when the store was created
    bool failed = false;           // a HIP call failed inside apply: counts and rows are no longer known
    // the device-id calls (observe_pairs, observe_local, free_ids, gather_ids)
    char* plan_base = nullptr;     // LmPlanMem, allocated at the first of them
    size_t plan_bytes = 0;
    int32_t* h_hdr = nullptr;      // pinned [LM_HDR]: the header's copy
    bool stale = false;            // the device's count[] has changed since `counts` was last equal to it
};

namespace {

LmStoreDev dev_of(const gfpl_lmstore* st) {
    const LmStoreMem m(st->base, st->lm_cap, st->obs_cap);
    return LmStoreDev{m.rows, m.count, m.med_idx, m.med, st->obs_cap};
}

LmPlanDev plan_of(const gfpl_lmstore* st) {
    const LmPlanMem m(st->plan_base, st->lm_cap, st->max_ops);
    return LmPlanDev{m.hdr, m.pend, m.op0, m.place, m.tile_w, m.tile_o, st->lm_cap, st->max_ops, st->min_g};
}

bool rows_ok(const uint8_t* p) { return p && ((uintptr_t)p & 15) == 0; }

// The mirror follows the device: a device-id call changes count[] without the host seeing it, so the
// host-route calls, whose checks run against the mirror, first bring it up to date (one copy of
// count[lm_cap]; nothing when no device-id call came in between).  DESIGN.md §4i.
int mirror_refresh(gfpl_lmstore* st) {
    if (!st->stale) return GFPL_OK;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(st->ctx)));
    hipStream_t s = stream_of(st->ctx);
    const hipError_t e = hipMemcpyAsync(st->counts.data(), dev_of(st).count, (size_t)st->lm_cap * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e != hipSuccess || es != hipSuccess) {
        (void)hipGetLastError();
        return GFPL_E_HIP;   // still stale: the next call tries again
    }
    st->stale = false;
    return GFPL_OK;
}

// a device-id call's start: the planner's scratch at the first one (pend all zero), the header zeroed,
// the first event
int dev_begin(gfpl_lmstore* st, hipStream_t* s) {
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(st->ctx)));
    *s = stream_of(st->ctx);
    st->timed = false;
    if (!st->plan_base) {
        const size_t bytes = LmPlanMem(nullptr, st->lm_cap, st->max_ops).bytes;
        char* base = nullptr;
        int32_t* h = nullptr;
        if (hipMalloc(&base, bytes) != hipSuccess || hipHostMalloc((void**)&h, LM_HDR * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            if (base) (void)hipFree(base);
            return GFPL_E_NOMEM;
        }
        if (hipMemsetAsync(base, 0, bytes, *s) != hipSuccess || hipStreamSynchronize(*s) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipHostFree(h);
            (void)hipFree(base);
            return GFPL_E_HIP;
        }
        st->plan_base = base;
        st->plan_bytes = bytes;
        st->h_hdr = h;
    }
    hipError_t e = hipMemsetAsync(plan_of(st).hdr, 0, LM_HDR * sizeof(int32_t), *s);
    if (e == hipSuccess) e = hipEventRecord(st->ev0, *s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return GFPL_E_HIP;   // nothing of the call was enqueued
    }
    return GFPL_OK;
}

// a device-id call's end: the second event, the header to the host, the call's one synchronisation.
// Returns the call's code: the device's refusal when there is one, GFPL_E_INVALID before GFPL_E_CAPACITY.
int dev_finish(gfpl_lmstore* st, hipStream_t s, hipError_t e, bool mutates, const char* what) {
    if (e == hipSuccess) e = hipEventRecord(st->ev1, s);
    if (e == hipSuccess) e = hipMemcpyAsync(st->h_hdr, plan_of(st).hdr, LM_HDR * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: lmstore_%s failed: %s\n", what, hipGetErrorString(e != hipSuccess ? e : es));
        (void)hipGetLastError();
        if (mutates) st->failed = true;   // some launches may have run: neither the rows nor the scratch are known
        return GFPL_E_HIP;
    }
    st->timed = true;
    const int err = st->h_hdr[LM_H_ERR];
    if (err & KFMAP_ERR_INVALID) return GFPL_E_INVALID;
    if (err & KFMAP_ERR_CAPACITY) return GFPL_E_CAPACITY;
    if (mutates) st->stale = true;
    return GFPL_OK;
}

}  // namespace

extern "C" {

int gfpl_lmstore_create(gfpl_ctx* c, int lm_cap, int obs_cap, int max_ops, gfpl_lmstore** out) {
    if (!c || !out || lm_cap < 1 || obs_cap < 1 || obs_cap > GFPL_LM_MAX_OBS || max_ops < 1) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(c)));
    gfpl_lmstore* st = new gfpl_lmstore();
    st->ctx = c;
    st->lm_cap = lm_cap;
    st->obs_cap = obs_cap;
    st->max_ops = max_ops;
    // GFPL_LM_MIN_LANES: every landmark through groups of at least so many lanes (tools/bench_lm_store.py
    // creates a store under 64 to measure what the buckets are worth)
    st->min_g = env_int("GFPL_LM_MIN_LANES", 0);
    st->store_bytes = LmStoreMem(nullptr, lm_cap, obs_cap).bytes;
    st->work_bytes = LmWorkMem(nullptr, max_ops).bytes;
    hipStream_t s = stream_of(c);
    bool ok = hipMalloc(&st->base, st->store_bytes + st->work_bytes) == hipSuccess &&
              hipHostMalloc((void**)&st->stage, st->work_bytes, hipHostMallocDefault) == hipSuccess;
    if (ok) {
        // every landmark empty: count 0, med_idx -1, a zeroed median row
        const LmStoreMem m(st->base, lm_cap, obs_cap);
        ok = hipMemsetAsync(m.count, 0, (size_t)lm_cap * sizeof(int32_t), s) == hipSuccess &&
             hipMemsetAsync(m.med_idx, 0xff, (size_t)lm_cap * sizeof(int32_t), s) == hipSuccess &&
             hipMemsetAsync(m.med, 0, (size_t)lm_cap * 32, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipHostFree(st->stage);
            (void)hipFree(st->base);
            delete st;
            return GFPL_E_HIP;
        }
    } else {
        (void)hipGetLastError();
        if (st->base) (void)hipFree(st->base);
        delete st;
        return GFPL_E_NOMEM;
    }
    if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) {
        (void)hipGetLastError();
        if (st->ev0) (void)hipEventDestroy(st->ev0);
        (void)hipHostFree(st->stage);
        (void)hipFree(st->base);
        delete st;
        return GFPL_E_HIP;
    }
    st->counts.assign((size_t)lm_cap, 0);
    st->slot.assign((size_t)lm_cap, -1);
    gfpl_ctx_attach(c);
    *out = st;
    return GFPL_OK;
}

int gfpl_lmstore_destroy(gfpl_lmstore* st) {
    if (!st) return GFPL_E_INVALID;
    (void)hipSetDevice(gfpl_ctx_device(st->ctx));
    (void)hipStreamSynchronize(stream_of(st->ctx));
    if (st->h_ids) (void)hipHostFree(st->h_ids);
    if (st->d_ids) (void)hipFree(st->d_ids);
    if (st->h_hdr) (void)hipHostFree(st->h_hdr);
    if (st->plan_base) (void)hipFree(st->plan_base);
    (void)hipEventDestroy(st->ev0);
    (void)hipEventDestroy(st->ev1);
    (void)hipHostFree(st->stage);
    (void)hipFree(st->base);
    gfpl_ctx_detach(st->ctx);
    delete st;
    return GFPL_OK;
}

int64_t gfpl_lmstore_bytes(const gfpl_lmstore* st) {
    return st ? (int64_t)(st->store_bytes + st->work_bytes + st->plan_bytes + (size_t)st->ids_cap * sizeof(int32_t)) : 0;
}

int gfpl_lmstore_apply(gfpl_lmstore* st, const gfpl_lm_op* ops, int n, const uint8_t* const* srcs,
                       const int32_t* src_rows, int n_srcs) {
    if (!st || n < 0 || (n > 0 && !ops) || n_srcs < 0 || (n_srcs > 0 && (!srcs || !src_rows))) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    if (n > st->max_ops) return GFPL_E_CAPACITY;
    if (n == 0) return GFPL_OK;
    if (const int rm = mirror_refresh(st)) return rm;
    const int rc = lm_plan(ops, n, st->counts.data(), st->lm_cap, st->obs_cap, src_rows, n_srcs, st->min_g, &st->plan,
                           st->slot.data());
    if (rc != GFPL_OK) return rc;
    const LmPlan& pl = st->plan;
    const LmWorkMem hm(st->stage, st->max_ops);
    bool aligned = true;
    for (int k = 0; k < n && aligned; ++k) {
        const gfpl_lm_op& op = ops[pl.order[(size_t)k]];
        LmOpDev& o = hm.ops[k];
        o.row = nullptr;
        o.kind = op.kind;
        o.pos = op.arg;
        if (op.kind == GFPL_LM_ADD) {
            const uint8_t* p = srcs[op.src];
            aligned = p && ((uintptr_t)p & 15) == 0;
            if (aligned) o.row = p + 32 * (size_t)op.arg;
        }
    }
    if (!aligned) {
        for (const LmWork& w : pl.work) st->counts[(size_t)w.lm] = w.count0;   // refused: the mirror as it was
        return GFPL_E_INVALID;
    }
    const int n_work = (int)pl.work.size();
    std::memcpy(hm.work, pl.work.data(), (size_t)n_work * sizeof(LmWork));

    if (hipSetDevice(gfpl_ctx_device(st->ctx)) != hipSuccess) {
        for (const LmWork& w : pl.work) st->counts[(size_t)w.lm] = w.count0;   // nothing was enqueued
        return GFPL_E_HIP;
    }
    hipStream_t s = stream_of(st->ctx);
    const LmWorkMem dm(st->base + st->store_bytes, st->max_ops);
    const LmStoreDev sd = dev_of(st);
    hipError_t e = hipMemcpyAsync(dm.work, hm.work, (size_t)n_work * sizeof(LmWork), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dm.ops, hm.ops, (size_t)n * sizeof(LmOpDev), hipMemcpyHostToDevice, s);
    st->timed = false;
    if (e == hipSuccess) e = hipEventRecord(st->ev0, s);
    for (int b = 0; b < LM_BUCKETS && e == hipSuccess; ++b)
        e = launch_lm_apply(sd, dm.work, dm.ops, pl.bucket_start[b], pl.bucket_start[b + 1] - pl.bucket_start[b], b, s);
    if (e == hipSuccess) e = hipEventRecord(st->ev1, s);
    const hipError_t es = hipStreamSynchronize(s);   // also on an error path: the staging is still in use
    st->timed = e == hipSuccess && es == hipSuccess;
    if (e != hipSuccess || es != hipSuccess) {
        // some of the launches may have run: neither the mirror's counts nor the ones before the call
        // describe the device any more, so the store refuses further use
        std::fprintf(stderr, "gfpl: lmstore_apply failed: %s\n", hipGetErrorString(e != hipSuccess ? e : es));
        st->failed = true;
        return GFPL_E_HIP;
    }
    return GFPL_OK;
}

int gfpl_lmstore_fuse(gfpl_lmstore* st, const gfpl_lm_op* ops, int n, const uint8_t* const* srcs,
                      const int32_t* src_rows, int n_srcs) {
    if (!st || n < 0 || (n > 0 && !ops) || n_srcs < 0 || (n_srcs > 0 && (!srcs || !src_rows))) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    if (n == 0) return GFPL_OK;
    if (const int rm = mirror_refresh(st)) return rm;
    int64_t n_rows = 0;
    LmFusePlan& pl = st->fuse_plan;
    const int rc = lm_fuse_plan(ops, n, st->counts.data(), st->lm_cap, st->obs_cap, src_rows, n_srcs, st->min_g, &n_rows,
                                &pl, st->slot.data());
    if (rc != GFPL_OK) return rc;
    auto refuse = [&](int code) {
        for (const LmFuseTouch& u : pl.touch) st->counts[(size_t)u.lm] = u.count0;   // the mirror as it was
        return code;
    };
    if (n_rows > st->max_ops) return refuse(GFPL_E_CAPACITY);
    // every gained row as an ADD from its origin: a source row, or a row of the store below its
    // landmark's count before the call, which no work item of this call writes
    const LmStoreDev sd = dev_of(st);
    const LmWorkMem hm(st->stage, st->max_ops);
    const int n_work = (int)pl.work.size();
    for (int w = 0; w < n_work; ++w) {
        const LmFuseTouch& u = pl.touch[(size_t)pl.work_touch[(size_t)w]];
        LmOpDev* o = hm.ops + pl.work[(size_t)w].op0;
        if (u.freed) {
            *o = LmOpDev{nullptr, GFPL_LM_FREE, 0};
            continue;
        }
        for (const LmOrigin& g : u.gained) {
            const uint8_t* p;
            if (g.src >= 0) {
                p = srcs[g.src];
                if (!p || ((uintptr_t)p & 15) != 0) return refuse(GFPL_E_INVALID);
                p += 32 * (size_t)g.row;
            } else {
                p = sd.rows + ((size_t)(-1 - g.src) * st->obs_cap + (size_t)g.row) * 32;
            }
            *o++ = LmOpDev{p, GFPL_LM_ADD, 0};
        }
    }
    std::memcpy(hm.work, pl.work.data(), (size_t)n_work * sizeof(LmWork));

    if (hipSetDevice(gfpl_ctx_device(st->ctx)) != hipSuccess) return refuse(GFPL_E_HIP);   // nothing was enqueued
    hipStream_t s = stream_of(st->ctx);
    const LmWorkMem dm(st->base + st->store_bytes, st->max_ops);
    hipError_t e = hipMemcpyAsync(dm.work, hm.work, (size_t)n_work * sizeof(LmWork), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(dm.ops, hm.ops, (size_t)pl.n_dev_ops * sizeof(LmOpDev), hipMemcpyHostToDevice, s);
    st->timed = false;
    if (e == hipSuccess) e = hipEventRecord(st->ev0, s);
    for (int b = 0; b < LM_BUCKETS && e == hipSuccess; ++b)
        e = launch_lm_apply(sd, dm.work, dm.ops, pl.bucket_start[b], pl.bucket_start[b + 1] - pl.bucket_start[b], b, s);
    if (e == hipSuccess) e = hipEventRecord(st->ev1, s);
    const hipError_t es = hipStreamSynchronize(s);   // also on an error path: the staging is still in use
    st->timed = e == hipSuccess && es == hipSuccess;
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: lmstore_fuse failed: %s\n", hipGetErrorString(e != hipSuccess ? e : es));
        st->failed = true;   // as in apply: neither the mirror nor the counts before the call describe the device
        return GFPL_E_HIP;
    }
    return GFPL_OK;
}

int gfpl_lmstore_gather(gfpl_lmstore* st, const int32_t* lm_ids, int n, uint8_t* desc_out, int32_t* med_idx_out) {
    if (!st || n < 0 || (n > 0 && (!lm_ids || !desc_out))) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    if (n == 0) return GFPL_OK;
    if ((uintptr_t)desc_out & 15) return GFPL_E_INVALID;
    if (const int rm = mirror_refresh(st)) return rm;
    for (int i = 0; i < n; ++i)
        if (lm_ids[i] < 0 || lm_ids[i] >= st->lm_cap || st->counts[(size_t)lm_ids[i]] == 0) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(st->ctx)));
    hipStream_t s = stream_of(st->ctx);
    if (n > st->ids_cap) {
        if (st->h_ids) (void)hipHostFree(st->h_ids);
        if (st->d_ids) (void)hipFree(st->d_ids);
        st->h_ids = nullptr;
        st->d_ids = nullptr;
        st->ids_cap = 0;
        const bool ok = hipMalloc(&st->d_ids, (size_t)n * sizeof(int32_t)) == hipSuccess &&
                        hipHostMalloc((void**)&st->h_ids, (size_t)n * sizeof(int32_t), hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (st->d_ids) (void)hipFree(st->d_ids);
            st->d_ids = nullptr;
            return GFPL_E_NOMEM;
        }
        st->ids_cap = n;
    }
    std::memcpy(st->h_ids, lm_ids, (size_t)n * sizeof(int32_t));
    hipError_t e = hipMemcpyAsync(st->d_ids, st->h_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s);
    st->timed = false;
    if (e == hipSuccess) e = hipEventRecord(st->ev0, s);
    if (e == hipSuccess) e = launch_lm_gather(dev_of(st), st->d_ids, n, desc_out, med_idx_out, s);
    if (e == hipSuccess) e = hipEventRecord(st->ev1, s);
    const hipError_t es = hipStreamSynchronize(s);
    st->timed = e == hipSuccess && es == hipSuccess;
    if (e != hipSuccess || es != hipSuccess) {
        std::fprintf(stderr, "gfpl: lmstore_gather failed: %s\n", hipGetErrorString(e != hipSuccess ? e : es));
        return GFPL_E_HIP;
    }
    return GFPL_OK;
}

int gfpl_lmstore_observe_pairs(gfpl_lmstore* st, const uint8_t* desc0, int n0, const uint8_t* desc1, int n1, const int32_t* pairs,
                               const int32_t* lm_out, int n, int first_new) {
    if (!st || n < 0 || n0 < 0 || n1 < 0 || (n > 0 && (!desc0 || !desc1 || !pairs || !lm_out))) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    if (first_new < 0 || first_new > st->lm_cap) return GFPL_E_INVALID;
    if (n == 0) return GFPL_OK;
    if (!rows_ok(desc0) || !rows_ok(desc1)) return GFPL_E_INVALID;
    if (n > st->max_ops) return GFPL_E_CAPACITY;
    hipStream_t s;
    if (const int rc = dev_begin(st, &s)) return rc;
    const LmWorkMem dm(st->base + st->store_bytes, st->max_ops);
    const LmObserve a{desc0, desc1, pairs, nullptr, lm_out, n, n0, n1, 0, first_new};
    return dev_finish(st, s, enqueue_lm_observe(dev_of(st), plan_of(st), a, dm.work, dm.ops, s), true, "observe_pairs");
}

int gfpl_lmstore_observe_local(gfpl_lmstore* st, const uint8_t* desc1, int n1, const int32_t* pairs, int n, const int32_t* unm_rows,
                               int n_unm, const int32_t* lm_out) {
    if (!st || n < 0 || n1 < 0 || n_unm < 0 || (n > 0 && (!desc1 || !pairs || !unm_rows || !lm_out))) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    if (n == 0) return GFPL_OK;
    if (!rows_ok(desc1)) return GFPL_E_INVALID;
    if (n > st->max_ops) return GFPL_E_CAPACITY;
    hipStream_t s;
    if (const int rc = dev_begin(st, &s)) return rc;
    const LmWorkMem dm(st->base + st->store_bytes, st->max_ops);
    const LmObserve a{nullptr, desc1, pairs, unm_rows, lm_out, n, 0, n1, n_unm, st->lm_cap};   // no id is a created one
    return dev_finish(st, s, enqueue_lm_observe(dev_of(st), plan_of(st), a, dm.work, dm.ops, s), true, "observe_local");
}

int gfpl_lmstore_free_ids(gfpl_lmstore* st, const int32_t* ids, int n) {
    if (!st || n < 0 || (n > 0 && !ids)) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    if (n == 0) return GFPL_OK;
    hipStream_t s;
    if (const int rc = dev_begin(st, &s)) return rc;
    return dev_finish(st, s, enqueue_lm_free_ids(dev_of(st), plan_of(st), ids, n, s), true, "free_ids");
}

int gfpl_lmstore_gather_ids(gfpl_lmstore* st, const int32_t* ids, int n, uint8_t* desc_out, int32_t* med_idx_out) {
    if (!st || n < 0 || (n > 0 && (!ids || !desc_out))) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    if (n == 0) return GFPL_OK;
    if (!rows_ok(desc_out)) return GFPL_E_INVALID;
    hipStream_t s;
    if (const int rc = dev_begin(st, &s)) return rc;
    return dev_finish(st, s, enqueue_lm_gather_ids(dev_of(st), plan_of(st), ids, n, desc_out, med_idx_out, s), false, "gather_ids");
}

int gfpl_lmstore_counts(gfpl_lmstore* st, int32_t* counts) {
    if (!st || !counts) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    st->stale = true;   // read from the device whatever the mirror holds, and the mirror with it
    if (const int rm = mirror_refresh(st)) return rm;
    std::memcpy(counts, st->counts.data(), (size_t)st->lm_cap * sizeof(int32_t));
    return GFPL_OK;
}

int gfpl_lmstore_read(gfpl_lmstore* st, int lm, int32_t* count, int32_t* med_idx, uint8_t* desc_list, uint8_t* med_desc) {
    if (!st || lm < 0 || lm >= st->lm_cap) return GFPL_E_INVALID;
    if (st->failed) return GFPL_E_STATE;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(st->ctx)));
    hipStream_t s = stream_of(st->ctx);
    const LmStoreDev sd = dev_of(st);
    hipError_t e = hipSuccess;
    if (count) e = hipMemcpyAsync(count, sd.count + lm, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && med_idx) e = hipMemcpyAsync(med_idx, sd.med_idx + lm, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && desc_list)
        e = hipMemcpyAsync(desc_list, sd.rows + (size_t)lm * st->obs_cap * 32, (size_t)st->obs_cap * 32,
                           hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && med_desc) e = hipMemcpyAsync(med_desc, sd.med + (size_t)lm * 32, 32, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e != hipSuccess || es != hipSuccess) return GFPL_E_HIP;
    return GFPL_OK;
}

int gfpl_lmstore_debug_ms(gfpl_lmstore* st, float* ms) {
    if (!st || !ms) return GFPL_E_INVALID;
    if (!st->timed) return GFPL_E_STATE;
    GFPL_HIPCHK(hipEventElapsedTime(ms, st->ev0, st->ev1));
    return GFPL_OK;
}

}  // extern "C"
