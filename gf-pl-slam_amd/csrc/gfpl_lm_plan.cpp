// gfpl_lm_plan.cpp — the planner of the landmark descriptor store (include/gfpl.h):
// gfpl_lm_ops_check and what gfpl_lmstore_apply runs before any device work.  One pass simulates
// the counts in array order (the first op that fails decides the return code) and numbers the
// touched landmarks by first touch; a counting sort over the six lane-group buckets orders them;
// a second pass places the ops, so the grouping is stable and linear in the number of ops.
#include "gfpl_lm_plan.hpp"

namespace gfpl {

static_assert(LM_MAX_OBS == GFPL_LM_MAX_OBS, "the lane-group layout and the public cap are one number");

namespace {
struct Touch {
    int32_t lm, n_ops, count0, peak;   // a touched landmark: its ops, its count before them, the longest list it reaches
};
}  // namespace

int lm_plan(const gfpl_lm_op* ops, int n, int32_t* counts, int lm_cap, int obs_cap, const int32_t* src_rows,
            int n_srcs, int min_g, LmPlan* plan, int32_t* slot) {
    if (n < 0 || lm_cap < 1 || obs_cap < 1 || obs_cap > GFPL_LM_MAX_OBS || !counts || (n > 0 && !ops) || n_srcs < 0 ||
        (n_srcs > 0 && !src_rows))
        return GFPL_E_INVALID;
    if (plan) {
        plan->order.clear();
        plan->work.clear();
        for (int b = 0; b <= LM_BUCKETS; ++b) plan->bucket_start[b] = 0;
    }
    if (n == 0) return GFPL_OK;
    std::vector<int32_t> own;
    if (!slot) {
        own.assign((size_t)lm_cap, -1);
        slot = own.data();
    }
    std::vector<Touch> t;   // in first-touch order
    int rc = GFPL_OK;
    for (int i = 0; i < n && rc == GFPL_OK; ++i) {
        const gfpl_lm_op& op = ops[i];
        if (op.lm < 0 || op.lm >= lm_cap) { rc = GFPL_E_INVALID; break; }
        int32_t& c = counts[op.lm];
        if (slot[op.lm] < 0) {
            if (c < 0 || c > obs_cap) { rc = GFPL_E_INVALID; break; }   // (a caller's counts; the store's mirror never is)
            slot[op.lm] = (int32_t)t.size();
            t.push_back(Touch{op.lm, 0, c, c});
        }
        Touch& u = t[(size_t)slot[op.lm]];
        switch (op.kind) {
        case GFPL_LM_ADD:
            if (op.src < 0 || op.src >= n_srcs || op.arg < 0 || op.arg >= src_rows[op.src]) rc = GFPL_E_INVALID;
            else if (c >= obs_cap) rc = GFPL_E_CAPACITY;
            else if (++c > u.peak) u.peak = c;
            break;
        case GFPL_LM_ERASE_OBS:
            if (op.arg < 0 || op.arg >= c) rc = GFPL_E_INVALID;
            else --c;
            break;
        case GFPL_LM_FREE:
            c = 0;
            break;
        default:
            rc = GFPL_E_INVALID;
        }
        if (rc == GFPL_OK) ++u.n_ops;
    }
    if (rc != GFPL_OK) {
        for (const Touch& u : t) {
            counts[u.lm] = u.count0;
            slot[u.lm] = -1;
        }
        return rc;
    }
    if (plan) {
        // buckets by the longest list a landmark reaches, then the ops' places in work order
        int fill[LM_BUCKETS + 1] = {};
        for (const Touch& u : t) ++fill[lm_bucket_of(u.peak, min_g) + 1];
        for (int b = 0; b < LM_BUCKETS; ++b) fill[b + 1] += fill[b];
        for (int b = 0; b <= LM_BUCKETS; ++b) plan->bucket_start[b] = fill[b];
        plan->work.resize(t.size());
        std::vector<int32_t> cursor(t.size());   // touch -> the next place of its ops in `order`
        for (size_t s = 0; s < t.size(); ++s) {
            const int w = fill[lm_bucket_of(t[s].peak, min_g)]++;
            cursor[s] = w;   // (the touch's work item, until the op ranges are known)
            plan->work[(size_t)w] = LmWork{t[s].lm, 0, t[s].n_ops, t[s].count0};
        }
        int32_t op0 = 0;
        for (LmWork& w : plan->work) {
            w.op0 = op0;
            op0 += w.n_ops;
        }
        for (size_t s = 0; s < t.size(); ++s) cursor[s] = plan->work[(size_t)cursor[s]].op0;
        plan->order.resize((size_t)n);
        for (int i = 0; i < n; ++i) plan->order[(size_t)cursor[(size_t)slot[ops[i].lm]]++] = i;
    }
    for (const Touch& u : t) slot[u.lm] = -1;
    return GFPL_OK;
}

}  // namespace gfpl

extern "C" int gfpl_lm_ops_check(const gfpl_lm_op* ops, int n, int32_t* counts, int lm_cap, int obs_cap,
                                 const int32_t* src_rows, int n_srcs) {
    return gfpl::lm_plan(ops, n, counts, lm_cap, obs_cap, src_rows, n_srcs, 0, nullptr, nullptr);
}
