// gfpl_lm_fuse_plan.cpp — the planner of gfpl_lmstore_fuse (include/gfpl.h):
// gfpl_lm_fuse_check and what gfpl_lmstore_fuse runs before any device work.  One pass runs the ops
// one after another over the whole list.  There is no erasure and a freed landmark is not named
// again, so a list only ever grows at its end and no row below a landmark's count before the call
// changes during the call: every element a list gains is either a source row or such a store row,
// and an append copies the origins of its source as they stand at that op.  The work items then
// carry plain ADDs whose rows point into the sources or into the store itself.
#include "gfpl_lm_fuse_plan.hpp"

namespace gfpl {

int lm_fuse_plan(const gfpl_lm_op* ops, int n, int32_t* counts, int lm_cap, int obs_cap, const int32_t* src_rows,
                 int n_srcs, int min_g, int64_t* n_rows, LmFusePlan* plan, int32_t* slot) {
    if (n_rows) *n_rows = 0;
    if (n < 0 || lm_cap < 1 || obs_cap < 1 || obs_cap > GFPL_LM_MAX_OBS || !counts || (n > 0 && !ops) || n_srcs < 0 ||
        (n_srcs > 0 && !src_rows))
        return GFPL_E_INVALID;
    LmFusePlan local;
    if (!plan) plan = &local;
    plan->touch.clear();
    plan->work.clear();
    plan->work_touch.clear();
    plan->n_dev_ops = 0;
    for (int b = 0; b <= LM_BUCKETS; ++b) plan->bucket_start[b] = 0;
    if (n == 0) return GFPL_OK;
    std::vector<int32_t> own;
    if (!slot) {
        own.assign((size_t)lm_cap, -1);
        slot = own.data();
    }
    std::vector<LmFuseTouch>& t = plan->touch;
    int64_t rows = 0;
    int rc = GFPL_OK;
    for (int i = 0; i < n && rc == GFPL_OK; ++i) {
        const gfpl_lm_op& op = ops[i];
        if (op.lm < 0 || op.lm >= lm_cap) { rc = GFPL_E_INVALID; break; }
        int32_t& c = counts[op.lm];
        if (slot[op.lm] < 0) {
            if (c < 0 || c > obs_cap) { rc = GFPL_E_INVALID; break; }   // (a caller's counts; the store's mirror never is)
            slot[op.lm] = (int32_t)t.size();
            t.push_back(LmFuseTouch{op.lm, c, false, {}});
        }
        const size_t ui = (size_t)slot[op.lm];
        if (t[ui].freed) { rc = GFPL_E_INVALID; break; }
        switch (op.kind) {
        case GFPL_LM_ADD:
            if (op.src < 0 || op.src >= n_srcs || op.arg < 0 || op.arg >= src_rows[op.src]) rc = GFPL_E_INVALID;
            else if (c >= obs_cap) rc = GFPL_E_CAPACITY;
            else {
                t[ui].gained.push_back(LmOrigin{op.src, op.arg});
                ++c;
                ++rows;
            }
            break;
        case GFPL_LM_ERASE_OBS:
            rc = GFPL_E_UNSUPPORTED;
            break;
        case GFPL_LM_FREE:
            t[ui].freed = true;
            t[ui].gained.clear();
            c = 0;
            ++rows;
            break;
        case GFPL_LM_APPEND_LM: {
            if (op.arg < 0 || op.arg >= lm_cap || op.arg == op.lm) { rc = GFPL_E_INVALID; break; }
            const int32_t from = counts[op.arg], fs = slot[op.arg];
            // the source as it stands at this op: its rows from before the call, then what it gained
            if (fs >= 0 ? t[(size_t)fs].freed : (from < 0 || from > obs_cap)) { rc = GFPL_E_INVALID; break; }
            if (from == 0 || c == 0) { rc = GFPL_E_INVALID; break; }
            if (c + from > obs_cap) { rc = GFPL_E_CAPACITY; break; }
            const int32_t from0 = fs >= 0 ? t[(size_t)fs].count0 : from;
            std::vector<LmOrigin>& g = t[ui].gained;
            for (int32_t p = 0; p < from0; ++p) g.push_back(LmOrigin{-1 - op.arg, p});
            if (fs >= 0) {
                const std::vector<LmOrigin>& fg = t[(size_t)fs].gained;   // (another vector: arg != lm)
                g.insert(g.end(), fg.begin(), fg.end());
            }
            c += from;
            rows += from;
            break;
        }
        default:
            rc = GFPL_E_INVALID;
        }
    }
    if (rc != GFPL_OK) {
        for (const LmFuseTouch& u : t) {
            counts[u.lm] = u.count0;
            slot[u.lm] = -1;
        }
        t.clear();
        return rc;
    }
    if (n_rows) *n_rows = rows;
    if (plan != &local) {
        // buckets by the final length (a list never shrinks before its FREE, and a freed landmark
        // runs the FREE alone), first-touch order within a bucket
        auto bucket = [&](const LmFuseTouch& u) {
            return lm_bucket_of(u.freed ? 0 : u.count0 + (int)u.gained.size(), min_g);
        };
        int fill[LM_BUCKETS + 1] = {};
        for (const LmFuseTouch& u : t) ++fill[bucket(u) + 1];
        for (int b = 0; b < LM_BUCKETS; ++b) fill[b + 1] += fill[b];
        for (int b = 0; b <= LM_BUCKETS; ++b) plan->bucket_start[b] = fill[b];
        plan->work.resize(t.size());
        plan->work_touch.resize(t.size());
        for (size_t s = 0; s < t.size(); ++s) {
            const int w = fill[bucket(t[s])]++;
            plan->work[(size_t)w] = LmWork{t[s].lm, 0, t[s].freed ? 1 : (int32_t)t[s].gained.size(), t[s].count0};
            plan->work_touch[(size_t)w] = (int32_t)s;
        }
        int32_t op0 = 0;
        for (LmWork& w : plan->work) {
            w.op0 = op0;
            op0 += w.n_ops;
        }
        plan->n_dev_ops = op0;
    }
    for (const LmFuseTouch& u : t) slot[u.lm] = -1;
    return GFPL_OK;
}

}  // namespace gfpl

extern "C" int gfpl_lm_fuse_check(const gfpl_lm_op* ops, int n, int32_t* counts, int lm_cap, int obs_cap,
                                  const int32_t* src_rows, int n_srcs, int64_t* n_rows) {
    return gfpl::lm_fuse_plan(ops, n, counts, lm_cap, obs_cap, src_rows, n_srcs, 0, n_rows, nullptr, nullptr);
}
