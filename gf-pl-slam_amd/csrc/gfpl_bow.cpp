// gfpl_bow.cpp — host side of the loop-closure candidate search (include/gfpl.h):
// the vocabulary object (validation, breadth-first renumbering, upload), the batched transform and
// score calls around k_bow.hip, the keyframe database (insertKFBowVectorP / L / PL,
// src/mapHandler.cpp:2865-3000) and the two pure host functions, vector_stdv of a keyframe's
// features and lookForLoopCandidates (:3002-3076).
#include <algorithm>
#include <cmath>

#include "gfpl_host.hpp"

using namespace gfpl;

struct gfpl_vocab {
    gfpl_ctx* ctx = nullptr;
    int device = 0;
    char* base = nullptr;
    BowVocabDev dev{};
};

struct gfpl_bowdb {
    gfpl_ctx* ctx = nullptr;
    const gfpl_vocab* voc[2] = {nullptr, nullptr};   // points, lines
    int mode = 0, kf_cap = 0, cap[2] = {0, 0};
    char* base = nullptr;
    int32_t* ids[2] = {nullptr, nullptr};            // [kf_cap][cap[k]]
    double* vals[2] = {nullptr, nullptr};
    BowSet* sets = nullptr;                          // [2] scratch of an insert
    int32_t* keys = nullptr;                         // [max cap]
    int32_t* nw = nullptr;                           // [2]
    BowPair* pairs = nullptr;                        // [2 kf_cap]
    double* scores = nullptr;                        // [2 kf_cap]
    std::vector<int> count[2];                       // words of keyframe i's vector
    std::vector<uint8_t> state;                      // 0 never inserted, 1 live, 2 erased
};

namespace {

// the scratch of a transform call over n sets of capacity cap
struct BowScratch {
    Carver c;
    BowSet* sets;
    int32_t* keys;
    int32_t* nw;
    size_t bytes;
    BowScratch(char* base, int n, int cap)
        : c{0, base}, sets(c.take<BowSet>((size_t)n)), keys(c.take<int32_t>((size_t)n * cap)),
          nw(c.take<int32_t>((size_t)n)), bytes(c.off) {}
};

// the database's one allocation
struct BowDbMem {
    Carver c;
    int32_t* ids[2];
    double* vals[2];
    BowSet* sets;
    int32_t* keys;
    int32_t* nw;
    BowPair* pairs;
    double* scores;
    size_t bytes;
    BowDbMem(char* base, int kf_cap, int pt_cap, int ls_cap, bool has_p, bool has_l) : c{0, base} {
        const int cap[2] = {has_p ? pt_cap : 0, has_l ? ls_cap : 0};
        for (int k = 0; k < 2; ++k) {
            ids[k] = c.take<int32_t>((size_t)kf_cap * cap[k]);
            vals[k] = c.take<double>((size_t)kf_cap * cap[k]);
        }
        sets = c.take<BowSet>(2);
        keys = c.take<int32_t>((size_t)std::max(std::max(cap[0], cap[1]), 1));
        nw = c.take<int32_t>(2);
        pairs = c.take<BowPair>(2 * (size_t)kf_cap);
        scores = c.take<double>(2 * (size_t)kf_cap);
        bytes = c.off;
    }
};

// vector_stdv (src/auxiliar.cpp:547-556) of the n values f(0) .. f(n - 1); v.size() is a size_t there
template <typename F>
double stdv(int n, F f) {
    // the divisions run on the FPU also for n = 0 (a compiler that folds the empty path picks a NaN of
    // its own sign): 1.0 / 0 * 0 is then the hardware's default NaN (ledger BW7)
    volatile double size = (double)(size_t)n;
    double mean = 0.0, e = 0.0;
    for (int i = 0; i < n; ++i) mean += f(i);
    mean /= size;
    for (int i = 0; i < n; ++i) e += (f(i) - mean) * (f(i) - mean);
    return std::sqrt(1.0 / size * e);
}

struct ConfEntry { double idx, score; };   // the reference's Vector2d (index, score)

// the host-side rules of gfpl_vocab_create; order[k]: the host node that becomes device node k (breadth
// first), leaves: (word id, device node) ascending
int vocab_check(const gfpl_vocab_desc* d, std::vector<int32_t>& order, std::vector<std::pair<int32_t, int32_t>>& leaves) {
    if (!d) return GFPL_E_INVALID;
    if (!d->child_off || !d->child || !d->desc || !d->weight || !d->word_id) return GFPL_E_INVALID;
    const int n = d->n_nodes;
    if (n < 2) return GFPL_E_INVALID;
    if (d->weighting < GFPL_BOW_TF_IDF || d->weighting > GFPL_BOW_BINARY) return GFPL_E_INVALID;
    if (d->scoring != GFPL_BOW_L1_NORM) return GFPL_E_UNSUPPORTED;
    if (d->child_off[0] != 0) return GFPL_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (d->child_off[i + 1] < d->child_off[i]) return GFPL_E_INVALID;
    if (d->child_off[1] == 0) return GFPL_E_INVALID;   // a root without children
    // breadth first from the root: order[k] = the host node that becomes device node k
    std::vector<uint8_t> seen((size_t)n, 0);
    order.reserve((size_t)n);
    order.push_back(0);
    seen[0] = 1;
    for (size_t k = 0; k < order.size(); ++k) {
        const int h = order[k];
        const int c0 = d->child_off[h], c1 = d->child_off[h + 1];
        if (c1 - c0 > BOW_MAX_CHILDREN) return GFPL_E_UNSUPPORTED;
        if (c1 == c0 && d->word_id[h] < 0) return GFPL_E_INVALID;   // a leaf without a word
        for (int j = c0; j < c1; ++j) {
            const int c = d->child[j];
            if (c < 0 || c >= n) return GFPL_E_INVALID;
            if (seen[c]) return GFPL_E_INVALID;   // reachable twice, or a cycle (the root included)
            seen[c] = 1;
            order.push_back(c);
        }
    }
    const int nd = (int)order.size();
    // leaves ranked by ascending word id; a word id on two leaves is refused
    for (int k = 0; k < nd; ++k)
        if (d->child_off[order[k]] == d->child_off[order[k] + 1]) leaves.emplace_back(d->word_id[order[k]], k);
    std::sort(leaves.begin(), leaves.end());
    for (size_t r = 1; r < leaves.size(); ++r)
        if (leaves[r].first == leaves[r - 1].first) return GFPL_E_INVALID;
    return GFPL_OK;
}

}  // namespace

extern "C" {

int gfpl_vocab_check(const gfpl_vocab_desc* d) {
    std::vector<int32_t> order;
    std::vector<std::pair<int32_t, int32_t>> leaves;
    return vocab_check(d, order, leaves);
}

int gfpl_vocab_create(gfpl_ctx* ctx, const gfpl_vocab_desc* d, gfpl_vocab** out) {
    if (!out) return GFPL_E_INVALID;
    std::vector<int32_t> order;
    std::vector<std::pair<int32_t, int32_t>> leaves;
    const int chk = vocab_check(d, order, leaves);
    if (chk != GFPL_OK) return chk;
    const int n = d->n_nodes, nd = (int)order.size(), nl = (int)leaves.size();
    if (!ctx) return GFPL_E_INVALID;

    const BowVocabMem size(nullptr, nd, nl);
    std::vector<char> img(size.bytes + 256, 0);
    char* hb = img.data() + ((256 - ((uintptr_t)img.data() & 255)) & 255);
    BowVocabMem H(hb, nd, nl);
    std::vector<int32_t> dev_of((size_t)n, -1);
    for (int k = 0; k < nd; ++k) dev_of[order[k]] = k;
    for (int k = 0; k < nd; ++k) {
        const int h = order[k];
        std::memcpy(H.desc + 32 * (size_t)k, d->desc + 32 * (size_t)h, 32);
        const int c0 = d->child_off[h], c1 = d->child_off[h + 1];
        // breadth first: the children of one node were appended together, in Node::children order
        H.node[k] = BowNode{c1 > c0 ? dev_of[d->child[c0]] : 0, c1 - c0, 0, 0};
    }
    for (int r = 0; r < nl; ++r) {
        const int k = leaves[r].second;
        const double w = d->weight[order[k]];
        H.rank_word[r] = leaves[r].first;
        H.rank_weight[r] = w;
        H.node[k].key = w > 0 ? r : BOW_STOP;   // "if(w > 0)": also drops NaN
    }
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(ctx)));
    char* base = nullptr;
    if (hipMalloc(&base, size.bytes) != hipSuccess) {
        (void)hipGetLastError();
        return GFPL_E_NOMEM;
    }
    if (hipMemcpy(base, hb, size.bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(base);
        return GFPL_E_HIP;
    }
    const BowVocabMem D(base, nd, nl);
    gfpl_vocab* v = new gfpl_vocab();
    v->ctx = ctx;
    v->device = gfpl_ctx_device(ctx);
    v->base = base;
    v->dev = BowVocabDev{D.desc, D.node, D.rank_word, D.rank_weight, d->weighting};
    gfpl_ctx_attach(ctx);
    *out = v;
    return GFPL_OK;
}

int gfpl_vocab_destroy(gfpl_vocab* v) {
    if (!v) return GFPL_E_INVALID;
    (void)hipSetDevice(v->device);
    (void)hipFree(v->base);
    gfpl_ctx_detach(v->ctx);
    delete v;
    return GFPL_OK;
}

int gfpl_bow_transform(gfpl_ctx* c, const gfpl_vocab* voc, int n, const uint8_t* const* desc_ptrs, const int* counts,
                       int cap, int32_t* word_ids, double* values, int* n_words) {
    if (!c || !voc || n < 0 || cap < 0) return GFPL_E_INVALID;
    if (voc->device != gfpl_ctx_device(c)) return GFPL_E_INVALID;
    if (n == 0) return GFPL_OK;
    if (!desc_ptrs || !counts || !n_words) return GFPL_E_INVALID;
    int max_count = 0;
    for (int i = 0; i < n; ++i) {
        if (counts[i] < 0) return GFPL_E_INVALID;
        if (counts[i] > 0 && (!desc_ptrs[i] || ((uintptr_t)desc_ptrs[i] & 15))) return GFPL_E_INVALID;
        max_count = std::max(max_count, counts[i]);
    }
    if (max_count > cap) return GFPL_E_CAPACITY;
    if (cap > GFPL_BOW_MAX_CAP || n > 65535) return GFPL_E_UNSUPPORTED;
    if (max_count > 0 && (!word_ids || !values)) return GFPL_E_INVALID;
    GFPL_HIPCHK(hipSetDevice(voc->device));
    hipStream_t s = stream_of(c);
    const BowScratch size(nullptr, n, cap);
    char* scr = nullptr;
    GFPL_HIPCHK(hipMalloc(&scr, size.bytes));
    const BowScratch S(scr, n, cap);
    std::vector<BowSet> hs((size_t)n);
    for (int i = 0; i < n; ++i) hs[i] = BowSet{desc_ptrs[i], counts[i], 0};
    std::vector<int32_t> hn((size_t)n, 0);
    hipError_t e = hipMemcpyAsync(S.sets, hs.data(), (size_t)n * sizeof(BowSet), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_bow_transform(voc->dev, S.sets, n, max_count, cap, S.keys, word_ids, values, S.nw, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hn.data(), S.nw, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    hipError_t es = hipStreamSynchronize(s);   // also on an error path: hs and scr are still in use
    hipError_t ef = hipFree(scr);
    if (e != hipSuccess || es != hipSuccess || ef != hipSuccess) return GFPL_E_HIP;
    for (int i = 0; i < n; ++i) n_words[i] = hn[i];
    return GFPL_OK;
}

int gfpl_bow_score(gfpl_ctx* c, const gfpl_bow_vec* a, const gfpl_bow_vec* b, int n_pairs, double* scores) {
    if (!c || n_pairs < 0) return GFPL_E_INVALID;
    if (n_pairs == 0) return GFPL_OK;
    if (!a || !b || !scores) return GFPL_E_INVALID;
    std::vector<BowPair> hp((size_t)n_pairs);
    for (int i = 0; i < n_pairs; ++i) {
        if (a[i].count < 0 || b[i].count < 0) return GFPL_E_INVALID;
        if (a[i].count > 0 && (!a[i].ids || !a[i].values)) return GFPL_E_INVALID;
        if (b[i].count > 0 && (!b[i].ids || !b[i].values)) return GFPL_E_INVALID;
        hp[i] = BowPair{a[i].ids, a[i].values, b[i].ids, b[i].values, a[i].count, b[i].count};
    }
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(c)));
    hipStream_t s = stream_of(c);
    BowPair* dp = nullptr;
    GFPL_HIPCHK(hipMalloc(&dp, (size_t)n_pairs * sizeof(BowPair)));
    hipError_t e = hipMemcpyAsync(dp, hp.data(), (size_t)n_pairs * sizeof(BowPair), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_bow_score(dp, n_pairs, scores, s);
    hipError_t es = hipStreamSynchronize(s);
    hipError_t ef = hipFree(dp);
    if (e != hipSuccess || es != hipSuccess || ef != hipSuccess) return GFPL_E_HIP;
    return GFPL_OK;
}

int gfpl_kf_bow_stats(const double* pl, int n_pt, const double* spl, const double* epl, int n_ls, gfpl_bow_stats* out) {
    if (!out || n_pt < 0 || n_ls < 0) return GFPL_E_INVALID;
    if ((n_pt > 0 && !pl) || (n_ls > 0 && (!spl || !epl))) return GFPL_E_INVALID;
    // std_pt = vector_stdv(pt_x) + vector_stdv(pt_y) (:2946); zero rows: 0/0, as the reference
    out->std_pt = stdv(n_pt, [&](int i) { return pl[2 * i]; }) + stdv(n_pt, [&](int i) { return pl[2 * i + 1]; });
    // mp = (spl + epl) * 0.5 (:2965)
    out->std_ls = stdv(n_ls, [&](int i) { return (spl[2 * i] + epl[2 * i]) * 0.5; }) +
                  stdv(n_ls, [&](int i) { return (spl[2 * i + 1] + epl[2 * i + 1]) * 0.5; });
    out->n_pt = n_pt;
    out->n_ls = n_ls;
    return GFPL_OK;
}

int gfpl_bowdb_create(gfpl_ctx* c, const gfpl_vocab* voc_p, const gfpl_vocab* voc_l, int mode, int kf_cap, int pt_cap,
                      int ls_cap, gfpl_bowdb** out) {
    if (!c || !out || mode < GFPL_BOW_MODE_P || mode > GFPL_BOW_MODE_PL || kf_cap < 1) return GFPL_E_INVALID;
    const bool has_p = mode != GFPL_BOW_MODE_L, has_l = mode != GFPL_BOW_MODE_P;
    if ((has_p && (!voc_p || pt_cap < 0)) || (has_l && (!voc_l || ls_cap < 0))) return GFPL_E_INVALID;
    if ((has_p && voc_p->device != gfpl_ctx_device(c)) || (has_l && voc_l->device != gfpl_ctx_device(c)))
        return GFPL_E_INVALID;
    if ((has_p && pt_cap > GFPL_BOW_MAX_CAP) || (has_l && ls_cap > GFPL_BOW_MAX_CAP)) return GFPL_E_UNSUPPORTED;
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(c)));
    const BowDbMem size(nullptr, kf_cap, pt_cap, ls_cap, has_p, has_l);
    char* base = nullptr;
    if (hipMalloc(&base, size.bytes) != hipSuccess) {
        (void)hipGetLastError();
        return GFPL_E_NOMEM;
    }
    const BowDbMem M(base, kf_cap, pt_cap, ls_cap, has_p, has_l);
    gfpl_bowdb* db = new gfpl_bowdb();
    db->ctx = c;
    db->voc[0] = has_p ? voc_p : nullptr;
    db->voc[1] = has_l ? voc_l : nullptr;
    db->mode = mode;
    db->kf_cap = kf_cap;
    db->cap[0] = has_p ? pt_cap : 0;
    db->cap[1] = has_l ? ls_cap : 0;
    db->base = base;
    for (int k = 0; k < 2; ++k) {
        db->ids[k] = M.ids[k];
        db->vals[k] = M.vals[k];
        db->count[k].assign((size_t)kf_cap, 0);
    }
    db->sets = M.sets; db->keys = M.keys; db->nw = M.nw; db->pairs = M.pairs; db->scores = M.scores;
    db->state.assign((size_t)kf_cap, 0);
    gfpl_ctx_attach(c);
    *out = db;
    return GFPL_OK;
}

int gfpl_bowdb_destroy(gfpl_bowdb* db) {
    if (!db) return GFPL_E_INVALID;
    (void)hipSetDevice(gfpl_ctx_device(db->ctx));
    (void)hipFree(db->base);
    gfpl_ctx_detach(db->ctx);
    delete db;
    return GFPL_OK;
}

int gfpl_bowdb_insert(gfpl_bowdb* db, int kf_idx, const gfpl_kf_view* kf, const gfpl_bow_stats* stats, double* row) {
    if (!db || !kf || !row || kf_idx < 0) return GFPL_E_INVALID;
    if (kf_idx >= db->kf_cap) return GFPL_E_CAPACITY;
    if (db->state[kf_idx] != 0) return GFPL_E_INVALID;
    if (db->mode == GFPL_BOW_MODE_PL && !stats) return GFPL_E_INVALID;
    const int rows[2] = {kf->n_pt, kf->n_ls};
    const uint8_t* desc[2] = {kf->pdesc, kf->ldesc};
    for (int k = 0; k < 2; ++k) {
        if (!db->voc[k]) continue;
        if (rows[k] < 0 || (rows[k] > 0 && (!desc[k] || ((uintptr_t)desc[k] & 15)))) return GFPL_E_INVALID;
        if (rows[k] > db->cap[k]) return GFPL_E_CAPACITY;
    }
    GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(db->ctx)));
    hipStream_t s = stream_of(db->ctx);
    // the keyframe's BowVectors, written into its slots (kf->descDBoW_P / _L)
    BowSet hs[2] = {{desc[0], rows[0], 0}, {desc[1], rows[1], 0}};
    int32_t hn[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(db->sets, hs, sizeof hs, hipMemcpyHostToDevice, s);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        if (!db->voc[k]) continue;
        const size_t o = (size_t)kf_idx * db->cap[k];
        e = launch_bow_transform(db->voc[k]->dev, db->sets + k, 1, rows[k], db->cap[k], db->keys, db->ids[k] + o,
                                 db->vals[k] + o, db->nw + k, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hn, db->nw, sizeof hn, hipMemcpyDeviceToHost, s);
    hipError_t es = hipStreamSynchronize(s);
    if (e != hipSuccess || es != hipSuccess) return GFPL_E_HIP;
    if (kf_idx == 0) {   // MapHandler::initialize: conf_matrix[0][0] = 1.0
        for (int k = 0; k < 2; ++k) db->count[k][0] = db->voc[k] ? hn[k] : 0;
        db->state[0] = 1;
        row[0] = 1.0;
        return GFPL_OK;
    }
    // one score launch: per kind the new vector against every live keyframe i < kf_idx, then against itself
    std::vector<int> who;
    for (int i = 0; i < kf_idx; ++i)
        if (db->state[i] == 1) who.push_back(i);
    who.push_back(kf_idx);
    const int np = (int)who.size();
    std::vector<BowPair> hp;
    hp.reserve(2 * (size_t)np);
    int kinds = 0;
    for (int k = 0; k < 2; ++k) {
        if (!db->voc[k]) continue;
        ++kinds;
        const size_t o = (size_t)kf_idx * db->cap[k];
        for (int i : who) {
            const size_t oi = (size_t)i * db->cap[k];
            const int ni = i == kf_idx ? hn[k] : db->count[k][i];
            hp.push_back(BowPair{db->ids[k] + o, db->vals[k] + o, db->ids[k] + oi, db->vals[k] + oi, hn[k], ni});
        }
    }
    std::vector<double> sc(hp.size());
    e = hipMemcpyAsync(db->pairs, hp.data(), hp.size() * sizeof(BowPair), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_bow_score(db->pairs, (int)hp.size(), db->scores, s);
    if (e == hipSuccess) e = hipMemcpyAsync(sc.data(), db->scores, sc.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    es = hipStreamSynchronize(s);
    if (e != hipSuccess || es != hipSuccess) return GFPL_E_HIP;
    for (int j = 0; j < np; ++j) {
        if (kinds == 1) {
            row[who[j]] = sc[j];
        } else {   // :2986-2988, :2995-2997, with the new keyframe's n and std
            const double score_p = sc[j], score_l = sc[np + j];
            const int n_pt = stats->n_pt, n_ls = stats->n_ls, n_pl = n_pt + n_ls;
            const double std_pt = stats->std_pt, std_ls = stats->std_ls, std_pl = std_ls + std_pt;
            double score = 0.0;
            score += (score_p * n_pt + score_l * n_ls) / n_pl;
            score += (score_p * std_pt + score_l * std_ls) / std_pl;
            row[who[j]] = score;
        }
    }
    for (int k = 0; k < 2; ++k) db->count[k][kf_idx] = db->voc[k] ? hn[k] : 0;
    db->state[kf_idx] = 1;
    return GFPL_OK;
}

int gfpl_bowdb_erase(gfpl_bowdb* db, int kf_idx) {
    if (!db || kf_idx < 0 || kf_idx >= db->kf_cap || db->state[kf_idx] != 1) return GFPL_E_INVALID;
    db->state[kf_idx] = 2;
    return GFPL_OK;
}

int gfpl_bowdb_vector(const gfpl_bowdb* db, int kind, int kf_idx, gfpl_bow_vec* out, int32_t* ids_host,
                      double* values_host) {
    if (!db || !out || (kind != 0 && kind != 1) || !db->voc[kind]) return GFPL_E_INVALID;
    if (kf_idx < 0 || kf_idx >= db->kf_cap || db->state[kf_idx] != 1) return GFPL_E_INVALID;
    const size_t o = (size_t)kf_idx * db->cap[kind];
    out->ids = db->ids[kind] + o;
    out->values = db->vals[kind] + o;
    out->count = db->count[kind][kf_idx];
    if ((ids_host || values_host) && out->count > 0) {
        GFPL_HIPCHK(hipSetDevice(gfpl_ctx_device(db->ctx)));
        GFPL_HIPCHK(hipStreamSynchronize(stream_of(db->ctx)));
        if (ids_host) GFPL_HIPCHK(hipMemcpy(ids_host, out->ids, (size_t)out->count * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (values_host)
            GFPL_HIPCHK(hipMemcpy(values_host, out->values, (size_t)out->count * sizeof(double), hipMemcpyDeviceToHost));
    }
    return GFPL_OK;
}

void gfpl_default_lc_search_params(gfpl_lc_search_params* p) {
    if (!p) return;
    p->lc_kf_dist = 100;        // src/config.cpp:68-70
    p->lc_kf_max_dist = 20;
    p->lc_nkf_closest = 4;
    p->min_lm_cov_graph = 30;   // :51
    p->min_kf_local_map = 3;    // :53
}

int gfpl_kf_loop_candidates(const double* conf_col, const uint8_t* alive, const int32_t* graph_col, int kf_curr_idx,
                            const gfpl_lc_search_params* prm, int* kf_prev_idx, gfpl_lc_search_info* info) {
    if (!prm || !kf_prev_idx || kf_curr_idx < 0) return GFPL_E_INVALID;
    if (kf_curr_idx > 0 && (!conf_col || !alive || !graph_col)) return GFPL_E_INVALID;
    if (prm->lc_kf_dist < 0 || prm->lc_kf_max_dist < 0 || prm->lc_nkf_closest < 0 || prm->min_lm_cov_graph < 0 ||
        prm->min_kf_local_map < 0)
        return GFPL_E_INVALID;
    int is_lc_candidate = 0;
    *kf_prev_idx = -1;
    // find the best matches (:3010-3021)
    std::vector<ConfEntry> max_confmat;
    for (int i = 0; i < kf_curr_idx - prm->lc_kf_dist; i++)
        if (alive[i]) max_confmat.push_back(ConfEntry{(double)i, conf_col[i]});
    std::sort(max_confmat.begin(), max_confmat.end(),
              [](const ConfEntry& a, const ConfEntry& b) { return a.score > b.score; });
    // the minimum score in the covisibility graph and / or the previous keyframes (:3024-3033)
    double lc_min_score = 1.0;
    for (int i = 0; i < kf_curr_idx; i++) {
        if (graph_col[i] >= prm->min_lm_cov_graph || kf_curr_idx - i <= prm->min_kf_local_map + 3) {
            const double score_i = conf_col[i];
            if (score_i < lc_min_score && score_i > 0.001) lc_min_score = score_i;
        }
    }
    int idx_max = -1, Nkf_closest = 0;
    if (max_confmat.size() > (size_t)prm->lc_kf_max_dist) {   // (:3036-3061)
        idx_max = int(max_confmat[0].idx);
        if (max_confmat[0].score >= lc_min_score) {
            for (size_t i = 1; i < max_confmat.size(); i++) {
                const int idx = int(max_confmat[i].idx);
                if (std::abs(idx - idx_max) <= prm->lc_kf_max_dist && max_confmat[i].score >= lc_min_score * 0.8)
                    Nkf_closest++;
            }
        }
        if (Nkf_closest >= prm->lc_nkf_closest) {
            is_lc_candidate = 1;
            *kf_prev_idx = idx_max;
        }
    }
    if (info) {
        info->lc_min_score = lc_min_score;
        info->nkf_closest = Nkf_closest;
        info->idx_max = idx_max;
        info->n_list = (int32_t)max_confmat.size();
        info->pad = 0;
    }
    return is_lc_candidate;
}

}  // extern "C"
