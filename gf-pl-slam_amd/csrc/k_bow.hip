// k_bow.hip — DBoW2 as the loop-closure candidate search uses it (src/mapHandler.cpp:2865-3000).
//
//  k_bow_descend : TemplatedVocabulary::transform(feature, word_id, weight)
//              (TemplatedVocabulary.h:1217-1259).  One descriptor per 16-lane DPP row, four per
//              wave: per level each lane takes child positions lane and lane + 16, loads the
//              child's 32-byte row (two 16-byte loads) and its node record, forms the key
//              (distance << 8) | position, and the row minimum over the DPP crossbar names the
//              first child of least distance (the reference replaces on d < best_d only).  The
//              winner's record comes from its lane by one permute, so a level is ONE dependent
//              gather.  Writes the leaf's rank (ascending word id), or BOW_STOP for a leaf whose
//              weight is not > 0.
//  k_bow_finish : the rest of transform(features, BowVector&) (:1065-1122) and
//              BowVector::normalize(L1), one workgroup per set: bitonic sort of the ranks in LDS,
//              run lengths, the value of a word met c times as w added c - 1 times to w (TF,
//              TF_IDF) or w (IDF, BINARY), the L1 norm summed by one lane in ascending word id,
//              every value divided by it.
//  k_bow_score : L1Scoring::score (ScoringObject.cpp:23-68), one wave per pair: the lanes search
//              their entries of the shorter vector in the longer one, and the wave adds the terms of
//              the hits in ascending word id, one after the other.
// Keyframe-rate work.  The shapes follow from the dependent-gather chain (descend) and the
// ordered sums (finish, score); DESIGN.md §5m records what was measured.
#include "gfpl_kernels.hpp"
#include "gfpl_wave.hpp"

namespace gfpl {

namespace {

constexpr int BOW_BLOCK = 256;

GFPL_DEV int bow_hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return ((__popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y)) + (__popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w))) +
           ((__popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y)) + (__popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w)));
}

// the minimum over the lane's 16-lane row, in every lane of the row
GFPL_DEV int row16_min(int k) {
    k = min(k, dpp_i32<DPP_XOR1>(k));
    k = min(k, dpp_i32<DPP_XOR2>(k));
    k = min(k, dpp_i32<DPP_HALF_MIRROR>(k));
    k = min(k, dpp_i32<DPP_ROW_MIRROR>(k));
    return k;
}

}  // namespace

__global__ void __launch_bounds__(BOW_BLOCK) k_bow_descend(BowVocabDev v, const BowSet* sets, int cap, int32_t* keys) {
    const int set = blockIdx.y;
    const BowSet s = sets[set];
    const int lane = threadIdx.x & 63, l16 = lane & 15;
    const int f = (int)((blockIdx.x * BOW_BLOCK + threadIdx.x) >> 4);   // the row's descriptor
    const bool mine = f < s.count;
    bool active = mine;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (mine) {
        const uint4* q = reinterpret_cast<const uint4*>(s.desc + 32 * (size_t)f);
        q0 = q[0];
        q1 = q[1];
    }
    const BowNode root = v.node[0];
    int c0 = root.child0, nc = root.n_child;   // the root has children (gfpl_vocab_create)
    int leaf_key = BOW_STOP;
    // every lane of the wave runs the loop until its last row is done: the DPP steps need their
    // source lanes executing, so nothing below returns or branches around them
    while (__builtin_amdgcn_ballot_w64(active)) {
        int k0 = 0x7fffffff, k1 = 0x7fffffff;
        BowNode m0 = {0, 0, 0, 0}, m1 = m0;
        if (active && l16 < nc) {
            const size_t c = (size_t)c0 + l16;
            const uint4* d = reinterpret_cast<const uint4*>(v.desc + 32 * c);
            const uint4 d0 = d[0], d1 = d[1];
            m0 = v.node[c];
            k0 = (bow_hamming(q0, q1, d0, d1) << 8) | l16;
        }
        if (active && l16 + 16 < nc) {
            const size_t c = (size_t)c0 + l16 + 16;
            const uint4* d = reinterpret_cast<const uint4*>(v.desc + 32 * c);
            const uint4 d0 = d[0], d1 = d[1];
            m1 = v.node[c];
            k1 = (bow_hamming(q0, q1, d0, d1) << 8) | (l16 + 16);
        }
        const int k = row16_min(min(k0, k1));
        const int p = k & 0xff;                      // the winning child position (row-uniform)
        const BowNode mw = p >= 16 ? m1 : m0;        // what this lane holds for that half
        const int src = (lane & ~15) | (p & 15);     // the lane that loaded the winner
        const int w_child0 = __shfl(mw.child0, src, 64);
        const int w_nchild = __shfl(mw.n_child, src, 64);
        const int w_key = __shfl(mw.key, src, 64);
        if (active) {
            c0 = w_child0;
            nc = w_nchild;
            if (nc == 0) { leaf_key = w_key; active = false; }
        }
    }
    if (mine && l16 == 0) keys[(size_t)set * cap + f] = leaf_key;
}

__global__ void __launch_bounds__(BOW_BLOCK) k_bow_finish(BowVocabDev v, const BowSet* sets, int cap, int p2, int max_count,
                                                          const int32_t* keys_in, int32_t* word_ids, double* values,
                                                          int32_t* n_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    BowFinishLds L(smem, p2, max_count);
    const int tid = threadIdx.x;
    const int set = blockIdx.x;
    const int count = sets[set].count;
    const int32_t* kin = keys_in + (size_t)set * cap;
    int32_t* wout = word_ids + (size_t)set * cap;
    double* vout = values + (size_t)set * cap;

    for (int i = tid; i < p2; i += BOW_BLOCK) L.keys[i] = i < count ? kin[i] : BOW_STOP;
    __syncthreads();
    // bitonic sort, ascending: ranks ascend with word ids, stopped features (BOW_STOP) go last
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (p2 >> 1); t += BOW_BLOCK) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const int a = L.keys[i], b = L.keys[l];
                const bool asc = (i & k) == 0;
                if ((a > b) == asc && a != b) { L.keys[i] = b; L.keys[l] = a; }
            }
            __syncthreads();
        }
    }
    // one entry per run of equal ranks, in order (BowVector is a std::map: ascending word id)
    const bool add = v.weighting == GFPL_BOW_TF_IDF || v.weighting == GFPL_BOW_TF;
    int m = 0;
    for (int c0 = 0; c0 < count; c0 += BOW_BLOCK) {
        const int i = c0 + tid;
        int key = BOW_STOP, head = 0;
        if (i < count) {
            key = L.keys[i];
            head = key != BOW_STOP && (i == 0 || L.keys[i - 1] != key);
        }
        int tot;
        const int pos = m + block_exclusive_scan<BOW_BLOCK>(head, L.scan, &tot);
        if (head) {
            const double w = v.rank_weight[key];
            double val = w;   // addWeight's insert; addIfNotExist
            if (add)
                for (int j = i + 1; j < count && L.keys[j] == key; ++j) val = val + w;   // v[id] += w, c - 1 times
            L.vals[pos] = val;
            wout[pos] = v.rank_word[key];
        }
        m += tot;
    }
    __syncthreads();
    // BowVector::normalize(L1): norm += fabs(value) in map order, then value /= norm when norm > 0
    if (tid == 0) {
        double norm = 0.0;
        for (int i = 0; i < m; ++i) norm = norm + fabs(L.vals[i]);
        L.norm[0] = norm;
        n_words[set] = m;
    }
    __syncthreads();
    const double norm = L.norm[0];
    for (int i = tid; i < m; i += BOW_BLOCK) vout[i] = norm > 0.0 ? L.vals[i] / norm : L.vals[i];
}

__global__ void __launch_bounds__(BOW_BLOCK) k_bow_score(const BowPair* pairs, int n, double* scores) {
    const int lane = threadIdx.x & 63;
    const int pr = (int)(blockIdx.x * (BOW_BLOCK / 64) + (threadIdx.x >> 6));
    if (pr >= n) return;   // wave-uniform
    const BowPair p = pairs[pr];
    const bool a_short = p.na <= p.nb;
    const int32_t* sid = a_short ? p.ia : p.ib;
    const int32_t* lid = a_short ? p.ib : p.ia;
    const int ns = a_short ? p.na : p.nb, nl = a_short ? p.nb : p.na;
    double score = 0.0;
    for (int base = 0; base < ns; base += 64) {
        const int i = base + lane;
        bool hit = false;
        double t = 0.0;
        if (i < ns) {
            const int id = sid[i];
            int lo = 0, hi = nl;   // lower_bound of id in the longer vector
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (lid[mid] < id) lo = mid + 1; else hi = mid;
            }
            if (lo < nl && lid[lo] == id) {
                hit = true;
                const double vi = p.va[a_short ? i : lo], wi = p.vb[a_short ? lo : i];
                t = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
            }
        }
        // score += term, for the common words in ascending id: the hits of this chunk in lane order
        unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        while (mask) {
            const int l = __builtin_ctzll(mask);
            score = score + readlane_f64(t, l);
            mask &= mask - 1;
        }
    }
    if (lane == 0) scores[pr] = -score / 2.0;   // no common word: -(+0.0) / 2 = -0.0
}

hipError_t launch_bow_transform(const BowVocabDev& v, const BowSet* sets, int n, int max_count, int cap, int32_t* keys,
                                int32_t* word_ids, double* values, int32_t* n_words, hipStream_t s) {
    static std::atomic<unsigned long long> lds_done{0};
    int p2 = 64;
    while (p2 < max_count) p2 <<= 1;
    const BowFinishLds L(nullptr, p2, max_count);
    if (L.bytes > 64 * 1024) {
        hipError_t e = ensure_dyn_lds((const void*)k_bow_finish, DYN_LDS_CEILING, &lds_done);
        if (e != hipSuccess) return e;
    }
    if (max_count > 0) {
        const int rows = BOW_BLOCK / 16;   // descriptors per block
        hipLaunchKernelGGL(k_bow_descend, dim3((max_count + rows - 1) / rows, n), dim3(BOW_BLOCK), 0, s, v, sets, cap, keys);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_bow_finish, dim3(n), dim3(BOW_BLOCK), L.bytes, s, v, sets, cap, p2, max_count, keys, word_ids,
                       values, n_words);
    return hipGetLastError();
}

hipError_t launch_bow_score(const BowPair* pairs, int n, double* scores, hipStream_t s) {
    const int per = BOW_BLOCK / 64;
    hipLaunchKernelGGL(k_bow_score, dim3((n + per - 1) / per), dim3(BOW_BLOCK), 0, s, pairs, n, scores);
    return hipGetLastError();
}

}  // namespace gfpl
