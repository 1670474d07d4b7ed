"""The reference's loop-closure candidate search restated in plain Python: DBoW2's
TemplatedVocabulary<FORB>::transform (3rdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1065-1122, 1217-1259),
BowVector::addWeight / addIfNotExist / normalize (BowVector.cpp:34-84), L1Scoring::score
(ScoringObject.cpp:23-68), MapHandler::insertKFBowVectorP / L / PL (src/mapHandler.cpp:2865-3000),
vector_stdv (src/auxiliar.cpp:547-556) and MapHandler::lookForLoopCandidates (:3002-3076).

Python floats are IEEE doubles and every sum below is an explicit loop in the reference's order, so
the results carry the reference's bits; the two divisions the reference may do by zero go through
ieee_div (Python raises where C++ follows IEEE).  DBoW2 cannot be compiled where OpenCV is missing,
so this restatement is pinned by the hand-computed known answers of tests/test_bow_cpu.py."""
import bisect
import math
import struct

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
LC_SEARCH_DEFAULTS = dict(lc_kf_dist=100, lc_kf_max_dist=20, lc_nkf_closest=4, min_lm_cov_graph=30, min_kf_local_map=3)


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def ieee_div(a: float, b: float) -> float:
    """a / b as C++ computes it, also for b = 0"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def ieee_mul(a: float, b: float) -> float:
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def as_int(desc) -> int:
    """a 32-byte descriptor as one integer (for the XOR / popcount of FORB::distance)"""
    return int.from_bytes(bytes(bytearray(int(b) for b in desc)), "little")


def distance(a: int, b: int) -> int:
    return bin(a ^ b).count("1")


class Vocabulary:
    """the flat arrays of gfpl_vocab_desc; children(i) in Node::children order"""

    def __init__(self, child_off, child, desc, weight, word_id, weighting=TF_IDF):
        self.child_off = [int(x) for x in child_off]
        self.child = [int(x) for x in child]
        self.desc = [as_int(d) for d in desc]
        self.weight = [float(w) for w in weight]
        self.word_id = [int(w) for w in word_id]
        self.weighting = weighting

    def children(self, i):
        return self.child[self.child_off[i]:self.child_off[i + 1]]

    def transform_one(self, f: int):
        """transform(feature, word_id, weight): from the root, the first child of least distance (a child
        replaces the best only on d < best_d), until a node without children"""
        final_id = 0
        while True:
            nodes = self.children(final_id)
            final_id = nodes[0]
            best_d = distance(f, self.desc[final_id])
            for nid in nodes[1:]:
                d = distance(f, self.desc[nid])
                if d < best_d:
                    best_d = d
                    final_id = nid
            if not self.children(final_id):
                break
        return self.word_id[final_id], self.weight[final_id]

    def transform(self, features):
        """transform(features, BowVector&) under L1 scoring (which normalises): [(word id, value)] in
        ascending word id"""
        v = {}
        add = self.weighting in (TF_IDF, TF)
        for f in features:
            wid, w = self.transform_one(as_int(f))
            if w > 0:   # not stopped (false for NaN too)
                if wid in v:
                    if add:
                        v[wid] += w   # addWeight; addIfNotExist leaves it
                else:
                    v[wid] = w
        items = sorted(v.items())
        norm = 0.0
        for _, x in items:
            norm += math.fabs(x)
        if norm > 0.0:
            items = [(i, x / norm) for i, x in items]
        return items


def score(v1, v2) -> float:
    """L1Scoring::score over two [(word id, value)] lists in ascending id, with its lower_bound jumps"""
    k1, k2 = [i for i, _ in v1], [i for i, _ in v2]
    i1 = i2 = 0
    s = 0.0
    while i1 < len(v1) and i2 < len(v2):
        vi, wi = v1[i1][1], v2[i2][1]
        if k1[i1] == k2[i2]:
            s += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
            i1 += 1
            i2 += 1
        elif k1[i1] < k2[i2]:
            i1 = bisect.bisect_left(k1, k2[i2])
        else:
            i2 = bisect.bisect_left(k2, k1[i1])
    return -s / 2.0


def vector_stdv(v) -> float:
    n = float(len(v))
    mean = 0.0
    e = 0.0
    for x in v:
        mean += x
    mean = ieee_div(mean, n)
    for x in v:
        e += (x - mean) * (x - mean)
    return math.sqrt(ieee_mul(ieee_div(1.0, n), e))   # no rows: sqrt(inf * 0) = NaN, as the reference


def bow_stats(pl, spl, epl):
    """(n_pt, n_ls, std_pt, std_ls) of :2940-2947 and :2961-2972"""
    pt_x = [float(p[0]) for p in pl]
    pt_y = [float(p[1]) for p in pl]
    ls_x = [(float(s[0]) + float(e[0])) * 0.5 for s, e in zip(spl, epl)]
    ls_y = [(float(s[1]) + float(e[1])) * 0.5 for s, e in zip(spl, epl)]
    return len(pt_x), len(ls_x), vector_stdv(pt_x) + vector_stdv(pt_y), vector_stdv(ls_x) + vector_stdv(ls_y)


def combine_pl(score_p, score_l, stats) -> float:
    """:2986-2988"""
    n_pt, n_ls, std_pt, std_ls = stats
    std_pl = std_ls + std_pt
    n_pl = n_pt + n_ls
    s = 0.0
    s += ieee_div(ieee_mul(score_p, float(n_pt)) + ieee_mul(score_l, float(n_ls)), float(n_pl))
    s += ieee_div(ieee_mul(score_p, std_pt) + ieee_mul(score_l, std_ls), std_pl)
    return s


class Database:
    """map_keyframes' BowVectors and the rows insertKFBowVector* write: insert returns {i: conf_matrix[idx][i]}
    for the live i < idx and for idx itself (as doubles: the reference then stores them as float)"""

    def __init__(self, voc_p, voc_l, mode):
        self.voc_p, self.voc_l, self.mode = voc_p, voc_l, mode   # mode "P", "L", "PL"
        self.kf = {}   # idx -> (bv_p, bv_l) or None once erased

    def insert(self, idx, pdesc, ldesc, stats=None):
        bv_p = self.voc_p.transform(pdesc) if "P" in self.mode else None
        bv_l = self.voc_l.transform(ldesc) if "L" in self.mode else None
        self.kf[idx] = (bv_p, bv_l)
        if idx == 0:
            return {0: 1.0}   # MapHandler::initialize

        def one(other):
            if self.mode == "P":
                return score(bv_p, other[0])
            if self.mode == "L":
                return score(bv_l, other[1])
            return combine_pl(score(bv_p, other[0]), score(bv_l, other[1]), stats)

        row = {}
        for i in range(idx):
            if self.kf.get(i) is not None:
                row[i] = one(self.kf[i])
        row[idx] = one((bv_p, bv_l))
        return row

    def erase(self, idx):
        self.kf[idx] = None


def look_for_loop_candidates(conf_col, alive, graph_col, kf_curr_idx, prm=None):
    """lookForLoopCandidates: (is_lc_candidate, kf_prev_idx, info).  The order std::sort leaves equal
    scores in is not restated (sorted() is stable): only max_confmat[0] depends on it."""
    p = dict(LC_SEARCH_DEFAULTS)
    p.update(prm or {})
    max_confmat = []
    for i in range(kf_curr_idx - p["lc_kf_dist"]):
        if alive[i]:
            max_confmat.append((float(i), float(conf_col[i])))
    max_confmat = sorted(max_confmat, key=lambda a: -a[1])
    lc_min_score = 1.0
    for i in range(kf_curr_idx):
        if graph_col[i] >= p["min_lm_cov_graph"] or kf_curr_idx - i <= p["min_kf_local_map"] + 3:
            score_i = float(conf_col[i])
            if score_i < lc_min_score and score_i > 0.001:
                lc_min_score = score_i
    is_cand, prev, idx_max, nkf = False, -1, -1, 0
    if len(max_confmat) > p["lc_kf_max_dist"]:
        idx_max = int(max_confmat[0][0])
        nkf = count_closest(max_confmat, 0, lc_min_score, p)
        if nkf >= p["lc_nkf_closest"]:
            is_cand, prev = True, idx_max
    return is_cand, prev, dict(lc_min_score=lc_min_score, nkf_closest=nkf, idx_max=idx_max, n_list=len(max_confmat))


def count_closest(max_confmat, top, lc_min_score, p) -> int:
    """Nkf_closest (:3041-3054) with entry `top` of the list standing first"""
    idx_max = int(max_confmat[top][0])
    nkf = 0
    if max_confmat[top][1] >= lc_min_score:
        for i, (idx, sc) in enumerate(max_confmat):
            if i == top:
                continue
            if abs(int(idx) - idx_max) <= p["lc_kf_max_dist"] and sc >= lc_min_score * 0.8:
                nkf += 1
    return nkf
