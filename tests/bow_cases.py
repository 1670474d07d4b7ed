"""Case families of the loop-closure candidate search (tests/test_bow_cpu.py, tests/test_bow_gpu.py):
vocabularies as the flat arrays of gfpl_vocab_desc, descriptor sets, BowVector pairs and a keyframe
sequence.  Everything is generated from fixed seeds; the expected values come from tests/bow_ref.py."""
import numpy as np

import bow_ref as R


def _desc(rng, sparse):
    """a 32-byte descriptor; sparse: few set bits, so that many distances are equal"""
    if not sparse:
        return rng.integers(0, 256, 32, dtype=np.uint8)
    d = np.zeros(32, np.uint8)
    for b in rng.choice(256, 6, replace=False):
        d[b // 8] |= np.uint8(1 << (b % 8))
    return d


def tree_vocab(kids_of, seed, weighting=R.TF_IDF, shuffle_nodes=True, shuffle_words=False, sparse=False,
               dup_siblings=False, bad_weights=False, all_stopped=False, weight=None):
    """A vocabulary over the tree kids_of (list: node -> list of children, node 0 the root, nodes in any
    order).  shuffle_nodes: renumber the nodes at random (the root stays 0), as a .yml vocabulary may;
    shuffle_words: word ids in a random order with gaps; dup_siblings: every second sibling repeats its
    elder's descriptor; bad_weights: a third of the leaves weigh 0, a negative number or NaN."""
    rng = np.random.default_rng(seed)
    n = len(kids_of)
    perm = np.arange(n)
    if shuffle_nodes:
        perm[1:] = 1 + rng.permutation(n - 1)
    kids = [None] * n
    for i, ks in enumerate(kids_of):
        kids[perm[i]] = [int(perm[c]) for c in ks]
    desc = np.zeros((n, 32), np.uint8)
    for i in range(n):
        for j, c in enumerate(kids[i]):
            desc[c] = desc[kids[i][j - 1]] if (dup_siblings and j % 2 == 1) else _desc(rng, sparse)
    leaves = [i for i in range(n) if not kids[i]]
    word_id = np.full(n, -1, np.int32)
    ids = np.arange(len(leaves))
    if shuffle_words:
        ids = rng.permutation(3 * len(leaves))[:len(leaves)]
    for i, w in zip(leaves, ids):
        word_id[i] = w
    wts = np.zeros(n, np.float64)
    for i in leaves:
        wts[i] = weight if weight is not None else (1.0 if weighting in (R.TF, R.BINARY) else rng.uniform(0.05, 6.0))
    if bad_weights:
        for j, i in enumerate(leaves):
            if j % 3 == 1:
                wts[i] = (0.0, -1.5, float("nan"), -0.0)[(j // 3) % 4]
    if all_stopped:
        for i in leaves:
            wts[i] = 0.0
    child_off = np.zeros(n + 1, np.int32)
    child_off[1:] = np.cumsum([len(k) for k in kids])
    child = np.array([c for ks in kids for c in ks], np.int32)
    return dict(child_off=child_off, child=child, desc=desc, weight=wts, word_id=word_id, weighting=weighting, scoring=0)


def full_tree(k, L):
    """k children per node, leaves at depth L, breadth first"""
    kids, level = [[]], [0]
    for _ in range(L):
        nxt = []
        for p in level:
            for _ in range(k):
                kids.append([])
                kids[p].append(len(kids) - 1)
                nxt.append(len(kids) - 1)
        level = nxt
    return kids


def ragged_tree():
    """a leaf at depth 1 beside depth-3 subtrees, and nodes with one child"""
    kids = [[1, 2, 3, 4]]           # root
    kids += [[], [5, 6, 7], [8], [9, 10]]   # 1 leaf; 2 inner; 3 one child; 4 inner
    kids += [[11, 12], [13], [], []]        # 5 inner, 6 one child, 7 leaf (depth 2), 8 leaf
    kids += [[14, 15, 16], []]              # 9 inner, 10 leaf
    kids += [[], [], [], [], [], []]        # 11-16 leaves at depth 3
    return kids


def ref_vocab(v):
    return R.Vocabulary(v["child_off"], v["child"], v["desc"], v["weight"], v["word_id"], v["weighting"])


def vocabularies():
    """name -> flat arrays"""
    out = {
        "k10_L3": tree_vocab(full_tree(10, 3), 11),
        "ragged": tree_vocab(ragged_tree(), 12, sparse=True),
        "shuffled_words": tree_vocab(full_tree(5, 2), 13, shuffle_words=True),
        "bad_weights": tree_vocab(full_tree(6, 2), 14, bad_weights=True),
        "dup_siblings": tree_vocab(full_tree(7, 2), 15, dup_siblings=True, sparse=True),
        "all_stopped": tree_vocab(full_tree(3, 2), 16, all_stopped=True),
        "tenth": tree_vocab(full_tree(4, 2), 17, weight=0.1),
    }
    for k in (1, 2, 16, 17, 20, 32):
        out[f"k{k}_L2"] = tree_vocab(full_tree(k, 2), 20 + k, sparse=(k in (17, 32)))
    for w, name in ((R.TF, "tf"), (R.IDF, "idf"), (R.BINARY, "binary")):
        out[name] = tree_vocab(full_tree(4, 2), 30 + w, weighting=w, sparse=True, weight=None if w == R.IDF else 1.0)
    return out


SET_SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 257)


def descriptor_sets(v, seed, sizes=SET_SIZES, sparse=False):
    """random sets of the given sizes; half of every set's rows are node descriptors of the vocabulary
    with a few bits flipped (they tie between duplicated siblings and land deep in the tree)"""
    rng = np.random.default_rng(seed)
    nodes = v["desc"]
    out = []
    for n in sizes:
        d = np.zeros((n, 32), np.uint8)
        for i in range(n):
            if i % 2:
                d[i] = nodes[rng.integers(1, len(nodes))]
                for b in rng.choice(256, rng.integers(0, 3), replace=False):
                    d[i][b // 8] ^= np.uint8(1 << (b % 8))
            else:
                d[i] = _desc(rng, sparse)
        out.append(d)
    return out


def ref_transform(v, sets):
    rv = ref_vocab(v)
    return [rv.transform(list(s)) for s in sets]


def bow_vector(rng, n, universe):
    """a random BowVector of n words out of range(universe): ([ids ascending], [values])"""
    ids = np.sort(rng.choice(universe, n, replace=False)).astype(np.int32)
    vals = rng.uniform(0.0, 1.0, n)
    if n:
        vals = vals / vals.sum()
    return ids, vals.astype(np.float64)


def score_pairs():
    """name -> (a, b), each (ids, values)"""
    rng = np.random.default_rng(40)
    e = (np.zeros(0, np.int32), np.zeros(0, np.float64))
    out = {"empty_empty": (e, e)}
    a = bow_vector(rng, 64, 500)
    out["empty_a"] = (e, a)
    out["a_empty"] = (a, e)
    out["identical"] = (a, a)
    out["one_word_self"] = ((np.array([7], np.int32), np.array([1.0])), (np.array([7], np.int32), np.array([1.0])))
    lo, hi = bow_vector(rng, 65, 1000), bow_vector(rng, 64, 1000)
    out["disjoint"] = ((lo[0], lo[1]), (hi[0] + 1000, hi[1]))
    big = bow_vector(rng, 2000, 6000)
    sub = (big[0][::7].copy(), rng.uniform(0, 1, len(big[0][::7])))
    out["nested"] = (sub, big)
    out["nested_rev"] = (big, sub)
    # an overlap in the middle with long runs of unshared words on either side
    ia = np.concatenate([np.arange(0, 900, 3), np.arange(3000, 3100), np.arange(5000, 5600, 2)]).astype(np.int32)
    ib = np.concatenate([np.arange(1, 900, 3), np.arange(3050, 3150), np.arange(5001, 5600, 2)]).astype(np.int32)
    out["runs"] = ((ia, rng.uniform(0, 1, len(ia))), (ib, rng.uniform(0, 1, len(ib))))
    for n in (1, 64, 65, 2000):
        out[f"len{n}"] = (bow_vector(rng, n, 3 * n + 5), bow_vector(rng, n, 3 * n + 5))
    out["signed"] = ((np.arange(70, dtype=np.int32), rng.uniform(-1, 1, 70)), (np.arange(0, 140, 2, dtype=np.int32),
                                                                                rng.uniform(-1, 1, 70)))
    return out


def ref_score(a, b):
    return R.score(list(zip(a[0].tolist(), a[1].tolist())), list(zip(b[0].tolist(), b[1].tolist())))


# ------------------------------------------------------------- keyframe sequence --
SEQ_N, SEQ_PT, SEQ_LS = 40, 96, 40
SEQ_REVISIT = 28          # keyframes from here on see the places of keyframes SEQ_REVISIT - 22 ...
SEQ_ERASE = {12: 7, 25: 20}   # after the insert of key: erase value
SEQ_SEARCH = dict(lc_kf_dist=5, lc_kf_max_dist=3, lc_nkf_closest=2, min_lm_cov_graph=30, min_kf_local_map=3)


def _flip(rng, d, flips):
    d = d.copy()
    for b in rng.choice(256, flips, replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def keyframe_sequence(pair=None):
    """SEQ_N keyframes along a stream of descriptors: place p sees rows [p S, p S + N) of the stream
    (S = N / 4, so neighbouring places share three quarters of their rows); keyframe i stands at place i
    until SEQ_REVISIT and at place i - 22 from there on, with 4 bits of every row flipped.  pair = (A, B,
    f0, f1): place A's rows are f0's descriptors, and keyframe B (which revisits A) gets f1's.  Returns per
    keyframe (pdesc, ldesc, pl, spl, epl)."""
    rng = np.random.default_rng(50)
    sp, sl = SEQ_PT // 4, SEQ_LS // 4
    n_place = SEQ_N
    ps = rng.integers(0, 256, (n_place * sp + SEQ_PT, 32), dtype=np.uint8)
    ls = rng.integers(0, 256, (n_place * sl + SEQ_LS, 32), dtype=np.uint8)
    if pair:
        A, B, f0, f1 = pair
        ps[A * sp:A * sp + SEQ_PT] = f0.arr["pdesc"][:SEQ_PT]
        ls[A * sl:A * sl + SEQ_LS] = f0.arr["ldesc"][:SEQ_LS]
    out = []
    for i in range(SEQ_N):
        p = i if i < SEQ_REVISIT else i - 22
        pd, ld = ps[p * sp:p * sp + SEQ_PT].copy(), ls[p * sl:p * sl + SEQ_LS].copy()
        if i >= SEQ_REVISIT:
            pd = np.stack([_flip(rng, d, 4) for d in pd])
            ld = np.stack([_flip(rng, d, 4) for d in ld])
        if pair and i == pair[1]:
            pd, ld = pair[3].arr["pdesc"][:SEQ_PT].copy(), pair[3].arr["ldesc"][:SEQ_LS].copy()
        n_pt, n_ls = SEQ_PT - (i % 5), SEQ_LS - (i % 3)   # stereo_pt / stereo_ls: fewer than the descriptor rows
        pl = rng.uniform(0, 640, (n_pt, 2))
        spl = rng.uniform(0, 640, (n_ls, 2))
        epl = spl + rng.uniform(-60, 60, (n_ls, 2))
        out.append((pd, ld, pl, spl, epl))
    return out


def graph_col(kf):
    """full_graph[i][kf]: a keyframe shares landmarks with its two predecessors"""
    return np.array([40 if kf - i <= 2 else 0 for i in range(kf)], np.int32)


def as_float_matrix(x):
    """what the reference's vector<vector<float>> conf_matrix holds of a score"""
    return float(np.float32(x))
