"""The loop-closure candidate search without a GPU: the Python reference (tests/bow_ref.py) pinned by
known answers worked by hand below, and the host-only part of the C ABI (gfpl_kf_bow_stats,
gfpl_kf_loop_candidates, the rules of gfpl_vocab_create, Vocabulary.from_text) through the loaded
library against that reference.
"""
import ctypes as C
import math

import numpy as np
import pytest

import bow_cases as BC
import bow_ref as R
import gfpl


def d32(first_byte):
    d = np.zeros(32, np.uint8)
    d[0] = first_byte
    return d


def tiny_vocab(weighting=R.TF_IDF, weights=(0.5, 1.0, 2.0, 4.0)):
    """k = 2, L = 2.  Node 0 the root; 1, 2 its children; 3, 4 under 1; 5, 6 under 2.  Only the first
    descriptor byte is used: 1: 00, 2: FF, 3: 01, 4: 0E, 5: F0, 6: FF.  Words 0..3 are nodes 3..6."""
    desc = np.stack([d32(0), d32(0x00), d32(0xFF), d32(0x01), d32(0x0E), d32(0xF0), d32(0xFF)])
    return dict(child_off=np.array([0, 2, 4, 6, 6, 6, 6, 6], np.int32), child=np.array([1, 2, 3, 4, 5, 6], np.int32),
                desc=desc, weight=np.array([0, 0, 0] + list(weights), np.float64),
                word_id=np.array([-1, -1, -1, 0, 1, 2, 3], np.int32), weighting=weighting, scoring=0)


# ---------------------------------------------------------- known answers --
def test_descent_known_words():
    v = BC.ref_vocab(tiny_vocab())
    # 03: |03^00| = 2 < |03^FF| = 6 -> node 1; |03^01| = 1 < |03^0E| = 3 -> word 0
    assert v.transform_one(R.as_int(d32(0x03))) == (0, 0.5)
    # F7: 7 > 1 -> node 2; |F7^F0| = 3 > |F7^FF| = 1 -> word 3
    assert v.transform_one(R.as_int(d32(0xF7))) == (3, 4.0)
    # F1: 5 > 3 -> node 2; |F1^F0| = 1 < |F1^FF| = 3 -> word 2
    assert v.transform_one(R.as_int(d32(0xF1))) == (2, 2.0)


def test_tie_between_children_goes_to_the_first():
    v = BC.ref_vocab(tiny_vocab())
    # 0F: |0F^00| = 4 = |0F^FF| -> the first, node 1; |0F^01| = 3 > |0F^0E| = 1 -> word 1
    assert v.transform_one(R.as_int(d32(0x0F))) == (1, 1.0)
    # F0: 4 = 4 -> node 1 again (not node 2, whose child 5 IS F0); |F0^01| = 5 < |F0^0E| = 7 -> word 0
    assert v.transform_one(R.as_int(d32(0xF0))) == (0, 0.5)


def test_transform_known_vector():
    v = BC.ref_vocab(tiny_vocab())
    # words 0, 1, 3, 0: word 0 = 0.5 + 0.5 = 1, word 1 = 1, word 3 = 4; norm 6
    bv = v.transform([d32(0x03), d32(0x0F), d32(0xF7), d32(0x03)])
    assert bv == [(0, 1.0 / 6.0), (1, 1.0 / 6.0), (3, 4.0 / 6.0)]
    # IDF / BINARY: a word counts once: 0.5, 1, 4; norm 5.5
    bv = BC.ref_vocab(tiny_vocab(R.IDF)).transform([d32(0x03), d32(0x0F), d32(0xF7), d32(0x03)])
    assert bv == [(0, 0.5 / 5.5), (1, 1.0 / 5.5), (3, 4.0 / 5.5)]


def test_repeated_addition_is_not_a_product():
    s = 0.1
    for _ in range(9):
        s += 0.1
    assert s != 1.0 and s == 0.9999999999999999
    v = BC.ref_vocab(tiny_vocab(weights=(0.1, 1.0, 2.0, 4.0)))
    bv = v.transform([d32(0x03)] * 10 + [d32(0x0F)])   # word 0 ten times, word 1 once
    norm = s + 1.0
    assert bv == [(0, s / norm), (1, 1.0 / norm)]
    assert bv != [(0, (10 * 0.1) / (10 * 0.1 + 1.0)), (1, 1.0 / (10 * 0.1 + 1.0))]


def test_stopped_and_nan_weights_are_dropped():
    v = BC.ref_vocab(tiny_vocab(weights=(0.0, float("nan"), -2.0, 4.0)))
    assert v.transform([d32(0x03), d32(0x0F), d32(0xF1), d32(0xF7)]) == [(3, 1.0)]
    assert v.transform([d32(0x03), d32(0x0F)]) == []


def test_score_known_answers():
    assert R.score([(7, 1.0)], [(7, 1.0)]) == 1.0   # (|0| - 1) - 1 = -2; 2 / 2
    z = R.score([(1, 0.5), (3, 0.5)], [(2, 0.5), (4, 0.5)])
    assert z == 0.0 and R.bits(z) == 0x8000000000000000   # -(+0.0) / 2
    assert R.bits(R.score([], [(2, 1.0)])) == 0x8000000000000000
    assert R.bits(R.score([], [])) == 0x8000000000000000
    # one common word: (|0.25 - 0.75| - 0.25) - 0.75 = -0.5 -> 0.25
    assert R.score([(1, 0.75), (5, 0.25)], [(5, 0.75), (9, 0.25)]) == 0.25


def test_pl_combination_known_answer():
    # (0.5 * 3 + 0.25 * 1) / 4 = 0.4375; (0.5 * 2 + 0.25 * 6) / 8 = 0.3125
    assert R.combine_pl(0.5, 0.25, (3, 1, 2.0, 6.0)) == 0.75
    assert math.isnan(R.combine_pl(0.5, 0.25, (0, 0, 2.0, 6.0)))   # n_pl = 0: 0 / 0


def test_stdv_known_answer():
    assert R.vector_stdv([1.0, 3.0]) == 1.0 and R.vector_stdv([2.0, 2.0, 2.0]) == 0.0
    assert math.isnan(R.vector_stdv([]))


def test_case_families_take_their_paths():
    vs = BC.vocabularies()
    rv = BC.ref_vocab(vs["dup_siblings"])
    ties = 0
    for s in BC.descriptor_sets(vs["dup_siblings"], 3, sizes=(65,), sparse=True):
        for f in s:
            kids = rv.children(0)
            ds = [R.distance(R.as_int(f), rv.desc[c]) for c in kids]
            ties += ds.count(min(ds)) > 1
    assert ties > 10
    assert BC.ref_transform(vs["all_stopped"], BC.descriptor_sets(vs["all_stopped"], 4, sizes=(65,))) == [[]]
    w = vs["shuffled_words"]["word_id"]
    leaves = w[w >= 0]
    assert (np.diff(leaves) < 0).any()   # node order and word order differ


# -------------------------------------------------------------------- C ABI --
NEW_SYMBOLS = ["gfpl_vocab_create", "gfpl_vocab_destroy", "gfpl_vocab_check", "gfpl_bow_transform", "gfpl_bow_score",
               "gfpl_kf_bow_stats", "gfpl_bowdb_create", "gfpl_bowdb_destroy", "gfpl_bowdb_insert", "gfpl_bowdb_erase",
               "gfpl_bowdb_vector", "gfpl_default_lc_search_params", "gfpl_kf_loop_candidates"]


def test_library_and_module_export_the_new_names():
    L = gfpl.hiplib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
    for a in ("Vocabulary", "BowDatabase", "lookForLoopCandidates", "bowStats", "BowStats", "BowVec", "LcSearchParams",
              "LcSearchInfo"):
        assert hasattr(gfpl, a), a
    for m in ("bowTransform", "bowScore"):
        assert hasattr(gfpl.Context, m), m
    for m in ("insertKFBowVectorP", "insertKFBowVectorL", "insertKFBowVectorPL", "erase", "vector", "close"):
        assert hasattr(gfpl.BowDatabase, m), m
    assert hasattr(gfpl.Vocabulary, "from_text") and hasattr(gfpl.Vocabulary, "close")
    assert L.gfpl_abi_version() == 6
    p = gfpl.LcSearchParams.default()
    assert (p.lc_kf_dist, p.lc_kf_max_dist, p.lc_nkf_closest, p.min_lm_cov_graph, p.min_kf_local_map) == (100, 20, 4, 30, 3)
    assert tuple(R.LC_SEARCH_DEFAULTS.values()) == (100, 20, 4, 30, 3)


def _check(v):
    keep = {k: np.ascontiguousarray(v[k]) for k in ("child_off", "child", "desc", "weight", "word_id")}
    d = gfpl.VocabDesc(len(keep["child_off"]) - 1, keep["child_off"].ctypes.data, keep["child"].ctypes.data,
                       keep["desc"].ctypes.data, keep["weight"].ctypes.data, keep["word_id"].ctypes.data,
                       v["weighting"], v["scoring"])
    L = gfpl.hiplib()
    code = L.gfpl_vocab_check(C.byref(d))
    h = C.c_void_p()
    # gfpl_vocab_create applies the same rules before it looks at the context: with a NULL context a
    # refused tree returns its own code, an accepted one GFPL_E_INVALID for the context
    assert L.gfpl_vocab_create(None, C.byref(d), C.byref(h)) == (code if code else -1)
    assert not h.value
    return code


def _edit(v, **kw):
    v = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in v.items()}
    for k, f in kw.items():
        v[k] = f(v[k]) if callable(f) else f
    return v


def _set(i, x):
    def f(a):
        a[i] = x
        return a
    return f


def test_vocab_rules():
    INVALID, UNSUPPORTED = -1, -7
    v = tiny_vocab()
    assert _check(v) == 0
    for name in BC.vocabularies():
        assert _check(BC.vocabularies()[name]) == 0, name
    assert _check(_edit(v, child=_set(3, 7))) == INVALID      # a child index out of range
    assert _check(_edit(v, child=_set(3, -1))) == INVALID
    assert _check(_edit(v, child=_set(3, 3))) == INVALID      # node 3 reachable twice
    assert _check(_edit(v, child=_set(3, 0))) == INVALID      # a cycle through the root
    # a cycle below the root: node 3 gets node 1 as its child
    cyc = _edit(v, child_off=np.array([0, 2, 4, 6, 7, 7, 7, 7], np.int32), child=np.array([1, 2, 3, 4, 5, 6, 1], np.int32))
    assert _check(cyc) == INVALID
    assert _check(_edit(v, word_id=_set(4, -1))) == INVALID   # a leaf without a word
    assert _check(_edit(v, word_id=_set(4, 0))) == INVALID    # word 0 on two leaves
    assert _check(_edit(v, scoring=1)) == UNSUPPORTED         # L2_NORM
    assert _check(_edit(v, weighting=4)) == INVALID
    assert _check(_edit(v, child_off=_set(0, 1))) == INVALID
    wide = BC.tree_vocab(BC.full_tree(33, 1), 1)
    assert _check(wide) == UNSUPPORTED                        # 33 children
    assert _check(BC.tree_vocab(BC.full_tree(32, 1), 1)) == 0
    root_only = dict(child_off=np.array([0, 0, 0], np.int32), child=np.zeros(1, np.int32), desc=np.zeros((2, 32), np.uint8),
                     weight=np.ones(2), word_id=np.array([0, 1], np.int32), weighting=0, scoring=0)
    assert _check(root_only) == INVALID                       # the reference indexes children[0] of the root
    assert gfpl.hiplib().gfpl_vocab_check(None) == INVALID
    # an inner node may carry a word id (the text format's isLeaf flag): it is not read
    assert _check(_edit(v, word_id=_set(1, 0))) == 0


def test_host_calls_refuse_bad_arguments_before_any_device_call():
    L = gfpl.hiplib()
    one = (C.c_int * 1)(1)
    ptrs = (C.c_void_p * 1)()
    assert L.gfpl_bow_transform(None, None, 1, ptrs, one, 1, None, None, one) == -1
    assert L.gfpl_bow_score(None, None, None, 1, None) == -1
    h = C.c_void_p()
    assert L.gfpl_bowdb_create(None, None, None, 0, 4, 4, 4, C.byref(h)) == -1
    assert L.gfpl_bowdb_insert(None, 0, None, None, None) == -1
    assert L.gfpl_bowdb_erase(None, 0) == -1
    assert L.gfpl_bowdb_vector(None, 0, 0, None, None, None) == -1
    assert L.gfpl_vocab_destroy(None) == -1 and L.gfpl_bowdb_destroy(None) == -1


def test_bow_stats_bits():
    rng = np.random.default_rng(5)
    for n_pt, n_ls in ((0, 0), (1, 1), (2, 0), (0, 3), (7, 5), (500, 120)):
        pl = rng.uniform(0, 752, (n_pt, 2))
        spl = rng.uniform(0, 752, (n_ls, 2))
        epl = spl + rng.uniform(-80, 80, (n_ls, 2))
        s = gfpl.bowStats(pl, spl, epl)
        r = R.bow_stats(pl, spl, epl)
        assert (s.n_pt, s.n_ls) == r[:2]
        assert (R.bits(s.std_pt), R.bits(s.std_ls)) == (R.bits(r[2]), R.bits(r[3])), (n_pt, n_ls)
    assert math.isnan(gfpl.bowStats(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2))).std_pt)
    out = gfpl.BowStats()
    assert gfpl.hiplib().gfpl_kf_bow_stats(None, 1, None, None, 0, C.byref(out)) == -1
    assert gfpl.hiplib().gfpl_kf_bow_stats(None, -1, None, None, 0, C.byref(out)) == -1


def _cand_case(n, scores, alive=None, graph=None, **prm):
    conf = np.zeros(n, np.float64)
    for i, s in scores.items():
        conf[i] = s
    alive = np.ones(n, np.uint8) if alive is None else alive
    graph = np.zeros(n, np.int32) if graph is None else graph
    p = dict(lc_kf_dist=5, lc_kf_max_dist=3, lc_nkf_closest=2, min_lm_cov_graph=30, min_kf_local_map=3)
    p.update(prm)
    return conf, alive, graph, n, p


def _both(case):
    conf, alive, graph, n, p = case
    ref = R.look_for_loop_candidates(conf, alive, graph, n, p)
    got = gfpl.lookForLoopCandidates(conf, alive, graph, n, gfpl.LcSearchParams(**p))
    return ref, got


def _same(case):
    ref, got = _both(case)
    assert (got[0], got[1]) == (ref[0], ref[1])
    i = got[2]
    assert (R.bits(i.lc_min_score), i.nkf_closest, i.idx_max, i.n_list) == (
        R.bits(ref[2]["lc_min_score"]), ref[2]["nkf_closest"], ref[2]["idx_max"], ref[2]["n_list"])
    return ref


def test_loop_candidates_against_the_reference():
    recent = {19: 0.3, 18: 0.3, 17: 0.3, 16: 0.3, 15: 0.3}   # kf - i <= 6: the recency arm (14 too, left at 0)
    # too few entries: 3 live entries in i < 20 - 5, the gate wants more than 3
    alive = np.zeros(20, np.uint8)
    alive[[2, 3, 4]] = 1
    alive[15:] = 1
    assert _same(_cand_case(20, {**recent, 2: 0.9, 3: 0.9, 4: 0.9}, alive=alive))[0] is False
    # the top score below lc_min_score
    r = _same(_cand_case(20, {**recent, 5: 0.29, 6: 0.28, 7: 0.27}))
    assert r[0] is False and r[2]["idx_max"] == 5 and r[2]["nkf_closest"] == 0
    # exactly lcNKFClosest - 1, lcNKFClosest and more close keyframes (0.8 * 0.3 = 0.24)
    assert _same(_cand_case(20, {**recent, 6: 0.9, 7: 0.25}))[:2] == (False, -1)
    assert _same(_cand_case(20, {**recent, 6: 0.9, 7: 0.25, 5: 0.24}))[:2] == (True, 6)
    assert _same(_cand_case(20, {**recent, 6: 0.9, 7: 0.25, 5: 0.24, 8: 0.5, 9: 0.6}))[:2] == (True, 6)
    # close in score but farther than lcKFMaxDist from the top
    assert _same(_cand_case(20, {**recent, 6: 0.9, 12: 0.8, 13: 0.8}))[:2] == (False, -1)
    # erased keyframes inside the range: the two that would have made it are gone
    alive = np.ones(20, np.uint8)
    alive[[5, 7]] = 0
    assert _same(_cand_case(20, {**recent, 6: 0.9, 7: 0.25, 5: 0.24}, alive=alive))[:2] == (False, -1)
    # the covisibility arm: keyframe 3 shares 30 landmarks and scores lower than the recent ones
    graph = np.zeros(20, np.int32)
    graph[3] = 30
    r = _same(_cand_case(20, {**recent, 3: 0.05, 6: 0.9, 7: 0.25, 5: 0.24}, graph=graph))
    assert r[2]["lc_min_score"] == 0.05 and r[0] is True
    graph[3] = 29
    assert _same(_cand_case(20, {**recent, 3: 0.05, 6: 0.9, 7: 0.25, 5: 0.24}, graph=graph))[2]["lc_min_score"] == 0.3
    # scores <= 0.001 are ignored by lc_min_score
    r = _same(_cand_case(20, {**recent, 19: 0.001, 18: 0.0, 17: -0.0, 6: 0.9, 7: 0.25, 5: 0.24}))
    assert r[2]["lc_min_score"] == 0.3
    # no qualifying recent score at all: lc_min_score stays 1.0
    assert _same(_cand_case(20, {6: 0.9, 7: 0.95, 5: 0.99}))[2]["lc_min_score"] == 1.0
    # lists longer than 16 (std::sort's insertion-sort threshold) with ties below the top
    big = {i: (0.5 if i % 3 else 0.26) for i in range(40)}
    big.update({45: 0.3, 44: 0.3, 43: 0.3, 42: 0.3, 41: 0.3, 40: 0.3, 20: 0.9})
    assert _same(_cand_case(46, big, lc_kf_max_dist=4, lc_nkf_closest=3))[:2] == (True, 20)
    assert _same(_cand_case(46, big, lc_kf_max_dist=4, lc_nkf_closest=9))[0] is False
    # kf_curr_idx = 0 and lc_kf_dist beyond it
    assert _same(_cand_case(0, {}))[:2] == (False, -1)
    assert _same(_cand_case(4, {0: 0.5, 1: 0.5}))[:2] == (False, -1)


def test_loop_candidates_tied_top():
    """two keyframes share the top score: which one std::sort puts first is the library's; the answer
    must be one of them, with the reference's count for that one"""
    recent = {29: 0.3, 28: 0.3, 27: 0.3, 26: 0.3, 25: 0.3, 24: 0.3}
    sc = {**recent, 4: 0.9, 5: 0.25, 3: 0.25, 2: 0.25, 14: 0.9, 15: 0.25}
    for i in (8, 9, 10, 18, 19, 20, 21, 22, 0, 1):
        sc[i] = 0.1
    case = _cand_case(30, sc, lc_nkf_closest=1)
    conf, alive, graph, n, p = case
    ok, prev, info = gfpl.lookForLoopCandidates(conf, alive, graph, n, gfpl.LcSearchParams(**p))
    assert ok and prev in (4, 14) and info.idx_max == prev
    lst = sorted([(float(i), conf[i]) for i in range(n - 5)], key=lambda a: -a[1])
    top = [k for k, e in enumerate(lst) if int(e[0]) == prev][0]
    full = dict(R.LC_SEARCH_DEFAULTS)
    full.update(p)
    assert info.nkf_closest == R.count_closest(lst, top, info.lc_min_score, full)
    assert R.count_closest(lst, 0, 0.3, full) != R.count_closest(lst, 1, 0.3, full)   # the two tops differ


def test_loop_candidates_refuses_negative_parameters():
    conf, alive, graph, n, p = _cand_case(20, {})
    for k in p:
        q = dict(p)
        q[k] = -1
        with pytest.raises(gfpl.GfplError):
            gfpl.lookForLoopCandidates(conf, alive, graph, n, gfpl.LcSearchParams(**q))
    prev = C.c_int(0)
    prm = gfpl.LcSearchParams.default()
    assert gfpl.hiplib().gfpl_kf_loop_candidates(None, None, None, 3, C.byref(prm), C.byref(prev), None) == -1
    assert gfpl.hiplib().gfpl_kf_loop_candidates(None, None, None, -1, C.byref(prm), C.byref(prev), None) == -1


def test_from_text_round_trip(tmp_path):
    v = tiny_vocab()
    # loadFromTextFile's order: a node's line follows its parent's; ids count up from 1 in file order
    lines = ["2 2 0 0"]
    parent = {1: 0, 2: 0, 3: 1, 4: 1, 5: 2, 6: 2}
    for i in range(1, 7):
        leaf = 1 if v["word_id"][i] >= 0 else 0
        lines.append(" ".join([str(parent[i]), str(leaf)] + [str(int(b)) for b in v["desc"][i]] + [repr(float(v["weight"][i]))]))
    p = tmp_path / "voc.txt"
    p.write_text("\n".join(lines) + "\n\n")   # a trailing blank line
    got = gfpl.Vocabulary.parse_text(str(p))
    for k in ("child_off", "child", "desc", "weight", "word_id"):
        np.testing.assert_array_equal(got[k], v[k], err_msg=k)
    assert (got["weighting"], got["scoring"]) == (0, 0)
    assert _check(got) == 0
    # without a device the constructor gets as far as the context
    with pytest.raises(gfpl.GfplError) as e:
        gfpl.Vocabulary.from_text(None, str(p))
    assert e.value.args and "-1" in str(e.value) or getattr(e.value, "code", -1) == -1
    # word ids count over the leaves in file order, children keep file order
    lines2 = ["3 1 0 0"] + [" ".join(["0", "1"] + ["9"] * 32 + ["0.25"]), "", " ".join(["0", "1"] + ["7"] * 32 + ["1.5"])]
    p.write_text("\n".join(lines2))
    got = gfpl.Vocabulary.parse_text(str(p))
    assert got["child"].tolist() == [1, 2] and got["word_id"].tolist() == [-1, 0, 1] and got["weight"].tolist() == [0, 0.25, 1.5]
