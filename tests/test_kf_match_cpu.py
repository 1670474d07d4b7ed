"""The keyframe match consumers' written cases (kf_match_cases.py) without a GPU: the numpy statement against the
oracle restatement of MapHandler::lookForCommonMatches (src/mapHandler.cpp:199-772), hand-checked answers, the
margin every rounding-dependent decision keeps from its threshold, the construction of the threshold cases, and
the proof that each family notices the kernel fault it is aimed at.

Bar: pairs, counts and order are integer results, compared exactly.
"""
import math

import numpy as np
import pytest

import oracle as O
import kf_match_cases as K


def _named(family, name, stage=None):
    got = [c for c in K.cases(family) if c.name == name and (stage is None or c.stage == stage)]
    assert got, (family, name, stage)
    return got[0]


def _pairs(rows):
    return np.array([(r, r) if isinstance(r, int) else r for r in rows], np.int32).reshape(-1, 2)


@pytest.mark.parametrize("family", list(K.FAMILIES))
def test_statement_equals_oracle(family):
    for c in K.cases(family):
        assert c.statement == (c.family != "wild"), c.what()      # no case is left out: only wild inputs are
        if not c.statement:                                        # the oracle's alone
            continue
        r, (op, ol) = c.expected(), c.oracle(O)
        np.testing.assert_array_equal(r.pp, op, err_msg=c.what())
        np.testing.assert_array_equal(r.lp, ol, err_msg=c.what())


def test_margins():
    """Every geometric decision of a statement-checked case is exact by construction (Case.exact: the threshold
    families) or at least 1e-9 (relative) from its threshold, so no association of the arithmetic decides it.
    No case is exempt otherwise: the share left out is 0."""
    checked = 0
    for c in K.cases():
        if c.statement and not c.exact:
            m = c.expected().margin
            assert m >= 1e-9, (c.what(), m)
            checked += 1
    assert {c.family for c in K.cases() if c.exact} == {"chi", "epip", "border"}
    assert checked == sum(c.statement for c in K.cases()) - sum(c.exact for c in K.cases()) and checked > 100


def test_known_answers():
    ratio = {"9/10@default": [0], "45/50@default": [0], "91/100@default": [], "0/7@default": [0], "0/0@default": [],
             "4/5@r08": [], "8/10@r08": [], "100/125@r08": [], "79/99@r08": [0],      # float32 0.8 > double 0.8
             "5/10@r05": [0], "64/128@r05": [0], "51/100@r05": []}
    assert set(ratio) == {c.name for c in K.cases("ratio") if "@" in c.name and "groups" not in c.name}
    for name, rows in ratio.items():
        for stage in ("common", "map"):
            np.testing.assert_array_equal(_named("ratio", name, stage).expected().pp, _pairs(rows), err_msg=name)
    assert float(np.float32(4) / np.float32(5)) > 0.8 and float(np.float32(100) / np.float32(125)) > 0.8 and 4 / 5 <= 0.8
    c = _named("ratio", "groups@default")
    left = set(c.expected().pp[:, 0].tolist())
    r = c.facts["rows"]
    assert {r[9, 10], r[45, 50], r[0, 7]} <= left and not {r[46, 50], r[10, 10]} & left
    c = _named("ratio", "groups@r08")
    left, r = set(c.expected().pp[:, 0].tolist()), c.facts["rows"]
    assert {r[7, 9], r[39, 50]} <= left and not {r[4, 5], r[8, 10]} & left
    # MAD: kf0 row i has its neighbours at kf1 rows 2 i and 2 i + 1
    mad = {"zero": [4, 5, 6],             # median 0, threshold 0: difference 0 rejected, 1 accepted
           "even": [3, 4, 5], "odd": [3, 4, 5, 6], "two": [1],
           "m20": [2, 3, 4, 5, 6],        # threshold 2.9652: 2 rejected, 3 accepted
           "m20even": [1, 2, 3, 4, 5, 6, 7], "filtered": [1, 2, 3]}
    for name, rows in mad.items():
        for c in [c for c in K.cases("mad") if c.name == name]:
            np.testing.assert_array_equal(c.expected().lp, _pairs([(i, 2 * i) for i in rows]), err_msg=c.what())
    assert 2.0 < (1.4826 * 20.0) * 0.1 < 3.0 and abs((1.4826 * 20.0) * 0.1 - 2.9652) < 1e-12
    for stage in ("common", "map"):
        np.testing.assert_array_equal(_named("mad", "d256", stage).expected().lp, _pairs([0, 1]))
    # filter borders: 0, width and height are out; the smallest positive double and nextafter(width, 0) are in
    c = _named("border", "exact")
    np.testing.assert_array_equal(c.expected().pp, _pairs([0, 1, 6, 10]))
    np.testing.assert_array_equal(c.expected().lp, _pairs([0, 1, 7]))
    c = _named("border", "corner")
    np.testing.assert_array_equal(c.expected().pp, _pairs([0, 1, 2, 3, 4, 5, 10]))
    np.testing.assert_array_equal(c.expected().lp, _pairs([0, 1, 2, 3]))
    for c in K.cases("border"):
        r = c.expected()
        assert r.pp[:, 0].tolist() == c.facts["pt"] and r.lp[:, 0].tolist() == c.facts["ls"], c.what()
    for k, n in (("keep0first", 0), ("keep1first", 0), ("keep1last", 0), ("keep2first", 2), ("keep2last", 2)):
        r = _named("border", k).expected()
        assert len(r.pp) == n and len(r.lp) == n
    np.testing.assert_array_equal(_named("border", "keep2last").expected().pp, _pairs([6, 7]))
    np.testing.assert_array_equal(_named("epip", "signed").expected().lp, _pairs([0, 2, 3]))
    # ties: the lower of two equally near kf0 rows is the mutual one; duplicates and 0 / 0 are rejected
    for c in [c for c in K.cases("ties") if c.name in ("small", "big")]:
        f, r = c.facts["pt"], c.expected()
        pp, left = set(map(tuple, r.pp.tolist())), set(r.pp[:, 0].tolist())
        for t, qs in f["first21"] + f["dup_q"]:
            assert (qs[0], t) in pp and qs[1] not in left, c.what()
        assert sorted(qs[0] for _, qs in f["first21"]) == [3, 31] + ([1023] if c.name == "big" else [])
        assert not {q for q, _ in f["first12"]} & left and not set(f["dup_t"]) & left and f["zero"] in left
        t, qs = f["closer"]
        assert (qs[1], t) in pp and qs[0] not in left
        i12, d12 = K.knn2(*c.descs(0))
        for q, ts in f["first12"]:
            assert i12[q].tolist() == ts and d12[q].tolist() == [10.0, 10.0]
        assert sorted(ts[0] for _, ts in f["first12"]) == [3, 31] + ([1023] if c.name == "big" else [])
        (q, ts), (q2, ts2) = f["second12"]
        assert i12[q].tolist() == ts[:2] and i12[q2].tolist() == [ts2[2], ts2[0]]


def test_sizes_turn_over_every_boundary():
    sizes = [c for c in K.cases("sizes") if "x" in c.name]
    for stage in ("common", "map"):
        assert [(c.n0[0], c.k1.n_pt) for c in sizes if c.stage == stage] == K.SIZE_PAIRS
    assert set(K.SIZES) == {2, 3, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 2049}
    for c in sizes:
        r, m = c.expected(), min(c.n0[0], c.k1.n_pt)
        assert len(r.pp) >= 0.7 * m and len(r.lp) >= 0.7 * m, c.what()         # most rows are accepted ...
        if m >= 1026 and c.stage == "common":                                      # ... and rows 1022-1025 alternate
            for p in (r.pp, r.lp):
                assert [x in set(p[:, 0].tolist()) for x in (1022, 1023, 1024, 1025)] == [False, True, False, True]
    for c in K.cases("sizes"):
        if "compacted" in c.name:
            cam, Twf = K.camera(c.cam), K.inverse_se3(c.k1.T)
            pf = K._project(cam, K._se3(Twf, c.a.P))
            assert int(((pf > 0).all(1) & (pf[:, 0] < cam.width) & (pf[:, 1] < cam.height)).sum()) == c.facts["compacted"]
    few = [c for c in K.cases("sizes") if c.family == "few"]
    assert len(few) == 2 * len(K.FEW)
    for c in few:
        r = c.expected()
        assert (len(r.pp) == 0) == (min(c.n0[0], c.k1.n_pt) < 2) and (len(r.lp) == 0) == (min(c.n0[1], c.k1.n_ls) < 2)
    assert {(a + b) % 4 for a, b in K.ALIGN} == {0, 1, 2, 3}       # the local-map scratch: every residue of n_pt + n_ls
    assert (201, 0) in K.ALIGN and (0, 81) in K.ALIGN


def test_threshold_cases_hit_their_thresholds():
    """The chi cases: under the statement's arithmetic the three neighbours give err <, == and > sqrt(7.815); the
    local-map cases: the gate equals the row's own error, or is the next double above it."""
    c = _named("chi", "neighbours")
    r = c.expected()
    for kind, got in (("pt", r.pp), ("ls", r.lp)):
        seen = {}
        for row, (a, b, s2, name, acc) in c.facts[kind].items():
            err = math.sqrt(a * a + b * b) * math.sqrt(s2)
            assert {"below": err < K.CHI, "at": err == K.CHI, "above": err > K.CHI}[name], (kind, row, err)
            assert abs(err - K.CHI) <= 4.5e-16 and acc == (name == "below")
            assert (row in got[:, 0].tolist()) == acc, (kind, row, name)
            seen.setdefault((a, b), set()).add(name)
        assert all(v == {"below", "at", "above"} for v in seen.values())
        assert ((3.0, 0.0) in seen and len(seen) >= 2) if kind == "pt" else len(seen) >= 1, seen
    pt = {(a, b) for a, b, *_ in c.facts["pt"].values()}
    assert (3.0, 4.0) in pt or (4.5, 6.0) in pt       # a two-term square root
    for k, ((ex, ey), l2) in enumerate(K.EPIP):
        at, above = _named("epip", f"at{k}"), _named("epip", f"above{k}")
        e = math.sqrt(ex * ex + ey * ey)
        assert at.ep == (e, 8.0 + l2) and above.ep == (float(np.nextafter(e, 9.0)), float(np.nextafter(8.0 + l2, 9.0)))
        for case, acc in ((at, False), (above, True)):
            r = case.expected()
            assert (1 in r.pp[:, 0].tolist()) == acc and (1 in r.lp[:, 0].tolist()) == acc
            assert {0, 2, 3, 4} <= set(r.pp[:, 0].tolist()) and {0, 2, 3, 4} <= set(r.lp[:, 0].tolist())


# alteration -> the case aimed at it: (family, name, stage); "knn": noticed in the knn-2 answer itself
AIMED = {"knn_tie_high": ("ties", "small", "common"), "second_tie_high": ("ties", "small", "knn"),
         "no_mutual": ("ties", "small", "map"), "ratio_lt": ("ratio", "5/10@r05", "common"),
         "ratio_double_div": ("ratio", "100/125@r08", "common"), "mad_median_lo": ("mad", "even", "common"),
         "mad_ge": ("mad", "zero", "map"), "mad_over_all_rows": ("mad", "filtered", "map"),
         "chi_le": ("chi", "neighbours", "common"), "sigma_not_sqrt": ("chi", "neighbours", "common"),
         "epip_le": ("epip", "at0", "map"), "line_abs": ("epip", "signed", "map"),
         "border_incl_lo": ("border", "exact", "map"), "border_incl_hi": ("border", "corner", "map"),
         "no_z_test": ("border", "exact", "map"), "one_endpoint": ("border", "exact", "map"),
         "pair_compact_row": ("sizes", "33x33", "map"), "chunk_offset": ("sizes", "1025x1025", "common"),
         "unordered": ("sizes", "2x2", "common")}


def _differs(c, rules, knn=False):
    if knn:
        return any(not np.array_equal(a, b) for lines in (0, 1) for q, t in (c.descs(lines), c.descs(lines)[::-1])
                   for a, b in zip(K.knn2(q, t), K.knn2(q, t, rules)))
    a, b = c.expected(), c.expected(rules)
    return not (np.array_equal(a.pp, b.pp) and np.array_equal(a.lp, b.lp))


def test_families_are_sensitive():
    """Each altered rule — the kernel fault it stands for is named in kf_match_cases.Rules — changes the statement's
    answer on the case built for that fault; the other small cases that notice it are counted too."""
    assert set(AIMED) == set(K.ALTERATIONS)
    small = [c for c in K.cases() if c.statement and max(c.n0 + (c.k1.n_pt, c.k1.n_ls)) <= 200]
    for name, rules in K.ALTERATIONS.items():
        family, case, stage = AIMED[name]
        c = _named(family, case, "common" if stage == "knn" else stage)
        assert _differs(c, rules, stage == "knn"), f"{c.what()} does not notice {name}"
        hits = {x.family for x in small if _differs(x, rules)}
        assert stage == "knn" or family in hits or family == "sizes", (name, sorted(hits))
    # the second neighbour's row never reaches a pair: only the knn answer shows it
    assert not any(_differs(x, K.ALTERATIONS["second_tie_high"]) for x in small)
    # the later chunks: both stages and both kinds notice a chunk offset
    for stage in ("common", "map"):
        a, b = (_named("sizes", "2049x2049", stage).expected(r) for r in (K.EXACT, K.ALTERATIONS["chunk_offset"]))
        assert len(b.pp) < len(a.pp) and len(b.lp) < len(a.lp)
