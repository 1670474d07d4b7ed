"""The numpy statement of the line matching stage (line_match_cases.py) on its own and against the oracle.

The GPU legs (test_line_match_gpu.py) compare k_stereo_lines / k_cross_lines with that statement on
hand-made descriptor sets; here the statement is pinned from three sides without a GPU: hand-checkable
answers on tiny sets, the C++ oracle's initialize / stereoLines / crossFrameMatchingLines on every
family and size (which also proves the keyline geometry lets every accepted pair through the
triangulation gates), and altered rules — one per fault of knn2_mfma the families aim at — that must
change an accepted list somewhere, or the families would not notice that fault in the kernel.
"""
import numpy as np
import pytest

import gfpl
import oracle as O
import line_match_cases as L

KP = 64


def _rows(*rows):
    return np.array(rows, np.uint8)


def _row(bits=(), fill=0x00):
    r = np.full(32, fill, np.uint8)
    for b in bits:
        r[b >> 3] ^= np.uint8(1 << (b & 7))
    return r


def test_reference_known_answers():
    Z, F = _row(), _row(fill=0xFF)
    # distances at both ends of the range
    assert L.distances(_rows(Z), _rows(F), 1).tolist() == [[256]]
    assert L.distances(_rows(Z), _rows(F), 2).tolist() == [[128]]
    assert L.distances(_rows(Z, F), _rows(Z, F), 1).tolist() == [[0, 256], [256, 0]]
    # one cell = two bits: 01, 10 and 11 each differ from 00 by one cell, and by 1, 1, 2 bits
    q = _rows(_row([0]), _row([1]), _row([0, 1]), _row([0, 2]))
    assert L.distances(q, _rows(Z), 1)[:, 0].tolist() == [1, 1, 2, 2]
    assert L.distances(q, _rows(Z), 2)[:, 0].tolist() == [1, 1, 1, 2]

    # a reverse tie: queries 0 and 1 identical, one bit from train 0; query 2 is train 1.
    # lr = [0, 0, 1], d0 = [1, 1, 0], d1 = [255, 255, 256]; rl[0] = 0 (the lower of the tied 0 and 1).
    # deviations sorted [254, 254, 256] -> th = 1.4826 * 254 * 0.1 = 37.66; candidates i < min(3, 2) = 2:
    # 0 is mutual and 254 > th; 1 is not mutual.
    q, t = _rows(_row([7]), _row([7]), F), _rows(Z, F)
    for cell in (1, 2):
        D = L.distances(q, t, cell)
        lr, d0, d1, rl = L.knn(D, q, t, cell)
        assert lr.tolist() == [0, 0, 1] and rl.tolist() == [0, 2]
        assert d0.tolist() == [1, 1, 0] and d1.tolist() == ([255, 255, 256] if cell == 1 else [128, 128, 128])   # (cell 2: the cell of bit 7 differs from 11 as well)
        assert L.stereo_pairs(D, q, t, cell).tolist() == [[0, 0]]
        # the tie to the higher index instead: rl[0] = 1, and 1 < 2 is then the mutual one
        assert L.stereo_pairs(D, q, t, cell, rules=L.Rules(rev_tie_high=True)).tolist() == [[1, 0]]
    # the cross matching walks every query: 2 is mutual too
    assert L.cross_pairs(L.distances(q, t, 1), q, t).tolist() == [[0, 0], [2, 1]]
    # max_num 1: budget = sorted d0 [0, 1, 1][0] = 0, so queries 0 and 1 (d0 = 1 > 1.2 * 0) are skipped
    assert L.cross_pairs(L.distances(q, t, 1), q, t, max_num=1).tolist() == [[2, 1]]
    # max_num 2: budget = sorted d0 [0, 1, 1, 2][1] = 1: a query 3 at d0 = 2 > 1.2 is skipped, the list ends at 2
    q4 = _rows(_row([7]), _row([7]), F, _row([8, 9], fill=0xFF))
    assert L.cross_pairs(L.distances(q4, t, 1), q4, t, max_num=2).tolist() == [[0, 0], [2, 1]]

    # a near tie: query 1 is train 0 itself, query 0 one bit away -> rl[0] = 1, and 1 < min(2, 2)
    q, t = _rows(_row([7]), Z), _rows(Z, F)
    assert L.stereo_pairs(L.distances(q, t, 1), q, t, 1).tolist() == [[1, 0]]

    # a forward duplicate: trains 0 and 2 identical, query 0 their exact copy: lr = 0, d1 - d0 = 0 -> rejected
    q, t = _rows(Z, F), _rows(Z, F, Z)
    D = L.distances(q, t, 1)
    lr, d0, d1, rl = L.knn(D, q, t, 1)
    assert lr.tolist() == [0, 1] and d0.tolist() == [0, 0] and d1.tolist() == [0, 256]
    assert L.stereo_pairs(D, q, t, 1).tolist() == [[1, 1]]        # th = 1.4826 * 256 * 0.1 (element 1 of [0, 256])
    # ... accepted with the lower index once the threshold is negative
    assert L.stereo_pairs(D, q, t, 1, desc_th_l=-1.0).tolist() == [[0, 0], [1, 1]]
    assert L.stereo_pairs(D, q, t, 1, desc_th_l=-1.0, rules=L.Rules(fwd_tie_high=True)).tolist() == [[0, 2], [1, 1]]

    # all rows equal: every distance 0, th = 0, 0 > 0 fails
    q = t = _rows(F, F, F)
    assert L.stereo_pairs(L.distances(q, t, 2), q, t, 2).tolist() == []
    assert L.cross_pairs(L.distances(q, t, 1), q, t).tolist() == []
    # fewer than two rows on a side: empty
    assert len(L.stereo_pairs(L.distances(q[:1], t, 1), q[:1], t, 1)) == 0
    assert len(L.cross_pairs(L.distances(q, t[:1], 1), q, t[:1])) == 0


def test_families_plant_what_they_claim():
    """What each family plants shows in the reference at every grid size."""
    for c in L.grid_cases("reverse_ties"):
        for cell in (1, 2):
            p = {tuple(x) for x in c.stereo(cell).tolist()}
            for a, b, T in c.facts["ties"]:
                assert c.D(cell)[a, T] == 16 and c.D(cell)[b, T] == 16
                assert (b, T) not in p, c.what()
                if a < min(c.nl, c.nr):
                    assert (a, T) in p, c.what()
    for c in L.grid_cases("reverse_near_ties"):
        for cell in (1, 2):
            p = {tuple(x) for x in c.stereo(cell).tolist()}
            for a, b, T in c.facts["ties"]:
                assert c.D(cell)[a, T] == 16 and c.D(cell)[b, T] == 15
                assert (a, T) not in p, c.what()
                if b < min(c.nl, c.nr):
                    assert (b, T) in p, c.what()
    for c in L.grid_cases("forward_dups"):
        assert c.facts["dups"]
        for lists in (c.stereo(1), c.stereo(2), c.cross()):
            p = {tuple(x) for x in lists.tolist()}
            for k, lo, hi in c.facts["dups"]:
                assert c.D(1)[k, lo] == 0 and c.D(1)[k, hi] == 0
                assert (k, lo) not in p and (k, hi) not in p, c.what()
    for c in L.grid_cases("forward_dups_open"):     # the same sets with the nn12 test open: the lower index
        p = {tuple(x) for x in c.cross().tolist()}
        for k, lo, hi in c.facts["dups"]:
            if c.nl > 2 and c.nr > 2:               # (two rows a side: the median deviation, and so the threshold, is 0)
                assert (k, lo) in p and (k, hi) not in p, c.what()
    for c in L.grid_cases("extremes"):
        i0, j0, blk = c.facts["extremes"]
        assert (c.D(1)[i0:i0 + blk, j0:] == 256).all() and (c.D(2)[i0:i0 + blk, j0:] == 128).all()
    for c in L.grid_cases("zero_rows"):
        if "zero" in c.facts:
            za, zb, tz = c.facts["zero"]
            assert c.D(2)[za, tz] == 0 and c.D(1)[zb, tz] == 0
            assert [za, tz] in c.stereo(2).tolist() and [zb, tz] not in c.stereo(2).tolist(), c.what()
        else:
            i, s = c.facts["sparse"]
            assert c.D(1)[i, s] == 16 and [i, s] in c.cross().tolist(), c.what()
    for c in L.grid_cases("all_equal"):
        assert len(c.stereo(1)) == 0 and len(c.stereo(2)) == 0 and len(c.cross()) == 0
    for c in L.grid_cases("edge_bytes"):
        x = c.q ^ c.q[0]
        assert not x[:, 4:28].any() and not (c.t ^ c.q[0])[:, 4:28].any()
    for fam in ("planted", "edge_bytes"):           # the accepted lists are long: most rows are mutual matches
        assert all(len(c.stereo(2)) >= min(c.nl, c.nr) * 3 // 4 for c in L.grid_cases(fam) if c.nl > 2 and c.nr > 2)
    for c in L.match_cap_cases():
        assert len(c.cross()) == 300 and len(c.cross(max_num=1000)) > 300
        over = set(c.facts["far"].tolist())
        assert over and not over & set(c.cross()[:, 0].tolist())
    for c in L.large_cases():
        assert c.stereo(1)[:, 1].max() > 1024 and len(c.cross()) == 300


def test_families_are_sensitive():
    """Each altered rule — the fault it stands for in knn2_mfma is named in line_match_cases.Rules —
    changes an accepted list of at least one family at at least one grid size, and the family built
    for that fault is among those that notice."""
    aimed = {"rev_tie_high": "reverse_ties", "fwd_tie_high": "forward_dups_open", "pad_trains": "zero_rows",
             "pad_queries": "zero_rows", "pad_dist0": "planted", "drop_last": "planted", "ge": "all_equal"}
    for name, rules in L.ALTERATIONS.items():
        hits = {}
        for fam in L.FAMILIES:
            for c in L.grid_cases(fam):
                n = sum(not np.array_equal(c.stereo(cell), c.stereo(cell, rules)) for cell in (1, 2))
                n += not np.array_equal(c.cross(), c.cross(rules))
                if n:
                    hits.setdefault(fam, []).append((c.nl, c.nr))
        assert hits, f"no family notices the alteration {name}"
        assert aimed[name] in hits, f"{aimed[name]} does not notice {name}; noticed by {sorted(hits)}"


@pytest.fixture(scope="module")
def cam():
    return gfpl.make_camera("vga", gfpl.default_config())


def _oracle_batch(cam, H, cases, cap):
    """initialize (cell 1), stereoLines (cell 2) and crossFrameMatchingLines of the oracle on one case
    per sequence, against the numpy statement."""
    bad = []
    fr = H.frames(0)
    for b, c in enumerate(cases):
        cfg = gfpl.default_config(**L.CFG_OVER.get(c.family, {}))
        o = O.OracleHandler(cam, cfg, KP, cap)
        o.initialize(fr, b)
        bad += L.check_stereo(o.read_frame(gfpl.PREV), c, 1, True, cap)
        o.begin_frame(fr, b)
        o.stereoLines()
        bad += L.check_stereo(o.read_frame(gfpl.CURR), c, 2, False, cap)
        bad += _oracle_cross(cam, cfg, c, cap)
    return bad


def _oracle_cross(cam, cfg, c, cap):
    o = O.OracleHandler(cam, cfg, KP, cap)
    P, C = L.cross_frames(c, KP, cap)
    o.write_frame(gfpl.PREV, P)
    o.write_frame(gfpl.CURR, C)
    o.crossFrameMatchingLines()
    return L.check_cross(o.read_frame(gfpl.PREV), o.read_frame(gfpl.CURR), o.read_track(), c)


def test_reference_vs_oracle(cam):
    """Every family x the size grid, and the large / odd-capacity / match-cap cases: the pairs the oracle
    emits equal the numpy statement's, as integers.  For the stereo stages this is also the proof that
    the keyline geometry drops no pair in triangulate, in either mode."""
    bad = []
    H = L.host_frames(cam, len(L.GRID_PAIRS), L.KL_CAP, KP)
    for fam in L.FAMILIES:
        L.fill_frames(H, 0, L.grid_cases(fam))
        bad += _oracle_batch(cam, H, L.grid_cases(fam), L.KL_CAP)
    for cases, cap in ((L.large_cases(), 2048), (L.odd_cases(), L.ODD_CAP)):
        H = L.host_frames(cam, len(cases), cap, KP)
        L.fill_frames(H, 0, cases)
        bad += _oracle_batch(cam, H, cases, cap)
    for c in L.match_cap_cases():
        bad += _oracle_cross(cam, gfpl.default_config(), c, L.MATCH_CAP_KL)
    assert not bad, "\n".join(bad[:30])
