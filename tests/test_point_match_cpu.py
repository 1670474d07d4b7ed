"""The numpy statement of the point matching stages (point_match_cases.py) on its own and against the oracle.

The GPU legs (test_point_match_gpu.py) compare k_stereo_points, k_init_points (behind the batched knn-2)
and k_cross_points with that statement on hand-made keypoints, descriptors and pyramids; here the
statement is pinned from three sides without a GPU: hand-checkable answers on tiny sets, the C++ oracle's
initialize / stereoPoints / crossFrameMatchingPoints on every family and size, bit for bit, and altered
rules — one per kernel fault the families aim at — that must change an output somewhere, or the families
would not notice that fault in the kernel.
"""
import numpy as np
import pytest

import gfpl
import oracle as O
import point_match_cases as M
from line_match_cases import distances

KL = 32


def _kp(*rows):
    return np.array(list(rows), gfpl.KEYPOINT_DT).reshape(-1)


def _desc(*bitsets):
    out = np.zeros((len(bitsets), 32), np.uint8)
    for r, bits in enumerate(bitsets):
        for b in bits:
            out[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def test_statement_known_answers():
    ct = M.camera("vga")
    assert M.roundf(np.float32([0.5, 2.5, -0.5, 1.4999999, -2.5])).tolist() == [1.0, 3.0, -1.0, 1.0, -3.0]
    rng = np.random.default_rng(0)
    q, t = rng.integers(0, 256, (5, 32), dtype=np.uint8), rng.integers(0, 256, (7, 32), dtype=np.uint8)
    assert np.array_equal(M.hamming(q, t), distances(q, t, 1))

    # --- SAD: vertical lines of 100 every 16 columns on black, level 0.  The left window at uL = 32 has
    # the line in its centre column: IL = -100 in ten columns, 0 in the centre.  A right window centred
    # on a line is the same (SAD 0); one that holds a line off centre differs by 200 in that column and
    # by 100 in nine others (1100 a row, 12100); one that holds no line by 100 in ten columns (11000).
    pyr = np.zeros(ct.pyr_bytes, np.uint8)
    ct.level(pyr, 0)[:, ::16] = 100
    # uR = 14: uR + s is on the line 16 at s = 2; s = -5, -4 put the centre at 9, 10: no line within +-5
    want = [11000, 11000, 12100, 12100, 12100, 12100, 12100, 0, 12100, 12100, 12100]
    assert M.sad_vector(ct, pyr, 0, 50, 32, 14).tolist() == want
    assert M.sad_vector(ct, pyr, 0, 50, 32, 14, M.Rules(row_twice=True)).tolist() == [v * 12 // 11 for v in want]
    kl, kr = _kp((32.0, 50.0, 0)), _kp((14.0, 50.0, 0))
    disp, det = M.sub_pixel(ct, pyr, kl[0], kr[0])
    assert det["inc"] == 2 and det["delta"] == 0 and disp == np.float32(16.0)     # 32 - 1 * (14 + 2 + 0)
    # the minimum at the last shift is no minimum: uR = 11 puts the line at s = 5
    assert M.sub_pixel(ct, pyr, kl[0], _kp((11.0, 50.0, 0))[0])[0] is None
    # window validity: uR - 10 >= 0, uR + 11 < cols, uL + 5 < cols, vL - 5 >= 0, vL + 5 < rows
    for xl, y, xr, ok in ((32, 50, 10, True), (32, 50, 9, False), (634, 50, 628, True), (635, 50, 628, False),
                          (634, 50, 629, False), (32, 5, 14, True), (32, 4, 14, False), (32, 474, 14, True),
                          (32, 475, 14, False)):
        got = M.sub_pixel(ct, pyr, _kp((xl, y, 0))[0], _kp((xr, y, 0))[0])[1]
        assert ("sad" in got) == ok, (xl, y, xr)

    # --- the band scan and the emission on that pyramid.  Right 0 and 1 carry the same descriptor, three
    # bits from left 0; right 2 is left 1's own.  Level 0: r = 2, so right y = 50.5 covers the rows 48..53.
    dl = _desc((), (200,))
    dr = _desc((0, 1, 2), (0, 1, 2), (200,))
    kr = _kp((46.0, 50.5, 0), (30.0, 50.5, 0), (110.0, 50.5, 2))
    mbf = np.float32(ct.cam.fx * ct.cam.b)
    for y, n in ((47.99, 0), (48.0, 1), (53.999, 1), (54.0, 0)):
        out = M.stereo_points(_kp((64.0, y, 0)), kr, dl[:1], dr, pyr, ct)
        assert len(out.rows) == n and out.n_subpix == n, y
    out = M.stereo_points(_kp((64.0, 50.0, 0), (128.0, 51.0, 0)), kr, dl, dr, pyr, ct)
    # left 0: the tie of right 0 and 1 at distance 3 goes to right 0 -> disparity 16; left 1 at level 0 does
    # not see right 2 (octave 2) and takes right 0 at distance 4: uL - uR = 82 = 16 * 5 + 2 -> disparity 80
    # (left 0: 64 - 46 = 16 + 2; right 1 at 30 is 32 + 2 away)
    assert [(i, lv) for i, _, lv in out.rows] == [(0, 0), (1, 0)] and out.n_subpix == 2
    assert [d for _, d, _ in out.rows] == [mbf / (mbf / np.float32(16.0)), mbf / (mbf / np.float32(80.0))]
    assert out.detail[0]["iR"] == 0 and out.detail[0]["dist"] == 3 and out.detail[1]["dist"] == 4
    high = M.stereo_points(_kp((64.0, 50.0, 0)), kr, dl[:1], dr, pyr, ct, M.Rules(ham_tie_high=True))
    assert high.detail[0]["iR"] == 1 and high.rows[0][1] == mbf / (mbf / np.float32(32.0))
    # at level 1 left 1 sees right 2 at distance 0 -> median element 1 of [(0, 1), (3, 0)] is 3, thDist 6.3: both
    out = M.stereo_points(_kp((64.0, 50.0, 0), (128.0, 51.0, 1)), kr, dl, dr, pyr, ct)
    assert out.detail[1]["iR"] == 2 and out.detail[1]["dist"] == 0
    # one match at distance 0: the median is 0 and nothing is below 0
    assert M.stereo_points(_kp((128.0, 51.0, 1)), kr, dl[1:], dr, pyr, ct).rows == []

    # --- the initial frame: left 0 / right 1 mutual at 1 against 3 (ratio 1/3); left 1 is nearest to right 1 as
    # well (distance 2) and not mutual; left 2 / right 2 mutual at 0 against 4 but 3 rows apart
    cfg = gfpl.default_config()
    dl = _desc((0,), (0, 1, 2), (100, 101, 102, 103))
    dr = _desc((0, 1, 2, 3), (0, 1), (100, 101, 102, 103))
    kl = _kp((100.0, 10.0, 0), (110.0, 10.0, 0), (120.0, 10.0, 0))
    kr = _kp((5.0, 10.0, 0), (99.0, 12.0, 0), (60.0, 13.0, 0))
    # D = [[3, 1, 5], [1, 1, 7], [8, 6, 0]]: lr = [1, 0, 2], rl = [1, 0, 2]: left 0 -> right 1 -> left 0 (tie of
    # lefts 0 and 1 at distance 1 goes to 0); left 1 -> right 0 (tie of rights 0, 1 goes to 0) -> left 1, ratio 1/1
    assert M.hamming(dl, dr).tolist() == [[3, 1, 5], [1, 1, 7], [8, 6, 0]]
    assert M.init_points(kl, kr, dl, dr, cfg) == [(0, 1)]
    assert M.init_points(kl, kr, dl, dr, cfg, M.Rules(epip_lt=True)) == []          # |dy| = 2.0
    assert M.init_points(kl, kr, dl, dr, cfg, M.Rules(disp_gt=True)) == []          # 100 - 99 = 1.0
    kr["y"][2] = 12.0
    assert M.init_points(kl, kr, dl, dr, cfg) == [(0, 1), (2, 2)]                   # 0 / 6 passes
    assert M.init_points(kl[:1], kr, dl[:1], dr, cfg) == []                         # fewer than two rows

    # --- cross: previous 0 and 1 project to (cx, cy) and (cx + 1, cy), same descriptor; current 0 is 10 px
    # from the first and 9 from the second, at Hamming distance 2; current 1 sits on previous 0
    P = np.array([[0.0, 0.0, 5.0], [1.0, 0.0, ct.fx]])
    dp, dc = _desc((), ()), _desc((3, 4), (7,))
    pl = np.array([[ct.cx + 10.0, ct.cy], [ct.cx, ct.cy]])
    out = M.cross_points(P, pl, dp, dc, cfg, ct)
    assert out.pairs == [(0, 0), (1, 0)] and out.obs_t.tolist() == [1, -1]
    assert M.cross_points(P, pl, dp, dc, cfg, ct, M.Rules(gate_ge=True)).pairs == [(0, 1), (1, 0)]
    assert M.cross_points(P, pl, dp, dc, cfg, ct, M.Rules(cross_tie_high=True)).pairs == [(0, 1), (1, 1)]
    assert M.cross_points(P, pl, dp, dc, cfg, ct, M.Rules(first_t=True)).obs_t.tolist() == [0, -1]
    one = gfpl.default_config(max_point_match_num=1)
    assert M.cross_points(P, pl, dp, dc, one, ct).pairs == [(0, 0)]
    assert M.cross_points(P, pl, dp, dc, one, ct).obs_t.tolist() == [0, -1]
    assert M.cross_points(P, pl, dp, dc, one, ct, M.Rules(beyond_cap=True)).obs_t.tolist() == [1, -1]


def _emitted(c):
    return {r[0] for r in c.stereo().rows}


def _by_family(cases):
    out = {}
    for c in cases:
        out.setdefault(c.family, []).append(c)
    return out


def test_families_plant_what_they_claim():
    """What each family plants shows in the statement."""
    small = _by_family(M.small_cases())
    for c in M.grid_cases() + M.tall_cases("vga8") + M.tall_cases("stress"):
        if c.family.startswith("grid"):
            assert len(c.stereo().rows) >= (c.facts["planted"] + 1) // 2, c.what()
    assert {(c.n, c.nr) for c in M.grid_cases()} == set(M.GRID_PAIRS)
    for cam_name, cases in (("vga", M.small_cases()), ("vga8", M.tall_cases("vga8")), ("stress", M.tall_cases("stress"))):
        ct = M.camera(cam_name)
        fam = _by_family(cases)
        assert len(fam["band_edges"]) == ct.n
        for o, c in enumerate(fam["band_edges"]):
            r = np.float32(2.0) * ct.scale[o]
            rows_in = {int(c.kp_l[i]["y"]) for i in c.facts["in"]}
            for j in range(4):      # every group's minr and maxr are rows of emitted left keypoints, the rows beyond are not
                y = c.kp_r[j]["y"]
                assert int(np.floor(y - r)) in rows_in and int(np.ceil(y + r)) in rows_in
            assert set(c.facts["in"]) == _emitted(c) and not set(c.facts["out"]) & set(c.stereo().detail), c.what()
            assert set(c.facts["edge"]) <= set(c.stereo().detail)           # matched on rows 0 and H - 1 ...
            assert not set(c.facts["outside"]) & set(c.stereo().detail)      # ... and never outside the image
        if cam_name == "vga8":
            h = max(int(np.ceil(k["y"] + 2 * ct.scale[7])) - int(np.floor(k["y"] - 2 * ct.scale[7]))
                    for k in fam["band_edges"][7].kp_r)
            assert h >= 43                                                   # above SP_MINR_PAD = 32
        c, = fam["sad_borders"]
        for name, iL in c.facts["at"]:
            assert iL in _emitted(c), (cam_name, name, c.stereo().detail.get(iL))
        for name, iL in c.facts["beyond"]:
            assert iL in c.stereo().detail and "sad" not in c.stereo().detail[iL], (cam_name, name)
        c, = fam["sad_align"]
        seen = {}
        for iL in c.facts["pairs"]:
            d = c.stereo().detail[iL]
            row0 = ct.off[d["o"]] + (d["vL"] - 5) * ct.cols[d["o"]]
            seen.setdefault(d["o"], set()).add(((row0 + d["uL"] - 5) & 3, (row0 + d["uR"] - 10) & 3))
            assert iL in _emitted(c)
        assert all(len(v) == 16 for v in seen.values()) and len(seen) == (4 if cam_name != "vga8" else 3), seen
    assert M.camera("vga").cols == [640, 533, 444, 370]
    for c in small["chunks"]:
        assert len(_emitted(c)) >= len(c.facts["best"]) // 2, c.what()
        for iL, iR in c.facts["best"]:
            assert c.stereo().detail[iL]["iR"] == iR, c.what()
    assert [int((c.kp_r["y"] == 100).sum()) for c in small["chunks"]] == list(M.CHUNK_RUNS)   # one (octave, minr) bin
    for c in small["octaves"] + _by_family(M.tall_cases("stress"))["octaves"]:
        for iL, iR in c.facts["accept"]:
            assert c.stereo().detail[iL]["iR"] == iR and iL in _emitted(c), c.what()
            assert (c.D()[iL] == 9).sum() >= 3                      # rivals at the same distance, some of them at +-2
        assert not set(c.facts["none"]) & set(c.stereo().detail)
    c, = small["ham"]
    for iL, lo, hi in c.facts["ties"]:
        assert c.D()[iL, lo] == c.D()[iL, hi] == c.D()[iL].min() and c.stereo().detail[iL]["iR"] == lo and iL in _emitted(c)
    assert c.facts["ties"][1][1] == 0 and c.facts["ties"][1][2] == c.nr - 1 and c.facts["ties"][0][1:] == (32, 33)
    for dist, (iL, iR) in c.facts["th"].items():    # (the planted right keypoint is the only one on that row)
        assert c.D()[iL, iR] == dist and (iL in c.stereo().detail) == (dist < 80)
    assert c.facts["th"][79][0] in _emitted(c)
    assert c.facts["alone"] not in c.stereo().detail
    for kind in M.SAD_KINDS:
        c, = small["sad_" + kind]
        for iL, k in c.facts["shift"]:
            d = c.stereo().detail[iL]
            if kind == "flat":
                assert not d["sad"].any() and d["inc"] == -5 and d["disp"] is None
                continue
            zeros = np.nonzero(d["sad"] == 0)[0] - 5
            assert zeros.tolist() == [z for z in ((k - 8, k, k + 8) if kind == "p8" else (k,)) if -5 <= z <= 5], (kind, k)
            assert d["inc"] == zeros[0] and (iL in _emitted(c)) == (abs(zeros[0]) < 5)
        if kind == "bw":      # a per-pixel difference of 510 occurs in both directions: (0 - 255) - (255 - 0) and back
            ct, hit = M.camera("vga"), set()
            for iL, k in c.facts["shift"]:
                d = c.stereo().detail[iL]
                img = ct.level(c.pyr, d["o"]).astype(int)
                IL = img[d["vL"] - 5:d["vL"] + 6, d["uL"] - 5:d["uL"] + 6] - img[d["vL"], d["uL"]]
                for s in range(-5, 6):
                    u = d["uR"] + s
                    hit |= set(np.unique(IL - (img[d["vL"] - 5:d["vL"] + 6, u - 5:u + 6] - img[d["vL"], u])).tolist()) & {-510, 510}
            assert hit == {-510, 510}
    c, = M.disparity_cases()
    f, rows = c.facts, {r[0]: r[1] for r in c.stereo().rows}
    ct = M.camera("vga544")
    zero = ct.mbf / (ct.mbf / np.float32(0.01))
    assert ct.maxD == 544.0 and rows[f["zero_same"]] == zero and rows[f["zero_shift"]] == zero
    assert c.stereo().detail[f["zero_same"]]["disp"] == 0 and c.stereo().detail[f["zero_shift"]]["inc"] == 3
    assert c.stereo().detail[f["at_maxD"]]["disp"] == ct.maxD and f["at_maxD"] not in rows
    assert c.stereo().detail[f["below_maxD"]]["disp"] == np.nextafter(np.float32(544.0), np.float32(0)) and f["below_maxD"] in rows
    assert c.kp_r[f["u_at_lo"]]["x"] == c.kp_l[f["u_at_lo"]]["x"] - ct.maxD and f["u_at_lo"] in rows
    assert f["u_below_lo"] not in c.stereo().detail and f["neg_maxU"] not in c.stereo().detail and f["small"] in rows
    med = {c.family[7:]: c for c in M.small_cases() + M.median_cases() if c.family.startswith("median_")}
    assert set(med) == set(M.MEDIAN_KINDS)
    th = lambda m: np.float32(1.5) * np.float32(1.4) * np.float32(m)
    assert len(med["odd"].stereo().rows) == 3 + 2 * (np.float32(21) < th(10))
    assert len(med["even"].stereo().rows) == 4 + (np.float32(41) < th(20)) + (np.float32(42) < th(20))
    assert len(med["m30"].stereo().rows) == 5 + sum(np.float32(d) < th(30) for d in (62, 63, 64))
    assert len(med["split"].stereo().rows) == 4 and med["zero"].stereo().rows == [] and med["zero"].stereo().n_subpix == 5
    for k in ("equal600", "equal1100"):
        assert [r[0] for r in med[k].stereo().rows] == list(range(med[k].n))
    got = [(med["spread"].facts["dists"][r[0]], r[0]) for r in med["spread"].stereo().rows]
    assert got == sorted(got) and len(got) == 240 and max(np.bincount([g[0] for g in got])) == 5

    for c in M.init_cases():
        got = c.init()
        if "ratio" in c.facts:
            i = c.facts["ratio"]
            lefts = {p[0] for p in got}
            assert {i["9/10"], i["45/50"], i["0/7"]} <= lefts and not {i["0/0"], i["46/50"]} & lefts, c.what()
            assert set(c.facts["epip"]["at"]) <= lefts and not set(c.facts["epip"]["beyond"]) & lefts
            assert c.facts["disp"]["at"] in lefts and c.facts["disp"]["below"] not in lefts
            assert c.facts["tie"][0] in lefts and c.facts["tie"][1] not in lefts
            assert len(got) >= min(c.n, c.nr) - 12
    assert {(c.n, c.nr) for c in M.init_cases()} >= {(0, 5), (1, 7), (2, 2), (2048, 2047)}

    x = {c.family: c for c in M.cross_cases() + M.cross_cfg_cases() if c.family not in ("cross_sizes", "cross_cap1500")}
    c = x["cross_gates"]
    pairs = set(c.cross().pairs)
    assert set(c.facts["gate_in"]) <= pairs and not {t for t, _ in c.facts["gate_out"]} & {t for t, _ in pairs}
    for t, lo, hi in c.facts["tie"]:
        assert (t, lo) in pairs and c._D[lo, t] == c._D[hi, t]
    q, ts = c.facts["multi"]
    assert all((t, q) in pairs for t in ts) and c.cross().obs_t[q] == ts[-1]
    c = x["cross_cells"]
    assert set((t, q) for q, t in c.facts["match"]) == set(c.cross().pairs) and len(c.facts["slow"]) == 3 and c.facts["cs"] == 16
    assert min(abs(c.pl[t][0]) for t in c.facts["slow"]) < 1e6 + 1
    assert {(q, t) for q, t in c.facts["match"] if 999990 < abs(c.pl[t][0]) < 1e6}
    assert [t for t, _ in x["cross_radius"].cross().pairs] == x["cross_radius"].facts["in"]
    assert x["cross_one_cell"].cross().n_found > 500 and len(x["cross_sparse"].cross().pairs) == 40
    sizes = [c for c in M.cross_cases() if c.family == "cross_sizes"]
    assert {(c.sp, c.sc) for c in sizes} == set(M.CROSS_SIZES)
    for c in sizes:
        w = c.cross()
        assert w.n_found >= c.facts["planted"] * 9 // 10 and len(w.pairs) == min(w.n_found, 500), c.what()
    big = [c for c in sizes if c.sc == 2048 and c.sp == 2048][0].cross()
    assert big.pairs[-1][0] < 1024                                            # the cap falls inside the first round
    caps = [c.cross() for c in M.cross_cfg_cases() if c.family == "cross_cap1500"]
    assert len(caps[0].pairs) == 1500 and caps[0].n_found > 1500 and caps[0].pairs[-1][0] >= 1024   # ... the second
    assert 1024 < len(caps[1].pairs) < 1500


def _small_cross():
    return [c for c in M.cross_cases() + M.cross_cfg_cases() if c.statement and c.sp * c.sc <= 1100000]


def test_families_are_sensitive():
    """Each altered rule — the kernel fault it stands for is named in point_match_cases.Rules — changes the
    statement's output on at least one case, and the family built for that fault is among those that notice."""
    aimed = {"ham_tie_high": "ham", "band_excl_min": "band_edges", "band_excl_max": "band_edges",
             "oct_gate0": "octaves", "oct_gate2": "octaves", "oct_clamped": "octaves", "u_strict_lo": "disparity",
             "u_strict_hi": "disparity", "le80": "ham", "sad_tie_last": "sad_p8", "win_left": "sad_borders",
             "win_right": "sad_borders", "win_top": "sad_borders", "win_bottom": "sad_borders", "row_twice": "sad_p16",
             "median_lo": "median_split", "emit_le": "median_zero", "unstable": "median_even",
             "epip_lt": "init", "disp_gt": "init", "cross_tie_high": "cross_gates", "gate_ge": "cross_gates",
             "radius_lt": "cross_gates", "first_t": "cross_gates", "beyond_cap": "cross_sizes"}
    assert set(aimed) == set(M.ALTERATIONS)
    stereo = M.small_cases() + M.disparity_cases()
    inits = [c for c in M.init_cases() if c.n <= 513]
    for name, rules in M.ALTERATIONS.items():
        hits = set()
        for c in stereo:
            a, b = c.stereo(), c.stereo(rules)
            if a.rows != b.rows:            # (what the GPU legs can read: the emitted rows)
                hits.add(c.family)
        hits |= {c.family for c in inits if c.init() != c.init(rules)}
        for c in _small_cross():
            a, b = c.cross(), c.cross(rules)
            if a.pairs != b.pairs or not np.array_equal(a.obs_t, b.obs_t):
                hits.add(c.family)
        assert hits, f"no family notices the alteration {name}"
        assert aimed[name] in hits, f"{aimed[name]} does not notice {name}; noticed by {sorted(hits)}"


def _oracle_stereo(cam_name, cases, cap):
    ct = M.camera(cam_name)
    H = M.host_frames(cam_name, len(cases), cap, KL)
    M.fill_stereo(H, 0, cases)
    fr = H.frames(0)
    bad = []
    for b, c in enumerate(cases):
        o = O.OracleHandler(ct.cam, M.config(cam_name), cap, KL)
        o.initialize(fr, b)
        o.begin_frame(fr, b)
        o.stereoPoints()
        bad += M.check_stereo(o.read_frame(gfpl.CURR), c)
    return bad


def test_statement_vs_oracle_stereo():
    """begin_frame + stereoPoints of the oracle on every stereo family, size and camera: the rows equal the
    statement's, by index, float32 disparity bits and level."""
    bad = []
    for name, cases in M.STEREO_FAMILIES.items():
        cases = cases()
        bad += _oracle_stereo(cases[0].cam_name, cases, max(64, max(max(c.n, c.nr) for c in cases)))
    assert not bad, "\n".join(bad[:30])


def test_statement_vs_oracle_initial():
    cases = M.init_cases()
    ct = M.camera("vga")
    H = M.host_frames("vga", len(cases), 2048, KL)
    M.fill_init(H, 0, cases)
    fr = H.frames(0)
    bad = []
    for b, c in enumerate(cases):
        o = O.OracleHandler(ct.cam, M.config("vga"), 2048, KL)
        o.initialize(fr, b)
        bad += M.check_init(o.read_frame(gfpl.PREV), c)
    assert not bad, "\n".join(bad[:30])


def oracle_cross(c, cap):
    o = O.OracleHandler(M.camera("vga").cam, c.cfg(), cap, KL)
    P, C = M.cross_frames(c, cap, KL)
    o.write_frame(gfpl.PREV, P)
    o.write_frame(gfpl.CURR, C)
    o.crossFrameMatchingPoints()
    return o.read_frame(gfpl.PREV), o.read_frame(gfpl.CURR), o.read_track()


def test_statement_vs_oracle_cross():
    """write_frame + crossFrameMatchingPoints of the oracle on every cross case the statement covers (the
    wild-bucket case has Z = 0 points and is the oracle's alone)."""
    bad = []
    for c in M.cross_cases() + M.cross_cfg_cases():
        prev, curr, track = oracle_cross(c, 2048)
        if c.statement:
            bad += M.check_cross(prev, curr, track, c)
        else:
            assert len(track["matched_pt"]) >= c.facts["planted"]
            wild = np.nonzero(c.P[:, 2] == 0)[0]
            assert set(wild.tolist()) & set(track["matched_pt"].tolist()), "no wild point wins a match"
    assert not bad, "\n".join(bad[:30])
