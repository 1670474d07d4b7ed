"""Landmark fusion without a GPU: gfpl_lm_fuse_check against the sequential model of
tests/lm_fuse_ref.py on every code of include/gfpl.h, from zero counts and from counts that are not
zero; the planner (gfpl_lm_fuse_plan.cpp) built with a small main under ASan + UBSan and its origin
resolution compared with the model (a stand-alone program; nothing is preloaded); the walk of
loopClosureFuseLandmarks on the Python map against the model run over the ops it emits.
"""
import os
import subprocess

import numpy as np
import pytest

import gfpl
import lm_fuse_cases as FC
import lm_fuse_ref as FR
import lm_store_cases as LC
import lm_store_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_CAP, OBS_CAP, SRC_ROWS = 1500, 8, [9, 4, 1]
LISTS = FC.planner_lists(LM_CAP, OBS_CAP, SRC_ROWS)


def _starts():
    """zero counts, and a first fill that leaves every named list its room: landmarks 20 and up"""
    zero = np.zeros(LM_CAP, np.int32)
    some = zero.copy()
    some[20:] = np.arange(LM_CAP - 20) % (OBS_CAP - 2)
    return [("zero", zero), ("filled", some)]


def test_exports_present():
    L = gfpl.hiplib()
    for n in ("gfpl_lm_fuse_check", "gfpl_lmstore_fuse"):
        assert hasattr(L, n), n
    assert gfpl.LM_APPEND_LM == FR.APPEND_LM == 3
    assert callable(gfpl.lm_fuse_check) and hasattr(gfpl.LandmarkStore, "fuse") and hasattr(gfpl.LandmarkStore, "fuse_rc")
    with open(os.path.join(ROOT, "include", "gfpl.h")) as f:
        h = f.read()
    assert "#define GFPL_ABI_VERSION 6 " in h and "#define GFPL_LM_APPEND_LM 3 " in h
    assert L.gfpl_abi_version() == 6


@pytest.mark.parametrize("start", [s[0] for s in _starts()])
@pytest.mark.parametrize("name,ops", LISTS, ids=[l[0] for l in LISTS])
def test_fuse_check_against_model(name, ops, start):
    counts = dict(_starts())[start]
    if name == "mixed" and start == "filled":
        ops = FC.random_mixed(LM_CAP, OBS_CAP, SRC_ROWS, 4000, 18, start=counts)
    m = FR.Model(LM_CAP, OBS_CAP)
    want_rc, want_cnt, want_rows, _ = m.fuse_check(ops, SRC_ROWS, counts)
    rc, cnt, n_rows = gfpl.lm_fuse_check(ops, counts, OBS_CAP, SRC_ROWS)
    assert rc == want_rc, (name, rc, want_rc)
    assert np.array_equal(cnt, want_cnt), name
    assert n_rows == want_rows, (name, n_rows, want_rows)
    if start == "zero":
        assert rc == FC.expected_code(name), name      # the model against the codes worked by hand
    if name == "mixed":
        assert len(ops) >= 3900 and sum(o[1] == FR.APPEND_LM for o in ops) >= 300 and rc == FR.OK


def test_fuse_check_counts_named():
    by = dict(LISTS)
    zero = np.zeros(LM_CAP, np.int32)
    run = lambda name: gfpl.lm_fuse_check(by[name], zero, OBS_CAP, SRC_ROWS)
    rc, cnt, n_rows = run("append_then_free")
    assert (rc, cnt[0], cnt[1], n_rows) == (FR.OK, 5, 0, 2 + 3 + 3 + 1)
    rc, cnt, n_rows = run("append_to_exactly_cap")
    assert (rc, cnt[3], cnt[4], n_rows) == (FR.OK, OBS_CAP, 2, OBS_CAP + 2)
    rc, cnt, n_rows = run("chain")
    assert (rc, cnt[0], cnt[1], cnt[2], n_rows) == (FR.OK, 2, 5, 6, 6 + 2 + 5)
    rc, cnt, n_rows = run("ring")
    assert (rc, cnt[6], cnt[7], n_rows) == (FR.OK, 2, 3, 2 + 1 + 2)
    rc, cnt, n_rows = run("append_twice")
    assert (rc, cnt[8], cnt[9]) == (FR.OK, 3, 1)
    rc, cnt, n_rows = run("append_one_over")
    assert rc == FR.E_CAPACITY and not cnt.any() and n_rows == 0
    # n_rows is what gfpl_lmstore_fuse holds against max_ops: an append counts its source's length
    rc, _, n_rows = gfpl.lm_fuse_check([(0, FR.APPEND_LM, 1, 0)] * 3, [1, 2, 0], OBS_CAP, [])
    assert (rc, n_rows) == (FR.OK, 6)


def test_ops_check_still_refuses_kind_3():
    for counts in ([2, 3], [0, 0]):
        rc, cnt = gfpl.lm_ops_check([(0, FR.APPEND_LM, 1, 0)], counts, OBS_CAP, SRC_ROWS)
        assert rc == R.E_INVALID and list(cnt) == counts


def test_fuse_check_arguments():
    L = gfpl.hiplib()
    ops = np.array([[0, FR.APPEND_LM, 1, 0]], np.int32)
    cnt = np.array([1, 2, 0, 0], np.int32)
    rows = np.array([2], np.int32)
    P = lambda a: a.ctypes.data
    assert L.gfpl_lm_fuse_check(P(ops), 1, P(cnt), 4, 4, P(rows), 1, None) == FR.OK and list(cnt) == [3, 2, 0, 0]   # n_rows NULL
    assert L.gfpl_lm_fuse_check(P(ops), 1, P(cnt), 4, 4, None, 0, None) == FR.E_CAPACITY                            # 3 + 2 > 4
    assert L.gfpl_lm_fuse_check(None, 1, P(cnt), 4, 4, P(rows), 1, None) == FR.E_INVALID
    assert L.gfpl_lm_fuse_check(P(ops), 1, None, 4, 4, P(rows), 1, None) == FR.E_INVALID
    assert L.gfpl_lm_fuse_check(P(ops), 1, P(cnt), 4, 4, None, 1, None) == FR.E_INVALID
    assert L.gfpl_lm_fuse_check(P(ops), -1, P(cnt), 4, 4, P(rows), 1, None) == FR.E_INVALID
    assert L.gfpl_lm_fuse_check(P(ops), 1, P(cnt), 0, 4, P(rows), 1, None) == FR.E_INVALID
    assert L.gfpl_lm_fuse_check(P(ops), 1, P(cnt), 4, 0, P(rows), 1, None) == FR.E_INVALID
    assert L.gfpl_lm_fuse_check(P(ops), 1, P(cnt), 4, 65, P(rows), 1, None) == FR.E_INVALID
    assert L.gfpl_lm_fuse_check(P(ops), 1, P(cnt), 4, 4, P(rows), -1, None) == FR.E_INVALID
    assert L.gfpl_lm_fuse_check(None, 0, P(cnt), 4, 4, None, 0, None) == FR.OK      # n = 0
    assert list(cnt) == [3, 2, 0, 0]
    for bad in ([-1, 2, 0, 0], [9, 2, 0, 0], [1, -1, 0, 0], [1, 9, 0, 0]):           # a count that is none, of lm or of arg
        b = np.array(bad, np.int32)
        assert L.gfpl_lm_fuse_check(P(ops), 1, P(b), 4, 4, P(rows), 1, None) == FR.E_INVALID and list(b) == bad


@pytest.fixture(scope="module")
def planner_exe(tmp_path_factory):
    """the planner's translation unit and tests/lm_fuse_plan_main.cpp, no HIP, under ASan + UBSan"""
    exe = str(tmp_path_factory.mktemp("lm_fuse_plan") / "lm_fuse_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "lm_fuse_plan_main.cpp"),
           os.path.join(ROOT, "gf-pl-slam_amd", "csrc", "gfpl_lm_fuse_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("min_g", [0, 64])
def test_planner_under_sanitizers(planner_exe, tmp_path, min_g):
    lm_cap, obs_cap = 80, 64
    lists = []
    for sname, start in (("zero", np.zeros(lm_cap, np.int32)), ("filled", np.r_[np.zeros(20), np.arange(26) % 2, 1 + np.arange(34) % 40].astype(np.int32))):
        lists += [(sname + ":" + name, start, ops) for name, ops in FC.planner_lists(lm_cap, obs_cap, SRC_ROWS)]
        # a destination of n / 2 rows and a source of the rest, for every n of the store's LENGTHS: every bucket
        ladder = []
        for k, n in enumerate(n for n in LC.LENGTHS if n >= 2):
            ladder += FC.adds(20 + 2 * k, n // 2 - start[20 + 2 * k], SRC_ROWS) + FC.adds(21 + 2 * k, n - n // 2 - start[21 + 2 * k], SRC_ROWS)
            ladder.append((20 + 2 * k, FR.APPEND_LM, 21 + 2 * k, 0))
        lists.append((sname + ":ladder", start, ladder))
        lists.append((sname + ":long_sources", start, FC.random_mixed(lm_cap, obs_cap, SRC_ROWS, 1500, 5, start=start, max_from=20)))
    path = tmp_path / "lists.txt"
    with open(path, "w") as f:
        f.write(f"{lm_cap} {obs_cap} {min_g} {len(SRC_ROWS)} {' '.join(map(str, SRC_ROWS))} {len(lists)}\n")
        for _, start, ops in lists:
            f.write(" ".join(map(str, start)) + f" {len(ops)} " + " ".join(str(v) for op in ops for v in op) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([planner_exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    out = r.stdout.strip().split("\n")
    assert len(out) == 3 * len(lists)
    buckets_seen, store_origins = set(), 0
    for k, (name, start, ops) in enumerate(lists):
        rc_l, cnt_l, org_l = ([int(v) for v in out[3 * k + j].split()[1:]] for j in range(3))
        want_rc, want_cnt, want_rows, want_org = FR.Model(lm_cap, obs_cap).fuse_check(ops, SRC_ROWS, start)
        assert rc_l == [want_rc, want_rows], name
        assert cnt_l == list(want_cnt), name
        got, p = {}, 0
        work = []
        while p < len(org_l):
            lm, b, count0, freed, ng = org_l[p:p + 5]
            pairs = [(org_l[p + 5 + 2 * i], org_l[p + 6 + 2 * i]) for i in range(ng)]
            p += 5 + 2 * ng
            # the final list: the rows from before the call, then what the landmark gained
            got[lm] = [] if freed else [(-1 - lm, q) for q in range(count0)] + pairs
            assert count0 == start[lm] and not (freed and ng), name
            work.append((b, lm))
            buckets_seen.add(b)
            store_origins += sum(s < 0 for s, _ in pairs)
        assert got == want_org, name
        # work items: buckets ascending, first-touch order within a bucket, bucket by the final length
        assert [w[0] for w in work] == sorted(w[0] for w in work), name
        first = list(want_org)
        for b in {w[0] for w in work}:
            lms = [w[1] for w in work if w[0] == b]
            assert lms == sorted(lms, key=first.index), name
        for b, lm in work:
            n = len(want_org[lm])
            want_b = 0
            while want_b < 5 and ((2 << want_b) < n or (2 << want_b) < min_g):
                want_b += 1
            assert b == want_b, (name, lm, n, b)
        # every origin in the store lies below its landmark's count before the call
        for l in want_org.values():
            assert all(0 <= row < start[-1 - s] for s, row in l if s < 0), name
    assert buckets_seen == ({5} if min_g == 64 else {0, 1, 2, 3, 4, 5})
    print('origins that are store rows:', store_origins)
    assert store_origins > 200   # the lists do reach into the store


def _walk_map(rng):
    """3 keyframes of 60 features, 40 landmarks of 1-3 observations each from keyframes 0 and 1"""
    kf_desc = [rng.integers(0, 256, (60, 32), dtype=np.uint8) for _ in range(3)]
    m = FR.Map(40, kf_desc)
    for lm in range(40):
        m.observe(lm, 0, lm)
        if lm % 2:
            m.observe(lm, 1, lm)
        if lm % 5 == 0:
            m.observe(lm, 2, lm)
    return m


# rows (lm_idx0, lm_ldx0, lm_idx1, lm_ldx1) of keyframes 0 (previous) and 2 (current)
WALK_ROWS = [
    (-1, 41, 3, 45),     # case 1: feature 41 of the previous keyframe joins landmark 3
    (4, 4, -1, 46),      # case 2
    (-1, 42, -1, 47),    # case 3: landmark 40 is created
    (6, 6, 7, 48),       # case 4: 7 into 6
    (-1, 43, 8, 49),     # 8 is added to ...
    (9, 9, 8, 50),       # ... and then merged into 9
    (7, 7, 11, 51),      # 7 was merged away: skipped
    (12, 12, 7, 52),     # and as the second landmark: skipped
    (-1, 44, 7, 53),     # case 1 onto a NULL landmark: skipped
    (6, 6, 13, 54),      # 6 takes a second merge
    (-1, 55, -1, 56),    # landmark 41
    (5, 5, 5, 57),       # the same landmark twice: nothing to merge
]


def test_loop_closure_walk_against_model():
    rng = np.random.default_rng(21)
    m = _walk_map(rng)
    model = FR.Model(64, 16)
    for lm, l in enumerate(m.lms):
        model.lists[lm] = [d.copy() for d in l.desc_list]
    ops, max_idx = FR.loop_closure_fuse_walk(m, 0, 2, WALK_ROWS, 40)
    assert max_idx == 42
    kinds = [o[1] for o in ops]
    assert kinds.count(FR.APPEND_LM) == 3 and kinds.count(FR.FREE) == 3 and kinds.count(FR.ADD) == 3 + 4
    rc, _, n_rows, _ = model.fuse_check(ops, [60, 60, 60])
    assert rc == FR.OK and n_rows >= len(ops)
    named = model.fuse(ops, m.kf_desc)
    assert set(named) == {3, 4, 40, 6, 7, 8, 9, 13, 41}
    for lm in range(42):
        want = [] if m.lms[lm] is None else m.lms[lm].desc_list
        assert len(model.lists[lm]) == len(want) and all(np.array_equal(a, b) for a, b in zip(model.lists[lm], want)), lm
        if m.lms[lm] is not None:     # the parallel list names the rows' origins
            assert all(np.array_equal(m.kf_desc[kf][row], d) for (kf, row), d in zip(m.lms[lm].obs_list, want)), lm
    assert m.lms[7] is None and m.lms[8] is None and m.lms[13] is None and len(m.lms[9].desc_list) == 2 + (1 + 1)


# ---- the search statement alone (lm_fuse_ref.search), cases worked by hand --------------------
CAM = dict(fx=256.0, fy=256.0, cx=320.0, cy=240.0, width=640, height=480)
EYE = np.eye(4).reshape(1, 16)


def _desc(*first_bytes):
    d = np.zeros((len(first_bytes), 32), np.uint8)
    d[:, 0] = first_bytes
    return d


def test_search_border_and_z():
    # z = 2: u = 320 + 256 x / 2, so x = -2.5 lands exactly on 0 and x = 2.5 exactly on width; v likewise with 1.875
    P = np.array([[-2.5, 0, 2], [2.5, 0, 2], [-2.4999, 0, 2], [2.4999, 0, 2], [0, -1.875, 2], [0, 1.875, 2], [0, 1.8749, 2],
                  [0, 0, 0], [1, 0, 0], [0, 0, -2], [0, 0, 1e-300]])
    loc, pairs, bad = FR.search(CAM, _desc(*range(len(P))), P, np.zeros(len(P), int), EYE)
    assert list(loc) == [2, 3, 6, 10] and not bad
    # T is applied as written: a translation of +1 in z brings z = -0.5 in front, and x with it
    T = np.eye(4)
    T[2, 3] = 1.0
    loc, _, _ = FR.search(CAM, _desc(1, 2), [[0, 0, -0.5], [0, 0, -1.0]], [1, 1], np.stack([EYE[0], T.reshape(16)]))
    assert list(loc) == [0]
    # lines: both endpoints must pass
    L = np.array([[0, 0, 2, 1, 0, 2], [0, 0, 2, 2.5, 0, 2], [2.5, 0, 2, 0, 0, 2], [0, 0, 2, 0, 0, 0]], float)
    loc, _, _ = FR.search(CAM, _desc(1, 2, 3, 4), L, np.zeros(4, int), EYE)
    assert list(loc) == [0]
    # a keyframe index out of range: not selected, reported
    loc, _, bad = FR.search(CAM, _desc(1, 2, 3), [[0, 0, 2]] * 3, [0, 1, -1], EYE)
    assert list(loc) == [0] and bad


def test_search_second_neighbour_and_identical_descriptors():
    # rows 0 and 1 share a descriptor: row 0's second neighbour is 1; row 1's first is 0 (the lower
    # index) and its second is itself, so it is skipped; row 2 is its own first and 0 its second (0 and 1 tie, 0 first)
    P = [[0, 0, 2], [0.01, 0, 2], [0.02, 0, 2]]
    loc, pairs, _ = FR.search(CAM, _desc(7, 7, 6), P, [0, 0, 0], EYE)
    assert list(loc) == [0, 1, 2] and pairs.tolist() == [[0, 1], [2, 0]]
    assert FR.knn2_self(_desc(7, 7, 6)).tolist() == [[0, 1], [0, 1], [2, 0]]
    # identical at a higher index: (1, 2) is there, its mirror is not (row 2's second neighbour is itself)
    loc, pairs, _ = FR.search(CAM, _desc(0xFF, 1, 1), P, [0, 0, 0], EYE)
    assert pairs.tolist() == [[0, 1], [1, 2]]
    # two selected rows: each is the other's second neighbour; one selected row: nothing
    loc, pairs, _ = FR.search(CAM, _desc(1, 0xF0), P[:2], [0, 0], EYE)
    assert pairs.tolist() == [[0, 1], [1, 0]]
    loc, pairs, _ = FR.search(CAM, _desc(1, 0xF0), [P[0], [0, 0, -1]], [0, 0], EYE)
    assert list(loc) == [0] and len(pairs) == 0
    loc, pairs, _ = FR.search(CAM, np.zeros((0, 32), np.uint8), np.zeros((0, 3)), [], EYE)
    assert len(loc) == 0 and len(pairs) == 0


def test_search_point_gate_is_strict():
    # |(0.1, 0, 0)| = sqrt(0.1 * 0.1 + (0 + 0)) = 0.1: not below the threshold 0.1
    assert float(np.sqrt(np.float64(0.1) * np.float64(0.1))) == 0.1
    for dx, ok in ((0.1, False), (0.09999999999999999, True), (0.2, False)):
        _, pairs, _ = FR.search(CAM, _desc(1, 3), [[0, 0, 2], [dx, 0, 2]], [0, 0], EYE)
        assert (len(pairs) == 2) == ok and len(pairs) in (0, 2), dx
    # FU3: the sum is a0 + (a1 + a2)
    a = np.array([[1e16, 1.0, 1.0]])
    assert float(FR._sum3(a[:, 0], a[:, 1], a[:, 2])[0]) == 1e16 + 2.0 != (1e16 + 1.0) + 1.0


def test_search_line_gate():
    base = [0, 0, 2, 1, 0, 2]
    cases = [([0, 0.05, 2, 1, 0.05, 2], True),        # parallel, 0.05 away
             ([0, 0.1, 2, 1, 0.1, 2], False),          # exactly 0.1 away: strict
             ([0, 0.05, 2, 1, 0.2, 2], False),         # the far endpoint 0.2 away (and the directions 0.15 apart)
             ([1, 0.01, 2, 0, 0.01, 2], False),        # the same line the other way round: |d1 - d2| = 2
             ([0.3, 0.01, 2, 0.3, 0.01, 2], False)]    # a zero-length line: NaN fails every comparison
    for other, ok in cases:
        for L in ([base, other], [other, base]):
            _, pairs, _ = FR.search(CAM, _desc(1, 3), np.array(L, float), [0, 0], EYE)
            assert (len(pairs) == 2) == ok and len(pairs) in (0, 2), other
    # both branches of d1.norm() > d2.norm() are taken by ordinary segments
    rng = np.random.default_rng(4)
    L = rng.normal(size=(4000, 6))
    branch = []
    FR.line_gate(L, np.arange(0, 4000, 2), np.arange(1, 4000, 2), FR.DEFAULT_FUSE_PARAMS, branch)
    frac = float(np.mean(branch))
    print("d1.norm() > d2.norm() on Gaussian segment pairs:", frac)
    assert 0.15 < frac < 0.35


def test_local_map_walk_as_written_and_as_meant():
    """pairs (0, 1), its mirror, and (2, 3) over selected landmarks 10 .. 13"""
    pairs, local = [(0, 1), (1, 0), (2, 3)], [10, 11, 12, 13]
    rng = np.random.default_rng(8)

    def fresh():
        m = FR.Map(16, [rng.integers(0, 256, (16, 32), dtype=np.uint8)])
        for lm in local:
            m.observe(lm, 0, lm)
            m.observe(lm, 0, lm - 8)
        return m
    counts = np.zeros(16, np.int32)
    counts[local] = 2
    # as written: pair 0 merges 11 into 10 and then frees the 0-th selected landmark, 10 itself; the mirror
    # merges the stale 10 into 11: the list names a freed landmark and is refused whole
    m = fresh()
    ops = FR.fuse_local_map_walk(m, local, pairs, as_written=True)
    assert ops[:3] == [(10, FR.APPEND_LM, 11, 0), (10, FR.FREE, 0, 0), (11, FR.APPEND_LM, 10, 0)]
    rc, cnt, n_rows = gfpl.lm_fuse_check(ops, counts, 8, [16])
    assert rc == FR.E_INVALID and np.array_equal(cnt, counts)
    # as meant: the merged landmark is freed, the mirror is skipped
    m = fresh()
    ops = FR.fuse_local_map_walk(m, local, pairs, as_written=False)
    assert ops == [(10, FR.APPEND_LM, 11, 0), (11, FR.FREE, 0, 0), (12, FR.APPEND_LM, 13, 0), (13, FR.FREE, 0, 0)]
    rc, cnt, n_rows = gfpl.lm_fuse_check(ops, counts, 8, [16])
    assert rc == FR.OK and [cnt[i] for i in local] == [4, 0, 4, 0] and n_rows == 6
    model = FR.Model(16, 8)
    for lm in local:
        model.lists[lm] = [m.kf_desc[0][lm].copy(), m.kf_desc[0][lm - 8].copy()]
    model.fuse(ops, m.kf_desc)
    for lm in local:
        want = [] if m.lms[lm] is None else m.lms[lm].desc_list
        assert len(want) == len(model.lists[lm]) and all(np.array_equal(a, b) for a, b in zip(want, model.lists[lm]))
