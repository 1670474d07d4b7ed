"""The landmark descriptor store without a GPU: the reference's known answers, the generator's
bar, gfpl_lm_ops_check against the model on every error of include/gfpl.h, the new exports, and
the planner (gfpl_lm_plan.cpp) built with a small main under ASan + UBSan and run over the
adversarial op lists (a stand-alone program; nothing is preloaded).
"""
import os
import subprocess

import numpy as np
import pytest

import gfpl
import lm_store_cases as LC
import lm_store_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_CAP, OBS_CAP, SRC_ROWS = 12, 6, [9, 4, 1]


@pytest.mark.parametrize("name,rows,idx", LC.written_lists(), ids=[w[0] for w in LC.WRITTEN])
def test_reference_known_answers(name, rows, idx):
    assert R.med_index(rows) == idx


def test_reference_n1_reads_nothing():
    # LM4: one observation is its own median row whatever it holds
    rng = np.random.default_rng(3)
    for _ in range(8):
        assert R.med_index([rng.integers(0, 256, 32, dtype=np.uint8)]) == 0
    assert R.med_index([]) == -1


def test_reference_order_matters_only_for_ties():
    # the written tie: reversing the list moves the winner to the other tied row's new place
    name, rows, idx = [w for w in LC.written_lists() if w[0] == "tie_smaller_index"][0]
    assert R.med_index(rows[::-1]) == 1 and idx == 1


def test_generator_is_adversarial():
    LC.assert_adversarial()


def test_exports_present():
    L = gfpl.hiplib()
    for n in ("gfpl_lmstore_create", "gfpl_lmstore_destroy", "gfpl_lmstore_bytes", "gfpl_lm_ops_check",
              "gfpl_lmstore_apply", "gfpl_lmstore_gather", "gfpl_lmstore_read", "gfpl_lmstore_debug_ms"):
        assert hasattr(L, n), n
    assert gfpl.LM_MAX_OBS == R.MAX_OBS == 64
    assert (gfpl.LM_ADD, gfpl.LM_ERASE_OBS, gfpl.LM_FREE) == (R.ADD, R.ERASE_OBS, R.FREE)
    assert callable(gfpl.lm_ops_check) and hasattr(gfpl.LandmarkStore, "apply") and hasattr(gfpl.LandmarkStore, "gather")
    with open(os.path.join(ROOT, "include", "gfpl.h")) as f:
        h = f.read()
    assert "#define GFPL_ABI_VERSION 6 " in h and "#define GFPL_LM_MAX_OBS 64 " in h
    assert L.gfpl_abi_version() == 6


@pytest.mark.parametrize("name,ops", LC.planner_lists(LM_CAP, OBS_CAP, SRC_ROWS),
                         ids=[l[0] for l in LC.planner_lists(LM_CAP, OBS_CAP, SRC_ROWS)])
def test_ops_check_against_model(name, ops):
    m = R.Model(LM_CAP, OBS_CAP)
    want_rc, want_cnt = m.check(ops, SRC_ROWS)
    rc, cnt = gfpl.lm_ops_check(ops, m.counts(), OBS_CAP, SRC_ROWS)
    assert rc == want_rc, (name, rc, want_rc)
    assert np.array_equal(cnt, want_cnt), (name, cnt, want_cnt)
    # the same from counts that are not zero: a first fill, then the list again
    first = [(lm, R.ADD, 0, 0) for lm in range(LM_CAP) for _ in range(lm % 4)]
    _, start = m.check(first, SRC_ROWS)
    want_rc, want_cnt = m.check(ops, SRC_ROWS, start)
    rc, cnt = gfpl.lm_ops_check(ops, start, OBS_CAP, SRC_ROWS)
    assert rc == want_rc and np.array_equal(cnt, want_cnt), (name, rc, want_rc, cnt, want_cnt)


def test_ops_check_codes_named():
    by = dict(LC.planner_lists(LM_CAP, OBS_CAP, SRC_ROWS))
    zero = np.zeros(LM_CAP, np.int32)
    code = lambda name: gfpl.lm_ops_check(by[name], zero, OBS_CAP, SRC_ROWS)[0]
    assert code("empty") == code("fill") == code("free_empty_twice") == code("add_erase_add") == R.OK
    assert code("over") == code("capacity_before_invalid") == R.E_CAPACITY
    for name in ("erase_empty", "erase_at_count", "erase_negative", "erase_after_free", "lm_negative", "lm_cap", "lm_huge",
                 "kind_unknown", "kind_negative", "src_negative", "src_past", "src_huge", "row_negative", "row_past",
                 "row_huge", "bad_after_good", "invalid_before_capacity"):
        assert code(name) == R.E_INVALID, name


def test_ops_check_arguments():
    L = gfpl.hiplib()
    ops = np.array([[0, R.ADD, 0, 0]], np.int32)
    cnt = np.zeros(4, np.int32)
    rows = np.array([2], np.int32)
    P = lambda a: a.ctypes.data
    assert L.gfpl_lm_ops_check(P(ops), 1, P(cnt), 4, 4, P(rows), 1) == R.OK and cnt[0] == 1
    assert L.gfpl_lm_ops_check(None, 1, P(cnt), 4, 4, P(rows), 1) == R.E_INVALID
    assert L.gfpl_lm_ops_check(P(ops), 1, None, 4, 4, P(rows), 1) == R.E_INVALID
    assert L.gfpl_lm_ops_check(P(ops), 1, P(cnt), 4, 4, None, 1) == R.E_INVALID
    assert L.gfpl_lm_ops_check(P(ops), -1, P(cnt), 4, 4, P(rows), 1) == R.E_INVALID
    assert L.gfpl_lm_ops_check(P(ops), 1, P(cnt), 0, 4, P(rows), 1) == R.E_INVALID
    assert L.gfpl_lm_ops_check(P(ops), 1, P(cnt), 4, 0, P(rows), 1) == R.E_INVALID
    assert L.gfpl_lm_ops_check(P(ops), 1, P(cnt), 4, 65, P(rows), 1) == R.E_INVALID
    assert L.gfpl_lm_ops_check(P(ops), 1, P(cnt), 4, 4, P(rows), -1) == R.E_INVALID
    assert L.gfpl_lm_ops_check(None, 0, P(cnt), 4, 4, None, 0) == R.OK      # n = 0
    assert L.gfpl_lm_ops_check(P(ops), 1, P(cnt), 4, 4, None, 0) == R.E_INVALID   # an ADD without sources
    assert cnt[0] == 1
    bad = np.array([9, 0, 0, 0], np.int32)                                   # a count above obs_cap on first touch
    assert L.gfpl_lm_ops_check(P(ops), 1, P(bad), 4, 4, P(rows), 1) == R.E_INVALID and bad[0] == 9


def _expected_plan(ops, lm_cap, obs_cap, min_g):
    """Stable grouping in first-touch order within buckets, buckets by the longest list reached."""
    ops = np.asarray(ops, np.int64).reshape(-1, 4)
    touched, per, cnt, peak = [], {}, {}, {}
    for i, (lm, kind, arg, src) in enumerate(ops):
        lm = int(lm)
        if lm not in per:
            touched.append(lm)
            per[lm], cnt[lm], peak[lm] = [], 0, 0
        per[lm].append(i)
        cnt[lm] = cnt[lm] + 1 if kind == R.ADD else (cnt[lm] - 1 if kind == R.ERASE_OBS else 0)
        peak[lm] = max(peak[lm], cnt[lm])

    def bucket(p):
        b = 0
        while b < 5 and ((2 << b) < p or (2 << b) < min_g):
            b += 1
        return b
    work = sorted(touched, key=lambda lm: bucket(peak[lm]))   # sorted() is stable
    order = [i for lm in work for i in per[lm]]
    return order, [(lm, len(per[lm]), 0, bucket(peak[lm])) for lm in work]


@pytest.fixture(scope="module")
def planner_exe(tmp_path_factory):
    """the planner's translation unit and tests/lm_plan_main.cpp, no HIP, under ASan + UBSan"""
    exe = str(tmp_path_factory.mktemp("lm_plan") / "lm_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "lm_plan_main.cpp"),
           os.path.join(ROOT, "gf-pl-slam_amd", "csrc", "gfpl_lm_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("min_g", [0, 64])
def test_planner_under_sanitizers(planner_exe, tmp_path, min_g):
    exe = planner_exe
    lm_cap, obs_cap = 40, 64
    lists = LC.planner_lists(lm_cap, obs_cap, SRC_ROWS)
    path = tmp_path / "lists.txt"
    with open(path, "w") as f:
        f.write(f"{lm_cap} {obs_cap} {min_g} {len(SRC_ROWS)} {' '.join(map(str, SRC_ROWS))} {len(lists)}\n")
        for _, ops in lists:
            f.write(f"{len(ops)} " + " ".join(str(v) for op in ops for v in op) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    out = r.stdout.strip().split("\n")
    assert len(out) == 4 * len(lists)
    buckets_seen = set()
    for k, (name, ops) in enumerate(lists):
        rc_l, cnt_l, ord_l, work_l = (out[4 * k + j].split()[1:] for j in range(4))
        want_rc, want_cnt = R.Model(lm_cap, obs_cap).check(ops, SRC_ROWS)
        assert int(rc_l[0]) == want_rc, name
        assert [int(v) for v in cnt_l] == list(want_cnt), name
        if want_rc != R.OK or not ops:
            assert ord_l == [] and work_l == [], name
            continue
        order, work = _expected_plan(ops, lm_cap, obs_cap, min_g)
        assert [int(v) for v in ord_l] == order, name
        got = [tuple(int(v) for v in work_l[5 * w:5 * w + 5]) for w in range(len(work))]
        assert [(g[0], g[2], g[3], g[4]) for g in got] == work, name
        assert [g[1] for g in got] == list(np.cumsum([0] + [w[1] for w in work[:-1]])), name
        buckets_seen |= {g[4] for g in got}
    assert buckets_seen == ({5} if min_g == 64 else {0, 1, 2, 3, 4, 5})
