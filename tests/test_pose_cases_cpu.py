"""The written pose problems (pose_cases.py) on the CPU oracle: every case takes the path it names, the
outlier decision of the planted-residual cases equals its numpy statement bit for bit, and the families
notice the faults they aim at (five altered rules each change a flag or a count somewhere)."""
import numpy as np
import pytest

import pose_cases as M

I4 = np.eye(4)


def _all_cases():
    return [c for f in M.FAMILIES for c in M.family(f)]


def _statement(c, **rule):
    """flags per feature and counts after removeOutliers by the numpy statement (cases with planted residuals)"""
    k = c.cfg().inlier_k
    per_feature = rule.pop("per_feature", False)
    return M.expected_after(c, M.mad_decision(c.mad["pt"], k, **rule), M.mad_decision(c.mad["ls"], k, **rule),
                            per_feature=per_feature)


def _path_failures(c):
    prev, curr, tr = M.oracle_result(c)
    w = c.written
    DT, cov, en = curr.get("DT"), curr.get("DT_cov"), float(curr.s.err_norm)
    counts = (tr["n_inliers"], tr["n_inliers_pt"], tr["n_inliers_ls"])
    counts_w = (w["n_inliers"], w["n_inliers_pt"], w["n_inliers_ls"])
    flags_kept = (np.array_equal(prev.arr["pt_inlier"], w["pt_inlier"]) and np.array_equal(prev.arr["ls_inlier"], w["ls_inlier"]))
    is_reset = np.array_equal(DT, I4) and not cov.any()
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(f"{c.what()}: {what}")

    if c.path.startswith("reset"):
        need(is_reset, f"DT identity and DT_cov zero expected, DT_cov max {np.nanmax(np.abs(cov))}")
        need(tr["num_frame_loss"] == 0, "num_frame_loss")
    if c.path == "reset_pre":
        need(w["n_inliers"] <= M.MIN_FEATURES and counts == counts_w and flags_kept, f"counts {counts} written {counts_w}")
        need(en == 0.0 or c.curr.s.time_stamp <= c.prev.s.time_stamp, f"err_norm {en}")
    elif c.path == "reset_outliers":
        need(w["n_inliers"] > M.MIN_FEATURES >= tr["n_inliers"], f"n_inliers {w['n_inliers']} -> {tr['n_inliers']}")
    elif c.path == "reset_nonfinite":
        need(w["n_inliers"] > M.MIN_FEATURES and counts == counts_w and flags_kept, f"counts {counts} written {counts_w}")
    elif c.path == "rejected":
        need(en == -1.0 and tr["num_frame_loss"] == 0, f"err_norm {en}, num_frame_loss {tr['num_frame_loss']}")
        need(np.array_equal(DT, I4) and np.array_equal(curr.get("Tfw"), c.prev.get("Tfw")), "DT identity, Tfw kept")
        need(np.array_equal(curr.get("Tfw_cov"), c.prev.get("Tfw_cov")), "Tfw_cov kept")
        need(cov.any() and tr["n_inliers"] > M.MIN_FEATURES, "a solved stage 2 expected behind the gate")
    elif c.path == "lost":
        need(w["num_frame_loss"] == 3 and tr["num_frame_loss"] == 4, f"num_frame_loss {tr['num_frame_loss']}")
        need(en == -1.0 and np.array_equal(DT, I4) and np.array_equal(curr.get("Tfw"), c.prev.get("Tfw")), "rolled back")
        need(tr["n_inliers"] > M.MIN_FEATURES and not np.isfinite(cov).all(), "stage 2 ran and left a non-finite H")
    elif c.path == "solved":
        need(not is_reset and en != -1.0 and tr["num_frame_loss"] == 0, f"err_norm {en}")
        need(tr["n_inliers"] > M.MIN_FEATURES and np.isfinite(DT).all(), f"n_inliers {tr['n_inliers']}")
        if c.pose_tol is not None:
            Ti = np.linalg.inv(c.T_cp)
            need(np.allclose(DT, Ti, rtol=0, atol=c.pose_tol), f"DT off by {np.abs(DT - Ti).max()}")
            need(np.allclose(curr.get("Tfw"), c.prev.get("Tfw") @ Ti, rtol=0, atol=10 * c.pose_tol), "Tfw")
            need(0.0 <= en, f"err_norm {en}")
    if c.expect_off is not None:   # the planted entries, and only they, are flagged
        ip, il = c.matched()
        pt, ls = w["pt_inlier"].copy(), w["ls_inlier"].copy()
        pt[ip[c.expect_off["pt"]]] = 0
        ls[il[c.expect_off["ls"]]] = 0
        n_off = len(c.expect_off["pt"]) + len(c.expect_off["ls"])
        need(np.array_equal(prev.arr["pt_inlier"], pt) and np.array_equal(prev.arr["ls_inlier"], ls), "planted flag set")
        need(tr["n_inliers"] == w["n_inliers"] - n_off and tr["n_inliers_pt"] == w["n_inliers_pt"] - len(c.expect_off["pt"])
             and tr["n_inliers_ls"] == w["n_inliers_ls"] - len(c.expect_off["ls"]), f"planted counts {counts}")
    return bad


@pytest.mark.parametrize("fam", list(M.FAMILIES))
def test_every_case_takes_its_path(fam):
    bad = []
    for c in M.family(fam):
        bad += _path_failures(c)
    assert not bad, "\n".join(bad[:40])


def test_every_path_is_taken_and_indices_stay_in_range():
    cases = _all_cases()
    assert {c.path for c in cases} == set(M.PATHS)
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        ip, il = c.matched()
        assert (len(ip) == 0 or (0 <= ip.min() and ip.max() < c.prev.s.n_pt)) and \
               (len(il) == 0 or (0 <= il.min() and il.max() < c.prev.s.n_ls)), c.what()
        for v in (c.prev.arr["pt_P"], c.prev.arr["pt_pl_obs"], c.prev.arr["ls_le_obs"], c.prev.arr["ls_sP"]):
            assert np.isfinite(v).all(), c.what()   # (every input finite; the one NaN is an explicit DT_ini)
    for ctx, k in M.CONTEXTS.items():
        assert any(c.ctx == ctx and c.tr.n_matched_pt == k["mpt"] and c.tr.n_matched_ls == k["mls"] for c in cases)


def test_outlier_decision_matches_numpy_statement():
    """np.sort, the median at n // 2, the float32 absolute deviation, 1.4826, strict >, flags and counts per list
    position: the oracle's flags and counts exactly."""
    cases = [c for c in _all_cases() if c.mad]
    assert len(cases) > 100
    bad = []
    for c in cases:
        prev, _, tr = M.oracle_result(c)
        pt, ls, counts = _statement(c)
        if not (np.array_equal(prev.arr["pt_inlier"], pt) and np.array_equal(prev.arr["ls_inlier"], ls)):
            bad.append(f"{c.what()}: flags differ at pt {np.flatnonzero(prev.arr['pt_inlier'] != pt)[:5]} "
                       f"ls {np.flatnonzero(prev.arr['ls_inlier'] != ls)[:5]}")
        if counts != (tr["n_inliers"], tr["n_inliers_pt"], tr["n_inliers_ls"]):
            bad.append(f"{c.what()}: counts {counts} vs oracle {(tr['n_inliers'], tr['n_inliers_pt'], tr['n_inliers_ls'])}")
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("rule", ["median_low", "mad_low", "double_dev", "ge", "per_feature"])
def test_altered_rule_is_noticed(rule):
    """A kernel that took the median, or the median of the deviations, at (n - 1) / 2, kept the deviation in double,
    compared with >= or counted per unique feature would differ from the oracle in a flag or a count of at least
    one case — in both contexts (the register selection and the LDS sort)."""
    kw = {"median_low": dict(median_at=lambda n: (n - 1) // 2), "mad_low": dict(mad_at=lambda n: (n - 1) // 2),
          "double_dev": dict(double_dev=True), "ge": dict(ge=True), "per_feature": dict(per_feature=True)}[rule]
    noticed = {"small": [], "big": []}
    for c in _all_cases():
        if not c.mad:
            continue
        pt, ls, counts = _statement(c)
        apt, als, acounts = _statement(c, **kw)
        if not (np.array_equal(pt, apt) and np.array_equal(ls, als) and counts == acounts):
            noticed[c.ctx].append(c.name)
    assert noticed["small"] and noticed["big"], noticed


def test_nan_aware_bitwise_helper():
    from parity import bitwise_equal, bitwise_equal_nan
    a = np.array([1.0, np.nan, -0.0, np.inf])
    b = a.copy()
    b[1] = -np.nan
    b.view(np.uint64)[1] |= 0x7
    assert not bitwise_equal(a, b) and bitwise_equal_nan(a, b)
    assert not bitwise_equal_nan(a, np.array([1.0, np.nan, 0.0, np.inf]))      # the sign of zero still counts
    assert not bitwise_equal_nan(a, np.array([1.0, 2.0, -0.0, np.inf]))        # a NaN matches only a NaN
    assert not bitwise_equal_nan(a, np.array([np.nan, 1.0, -0.0, np.inf]))     # ... at the same position
    assert not bitwise_equal_nan(a, a[:3])
    assert bitwise_equal_nan(np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32))
