"""The Python reference of the loop-closure check (tests/loop_closure_ref.py) pinned without a GPU:
its new numeric pins (N6 acos, N7 3x3 inverse, N8 logmap_se3), that every case family of
tests/loop_closure_cases.py takes the path it is built for, that four plausible misreadings of the
reference each change a result, and the C ABI's host-side part.
"""
import ctypes as C
import math

import numpy as np
import pytest

import gfpl
import loop_closure_cases as LC
import loop_closure_ref as R
import oracle as O


# ------------------------------------------------------------------- pins --
def test_acos_within_one_ulp_of_libm():
    xs = np.concatenate([np.linspace(-1.0, 1.0, 4001), [0.5 - 2 ** -54, 0.5 + 2 ** -53, -0.5 + 2 ** -54, 1e-20, -1e-20,
                                                         1.0 - 2 ** -53, -1.0 + 2 ** -53]])
    for x in xs:
        a, b = float(R.acos(x)), math.acos(x)
        assert abs(a - b) <= np.spacing(b), (x, a, b)
    for x in (1.0, -1.0, 0.0, 0.5, -0.5):
        assert float(R.acos(x)) == math.acos(x), x
    assert np.isnan(R.acos(1.0000001)) and np.isnan(R.acos(np.nan))


def test_inverse3_against_numpy():
    """cofactor inverse of a matrix with condition number k: relative error about k eps; the random
    matrices below are kept at k < 1e3, so 1e-12 leaves two orders of margin"""
    rng = np.random.default_rng(7)
    n = 0
    while n < 50:
        m = rng.uniform(-2, 2, (3, 3))
        if np.linalg.cond(m) > 1e3:
            continue
        n += 1
        ref = np.linalg.inv(m)
        assert np.abs(R.inverse3(m) - ref).max() <= 1e-12 * np.abs(ref).max()
    d = R.inverse3(np.diag([2.0, 4.0, 8.0]))
    np.testing.assert_array_equal(d, np.diag([0.5, 0.25, 0.125]))   # det = 64: every step exact


def test_logmap_inverts_expmap():
    """theta is recovered through acos(cosine), whose error is about eps / sin(theta) (2e-15 at the
    smallest angle used, 0.1) and the same again near pi (largest angle 3.0: sin = 0.14); the
    translation goes through a 3x3 inverse of V (condition < 10 for theta <= 3): 1e-12 bounds both"""
    rng = np.random.default_rng(8)
    for _ in range(40):
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w) * rng.uniform(0.1, 3.0)
        x = np.concatenate([rng.uniform(-2, 2, 3), w])
        back = R.logmap_se3(O.expmap_se3(x))
        assert np.abs(back - x).max() <= 1e-12, (x, back)


def test_logmap_branches():
    # theta <= 1e-6: w = 0 and V = I, whose cofactor inverse is exactly I: t comes back as it went in
    T = np.eye(4)
    T[:3, 3] = [0.3, -0.2, 0.7]
    np.testing.assert_array_equal(R.logmap_se3(T), [0.3, -0.2, 0.7, 0.0, 0.0, 0.0])
    # a half turn: cosine = -1, sine = 0; R - R^T = 0, so w_hat = (pi * 0) / 0 = NaN (IEEE, unguarded)
    T = np.diag([1.0, -1.0, -1.0, 1.0])
    x = R.logmap_se3(T)
    assert np.isnan(x[3:]).all()
    # the clamp: a trace above 3 by rounding still takes acos(1) = 0
    T = np.eye(4)
    T[0, 0] = 1.0 + 2 ** -52
    np.testing.assert_array_equal(R.logmap_se3(T)[3:], [0.0, 0.0, 0.0])


# ----------------------------------------------------------- known answers --
def _pose_err(name):
    c = LC.all_cases()[name]
    return float(np.abs(LC.reference(name).T_inc - c.T).max())


WELL_POSED = [f"size_{a}_{b}" for a, b in LC.SIZES if a >= 63]


def test_noise_free_pair_recovers_the_pose():
    """Five iterations from the identity do not converge to rounding: over the sizes family (the
    cases with >= 63 + 64 features; fewer rows leave the pose under-determined) the reference's own
    error max |T_inc - T| is 4.41e-7 (measured: 4.41e-7, 3.66e-7, 3.41e-7, 3.98e-7 for (63, 64),
    (65, 129), (300, 120), (2048, 1024)).  Other seeds get 10 times that."""
    own = max(_pose_err(n) for n in WELL_POSED)
    print("own error over the sizes family:", [(n, _pose_err(n)) for n in WELL_POSED])
    assert own <= 4.41e-7 * 1.001
    cam, cfg = LC.setup()
    for seed, (n_pt, n_ls) in [(101, (63, 64)), (102, (300, 120)), (103, (65, 129))]:
        f0, f1 = LC.make_pair(cam, n_pt, n_ls, seed=seed)
        r = R.is_loop_closure(cam, cfg, f0, f1)
        err = float(np.abs(r.T_inc - LC.T_DEFAULT).max())
        print(seed, n_pt, n_ls, err)
        assert err <= 4.41e-6
        assert r.is_lc and r.gates == 31
        # pose_inc is the inverse motion
        np.testing.assert_allclose(O.expmap_se3(r.pose_inc) @ r.T_inc, np.eye(4), atol=1e-9)


@pytest.mark.parametrize("name", [n for n in LC.all_cases()])
def test_case_takes_its_path(name):
    c, r = LC.all_cases()[name], LC.reference(name)
    x = c.expect
    for k in ("n_pt", "n_ls", "n_pt_inl", "n_ls_inl", "iters", "exit", "gates"):
        if k in x:
            assert getattr(r, k) == x[k], (name, k, getattr(r, k), x[k])
    assert r.is_lc == int(r.gates == 31)
    assert len(r.pt_pairs) == r.n_pt == len(r.pt_inlier) and len(r.ls_pairs) == r.n_ls == len(r.ls_inlier)
    if x.get("all_inliers"):
        assert r.n_pt_inl == r.n_pt and r.n_ls_inl == r.n_ls
    if x.get("e_nan"):
        assert np.isnan(r.e) and np.isnan(r.ratio_inliers) and not r.gates & 1 and not r.gates & 4
    if x.get("identity"):
        np.testing.assert_array_equal(r.T_inc, np.eye(4))
        np.testing.assert_array_equal(r.x_inc, np.zeros(6))
    if "e" in x:
        assert r.e == x["e"]
    if "inlier_row0" in x:
        k = list(r.pt_pairs[:, 0]).index(0)
        assert r.pt_inlier[k] == x["inlier_row0"]
    if not r.is_lc:
        np.testing.assert_array_equal(r.pose_inc, np.zeros(6))


def test_sizes_with_too_few_rows_match_nothing():
    r = LC.reference("size_1_5")
    assert r.n_pt == 0 and r.n_ls == 5   # U4: one point row on each side yields no pairs; the lines match


def test_mutuality_cases_drop_the_broken_rows():
    # duplicate rows 20 / 21 (points) and 40 / 41 (lines) of kf1: the lower index answers, the kf0 row
    # whose partner was overwritten has no mutual match
    r = LC.reference("dup_kf1_desc")
    assert 21 not in r.pt_pairs[:, 1] and 20 in r.pt_pairs[:, 1]
    assert 41 not in r.ls_pairs[:, 1] and 40 in r.ls_pairs[:, 1]
    # the tie: kf0 row 5 takes the lower of its two equidistant kf1 rows
    c, r = LC.all_cases()["knn_tie"], LC.reference("knn_tie")
    for key, pairs in (("pdesc", r.pt_pairs), ("ldesc", r.ls_pairs)):
        d = [O.hamming(c.f0.arr[key][5], c.f1.arr[key][j]) for j in range(64)]
        ties = [j for j in range(64) if d[j] == min(d)]
        assert len(ties) == 2 and min(d) == 8
        row = pairs[list(pairs[:, 0]).index(5)]
        assert row[1] == min(ties)


def test_half_turn_is_rejected():
    r = LC.reference("half_turn")
    assert not r.is_lc and not r.gates & 16 and r.rot > 35.0


def test_below_homog_th_uses_the_threshold():
    c = LC.all_cases()["below_homog_th"]
    cam, cfg = LC.setup()
    gz = c.f0.arr["pt_P"][c.expect["homog_row"]][2]
    assert gz * gz < cfg.homog_th
    other = R.is_loop_closure(cam, gfpl.default_config(homog_th=1e-9), c.f0, c.f1)
    assert not np.array_equal(other.x_inc, LC.reference("below_homog_th").x_inc)


def test_exit_conditions_are_all_taken():
    exits = {LC.reference(n).exit for n in LC.all_cases()}
    assert exits == {R.EXIT_BUDGET, R.EXIT_DE, R.EXIT_E, R.EXIT_X}
    r = LC.reference("stall_exit_de")
    assert 5 < r.iters < 100


# ------------------------------------------------------------ altered rules --
def _differs(a, b):
    return not (np.array_equal(a.x_inc, b.x_inc) and a.e == b.e)


def test_rule_sigma2_is_the_class_default():
    c, cam = LC.all_cases()["gates_all_hold"], LC.setup()[0]
    alt = R.is_loop_closure(cam, gfpl.default_config(), c.f0, c.f1, stereo_sigma2=True)
    assert _differs(alt, LC.reference("gates_all_hold"))


def test_rule_sums_run_in_list_order():
    c, cam = LC.all_cases()["size_300_120"], LC.setup()[0]
    alt = R.is_loop_closure(cam, gfpl.default_config(), c.f0, c.f1, pairwise=True)
    assert _differs(alt, LC.reference("size_300_120"))


def test_rule_outlier_test_is_strict():
    c = LC.all_cases()["on_chi_threshold"]
    cam, _ = LC.setup(c.cam_over)
    ref = LC.reference("on_chi_threshold")
    alt = R.is_loop_closure(cam, gfpl.default_config(max_iters=0), c.f0, c.f1, outlier_ge=True)
    k = list(ref.pt_pairs[:, 0]).index(0)
    assert ref.pt_inlier[k] == 1 and alt.pt_inlier[k] == 0
    assert alt.n_pt_inl == ref.n_pt_inl - 1


def test_rule_budget_is_max_iters():
    c, cam = LC.all_cases()["gates_all_hold"], LC.setup()[0]
    alt = R.is_loop_closure(cam, gfpl.default_config(), c.f0, c.f1, budget_ref=True)
    ref = LC.reference("gates_all_hold")
    assert alt.iters == 10 and ref.iters == 5 and _differs(alt, ref)


# ------------------------------------------------------------------- C ABI --
def test_library_exports_the_loop_closure_call():
    L = gfpl.hiplib()
    assert hasattr(L, "gfpl_kf_loop_closure") and hasattr(L, "gfpl_default_loop_params")
    p = gfpl.LoopParams.default()
    assert (p.lc_res, p.lc_unc, p.lc_inl, p.lc_trs, p.lc_rot) == R.LC_DEFAULTS == (1.5, 0.01, 0.3, 1.5, 35.0)
    assert C.sizeof(gfpl.LoopResult) == 8 * 4 + 8 * (5 + 6 + 6 + 16)
    out = (gfpl.LoopResult * 1)()
    v = (gfpl.KFViewStruct * 1)()
    # a NULL context is refused before any device call
    assert L.gfpl_kf_loop_closure(None, v, v, 1, C.byref(p), 0, 0, None, None, None, None, out) == -1
    assert L.gfpl_kf_loop_closure(None, v, v, 0, C.byref(p), 0, 0, None, None, None, None, out) == -1
    assert L.gfpl_abi_version() == 6
