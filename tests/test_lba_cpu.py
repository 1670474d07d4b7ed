"""tests/lba_ref.py, the Python statement of MapHandler::levMarquardtOptimizationLBA, pinned without a
GPU: hand-worked answers, every ledger rule altered once and shown to change a
result, the `rejects` family, the pinned elimination against numpy.linalg.solve on every system, and the
host-only part of the C ABI (gfpl_lba_check, gfpl_lba_workspace, defaults, exports).
"""
import ctypes as C
import types

import numpy as np
import pytest

import gfpl
import lba_cases as LC
import lba_ref as R

CAM = types.SimpleNamespace(fx=100.0, fy=100.0, cx=320.0, cy=240.0)
HOMOG = 1e-7
EYE = np.eye(4).reshape(1, 16)


def one_point(sigma, P=(1.0, 2.0, 4.0)):
    """local keyframe 0 sees nothing; fixed keyframe 0 (identity) sees the point P once, 3 px left of and
    4 px above its projection"""
    obs = [320.0 + 100.0 * P[0] / P[2] - 3.0, 240.0 + 100.0 * P[1] / P[2] - 4.0]
    return gfpl.LbaProblem(np.zeros((1, 6)), EYE, EYE, [list(P)], np.zeros((0, 6)), [0], [-1], [obs], [sigma],
                           [], [], np.zeros((0, 3)), [])


# ------------------------------------------------------------- hand-worked --
def test_one_fixed_keyframe_one_point_one_observation():
    # d = obs - proj = (-3, -4), |err| = 5; gz2 = 1/16, fx dx = -300, fy dy = -400:
    # J = (-300/16 * 4, -400/16 * 4, -(1/16)(-300 - 800)) = (-75, -100, 68.75); R = I, so J_X = J / 5;
    # sigma = 0.04: w = 1 / (1 + 25 * 0.04) = 0.5
    a = one_point(0.04).a
    lay = R.layout_of(a)
    H, g, esum = R.build_system(CAM, HOMOG, a, lay, None, 0)
    JX = np.array([-15.0, -20.0, 13.75])
    want = np.zeros((9, 9))
    want[6:, 6:] = np.outer(JX, JX) * 0.5
    assert np.array_equal(H, want)
    assert np.array_equal(g, np.concatenate([np.zeros(6), JX * 5.0 * 0.5]))
    assert esum == 12.5
    r = R.lba(CAM, HOMOG, a, (0.001, 10.0, 1))
    assert r.err == np.inf and r.err_prev == np.inf      # 12.5 / (0 + 0)
    assert r.hmax == 200 and r.lambda_ == np.float64(0.001) * 200.0   # the largest diagonal is 20^2 * 0.5
    assert r.status == R.SINGULAR and r.iters == 1         # the unobserved keyframe's block is zero


def test_hmax_truncates_5_9_to_5():
    r = R.lba(CAM, HOMOG, one_point(2.68).a, (0.001, 10.0, 1))   # w = 1 / 68, max diagonal 400 / 68 = 5.88
    assert r.hmax == 5 and r.lambda_ == np.float64(0.001) * 5.0


def test_hmax_below_one_gives_lambda_zero_for_good():
    r = R.lba(CAM, HOMOG, one_point(17.76).a, (0.001, 10.0, 5))   # w = 1 / 445, max diagonal 0.899
    assert r.hmax == 0 and r.lambda_ == 0.0


def test_hmax_out_of_int_range_is_a_status():
    # 1 mm in front of the camera: gz2 = 1e6, J_X[0] = (1e6 * -300) * 1e-3 / 5 = -6e4, w = 1: a diagonal of 3.6e9 >= 2^31
    p = one_point(0.0, P=(0.0, 0.0, 0.001))
    r = R.lba(CAM, HOMOG, p.a, (0.001, 10.0, 5))
    assert r.status == R.HMAX_RANGE and r.iters == 1 and r.hmax == 0x7FFFFFFF
    assert np.array_equal(r.pt, p.a["pt"]) and np.array_equal(r.T_kf.reshape(-1, 16), p.a["T_kf"])


def test_exact_zero_residual_has_a_nan_err_prev_and_ends_at_iteration_1():
    r = LC.reference(LC.all_cases()["zero_residual"])
    assert np.isnan(r.err_prev) and r.iters == 1 and r.stop == R.STOP_ERR
    assert r.status == R.SINGULAR   # H = 0: the first solve is dropped, X stays (ledger BA13)


def test_add_at_is_the_list_order_loop():
    c = LC.all_cases()["twice_by_one_keyframe"]
    cam, cfg = LC.setup()
    a, lay = c.prob.a, R.layout_of(c.prob.a)
    H, g, _ = R.build_system(cam, cfg.homog_th, a, lay, None, 0)
    Ti = {s: R.O.inverse_se3(T.reshape(4, 4)) for s, T in enumerate(a["T_kf"])}
    Ti.update({-1 - f: R.O.inverse_se3(T.reshape(4, 4)) for f, T in enumerate(a["T_fix"])})
    H2, g2 = np.zeros_like(H), np.zeros_like(g)
    for o in range(len(a["pt_obs_lm"])):
        j, s = int(a["pt_obs_lm"][o]), int(a["pt_obs_kf"][o])
        JT, JL, nrm, w = R.point_rows(cam, np.float64(cfg.homog_th), Ti[s][None], a["pt"][j][None], a["pt_obs"][o][None],
                                      a["pt_sigma"][o])
        jd = 6 * lay.nkf + 3 * j
        g2[jd:jd + 3] += JL[0] * nrm[0] * w[0]
        H2[jd:jd + 3, jd:jd + 3] += np.outer(JL[0], JL[0]) * w[0]
        if s >= 0:
            g2[6 * s:6 * s + 6] += JT[0] * nrm[0] * w[0]
            H2[6 * s:6 * s + 6, 6 * s:6 * s + 6] += np.outer(JT[0], JT[0]) * w[0]
            H2[jd:jd + 3, 6 * s:6 * s + 6] += np.outer(JL[0], JT[0]) * w[0]
            H2[6 * s:6 * s + 6, jd:jd + 3] += (np.outer(JL[0], JT[0]) * w[0]).T
    n = 6 * lay.nkf + 3 * lay.npt
    assert np.array_equal(H[:n, 6 * lay.nkf:n], H2[:n, 6 * lay.nkf:n])     # every entry the points alone feed
    assert np.array_equal(g[6 * lay.nkf:n], g2[6 * lay.nkf:n])


# ------------------------------------------------------------ altered rules --
def _differs(a, b):
    return (a.iters, a.stop, a.status, a.hmax, a.rejected) != (b.iters, b.stop, b.status, b.hmax, b.rejected) or \
        not np.array_equal(a.X, b.X) or a.lambda_ != b.lambda_ or not (a.err == b.err)


@pytest.mark.parametrize("case,rule", [
    ("both", "lines_read_x"),
    ("both", "hmax_double"),
    ("points_only", "finite_first"),
    ("rejects_304", "apply_on_reject"),
    ("points_only", "divisor_obs"),
    ("stale_x_kf", "x_from_T"),
])
def test_an_altered_rule_changes_a_result(case, rule):
    c = LC.all_cases()[case]
    assert _differs(LC.reference(c), LC.reference(c, **{rule: True})), (case, rule)


def test_consistent_x_kf_makes_x_from_T_no_change():
    c = LC.all_cases()["points_only"]          # x_kf = logmap(T_kf) there: the rule only shows on a stale x_kf
    assert not _differs(LC.reference(c), LC.reference(c, x_from_T=True))


def test_rejects_family_takes_err_above_err_prev():
    for s in LC.REJECT_SEEDS:
        assert LC.reference(LC.all_cases()[f"rejects_{s}"]).rejected >= 1, s


def test_stop_3_is_reached_while_the_error_still_changes():
    r = LC.reference(LC.all_cases()["points_only"])
    assert r.stop == R.STOP_STEP and abs(r.err - r.err_prev) >= R.EPS


# ------------------------------------------------------------------ solvers --
def solver_figures(case):
    """per solved system of the case: (N, eta_pinned, eta_dense, relative difference of the solutions)"""
    cam, cfg = LC.setup(case.cam_over)
    ref = R.lba(cam, cfg.homog_th, case.prob.a, case.prm, keep=True)
    lay = R.layout_of(case.prob.a)
    out = []
    for s in ref.systems:
        if not s.get("ok"):
            continue
        Hd, g, d = s["Hd"], s["g"], s["DX"]
        dd, okd, _ = R.solve_dense(Hd, g, lay)
        assert okd
        hn = np.max(np.abs(np.linalg.eigvalsh(Hd)))
        eta = lambda x: np.linalg.norm(Hd @ x - g) / (hn * np.linalg.norm(x) + np.linalg.norm(g))
        out.append((lay.N, eta(d), eta(dd), np.linalg.norm(d - dd) / np.linalg.norm(dd)))
    return out


@pytest.mark.parametrize("name", list(LC.all_cases()))
def test_pinned_and_dense_solves_are_backward_stable(name):
    """eta = |H d - g| / (|H| |d| + |g|) <= N 2^-53, the a-priori bound of a Cholesky-type solve, for both
    solvers on every system a case solves.  Observed maxima over all cases (profiles/lba/solver_agreement.txt):
    see that file."""
    for N, ep, ed, rel in solver_figures(LC.all_cases()[name]):
        print(f"{name} N {N} eta_pinned {ep:.3e} eta_dense {ed:.3e} rel_diff {rel:.3e}")
        assert ep <= N * 2.0 ** -53, (name, N, ep)
        assert ed <= N * 2.0 ** -53, (name, N, ed)


# ------------------------------------------------------------------ the ABI --
def _problem(pt_lm, pt_kf, ls_lm=(), ls_kf=(), n_kf=2, n_fix=1, n_pt=None, n_ls=None):
    n_pt = (max(pt_lm) + 1 if len(pt_lm) else 0) if n_pt is None else n_pt
    n_ls = (max(ls_lm) + 1 if len(ls_lm) else 0) if n_ls is None else n_ls
    return gfpl.LbaProblem(np.zeros((n_kf, 6)), np.tile(EYE, (n_kf, 1)), np.tile(EYE, (n_fix, 1)), np.zeros((n_pt, 3)),
                           np.zeros((n_ls, 6)), pt_lm, pt_kf, np.zeros((len(pt_lm), 2)), np.ones(len(pt_lm)), ls_lm, ls_kf,
                           np.zeros((len(ls_lm), 3)), np.ones(len(ls_lm)))


def test_check_accepts_and_refuses():
    assert _problem([0, 0, 1], [0, -1, 1], [0, 1, 1], [1, 1, -1]).check() == 0
    assert _problem([1, 1, 2], [0, 0, 0], n_pt=3).check() == -1            # ids do not start at 0
    assert _problem([0, 2], [0, 0]).check() == -1                          # a step of 2
    assert _problem([0, 1, 0], [0, 0, 0]).check() == -1                    # falling
    assert _problem([0, 1], [0, 0], n_pt=3).check() == -1                  # landmark 2 has no observation
    assert _problem([0], [2]).check() == -1                                # slot = n_kf
    assert _problem([0], [-2]).check() == -1                               # fixed pose 1 of 1
    assert _problem([0], [-1], n_fix=0).check() == -1
    assert _problem([0], [0], n_kf=0).check() == -1                        # Nkf < 1
    assert _problem([], []).check() == -1                                  # no observation at all
    assert _problem([], [], [0], [0]).check() == 0                         # lines alone are a problem
    assert _problem([0], [0], n_kf=gfpl.LBA_MAX_KFS + 1).check() == -5
    assert gfpl.hiplib().gfpl_lba_check(None) == -1


def test_workspace_lds_bound_monotone_and_capacity():
    prev = 0
    for n_kf in range(1, gfpl.LBA_MAX_KFS + 1):
        rc, hbm, lds = gfpl.lbaWorkspace(n_kf, 2, 300, 65, 1200, 260)
        assert rc == 0 and lds > prev and hbm > 0
        prev = lds
    assert prev <= 163840
    assert gfpl.lbaWorkspace(gfpl.LBA_MAX_KFS + 1, 2, 300, 65, 1200, 260)[0] == -5
    assert gfpl.lbaWorkspace(0, 2, 300, 65, 1200, 260)[0] == -1
    small, big = gfpl.lbaWorkspace(4, 0, 10, 0, 30, 0)[1], gfpl.lbaWorkspace(4, 0, 11, 0, 33, 0)[1]
    assert big >= small


def test_exports_and_defaults():
    L = gfpl.hiplib()
    for n in ("gfpl_default_lba_params", "gfpl_lba_check", "gfpl_lba_workspace", "gfpl_lba_create", "gfpl_lba_destroy",
              "gfpl_lba_solve", "gfpl_lba_debug_system"):
        assert hasattr(L, n), n
    p = gfpl.LbaParams.default()
    assert (p.lambda_lm, p.lambda_k, p.max_iters) == R.LBA_DEFAULTS == (0.001, 10.0, 20)
    assert C.sizeof(gfpl.LbaResult) == 40 and C.sizeof(gfpl.LbaParams) == 24
    assert L.gfpl_abi_version() == 6
