"""tests/gba_ref.py, the Python statement of MapHandler::levMarquardtOptimizationGBA, pinned without a
GPU: hand-worked answers, the `+=` order against a plain loop, every ledger rule
altered once and shown to change a result of a named case, the consequences of the zero divisor, the
negative pivots of the pre-pass, the pinned elimination against numpy.linalg.solve, the planner and the
layouts as stand-alone programs under ASan + UBSan (nothing is preloaded; no Python-loaded code runs
under a sanitizer), and the host-only part of the C ABI.
"""
import os
import subprocess
import types

import numpy as np
import pytest

import gfpl
import gba_cases as GC
import gba_ref as G
import lba_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = types.SimpleNamespace(fx=100.0, fy=100.0, cx=320.0, cy=240.0)
HOMOG = 1e-7
EYE = np.eye(4).reshape(1, 16)


def one_point(sigma, P=(1.0, 2.0, 4.0)):
    """local keyframe 0 sees nothing; keyframe 0 of the map (fixed, identity) sees the point P once,
    3 px left of and 4 px above its projection"""
    obs = [320.0 + 100.0 * P[0] / P[2] - 3.0, 240.0 + 100.0 * P[1] / P[2] - 4.0]
    return gfpl.LbaProblem(np.zeros((1, 6)), EYE, EYE, [list(P)], np.zeros((0, 6)), [0], [-1], [obs], [sigma],
                           [], [], np.zeros((0, 3)), [])


# ------------------------------------------------------------- hand-worked --
def test_one_fixed_keyframe_one_point_one_observation():
    # d = (-3, -4), |err| = 5; gz2 = 1/16, fx dx = -300, fy dy = -400:
    # J = (-300/16 * 4, -400/16 * 4, -(1/16)(-300 - 800)) = (-75, -100, 68.75); R = I, so J_X = J / 5 = (-15, -20, 13.75);
    # sigma = 0.04: w = 1 / (1 + 25 * 0.04) = 0.5
    a = one_point(0.04).a
    lay = R.layout_of(a)
    H, g, esum = G.build_system(CAM, HOMOG, a, lay, None, 0)
    JX = np.array([-15.0, -20.0, 13.75])
    assert np.array_equal(H[6:9, 6:9], np.outer(JX, JX) * 0.5)
    assert np.array_equal(g[6:9], JX * 5.0 * 0.5)
    assert not H[:6].any() and not H[:, :6].any() and esum == 12.5
    r = G.gba(CAM, HOMOG, a, (0.001, 10.0, 1))
    assert r.err == np.inf and r.err_prev == np.inf          # 12.5 / (0 + 0)
    assert r.hmax == 200 and r.lambda_ == np.float64(0.001) * 200.0
    assert r.status == G.SINGULAR and r.iters == 1             # the unobserved keyframe's block is zero: X kept
    assert np.array_equal(r.pt, a["pt"])


def test_hmax_truncates_and_leaves_the_int_range():
    assert G.gba(CAM, HOMOG, one_point(2.68).a, (0.001, 10.0, 1)).hmax == 5     # 400 / 68 = 5.88
    p = one_point(0.0, P=(0.0, 0.0, 0.001))
    r = G.gba(CAM, HOMOG, p.a, (0.001, 10.0, 5))
    assert r.status == G.HMAX_RANGE and r.iters == 1 and r.hmax == 0x7FFFFFFF
    assert np.array_equal(r.pt, p.a["pt"])


def _loop_system(cam, homog, a, lay, it, X):
    """H and g by a plain Python loop over the two lists, written as the reference's text has it"""
    N, nkf, npt = lay.N, lay.nkf, lay.npt
    H, g = np.zeros((N, N)), np.zeros(N)
    Ti = {s: R.O.inverse_se3(T.reshape(4, 4)) for s, T in enumerate(a["T_kf"])}
    Ti.update({-1 - f: R.O.inverse_se3(T.reshape(4, 4)) for f, T in enumerate(a["T_fix"])})
    Tx = dict(Ti)
    if it > 0:
        Tx.update({s: R.O.inverse_se3(R.O.expmap_se3(X[6 * s:6 * s + 6])) for s in range(nkf)})
    th = np.float64(homog)
    for o in range(len(a["pt_obs_lm"])):
        j, s = int(a["pt_obs_lm"][o]), int(a["pt_obs_kf"][o])
        Xw = X[6 * nkf + 3 * j:6 * nkf + 3 * j + 3] if it > 0 else a["pt"][j]
        JT, JL, nrm, w = R.point_rows(cam, th, Tx[s][None], Xw[None], a["pt_obs"][o][None], a["pt_sigma"][o])
        JT, JL, nrm, w = JT[0], JL[0], nrm[0], w[0]
        jd = 6 * nkf + 3 * j
        for i in range(3):
            g[jd + i] += (JL[i] * nrm) * w
            for k in range(3):
                H[jd + i, jd + k] += (JL[i] * JL[k]) * w
        if s >= 0:
            for i in range(6):
                g[6 * s + i] += (JT[i] * nrm) * w
                for k in range(6):
                    H[6 * s + i, 6 * s + k] += (JT[i] * JT[k]) * w
            for i in range(3):
                for k in range(6):
                    H[jd + i, 6 * s + k] += (JL[i] * JT[k]) * w      # :2070
                    H[6 * s + k, jd + i] += (JL[i] * JT[k]) * w      # :2071
    for o in range(len(a["ls_obs_lm"])):
        j, s = int(a["ls_obs_lm"][o]), int(a["ls_obs_kf"][o])
        JT, JL, nrm, w = R.line_rows(cam, th, Ti[s][None], a["ls"][j][None], a["ls_obs"][o][None], a["ls_sigma"][o])
        JT, JL, nrm, w = JT[0], JL[0], nrm[0], w[0]
        jd = 6 * nkf + 3 * npt + 6 * j
        for i in range(6):
            g[jd + i] += (JL[i] * nrm) * w
            for k in range(6):
                H[jd + i, jd + k] += (JL[i] * JL[k]) * w
        if s >= 0:
            Hij = np.array([[(JL[i] * JT[k]) * w for k in range(6)] for i in range(6)])
            for i in range(6):
                g[6 * s + i] += (JT[i] * nrm) * w
                for k in range(6):
                    H[6 * s + i, 6 * s + k] += (JT[i] * JT[k]) * w
                    H[6 * s + i, jd + k] += Hij[i, k]                                   # :2197 / :2472
                    H[jd + k, 6 * s + i] += Hij[i, k] if it == 0 else Hij[k, i]         # :2198 / :2473
    return H, g


@pytest.mark.parametrize("it", (0, 1))
def test_add_at_is_the_list_order_loop(it):
    c = GC.all_cases()["twice_by_one_keyframe"]
    cam, cfg = GC.setup()
    a, lay = c.prob.a, R.layout_of(c.prob.a)
    X = GC.reference(c, prm=(0.001, 10.0, 1)).X if it else None
    H, g, _ = G.build_system(cam, cfg.homog_th, a, lay, X, it)
    H2, g2 = _loop_system(cam, cfg.homog_th, a, lay, it, X)
    assert np.array_equal(H, H2) and np.array_equal(g, g2)
    n6 = 6 * lay.nkf
    lines = slice(n6 + 3 * lay.npt, lay.N)
    if it == 0:
        assert np.array_equal(H[lines, :n6], H[:n6, lines].T)          # symmetric, and both wrong
    else:
        assert not np.array_equal(H[lines, :n6], H[:n6, lines].T)      # the lower block right, the upper not


# ------------------------------------------------------------ altered rules --
def _differs(a, b):
    return (a.iters, a.stop, a.status, a.hmax) != (b.iters, b.stop, b.status, b.hmax) or \
        not np.array_equal(a.X, b.X, equal_nan=True) or a.lambda_ != b.lambda_ or \
        np.float64(a.err).tobytes() != np.float64(b.err).tobytes()


ALTERED = [
    ("points_only", dict(divisor_zero=False), None),          # GB3: the divisor
    ("lines_small_lambda", dict(prepass_transposed=False), None),   # GB5: the pre-pass coupling
    ("both", dict(lower_triangle=False), None),               # GB6: which triangle the solve reads
    ("both", dict(line_th_homog=False), 5.0),                 # GB7: homogTh in the iterations' line terms (homogTh = 5)
    ("lines_small_lambda", dict(any_sign_pivot=False), None), # GB9: the pivot sign rule
    ("stale_x_kf", dict(x_from_T=True), None),                # GB1: x_kf_w, not logmap(T_kf_w)
]


@pytest.mark.parametrize("case,rule,homog", ALTERED)
def test_an_altered_rule_changes_a_result(case, rule, homog):
    c = GC.all_cases()[case]
    cam, cfg = GC.setup(c.cam_over)
    h = cfg.homog_th if homog is None else homog
    base = G.gba(cam, h, c.prob.a, c.prm)
    alt = G.gba(cam, h, c.prob.a, c.prm, rules=G.Rules(**rule))
    assert _differs(base, alt), (case, rule)


def test_the_err_start_shows_on_an_exactly_zero_sum():
    """GB2: `double err` is uninitialised; pinned to 0.0.  Only an exactly zero sum tells a start of 0
    (0 / 0 = NaN) from any positive one (+inf)"""
    c = GC.all_cases()["zero_residual"]
    cam, cfg = GC.setup()
    base = G.gba(cam, cfg.homog_th, c.prob.a, (0.001, 10.0, 1))
    alt = G.gba(cam, cfg.homog_th, c.prob.a, (0.001, 10.0, 1), rules=G.Rules(err_start=1.0))
    assert np.isnan(base.err) and alt.err == np.inf


def test_consistent_x_kf_makes_x_from_T_no_change():
    c = GC.all_cases()["points_only"]
    assert not _differs(GC.reference(c), GC.reference(c, rules=G.Rules(x_from_T=True)))


@pytest.mark.parametrize("name", list(GC.all_cases()))
def test_zero_divisor_consequences(name):
    """GB3: err is +inf or NaN in every iteration, neither error stop fires, no step is rejected, lambda
    is multiplied every iteration, and a problem ends by |DX| < eps or by running out of iterations"""
    c = GC.all_cases()[name]
    r = GC.reference(c, keep=True)
    assert all(np.isinf(s["err"]) and s["err"] > 0 or np.isnan(s["err"]) for s in r.systems)
    assert r.stop in (G.STOP_ITERS, G.STOP_STEP) and r.rejected == 0
    if not r.status & G.HMAX_RANGE:
        solved = len(r.negative)
        want = np.float64(c.prm[0]) * np.float64(r.hmax)
        for _ in range(solved - 1):
            want = want * np.float64(c.prm[1])
        assert r.lambda_ == want


def test_prepass_is_indefinite_with_lines_only():
    neg = {n: GC.reference(GC.all_cases()[n]).negative for n in GC.all_cases()}
    assert any(neg[n][0] > 0 for n in ("lines_small_lambda", "both_small_lambda"))
    for n in GC.points_only():
        assert not any(neg[n]), n
    for n, v in neg.items():
        assert not any(v[1:]), n     # the iterations write the block under the diagonal right


# ------------------------------------------------------------------ solvers --
AGREEMENT = list(GC.all_cases())
_agreement_cache = {}


def _agreement(name):
    """per solved system of the case without a negative pivot: (iteration, N, eta_pinned, eta_dense); and the
    iterations of the systems with one.  eta = |H d - g| / (|H|_2 |d| + |g|), H rebuilt from the lower triangle"""
    if name not in _agreement_cache:
        c = GC.all_cases()[name]
        ref = GC.reference(c, keep=True)
        lay = R.layout_of(c.prob.a)
        rows, left_out = [], []
        for s in ref.systems:
            if not s.get("ok"):
                continue
            if s["negative"]:
                left_out.append(s["it"])
                continue
            Hs = np.tril(s["Hd"]) + np.tril(s["Hd"], -1).T
            g, d = s["g"], s["DX"]
            dd, okd, _, _ = G.solve_dense(s["Hd"], g, lay)
            assert okd
            hn = np.max(np.abs(np.linalg.eigvalsh(Hs)))
            eta = lambda x: np.linalg.norm(Hs @ x - g) / (hn * np.linalg.norm(x) + np.linalg.norm(g))
            rows.append((s["it"], lay.N, eta(d), eta(dd)))
        _agreement_cache[name] = (rows, left_out)
    return _agreement_cache[name]


@pytest.mark.parametrize("name", AGREEMENT)
def test_pinned_and_dense_solves_are_backward_stable(name):
    """eta <= N 2^-53 (the bound tests/test_lba_cpu.py uses) for both solvers on every system WITHOUT a
    negative pivot.  Systems with one are left out (no such bound exists for an unpivoted LDL^T of an
    indefinite matrix) and counted; none of a case without lines and none of an iteration >= 1 may be.

    The landmark blocks go through their own LDL^T (ledger GB11): with the LBA's explicit inverse3 the case
    `lambda_0` misses this bound (test_explicit_inverse_of_the_landmark_blocks_misses_the_bound)."""
    rows, left_out = _agreement(name)
    assert all(it == 0 for it in left_out), (name, left_out)
    if len(GC.all_cases()[name].prob.a["ls"]) == 0:
        assert not left_out, (name, left_out)
    for it, N, ep, ed in rows:
        print(f"{name} it {it} N {N} eta_pinned {ep:.3e} eta_dense {ed:.3e}")
        assert ep <= N * 2.0 ** -53, (name, it, ep)
        assert ed <= N * 2.0 ** -53, (name, it, ed)
    print(f"{name}: {len(left_out)} system(s) with a negative pivot left out of the bound")


def test_fixed_only_landmarks_reach_the_solve():
    """landmarks seen by fixed poses only go through the elimination: the case has such landmarks, and solved systems"""
    c = GC.all_cases()["fixed_only_landmarks"]
    lay = R.layout_of(c.prob.a)
    assert sum(1 for m in lay.masks if not m) >= 7 and all(len(m) for m in lay.masks if m)
    ref = GC.reference(c, keep=True)
    assert not ref.status & G.SINGULAR and len(ref.systems) >= 3 and all(s["ok"] for s in ref.systems)
    free = [j for j, m in enumerate(lay.masks) if not m]
    r0 = lay.lm(free[0])[0]
    assert np.any(ref.systems[0]["DX"][r0:r0 + 3] != 0.0) and not np.array_equal(ref.pt[free[0]], c.prob.a["pt"][free[0]])


def test_explicit_inverse_of_the_landmark_blocks_misses_the_bound():
    """GB11: why the GBA does not take BA12's inverse3 / inverse6.  `lambda_0` (lambda = 0, every step applied)
    never settles; where a point's 3 x 3 block is worst conditioned the products with its explicit inverse
    leave the bound by orders of magnitude, the block's own LDL^T with substitutions stays inside it."""
    c = GC.all_cases()["lambda_0"]
    cam, cfg = GC.setup()
    lay = R.layout_of(c.prob.a)
    ref = G.gba(cam, cfg.homog_th, c.prob.a, c.prm, keep=True, rules=G.Rules(explicit_inverse=True))
    n6 = 6 * lay.nkf
    cond = lambda s: max(np.linalg.cond(s["Hd"][n6 + 3 * j:n6 + 3 * j + 3, n6 + 3 * j:n6 + 3 * j + 3]) for j in range(lay.npt))
    s = max((s for s in ref.systems if s.get("ok")), key=cond)
    Hs = np.tril(s["Hd"]) + np.tril(s["Hd"], -1).T
    hn = np.max(np.abs(np.linalg.eigvalsh(Hs)))
    eta = lambda x: np.linalg.norm(Hs @ x - s["g"]) / (hn * np.linalg.norm(x) + np.linalg.norm(s["g"]))
    factored = G.solve_pinned(s["Hd"], s["g"], lay)[0]
    print(f"iteration {s['it']}: largest block condition {cond(s):.3e}, eta explicit {eta(s['DX']):.3e}, factored {eta(factored):.3e}")
    assert cond(s) > 1e7
    assert eta(s["DX"]) > 10 * lay.N * 2.0 ** -53
    assert eta(factored) <= lay.N * 2.0 ** -53
    assert _differs(ref, GC.reference(c))      # and the rule changes the case's result


def test_left_out_count_is_written():
    """the count of systems left out of the bound and every system's figures, printed and written to
    profiles/gba/solver_agreement.txt (rewritten only when its contents change)"""
    total, lines, worst = 0, [], []
    for n in AGREEMENT:
        rows, left_out = _agreement(n)
        total += len(left_out)
        for it, N, ep, ed in rows:
            lines.append(f"{n} it {it} N {N} eta_pinned {ep:.3e} eta_dense {ed:.3e}")
            worst.append((ep / (N * 2.0 ** -53), lines[-1]))
        lines.append(f"{n}: {len(left_out)} system(s) with a negative pivot left out of the bound")
    print(f"systems with a negative pivot left out of the backward-error bound: {total}")
    text = ("tests/test_gba_cpu.py::test_left_out_count_is_written, every case of tests/gba_cases.py\n"
            "eta = |H d - g| / (|H|_2 |d| + |g|), bound N 2^-53, H rebuilt from the lower triangle of the damped system\n"
            f"systems with a negative pivot, left out: {total}\n"
            "(all of them pre-pass systems of cases with lines; none of a case without lines, none of an iteration >= 1)\n"
            "every other system is inside the bound\n\nthe eight largest eta_pinned / bound:\n"
            + "".join(f"  {r:9.5f}  {l}\n" for r, l in sorted(worst, reverse=True)[:8]) + "\nper system:\n" + "\n".join(lines) + "\n")
    path = os.path.join(ROOT, "profiles", "gba", "solver_agreement.txt")
    old = open(path).read() if os.path.exists(path) else ""
    if old != text:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    assert f"left out: {total}" in open(path).read() and total >= 1


# ------------------------------------------------- stand-alone, sanitised --
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include")]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


def _build(tmp, name, sources):
    exe = str(tmp / name)
    r = subprocess.run(SAN + sources + ["-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r.stdout


def _python_plan(a):
    """the planner's lists from the arrays of an LbaProblem, by the statement of include/gfpl.h"""
    lay = R.layout_of(a)
    nkf, npt = lay.nkf, lay.npt
    obs_lm = [int(j) for j in a["pt_obs_lm"]] + [npt + int(j) for j in a["ls_obs_lm"]]
    obs_kf = [int(s) for s in a["pt_obs_kf"]] + [int(s) for s in a["ls_obs_kf"]]
    nlm = npt + lay.nls
    lm_start = [obs_lm.index(j) for j in range(nlm)] + [len(obs_lm)]
    pair_start, pair_kf = [0], []
    for j in range(nlm):
        pair_kf += lay.masks[j]
        pair_start.append(len(pair_kf))
    obs_pair = [pair_start[j] + lay.masks[j].index(s) if s >= 0 else -1 for j, s in zip(obs_lm, obs_kf)]
    by_kf = [[o for o, s in enumerate(obs_kf) if s == k] for k in range(nkf)]
    kf_start = [0]
    for l in by_kf:
        kf_start.append(kf_start[-1] + len(l))
    blocks = {}
    for j in range(nlm):
        for ia, sa in enumerate(lay.masks[j]):
            for ib, sb in enumerate(lay.masks[j][:ia + 1]):
                blocks.setdefault(sa * (sa + 1) // 2 + sb, []).append((j, pair_start[j] + ia, pair_start[j] + ib))
    blk_start, terms = [0], []
    for b in range(nkf * (nkf + 1) // 2):
        terms += [v for t in blocks.get(b, []) for v in t]
        blk_start.append(len(terms) // 3)
    npp = pair_start[npt]
    return dict(counts=[npp, len(pair_kf) - npp, len(terms) // 3], lm_start=lm_start, obs_lm=obs_lm, obs_kf=obs_kf,
                obs_pair=obs_pair, pair_start=pair_start, pair_kf=pair_kf, kf_start=kf_start,
                kf_obs=[o for l in by_kf for o in l], blk_start=blk_start, terms=terms)


PLAN_CASES = ("twice_by_one_keyframe", "fixed_only_landmarks", "seen_by_all_70", "no_common_landmark", "idle_keyframe",
              "size_kf2_pt0_ls1", "size_kf17_pt65_ls65")
BAD_PLANS = [  # (n_kf n_fix n_pt n_ls, pt_lm, pt_kf, ls_lm, ls_kf, rc)
    ((0, 1, 1, 0), [0], [-1], [], [], -1), ((2, 1, 1, 0), [0], [2], [], [], -1), ((2, 1, 1, 0), [0], [-2], [], [], -1),
    ((2, 1, 2, 0), [0, 0], [0, 1], [], [], -1), ((2, 1, 0, 0), [], [], [], [], -1), ((2, 1, 2, 0), [1, 0], [0, 0], [], [], -1),
    ((gfpl.GBA_MAX_KFS + 1, 1, 1, 0), [0], [0], [], [], -5), ((gfpl.GBA_MAX_KFS, 1, 0, 1), [], [], [0], [255], 0),
]


def test_planner_under_asan_equals_the_python_plan(tmp_path):
    exe = _build(tmp_path, "gba_plan_asan", [os.path.join(ROOT, "tests", "gba_plan_main.cpp"),
                                             os.path.join(ROOT, "gf-pl-slam_amd", "csrc", "gfpl_gba_plan.cpp")])
    flat = lambda v: " ".join(str(int(x)) for x in v)
    path = tmp_path / "problems.txt"
    arrays = [GC.all_cases()[n].prob.a for n in PLAN_CASES]
    with open(path, "w") as f:
        f.write(f"{len(arrays) + len(BAD_PLANS)}\n")
        for a in arrays:
            f.write(flat([len(a["x_kf"]), len(a["T_fix"]), len(a["pt"]), len(a["ls"]), len(a["pt_obs_lm"]), len(a["ls_obs_lm"])]) + "\n")
            for k in ("pt_obs_lm", "pt_obs_kf", "ls_obs_lm", "ls_obs_kf"):
                f.write(flat(a[k]) + "\n")
        for (n, plm, pkf, llm, lkf, _) in BAD_PLANS:
            f.write(flat(list(n) + [len(plm), len(llm)]) + "\n")
            for v in (plm, pkf, llm, lkf):
                f.write(flat(v) + "\n")
    out = _run([exe, str(path)]).rstrip("\n").split("\n")
    k = 0
    for n, a in zip(PLAN_CASES, arrays):
        assert out[k] == "rc 0", (n, out[k])
        want = _python_plan(a)
        for key in ("counts", "lm_start", "obs_lm", "obs_kf", "obs_pair", "pair_start", "pair_kf", "kf_start", "kf_obs",
                    "blk_start", "terms"):
            k += 1
            w = out[k].split()
            assert w[0] == key and [int(x) for x in w[1:]] == want[key], (n, key)
        k += 1
        rc, cnt = gfpl.gbaCheck(GC.all_cases()[n].prob)      # the library's entry point agrees with the program
        assert rc == 0 and [cnt.n_pt_pairs, cnt.n_ls_pairs, cnt.n_terms] == want["counts"]
    for bad in BAD_PLANS:
        assert out[k] == f"rc {bad[5]}", (bad, out[k])
        k += 12 if bad[5] == 0 else 1
    assert k == len(out)


LAYOUT_SHAPES = [(1, 1, 0, 1, 1, 0, 1, 1), (17, 65, 65, 390, 169, 181, 664, 6), (70, 41, 2, 263, 150, 72, 5093, 24),
                 (256, 1000, 333, 5001, 4000, 1300, 20011, 6)]


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=["smallest", "odd", "seventy", "cap"])
def test_layouts_under_asan(tmp_path, shape):
    exe = _build(tmp_path, "gba_layout_check", [os.path.join(ROOT, "tests", "gba_layout_check.cpp")])
    fields, total = {}, {}
    for line in _run([exe] + [str(v) for v in shape]).strip().split("\n"):
        w = line.split()
        if w[1] == "bytes":
            assert w[2] == w[3], line
            total[w[0]] = int(w[2])
        else:
            fields.setdefault(w[0], []).append((w[1], int(w[2]), int(w[3]), int(w[4])))
    assert set(fields) == set(total) == {"GbaMem", "GbaIdx", "GbaLdltLds", "GbaSubstLds"}
    for lay, fs in fields.items():
        end = 0
        for name, off, nbytes, align in fs:
            assert off % align == 0 and off >= end, (lay, name, off, align, end)
            if lay in ("GbaMem", "GbaIdx"):
                assert off % 256 == 0, (lay, name, off)
            end = off + nbytes
        assert end <= total[lay], (lay, end, total[lay])
    assert max(total["GbaLdltLds"], total["GbaSubstLds"]) <= 64 * 1024
    n_kf, n_pt, n_ls, n_obs, npp, nlp, nt, _ = shape
    rc, hbm, lds = gfpl.gbaWorkspace([n_kf, 1, n_pt, n_ls, n_obs, 0, npp, nlp, nt])
    assert rc == 0 and hbm == total["GbaMem"] + total["GbaIdx"] and lds >= total["GbaSubstLds"]


# ------------------------------------------------------------------ the ABI --
def _problem(pt_lm, pt_kf, ls_lm=(), ls_kf=(), n_kf=2, n_fix=1, n_pt=None, n_ls=None):
    n_pt = (max(pt_lm) + 1 if len(pt_lm) else 0) if n_pt is None else n_pt
    n_ls = (max(ls_lm) + 1 if len(ls_lm) else 0) if n_ls is None else n_ls
    return gfpl.LbaProblem(np.zeros((n_kf, 6)), np.tile(EYE, (n_kf, 1)), np.tile(EYE, (n_fix, 1)), np.zeros((n_pt, 3)),
                           np.zeros((n_ls, 6)), pt_lm, pt_kf, np.zeros((len(pt_lm), 2)), np.ones(len(pt_lm)), ls_lm, ls_kf,
                           np.zeros((len(ls_lm), 3)), np.ones(len(ls_lm)))


def test_check_accepts_and_refuses():
    rc, c = gfpl.gbaCheck(_problem([0, 0, 1], [0, -1, 1], [0, 1, 1], [1, 1, -1]))
    assert rc == 0 and (c.n_pt_pairs, c.n_ls_pairs, c.n_terms) == (2, 2, 4)     # four landmarks, one local keyframe each
    rc, c = gfpl.gbaCheck(_problem([0, 0, 0, 0], [1, 0, 1, -1]))
    assert rc == 0 and (c.n_pt_pairs, c.n_ls_pairs, c.n_terms) == (2, 0, 3)     # blocks (0,0), (1,0), (1,1)
    assert gfpl.gbaCheck(_problem([1, 1, 2], [0, 0, 0], n_pt=3))[0] == -1
    assert gfpl.gbaCheck(_problem([0, 2], [0, 0]))[0] == -1
    assert gfpl.gbaCheck(_problem([0, 1, 0], [0, 0, 0]))[0] == -1
    assert gfpl.gbaCheck(_problem([0, 1], [0, 0], n_pt=3))[0] == -1
    assert gfpl.gbaCheck(_problem([0], [2]))[0] == -1
    assert gfpl.gbaCheck(_problem([0], [-2]))[0] == -1
    assert gfpl.gbaCheck(_problem([], []))[0] == -1
    assert gfpl.gbaCheck(_problem([], [], [0], [0]))[0] == 0
    assert gfpl.gbaCheck(_problem([0], [0], n_kf=gfpl.LBA_MAX_KFS + 1))[0] == 0        # beyond the LBA's cap
    assert _problem([0], [0], n_kf=gfpl.LBA_MAX_KFS + 1).check() == -5
    assert gfpl.gbaCheck(_problem([0], [0], n_kf=gfpl.GBA_MAX_KFS))[0] == 0
    assert gfpl.gbaCheck(_problem([0], [0], n_kf=gfpl.GBA_MAX_KFS + 1))[0] == -5
    assert gfpl.hiplib().gfpl_gba_check(None, None) == -1


def test_workspace_is_monotone_in_the_counts():
    base = [40, 1, 300, 65, 1200, 260, 1100, 250, 4000]
    rc, hbm0, lds0 = gfpl.gbaWorkspace(base)
    assert rc == 0 and hbm0 > 0 and 0 < lds0 <= 64 * 1024
    for k in (0, 2, 3, 4, 5, 6, 7, 8):
        more = list(base)
        more[k] += 7
        rc, hbm, lds = gfpl.gbaWorkspace(more)
        assert rc == 0 and hbm >= hbm0 and lds >= lds0, k
    assert gfpl.gbaWorkspace([gfpl.GBA_MAX_KFS + 1] + base[1:])[0] == -5
    assert gfpl.gbaWorkspace([0] + base[1:])[0] == -1
    assert gfpl.gbaWorkspace(base[:6] + [-1, 0, 0])[0] == -1


def test_exports_and_defaults():
    L = gfpl.hiplib()
    for n in ("gfpl_default_gba_params", "gfpl_gba_check", "gfpl_gba_workspace", "gfpl_gba_create", "gfpl_gba_destroy",
              "gfpl_gba_solve", "gfpl_gba_debug_system"):
        assert hasattr(L, n), n
    p = gfpl.GbaParams()
    L.gfpl_default_gba_params(gfpl.C.byref(p))
    assert (p.lambda_lm, p.lambda_k, p.max_iters) == G.GBA_DEFAULTS == (0.001, 10.0, 20)
    assert gfpl.GBA_MAX_KFS >= 256 and L.gfpl_abi_version() == 6
