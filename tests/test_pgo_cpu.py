"""The loop-closure pose graph without a GPU: the exports, the graph builder (gfpl_pgo_plan.cpp)
against the statement (tests/pgo_ref.py) by equality — through gfpl_pgo_check and through a
stand-alone program built under ASan + UBSan (nothing is preloaded) —, every refusal code, two
hand-worked minimisers, the analytic Jacobians against central differences, the agreement of the
statement's two solvers, and six altered rules that each change a named case.
"""
import os
import subprocess

import numpy as np
import pytest

import gfpl
import oracle as O
import loop_closure_ref as LR
import pgo_cases as PC
import pgo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float64
NAMES = [c["name"] for c in PC.all_cases()]


def test_exports_present():
    L = gfpl.hiplib()
    for n in ("gfpl_default_pgo_params", "gfpl_pgo_check", "gfpl_pgo_workspace", "gfpl_pgo_create", "gfpl_pgo_destroy",
              "gfpl_pgo_solve", "gfpl_pgo_debug_system", "gfpl_pgo_debug_ms"):
        assert hasattr(L, n), n
    assert L.gfpl_abi_version() == 6
    for n in ("PoseGraphParams", "PoseGraphProblem", "PoseGraph"):
        assert hasattr(gfpl, n), n
    assert hasattr(gfpl.Context, "loopClosureOptimization")
    p = gfpl.PoseGraphParams.default()
    assert (p.min_lm_ess_graph, p.min_lm_cov_graph, p.variant, p.max_iters, p.max_rejects, p.lambda_init) == (100, 30, 0, 100, 10, 1e-10)
    assert (gfpl.PGO_COV, gfpl.PGO_ESS) == (R.COV, R.ESS)
    assert (gfpl.PGO_VERT_FIXED, gfpl.PGO_VERT_LC_J, gfpl.PGO_VERT_LC_I) == (R.FIXED, R.LC_J, R.LC_I)


# ------------------------------------------------------------------ builder --
def _n_jobs(own, freed):
    return sum(1 for l in own for j in l if j >= 0 and not (freed is not None and freed[j]))


@pytest.mark.parametrize("name", NAMES)
def test_check_counts_against_statement(name):
    c = PC.by_name(name)
    g = PC.graph_of(c)
    rc, cnt = PC.problem(c).check(PC.params(c))
    assert rc == 0
    want = (c["n_kf"], len(c["lc"]), len(g.vert), g.n_free, len(g.edge), g.env_blocks, _n_jobs(c["pt_own"], c["pt_freed"]),
            _n_jobs(c["ls_own"], c["ls_freed"]))
    assert tuple(getattr(cnt, f) for f, _ in gfpl.PgoCounts._fields_) == want
    rc, hbm, lds = gfpl.pgoWorkspace(cnt)
    assert rc == 0 and hbm > 0 and 0 < lds <= 64 * 1024


def test_ess_against_cov_on_the_same_input():
    a, b = PC.graph_of(PC.by_name("thresholds")), PC.graph_of(PC.by_name("thresholds_ess"))
    assert a.first == 0 and b.first == 1
    kf = lambda g: sorted((g.vert[i][0], g.vert[j][0]) for i, j, l, _ in g.edge if l < 0)
    # on and above minLMCovGraph joins COV only; on and above minLMEssGraph joins both; one below neither
    assert (0, 3) not in kf(a) and (0, 4) in kf(a) and (0, 5) in kf(a)
    assert (1, 4) in kf(a) and (1, 4) not in kf(b) and (1, 5) in kf(b) and (2, 6) in kf(b)
    fixed = lambda g: [v[0] for v in g.vert if v[1] & R.FIXED]
    assert fixed(a) == [0] and fixed(b) == [1, 6]


def refusals():
    """(name, expected code, edit of a copy of the `dead_inside` case, params edit)"""
    out = []

    def add(name, code, edit=None, prm=None):
        out.append((name, code, edit or (lambda c: None), prm or {}))
    add("ok", R.OK)
    add("alive_null", R.E_INVALID, lambda c: c.update(alive=None))
    add("graph_null", R.E_INVALID, lambda c: c.update(full_graph=None))
    add("lc_null", R.E_INVALID, lambda c: c.update(lc=None))
    add("lc_pose_null", R.E_INVALID, lambda c: c.update(lc_pose=None))
    add("lc_empty", R.E_INVALID, lambda c: c.update(lc=np.zeros((0, 3), np.int32), lc_pose=np.zeros((0, 6))))
    add("prev_negative", R.E_INVALID, lambda c: c["lc"].__setitem__((0, 0), -1))
    add("curr_at_n_kf", R.E_INVALID, lambda c: c["lc"].__setitem__((0, 1), 7))
    add("prev_equals_curr", R.E_INVALID, lambda c: c["lc"].__setitem__((0, 0), 5))
    add("prev_above_curr", R.E_INVALID, lambda c: c["lc"].__setitem__((0, slice(0, 2)), [5, 1]))
    add("dead_prev", R.E_INVALID, lambda c: c["lc"].__setitem__((0, 0), 3))
    add("dead_curr", R.E_INVALID, lambda c: c["alive"].__setitem__(5, 0))
    add("kf0_dead_cov", R.E_INVALID, lambda c: c["alive"].__setitem__(0, 0))
    add("kf0_dead_ess", R.OK, lambda c: c["alive"].__setitem__(0, 0), dict(variant=R.ESS))
    add("ess_negative", R.E_INVALID, prm=dict(min_lm_ess_graph=-1))
    add("cov_negative", R.E_INVALID, prm=dict(min_lm_cov_graph=-1))
    add("variant_unknown", R.E_INVALID, prm=dict(variant=2))
    add("landmark_twice", R.E_INVALID, lambda c: c["pt_own"].__setitem__(0, [c["pt_own"][1][0]]))
    add("landmark_past", R.E_INVALID, lambda c: c["pt_own"].__setitem__(0, [len(c["pt"])]))
    return out


def _copy(c):
    return {k: (v.copy() if isinstance(v, np.ndarray) else ([list(x) for x in v] if k.endswith("_own") else v)) for k, v in c.items()}


def _check_raw(c, prm):
    """gfpl_pgo_check with arrays that may be None"""
    p = PC.problem(dict(c, alive=c["alive"] if c["alive"] is not None else np.ones(c["n_kf"], np.uint8),
                        full_graph=c["full_graph"] if c["full_graph"] is not None else np.zeros((c["n_kf"], c["n_kf"]), np.int32),
                        lc=c["lc"] if c["lc"] is not None else np.zeros((1, 3), np.int32),
                        lc_pose=c["lc_pose"] if c["lc_pose"] is not None else np.zeros((1, 6))))
    s = p.struct()
    for k in ("alive", "full_graph", "lc", "lc_pose"):
        if c[k] is None:
            setattr(s, k, None)
    cnt = gfpl.PgoCounts()
    import ctypes as C
    return gfpl.hiplib().gfpl_pgo_check(C.byref(s), C.byref(prm), C.byref(cnt))


@pytest.mark.parametrize("name,code,edit,prm", refusals(), ids=[r[0] for r in refusals()])
def test_every_refusal_code(name, code, edit, prm):
    c = _copy(PC.by_name("dead_inside"))
    edit(c)
    p = PC.params(c)
    for k, v in prm.items():
        setattr(p, k, v)
    assert _check_raw(c, p) == code
    if all(c[k] is not None for k in ("alive", "full_graph", "lc")):
        assert R.check(c["alive"], c["full_graph"], c["lc"], p.min_lm_ess_graph, p.min_lm_cov_graph, p.variant) == (
            code if not name.startswith("landmark") and name != "lc_pose_null" else R.OK)


def test_null_problem_and_capacity_of_workspace():
    import ctypes as C
    L = gfpl.hiplib()
    p = gfpl.PoseGraphParams.default()
    assert L.gfpl_pgo_check(None, C.byref(p), None) == R.E_INVALID
    assert L.gfpl_pgo_check(C.byref(PC.problem(PC.by_name("free1")).struct()), None, None) == R.E_INVALID
    big = gfpl.PgoCounts(4, 1, 4, 3, 4, 2 ** 31 // 64 + 1, 0, 0)
    assert gfpl.pgoWorkspace(big)[0] == R.E_CAPACITY
    assert gfpl.pgoWorkspace(gfpl.PgoCounts(0, 1, 0, 0, 1, 0, 0, 0))[0] == R.E_INVALID


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    """the builder's translation unit and tests/pgo_plan_main.cpp, no HIP, under ASan + UBSan"""
    exe = str(tmp_path_factory.mktemp("pgo_plan") / "pgo_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pgo_plan_main.cpp"),
           os.path.join(ROOT, "gf-pl-slam_amd", "csrc", "gfpl_pgo_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _flat(a):
    return " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))


def _expected_lines(c, g):
    nf = g.n_free
    inc_start = np.concatenate([[0], np.cumsum([len(l) for l in g.inc])]).astype(int)
    env_off = np.concatenate([[0], np.cumsum([r - f + 1 for r, f in enumerate(g.env_first)])]).astype(int)
    reach = [max(r for r in range(nf) if g.env_first[r] <= col) for col in range(nf)]
    jobs = []
    for own in (c["pt_own"], c["ls_own"]):   # (the program passes no freed marks and no dir arrays)
        for kf, l in enumerate(own):
            for j in l:
                if j >= 0:
                    jobs += [j, kf, 0, 0]
    fmt = lambda name, v: (name + " " + _flat(v)).rstrip() if len(v) else name
    return [fmt("vert", g.vert), fmt("edge", g.edge), fmt("inc_start", inc_start), fmt("inc", [e for l in g.inc for e in l]),
            fmt("env_first", g.env_first), fmt("env_off", env_off), fmt("reach", reach), fmt("jobs", jobs)]


def test_builder_under_sanitizers_against_statement(plan_exe, tmp_path):
    probs = [(c, PC.params(c)) for c in PC.all_cases()]
    for name, code, edit, prm in refusals():
        c = _copy(PC.by_name("dead_inside"))
        edit(c)
        if any(c[k] is None for k in ("alive", "full_graph", "lc", "lc_pose")):
            continue   # (a NULL array is gfpl_pgo_check's test above)
        p = PC.params(c)
        for k, v in prm.items():
            setattr(p, k, v)
        probs.append((dict(c, name="refusal_" + name, code=code), p))
    path = tmp_path / "problems.txt"
    with open(path, "w") as f:
        f.write(f"{len(probs)}\n")
        for c, p in probs:
            f.write(f"{p.variant} {p.min_lm_ess_graph} {p.min_lm_cov_graph} {c['n_kf']} {len(c['lc'])} {len(c['pt'])} {len(c['ls'])}\n")
            f.write(_flat(c["alive"]) + "\n" + _flat(c["full_graph"]) + "\n" + _flat(c["lc"]) + "\n")
            for own in (c["pt_own"], c["ls_own"]):
                start, idx = gfpl._csr(own, c["n_kf"])
                f.write(_flat(start) + "\n" + _flat(idx) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([plan_exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    out = r.stdout.rstrip("\n").split("\n")
    k = 0
    for c, p in probs:
        code = c.get("code", 0)
        assert out[k] == f"rc {code}", (c["name"], out[k])
        k += 1
        if code != 0:
            continue
        g = R.build_graph(c["alive"], c["full_graph"], [tuple(int(v) for v in l) for l in c["lc"]], p.min_lm_ess_graph,
                          p.min_lm_cov_graph, p.variant)
        assert out[k + 1] == f"range {g.first} {g.kf_curr}", c["name"]
        got = [l.rstrip() for l in out[k + 2:k + 10]]
        # the program's jobs carry no dir rows (it passes no dir arrays)
        assert got == _expected_lines(c, g), (c["name"], got, _expected_lines(c, g))
        k += 10
    assert k == len(out)


# -------------------------------------------------------------- the objective --
def _trans(t):
    T = np.eye(4, dtype=F)
    T[:3, 3] = t
    return T


def _solve_simple(T, lc, lc_pose, graph_zero=True):
    n = len(T)
    fg = np.zeros((n, n), np.int32)
    g = R.build_graph(np.ones(n, np.uint8), fg, lc)
    return g, R.solve(g, np.array(T, F), lc, np.array(lc_pose, F))


def test_hand_worked_two_vertices():
    # vertex 0 fixed at I; edges x1 - t1 (keyframe edge) and x1 - d (loop edge): x1 = (t1 + d) / 2, chi2 = |t1 - d|^2 / 2
    t1, d = np.array([1.0, 2.0, -0.5]), np.array([1.5, 1.0, 0.25])
    g, r = _solve_simple([np.eye(4), _trans(t1)], [(0, 1, 1)], [np.concatenate([d, np.zeros(3)])])
    assert np.array_equal(r.X0[1], _trans(d))   # the is_lc_j start pose (:4253)
    # LM stops once a step or a chi2 decrease is below 64 eps relative: the translation is exact to a few hundred eps
    assert np.max(np.abs(r.X[1][:3, 3] - (t1 + d) / 2)) <= 512 * R.EPS * 2.0
    assert np.array_equal(r.X[1][:3, :3], np.eye(3))
    assert abs(r.chi2 - np.sum((t1 - d) ** 2) / 2) <= 512 * R.EPS
    assert r.chi2_0 == np.sum((t1 - d) ** 2)


def test_hand_worked_three_vertex_chain():
    # x1 = (a + d) / 3, x2 = 2 (a + d) / 3 minimise |x1 - a|^2 + |x2 - x1 - a|^2 + |x2 - d|^2
    # (a and d collinear: every residual lies along the chain, so no rotation lowers chi2 — a rotation by
    # theta gains at most |residual| |a| theta^2 / 2 = 0.08 theta^2 and costs theta^2 / 2 in two edges)
    a, d = np.array([1.0, 0.0, 0.0]), np.array([2.5, 0.0, 0.0])
    g, r = _solve_simple([np.eye(4), _trans(a), _trans(2 * a)], [(0, 2, 1)], [np.concatenate([d, np.zeros(3)])])
    assert [e[:3] for e in g.edge] == [(0, 1, -1), (1, 2, -1), (0, 2, 0)]
    assert np.max(np.abs(r.X[1][:3, 3] - (a + d) / 3)) <= 512 * R.EPS * 3.0
    assert np.max(np.abs(r.X[2][:3, 3] - 2 * (a + d) / 3)) <= 512 * R.EPS * 3.0
    assert r.stop in (R.STOP_STEP, R.STOP_DCHI2) and r.status == 0


def test_jacobians_against_central_differences():
    rng = np.random.default_rng(7)
    h = 1e-6
    worst = 0.0
    for k in range(12):
        rot = 0.4 if k < 8 else 2.6   # the last four have error rotations past 120 degrees (the other quaternion branches)
        Xi = O.expmap_se3(np.concatenate([rng.normal(0, 2, 3), rng.normal(0, 0.4, 3)]))
        Xj = O.expmap_se3(np.concatenate([rng.normal(0, 2, 3), rng.normal(0, rot, 3)]))
        Z = O.expmap_se3(np.concatenate([rng.normal(0, 2, 3), rng.normal(0, 0.4, 3)]))
        e, Ji, Jj = R.edge(Xi, Xj, Z)
        tmax = 1.0 + max(np.max(np.abs(M[:3, 3])) for M in (Xi, Xj, Z)) * 3.0
        # central differences of e: truncation h^2 |e'''| / 6 with |e'''| <= 8 tmax (products of three rotation
        # derivatives, each <= 2, times the lever), rounding 2 eps |e| / (2 h) with |e| <= tmax
        bound = h * h * 8.0 * tmax / 6.0 + 2.0 * R.EPS * tmax / h
        for a in range(6):
            d = np.zeros(6)
            d[a] = h
            for which, J in ((0, Ji), (1, Jj)):
                ep = R.edge(R.update(Xi, d) if which == 0 else Xi, R.update(Xj, d) if which == 1 else Xj, Z, jac=False)
                em = R.edge(R.update(Xi, -d) if which == 0 else Xi, R.update(Xj, -d) if which == 1 else Xj, Z, jac=False)
                err = np.max(np.abs((ep - em) / (2 * h) - J[:, a]))
                worst = max(worst, err / bound)
                assert err <= bound, (k, a, which, err, bound)
    assert worst > 0.0


def test_sums_are_in_incident_edge_order():
    # the statement's system against an explicit dense J^T J built edge by edge in EDGE-LIST order: the same
    # numbers to rounding, and identical when a vertex has one incident edge
    c = PC.by_name("free3")
    g, r = PC.solved(c)
    H, b, chi2 = r.first["H"], r.first["b"], r.first["chi2"]
    assert chi2 == r.chi2_0 and np.array_equal(H, H.T)
    J = np.zeros((6 * len(g.edge), 6 * g.n_free))
    ev = np.zeros(6 * len(g.edge))
    for e, (vi, vj, _, _) in enumerate(g.edge):
        er, Ji, Jj = R.edge(r.X0[vi], r.X0[vj], r.Z[e])
        ev[6 * e:6 * e + 6] = er
        for v, Jv in ((vi, Ji), (vj, Jj)):
            f = g.vert[v][3]
            if f >= 0:
                J[6 * e:6 * e + 6, 6 * f:6 * f + 6] = Jv
    assert np.allclose(H, J.T @ J, rtol=0, atol=64 * R.EPS * np.max(np.abs(H)))
    assert np.allclose(b, J.T @ ev, rtol=0, atol=64 * R.EPS * np.max(np.abs(J)) * np.max(np.abs(ev)) * 6)


# ------------------------------------------------------- both solvers agree --
@pytest.mark.parametrize("name", NAMES)
def test_both_solvers_agree(name):
    c = PC.by_name(name)
    g, a = PC.solved(c, "envelope")
    _, b = PC.solved(c, "dense")
    s = PC.spread(c)
    if g.n_free == 0:
        assert s == 0.0 and a.iters == 0 and a.stop == R.STOP_NOFREE
        return
    # both stop where a step or a chi2 decrease falls below 64 eps relative.  The iteration converges
    # linearly at these residuals, so where it stops moves with the rounding of the solves: a decrease of
    # 64 eps chi2 of a quadratic bowl is a distance of sqrt(64 eps chi2 / mu_min) from the minimiser,
    # mu_min the smallest eigenvalue of H; the two stops are at most twice that apart
    H = a.first["H"]
    mu = np.linalg.eigvalsh(H)
    mu_min = max(mu[mu > 1e-12 * mu[-1]][0], 1e-300)
    bound = 2.0 * np.sqrt(64 * R.EPS * max(a.chi2, R.EPS) / mu_min) + 64 * R.EPS * np.max(np.abs(a.X))
    assert s <= bound, (name, s, bound)
    assert abs(a.chi2 - b.chi2) <= 1024 * R.EPS * a.chi2
    if os.environ.get("GFPL_PGO_PROFILE"):
        with open(os.environ["GFPL_PGO_PROFILE"], "a") as f:
            f.write(f"{name} spread {s:.3e} bound {bound:.3e} iters {a.iters} {b.iters} stop {a.stop} {b.stop}\n")


# ------------------------------------------------------------ altered rules --
def test_altered_edge_order_changes_shared_prev():
    c = PC.by_name("shared_prev")
    g, alt = PC.graph_of(c), PC.graph_of(c, alt_lc_edges_first=True)
    assert g.edge != alt.edge and sorted(g.edge) == sorted(alt.edge)
    assert g.inc != alt.inc
    lc = [tuple(int(v) for v in l) for l in c["lc"]]
    X0, Z = R.start(g, c["T_kf"], lc, c["lc_pose"])
    X0a, Za = R.start(alt, c["T_kf"], lc, c["lc_pose"])
    Ha, Hb = R.system(g, X0, Z)[0], R.system(alt, X0a, Za)[0]
    assert not np.array_equal(Ha, Hb) and np.allclose(Ha, Hb)   # the same sums in another order: other bits


def test_altered_break_changes_chained_lc():
    c = PC.by_name("chained_lc")
    g, alt = PC.graph_of(c), PC.graph_of(c, alt_no_break=True)
    v = next(v for v in g.vert if v[0] == 3)
    w = next(v for v in alt.vert if v[0] == 3)
    assert v[1] & R.LC_J and not v[1] & R.LC_I and v[2] == 0   # entry 0 names keyframe 3 first, in its kf_curr column
    assert w[2] == 1 and w != v


def test_altered_w_sign_changes_a_half_turn_error():
    th = -170.0 * np.pi / 180.0
    Xj = np.eye(4, dtype=F)
    Xj[1:3, 1:3] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    e = R.edge(np.eye(4), Xj, np.eye(4), jac=False)
    ea = R.edge(np.eye(4), Xj, np.eye(4), jac=False, alt_no_w_flip=True)
    assert e[3] < 0 and np.array_equal(ea[3:], -e[3:])   # -170 degrees about x: (sin(-85), 0, 0, cos(85))


def test_altered_update_side_changes_free2():
    c = PC.by_name("free2")
    g, a = PC.solved(c)
    lc = [tuple(int(v) for v in l) for l in c["lc"]]
    one = R.solve(g, c["T_kf"], lc, c["lc_pose"], max_iters=1)
    b = R.solve(g, c["T_kf"], lc, c["lc_pose"], max_iters=1, alt_left=True)
    # the Jacobians belong to the right-multiplied update: on the left the same step lands on another pose
    assert np.max(np.abs(one.X - b.X)) > 1e-3 and b.chi2 > one.chi2 * 1.01
    assert one.chi2 < 0.5 * one.chi2_0 and a.iters > 1


def test_altered_later_keyframes_and_directions_change_later_kfs():
    c = PC.by_name("later_kfs")
    g, a = PC.solved(c)
    want = PC.corrected(c, g, a.X)
    own = PC.corrected(c, g, a.X, alt_own_corr=True)
    assert not np.array_equal(want[0][6], own[0][6]) and np.array_equal(want[0][:6], own[0][:6])
    undir = PC.corrected(c, g, a.X, alt_dir_untranslated=True)
    assert np.array_equal(want[2], undir[2]) and any(len(x) and not np.array_equal(x, y) for x, y in zip(want[4], undir[4]))
    # the dead keyframe after kf_curr and everything it owns stay as they were
    assert np.array_equal(want[0][7], c["T_kf"][7]) and np.isnan(want[1][7]).all()
