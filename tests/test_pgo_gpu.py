"""gfpl_pgo_solve (k_pgo.hip) through Context.loopClosureOptimization / PoseGraph against the statement
(tests/pgo_ref.py) on every case of tests/pgo_cases.py.

By bits: the vertex, flag and edge lists, every Z and start pose, iteration 0's chi2, b and all H
blocks (gfpl_pgo_debug_system), and the whole map correction given the poses the device produced.
By a measured bar: the returned poses against the statement's, at most 8 x the spread of the
statement's own two solvers on the same case, and the statement's gradient norm at the device's poses
at most 8 x that at the statement's own.  No case is left out.

With GFPL_PGO_PROFILE naming a file, the measured values are appended to it.
"""
import os

import numpy as np
import pytest

import gfpl
import pgo_cases as PC
import pgo_ref as R

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in PC.all_cases()]


def _same_bits(name, what, got, ref):
    got = np.ascontiguousarray(np.asarray(got, np.float64).reshape(-1))
    ref = np.ascontiguousarray(np.asarray(ref, np.float64).reshape(-1))
    assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (name, what, got, ref)
    g, r = got.view(np.uint64)[~nan], ref.view(np.uint64)[~nan]
    bad = np.nonzero(g != r)[0]
    assert len(bad) == 0, (name, what, len(bad), got[~nan][bad[:4]], ref[~nan][bad[:4]])


@pytest.fixture(scope="module")
def ctx():
    cfg = gfpl.default_config()
    c = gfpl.Context(gfpl.make_camera("vga", cfg), cfg)
    yield c
    c.close()


@pytest.fixture(scope="module")
def solved(ctx):
    """every case through the device, COV and ESS cases each in one batched call"""
    out = {}
    for variant in (R.COV, R.ESS):
        cs = [c for c in PC.all_cases() if c["variant"] == variant]
        res = ctx.loopClosureOptimization([PC.problem(c) for c in cs], PC.params(cs[0]))
        out.update({c["name"]: r for c, r in zip(cs, res)})
    return out


@pytest.mark.parametrize("name", NAMES)
def test_lists_and_first_system_by_bits(ctx, name):
    c = PC.by_name(name)
    g, ref = PC.solved(c)
    res, s = ctx.pgoDebugSystem(PC.problem(c), PC.params(c))
    assert res[0]["guards_ok"]
    assert [tuple(v) for v in s["vert"].tolist()] == g.vert
    assert [tuple(e) for e in s["edge"].tolist()] == g.edge
    assert s["env_first"].tolist() == g.env_first
    _same_bits(name, "Z", s["Z"], ref.Z)
    _same_bits(name, "X0", s["X0"], ref.X0)
    _same_bits(name, "chi2", [s["chi2"]], [ref.chi2_0])
    _same_bits(name, "chi2_0", [res[0]["result"].chi2_0], [ref.chi2_0])
    if g.n_free:
        _same_bits(name, "b", s["b"], ref.first["b"])
        _same_bits(name, "H", np.tril(s["H"]), np.tril(ref.first["H"]))
        _same_bits(name, "diag", s["diag"], [ref.first["H"][6 * r_:6 * r_ + 6, 6 * r_:6 * r_ + 6] for r_ in range(g.n_free)])
        # the diagonal places of the envelope rows stay zero; the blocks between are the off-diagonal ones
        o = 0
        for r_, f in enumerate(g.env_first):
            assert not s["env"][o + r_ - f].any()
            o += r_ - f + 1


@pytest.mark.parametrize("name", NAMES)
def test_minimiser_within_the_measured_bar(solved, name):
    c = PC.by_name(name)
    g, ref = PC.solved(c)
    got = solved[name]
    res = got["result"]
    assert (res.n_vert, res.n_free, res.n_edge, res.kf_curr) == (len(g.vert), g.n_free, len(g.edge), g.kf_curr)
    assert res.status == ref.status == 0
    spread = PC.spread(c)
    T_ref = PC.written_back(c, g, ref.X)
    T_dev = np.array([got["T_kf"][v[0]] for v in g.vert])
    diff = float(np.max(np.abs(T_dev - T_ref)))
    lc = [tuple(int(v) for v in l) for l in c["lc"]]
    _, Z = R.start(g, c["T_kf"], lc, c["lc_pose"])
    n = lambda X: float(np.sqrt(np.sum(R.gradient(g, X, Z) ** 2))) if g.n_free else 0.0
    g_dev, g_ref = n(T_dev), n(T_ref)
    line = (f"{name} pose_diff {diff:.3e} spread {spread:.3e} grad_dev {g_dev:.3e} grad_ref {g_ref:.3e} "
            f"iters {res.iters}/{ref.iters} stop {res.stop}/{ref.stop} rejects {res.rejects}/{ref.rejects}")
    print(line)
    if os.environ.get("GFPL_PGO_PROFILE"):
        with open(os.environ["GFPL_PGO_PROFILE"], "a") as f:
            f.write(line + "\n")
    assert diff <= 8.0 * spread, line
    assert g_dev <= 8.0 * g_ref, line


@pytest.mark.parametrize("name", NAMES)
def test_map_correction_by_bits(solved, name):
    c = PC.by_name(name)
    g, _ = PC.solved(c)
    got = solved[name]
    assert got["guards_ok"]
    # the statement's correction from the poses the device wrote back
    T, x, pt, ls, pd, ld = PC.corrected(c, g, None, T_given=got["T_kf"])
    _same_bits(name, "T_kf", got["T_kf"], T)
    _same_bits(name, "x_kf", got["x_kf"], x)
    _same_bits(name, "pt", got["pt"], pt)
    _same_bits(name, "ls", got["ls"], ls)
    for what, a, b in (("pt_dirs", got["pt_dirs"], pd), ("ls_dirs", got["ls_dirs"], ld)):
        assert (a is None) == (b is None) == (c[what] is None)
        if a is not None:
            assert len(a) == len(b)
            for j, (u, v) in enumerate(zip(a, b)):
                _same_bits(name, f"{what}[{j}]", u, v)
    # keyframes outside the list and not after kf_curr (dead ones) keep their pose; x_kf is not written
    moved = {v[0] for v in g.vert} | {i for i in range(g.kf_curr + 1, c["n_kf"]) if c["alive"][i]}
    for i in range(c["n_kf"]):
        if i not in moved:
            _same_bits(name, "T_kf kept", got["T_kf"][i], c["T_kf"][i])
            assert np.isnan(got["x_kf"][i]).all()


def test_later_keyframes_freed_landmarks_and_empty_owners_are_covered():
    c = PC.by_name("later_kfs")
    g = PC.graph_of(c)
    assert g.kf_curr == 5 and c["n_kf"] == 9 and not c["alive"][7]
    assert any(len(l) == 0 for l in c["pt_own"][:6]) and any(j < 0 for l in c["pt_own"] for j in l) and c["ls_freed"].any()
    assert PC.by_name("no_dirs")["pt_dirs"] is None


def test_isolated_vertex_keeps_its_pose(ctx, solved):
    c = PC.by_name("isolated")
    g, ref = PC.solved(c)
    v = next(v for v in g.vert if v[0] == 3)
    assert v[3] >= 0 and g.inc[v[3]] == []
    _, s = ctx.pgoDebugSystem(PC.problem(c), PC.params(c))
    r = v[3]
    assert not s["b"][6 * r:6 * r + 6].any() and not s["diag"][r].any()   # H = 0, b = 0
    # a step of exactly 0: the pose is the start pose through the write-back alone
    import oracle as O
    import loop_closure_ref as LR
    want = O.expmap_se3(LR.logmap_se3(c["T_kf"][3]))
    _same_bits("isolated", "T_kf[3]", solved["isolated"]["T_kf"][3], want)
    _same_bits("isolated", "X[3]", ref.X[g.vert.index(v)], c["T_kf"][3])


def test_no_free_vertex_succeeds(solved):
    res = solved["ess_nofree"]["result"]
    assert (res.iters, res.stop, res.n_free, res.status) == (0, gfpl.PGO_STOP_NOFREE, 0, 0)
    assert res.chi2 == res.chi2_0


BATCH = ["free1", "free3", "dead_inside", "shared_prev", "later_kfs", "span16", "edges256", "no_map"]


def _key(r):
    res = r["result"]
    parts = [np.array([res.iters, res.stop, res.status, res.rejects], np.float64), np.array([res.lambda_, res.chi2_0, res.chi2]),
             r["T_kf"], r["x_kf"], r["pt"], r["ls"]] + [d for k in ("pt_dirs", "ls_dirs") if r[k] is not None for d in r[k]]
    return np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in parts]).tobytes()


def test_batch_independence(ctx, solved):
    cs = [PC.by_name(n) for n in BATCH]
    assert len({PC.graph_of(c).n_free for c in cs}) >= 6   # different sizes
    prm = PC.params(cs[0])
    together = ctx.loopClosureOptimization([PC.problem(c) for c in cs], prm)
    backwards = ctx.loopClosureOptimization([PC.problem(c) for c in cs[::-1]], prm)[::-1]
    for c, a, b in zip(cs, together, backwards):
        alone = ctx.loopClosureOptimization(PC.problem(c), prm)
        assert _key(a) == _key(alone) == _key(b) == _key(solved[c["name"]]), c["name"]


def test_capacity_and_reuse(ctx):
    small, big = PC.by_name("free2"), PC.by_name("span16")
    prm = PC.params(small)
    _, caps = PC.problem(small).check(prm)
    pg = gfpl.PoseGraph(ctx, caps, 2)
    try:
        first = pg.solve([PC.problem(small)], prm)[0]
        with pytest.raises(gfpl.GfplError) as e:
            pg.solve([PC.problem(big)], prm)
        assert e.value.code == R.E_CAPACITY
        with pytest.raises(gfpl.GfplError) as e:
            pg.solve([PC.problem(small)] * 3, prm)
        assert e.value.code == R.E_CAPACITY
        bad = PC.problem(small)
        bad.a["lc"][0, 1] = 99
        with pytest.raises(gfpl.GfplError) as e:
            pg.solve([bad], prm)
        assert e.value.code == R.E_INVALID
        # the object is usable after the refused calls, with the same answer
        again = pg.solve([PC.problem(small), PC.problem(small)], prm)
        assert _key(again[0]) == _key(again[1]) == _key(first)
        ms = pg.ms()
        assert ms[0] > 0.0 and ms[1] >= 0.0
    finally:
        pg.close()
