"""gfpl_gba_solve (k_gba.hip) through Context.globalBundleAdjustment / GbaSolver against the Python
reference (tests/gba_ref.py with solve_pinned) on every case of tests/gba_cases.py.

Bar: equality.  The integer fields of the result record are compared as integers; every double of
T_kf, pt, ls, the pose part of X and the record is compared by its bits (a NaN matches a NaN only
where the reference has one).  The debug hook's blocks, g and err of iterations 0 and 1 are compared
by bits against the reference's dense H (its blocks under the diagonal).  No tolerance, no case skipped.
"""
import os

import numpy as np
import pytest

import gfpl
import gba_cases as GC
import gba_ref as G
import lba_ref as R

pytestmark = pytest.mark.gpu

INTS = ("iters", "stop", "status", "hmax")
SCALARS = (("lambda_", "lambda_"), ("err", "err"), ("err_prev", "err_prev"))


def _same_bits(name, what, got, ref):
    got = np.ascontiguousarray(np.asarray(got, np.float64).reshape(-1))
    ref = np.ascontiguousarray(np.asarray(ref, np.float64).reshape(-1))
    assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (name, what, got, ref)
    g, r = got.view(np.uint64)[~nan], ref.view(np.uint64)[~nan]
    bad = np.nonzero(g != r)[0]
    assert len(bad) == 0, (name, what, len(bad), got[~nan][bad[:4]], ref[~nan][bad[:4]])


def assert_same(name, got, ref):
    res = got["result"]
    for k in INTS:
        assert getattr(res, k) == getattr(ref, k), (name, k, getattr(res, k), getattr(ref, k))
    for k, rk in SCALARS:
        _same_bits(name, k, [getattr(res, k)], [getattr(ref, rk)])
    nkf = len(got["x_kf"])
    _same_bits(name, "x_kf", got["x_kf"], ref.X[:6 * nkf])
    _same_bits(name, "T_kf", got["T_kf"], ref.T_kf)
    _same_bits(name, "pt", got["pt"], ref.pt)
    _same_bits(name, "ls", got["ls"], ref.ls)


def _params(prm):
    return gfpl.LbaParams.default(lambda_lm=prm[0], lambda_k=prm[1], max_iters=prm[2])


class _Contexts:
    """one context per camera the cases use"""

    def __init__(self):
        self.by_cam = {}

    def get(self, cam_over=()):
        if cam_over not in self.by_cam:
            cam, cfg = GC.setup(cam_over)
            self.by_cam[cam_over] = gfpl.Context(cam, cfg)
        return self.by_cam[cam_over]

    def close(self):
        for c in self.by_cam.values():
            c.close()


@pytest.fixture(scope="module")
def ctxs():
    c = _Contexts()
    yield c
    c.close()


def _groups():
    g = {}
    for c in GC.all_cases().values():
        g.setdefault(c.group, []).append(c)
    return g


@pytest.fixture(scope="module")
def batched(ctxs):
    """every case, solved in one call per (parameters, camera) group"""
    out = {}
    for (prm, cam_over), cs in _groups().items():
        res = ctxs.get(cam_over).globalBundleAdjustment([c.prob for c in cs], _params(prm))
        out.update({c.name: r for c, r in zip(cs, res)})
    return out


@pytest.mark.parametrize("name", list(GC.all_cases()))
def test_case_equals_reference(batched, name):
    assert_same(name, batched[name], GC.reference(GC.all_cases()[name]))


def test_seventeen_keyframes_are_beyond_the_lba(ctxs):
    """the first size gfpl_lba_solve refuses (GFPL_E_CAPACITY) is solved here"""
    c = GC.all_cases()["size_kf17_pt65_ls65"]
    assert c.prob.check() == -5
    with pytest.raises(gfpl.GfplError) as e:
        ctxs.get().localBundleAdjustment(c.prob)
    assert e.value.code == -5
    rc, cnt = gfpl.gbaCheck(c.prob)
    assert rc == 0 and cnt.n.n_kf == 17


def test_idle_keyframe_is_singular_and_keeps_x(batched):
    c = GC.all_cases()["idle_keyframe"]
    got = batched["idle_keyframe"]
    assert got["result"].status & gfpl.GBA_SINGULAR
    _same_bits("idle_keyframe", "x_kf kept", got["x_kf"], c.prob.a["x_kf"])
    _same_bits("idle_keyframe", "pt kept", got["pt"], c.prob.a["pt"])


def test_indefinite_bit_only_with_lines(batched):
    for n in ("lines_small_lambda", "both_small_lambda"):
        assert batched[n]["result"].status & gfpl.GBA_INDEFINITE, n
    for n in GC.points_only():
        assert not batched[n]["result"].status & gfpl.GBA_INDEFINITE, n


RAGGED = ("size_kf2_pt1_ls0", "size_kf17_pt65_ls65", "size_kf2_pt0_ls65", "seventy_by_two_keyframes", "size_kf17_pt300_ls0",
          "fixed_only_landmarks", "both")


def test_seven_ragged_problems_equal_single_calls(ctxs):
    ctx = ctxs.get()
    cases = [GC.all_cases()[n] for n in RAGGED]
    assert len({c.group for c in cases}) == 1
    together = ctx.globalBundleAdjustment([c.prob for c in cases])
    for c, got in zip(cases, together):
        alone = ctx.globalBundleAdjustment(c.prob)
        ref = GC.reference(c)
        assert_same(c.name + " (of seven)", got, ref)
        assert_same(c.name + " (alone)", alone, ref)


def _caps(cases):
    return [max(col) for col in zip(*[gfpl.gbaCheck(c.prob)[1].flat() for c in cases])]


def test_second_and_third_call_on_the_same_object_are_unaffected(ctxs):
    ctx = ctxs.get()
    big, small, mid = (GC.all_cases()[n] for n in ("size_kf17_pt65_ls65", "size_kf2_pt1_ls0", "twice_by_one_keyframe"))
    solver = gfpl.GbaSolver(ctx, _caps((big, small, mid)), 2)
    try:
        first = solver.solve([big.prob, mid.prob])
        second = solver.solve([small.prob, big.prob])
        third = solver.solve([mid.prob])
    finally:
        solver.close()
    assert_same("first/big", first[0], GC.reference(big))
    assert_same("first/mid", first[1], GC.reference(mid))
    assert_same("second/small", second[0], GC.reference(small))
    assert_same("second/big", second[1], GC.reference(big))
    assert_same("third/mid", third[0], GC.reference(mid))


DEBUG_CASES = ("both", "size_kf17_pt65_ls65", "twice_by_one_keyframe", "fixed_only_landmarks", "stale_x_kf")


@pytest.mark.parametrize("name", DEBUG_CASES)
@pytest.mark.parametrize("iteration", (0, 1))
def test_debug_system_equals_dense_h(ctxs, name, iteration):
    c = GC.all_cases()[name]
    ref = GC.reference(c, prm=(c.prm[0], c.prm[1], iteration + 1), keep=True)
    assert len(ref.systems) == iteration + 1
    sysr = ref.systems[iteration]
    lay = R.layout_of(c.prob.a)
    want = G.blocks_of(sysr["H"], sysr["g"], lay)
    got = ctxs.get(c.cam_over).gbaDebugSystem(c.prob, iteration, _params(c.prm))
    assert np.array_equal(got["pairs"], want["pairs"])
    for k in ("U", "g", "V_pt", "V_ls", "W_pt", "W_ls"):
        _same_bits(name, f"{k} of iteration {iteration}", got[k], want[k])
    _same_bits(name, f"err of iteration {iteration}", [got["err"]], [sysr["err"]])
    if iteration == 0 and lay.nls and len(want["W_ls"]):
        # the pre-pass shows the transposed line blocks: they are not the blocks of a Gauss-Newton system
        right = G.build_system(*_cam_homog(c), c.prob.a, lay, None, 0, G.Rules(prepass_transposed=False))[0]
        assert not np.array_equal(G.blocks_of(right, sysr["g"], lay)["W_ls"], want["W_ls"])


def _cam_homog(c):
    cam, cfg = GC.setup(c.cam_over)
    return cam, cfg.homog_th


def test_context_refuses_destruction_while_a_solver_lives():
    cam, cfg = GC.setup()
    ctx = gfpl.Context(cam, cfg)
    solver = gfpl.GbaSolver(ctx, [2, 1, 4, 0, 8, 0, 8, 0, 16], 1)
    with pytest.raises(gfpl.GfplError):
        ctx.close()
    solver.close()
    ctx.close()


def test_capacity_and_invalid_problems_are_refused_before_device_work(ctxs):
    ctx = ctxs.get()
    c = GC.all_cases()["points_only"]
    solver = gfpl.GbaSolver(ctx, [2, 1, 4, 0, 8, 0, 8, 0, 16], 1)
    try:
        with pytest.raises(gfpl.GfplError) as e:
            solver.solve([c.prob])
        assert e.value.code == -5
        a = c.prob.a
        bad = gfpl.LbaProblem(a["x_kf"], a["T_kf"], a["T_fix"], a["pt"], a["ls"], a["pt_obs_lm"], a["pt_obs_kf"] + 50, a["pt_obs"],
                              a["pt_sigma"], a["ls_obs_lm"], a["ls_obs_kf"], a["ls_obs"], a["ls_sigma"])
        with pytest.raises(gfpl.GfplError) as e:
            solver.solve([bad])
        assert e.value.code == -1
    finally:
        solver.close()


@pytest.mark.parametrize("name", ("size_kf17_pt65_ls65", "seen_by_all_70", "no_common_landmark"))
def test_grid_independence(ctxs, name):
    """the same problem with two other cuts of the wide phases into workgroups gives the same bits:
    no sum follows the grid.  The override is read when the solver is created."""
    ctx = ctxs.get()
    c = GC.all_cases()[name]
    ref = GC.reference(c)
    for block, kfs in ((64, 1), (128, 11)):
        os.environ["GFPL_GBA_BLOCK"], os.environ["GFPL_GBA_LDLT_KFS"] = str(block), str(kfs)
        try:
            solver = gfpl.GbaSolver(ctx, _caps((c,)), 1)
        finally:
            del os.environ["GFPL_GBA_BLOCK"], os.environ["GFPL_GBA_LDLT_KFS"]
        try:
            got = solver.solve([c.prob], _params(c.prm))[0]
        finally:
            solver.close()
        assert_same(f"{name} block {block} ldlt {kfs}", got, ref)
