"""gfpl_lba_solve (k_lba.hip) through Context.localBundleAdjustment / LbaSolver against the Python
reference (tests/lba_ref.py with solve_pinned) on every case of tests/lba_cases.py.

Bar: equality.  The integer fields of the result record are compared as integers; every double of
T_kf, pt, ls, the pose part of X and the record is compared by its bits (a NaN matches a NaN only
where the reference has one).  The debug hook's blocks, g and err of iterations 0 and 1 are compared
by bits against the reference's dense H.  No tolerance, no case skipped.
"""
import numpy as np
import pytest

import gfpl
import lba_cases as LC
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


class _Contexts:
    """one context per camera the cases use"""

    def __init__(self):
        self.by_cam = {}

    def get(self, cam_over=()):
        if cam_over not in self.by_cam:
            cam, cfg = LC.setup(cam_over)
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
    for c in LC.all_cases().values():
        g.setdefault(c.group, []).append(c)
    return g


@pytest.fixture(scope="module")
def batched(ctxs):
    """every case, solved in one call per (parameters, camera) group"""
    out = {}
    for (prm, cam_over), cs in _groups().items():
        res = ctxs.get(cam_over).localBundleAdjustment([c.prob for c in cs], gfpl.LbaParams.default(
            lambda_lm=prm[0], lambda_k=prm[1], max_iters=prm[2]))
        out.update({c.name: r for c, r in zip(cs, res)})
    return out


@pytest.mark.parametrize("name", list(LC.all_cases()))
def test_case_equals_reference(batched, name):
    assert_same(name, batched[name], LC.reference(LC.all_cases()[name]))


def test_rejects_family_rejects(batched):
    for s in LC.REJECT_SEEDS:
        assert LC.reference(LC.all_cases()[f"rejects_{s}"]).rejected >= 1


RAGGED = ("size_kf1_pt1_ls0", "size_kf16_pt65_ls65", "size_kf2_pt0_ls65", "more_than_a_wave", "size_kf5_pt300_ls0",
          "fixed_only_landmarks", "both")


def test_seven_ragged_problems_equal_single_calls(ctxs, batched):
    ctx = ctxs.get()
    cases = [LC.all_cases()[n] for n in RAGGED]
    assert len({c.group for c in cases}) == 1
    together = ctx.localBundleAdjustment([c.prob for c in cases])
    for c, got in zip(cases, together):
        alone = ctx.localBundleAdjustment(c.prob)
        ref = LC.reference(c)
        assert_same(c.name + " (of seven)", got, ref)
        assert_same(c.name + " (alone)", alone, ref)


def test_second_call_on_the_same_object_is_unaffected(ctxs):
    ctx = ctxs.get()
    big, small, mid = (LC.all_cases()[n] for n in ("size_kf16_pt65_ls65", "size_kf2_pt1_ls0", "twice_by_one_keyframe"))
    caps = [max(getattr(c.prob.counts, f) for c in (big, small, mid)) for f, _ in gfpl.LbaCounts._fields_]
    solver = gfpl.LbaSolver(ctx, caps, 2)
    try:
        first = solver.solve([big.prob, mid.prob])
        second = solver.solve([small.prob, big.prob])
        third = solver.solve([mid.prob])
    finally:
        solver.close()
    assert_same("first/big", first[0], LC.reference(big))
    assert_same("first/mid", first[1], LC.reference(mid))
    assert_same("second/small", second[0], LC.reference(small))
    assert_same("second/big", second[1], LC.reference(big))
    assert_same("third/mid", third[0], LC.reference(mid))


DEBUG_CASES = ("both", "size_kf5_pt65_ls65", "twice_by_one_keyframe", "fixed_only_landmarks", "stale_x_kf", "more_than_a_wave")


@pytest.mark.parametrize("name", DEBUG_CASES)
@pytest.mark.parametrize("iteration", (0, 1))
def test_debug_system_equals_dense_h(ctxs, name, iteration):
    c = LC.all_cases()[name]
    cam, cfg = LC.setup(c.cam_over)
    ref = R.lba(cam, cfg.homog_th, c.prob.a, (c.prm[0], c.prm[1], iteration + 1), keep=True)
    assert len(ref.systems) == iteration + 1   # (a singular first solve still goes on to iteration 1, ledger BA13)
    sysr = ref.systems[iteration]
    want = R.blocks_of(sysr["H"], sysr["g"], R.layout_of(c.prob.a))
    got = ctxs.get(c.cam_over).lbaDebugSystem(c.prob, iteration, gfpl.LbaParams.default(lambda_lm=c.prm[0], lambda_k=c.prm[1]))
    for k in ("U", "g", "V_pt", "V_ls", "W_pt", "W_ls"):
        _same_bits(name, f"{k} of iteration {iteration}", got[k], want[k])
    _same_bits(name, f"err of iteration {iteration}", [got["err"]], [sysr["err"]])


def test_context_refuses_destruction_while_a_solver_lives():
    cam, cfg = LC.setup()
    ctx = gfpl.Context(cam, cfg)
    solver = gfpl.LbaSolver(ctx, [2, 1, 4, 0, 8, 0], 1)
    with pytest.raises(gfpl.GfplError):
        ctx.close()
    solver.close()
    ctx.close()


def test_capacity_and_invalid_problems_are_refused_before_device_work(ctxs):
    ctx = ctxs.get()
    c = LC.all_cases()["points_only"]
    solver = gfpl.LbaSolver(ctx, [2, 1, 4, 0, 8, 0], 1)
    try:
        with pytest.raises(gfpl.GfplError) as e:
            solver.solve([c.prob])
        assert e.value.code == -5
    finally:
        solver.close()
