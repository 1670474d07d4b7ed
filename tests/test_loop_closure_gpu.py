"""gfpl_kf_loop_closure (k_loop.hip) through Context.isLoopClosure against the Python reference
(tests/loop_closure_ref.py) on every case family of tests/loop_closure_cases.py.

Bar: equality.  The (kf0 row, kf1 row) pairs, the inlier bytes and the integer fields are integers;
every double of the result record is compared by its bits (a NaN matches a NaN only where the
reference has one).  No tolerance, no case skipped.
"""
import ctypes as C

import numpy as np
import pytest

import gfpl
import loop_closure_cases as LC

pytestmark = pytest.mark.gpu

INTS = ("is_lc", "gates", "n_pt", "n_ls", "n_pt_inl", "n_ls_inl", "iters")
SCALARS = ("e", "unc", "ratio_inliers", "trs", "rot")
VECTORS = ("x_inc", "pose_inc", "T_inc")


def _same_bits(name, what, got, ref):
    got = np.ascontiguousarray(np.asarray(got, np.float64).reshape(-1))
    ref = np.ascontiguousarray(np.asarray(ref, np.float64).reshape(-1))
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (name, what, got, ref)
    g, r = got.view(np.uint64)[~nan], ref.view(np.uint64)[~nan]
    assert np.array_equal(g, r), (name, what, got, ref)


def assert_same(name, got, ref):
    res, pp, pi, lp, li = got
    np.testing.assert_array_equal(pp, ref.pt_pairs, err_msg=f"{name} pt_pairs")
    np.testing.assert_array_equal(lp, ref.ls_pairs, err_msg=f"{name} ls_pairs")
    for k in INTS:
        assert getattr(res, k) == getattr(ref, k), (name, k, getattr(res, k), getattr(ref, k))
    np.testing.assert_array_equal(pi, ref.pt_inlier, err_msg=f"{name} pt_inlier")
    np.testing.assert_array_equal(li, ref.ls_inlier, err_msg=f"{name} ls_inlier")
    for k in SCALARS:
        _same_bits(name, k, [getattr(res, k)], [getattr(ref, k)])
    for k in VECTORS:
        _same_bits(name, k, getattr(res, k)[:], getattr(ref, k))


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


@pytest.fixture(scope="module")
def ctx(ctxs):
    return ctxs.get()


@pytest.fixture(scope="module")
def views():
    return {n: (gfpl.KeyFrameView(c.f0, np.eye(4), "cuda"), gfpl.KeyFrameView(c.f1, np.eye(4), "cuda"))
            for n, c in LC.all_cases().items()}


def _groups():
    g = {}
    for n, c in LC.all_cases().items():
        if n != LC.BIG:
            g.setdefault(c.group, []).append(n)
    return g


def _call(ctxs, views, names):
    c0 = LC.all_cases()[names[0]]
    ctx = ctxs.get(c0.cam_over)
    ctx.set_config(gfpl.default_config(max_iters=c0.max_iters))
    return ctx.isLoopClosure([views[n][0] for n in names], [views[n][1] for n in names],
                             gfpl.LoopParams(*c0.prm))


def test_batched_calls(ctxs, views):
    """every family but the 2048 / 1024 case: the cases that share a config and thresholds in ONE call
    (the default group mixes all the sizes)"""
    groups = _groups()
    assert max(len(v) for v in groups.values()) >= 10
    seen = 0
    for names in groups.values():
        got = _call(ctxs, views, names)
        assert len(got) == len(names)
        for n, g in zip(names, got):
            assert_same(n, g, LC.reference(n))
            seen += 1
    assert seen == len(LC.all_cases()) - 1


def test_one_pair_per_call(ctxs, views):
    for n in LC.all_cases():
        if n == LC.BIG:
            continue
        (g,) = _call(ctxs, views, [n])
        assert_same(n, g, LC.reference(n))


def test_largest_lists(ctxs, views):
    """2048 points + 1024 lines: 8 and 4 chunks of the reduction"""
    (g,) = _call(ctxs, views, [LC.BIG])
    ref = LC.reference(LC.BIG)
    assert ref.n_pt == 2048 and ref.n_ls == 1024
    assert_same(LC.BIG, g, ref)


def _raw(ctx, v0, v1, n, prm, pt_cap, ls_cap, bufs=True):
    import torch
    pp = torch.zeros((max(n, 1), max(pt_cap, 1), 2), dtype=torch.int32, device="cuda")
    pi = torch.zeros((max(n, 1), max(pt_cap, 1)), dtype=torch.uint8, device="cuda")
    lp = torch.zeros((max(n, 1), max(ls_cap, 1), 2), dtype=torch.int32, device="cuda")
    li = torch.zeros((max(n, 1), max(ls_cap, 1)), dtype=torch.uint8, device="cuda")
    out = (gfpl.LoopResult * max(n, 1))()
    torch.cuda.synchronize()
    p = (lambda t: t.data_ptr()) if bufs else (lambda t: None)
    return ctx.L.gfpl_kf_loop_closure(ctx.h, v0, v1, n, C.byref(prm) if prm is not None else None, pt_cap, ls_cap,
                                      p(pp), p(pi), p(lp), p(li), out)


def test_error_paths(ctx, views):
    k0, k1 = views["size_63_64"]
    prm = gfpl.LoopParams.default()
    one0, one1 = (gfpl.KFViewStruct * 1)(k0.s), (gfpl.KFViewStruct * 1)(k1.s)
    assert _raw(ctx, one0, one1, 1, prm, 63, 64) == 0
    assert _raw(ctx, one0, one1, 0, prm, 0, 0) == 0                       # n = 0
    assert _raw(ctx, None, None, 0, prm, 0, 0) == 0
    assert _raw(ctx, one0, one1, 1, prm, 62, 64) == -5                    # GFPL_E_CAPACITY: n_pt > pt_cap
    assert _raw(ctx, one0, one1, 1, prm, 63, 63) == -5
    assert _raw(ctx, one0, one1, -1, prm, 63, 64) == -1                   # GFPL_E_INVALID
    assert _raw(ctx, one0, one1, 1, None, 63, 64) == -1
    assert _raw(ctx, None, one1, 1, prm, 63, 64) == -1
    assert _raw(ctx, one0, one1, 1, prm, 63, 64, bufs=False) == -1
    assert ctx.L.gfpl_kf_loop_closure(ctx.h, one0, one1, 1, C.byref(prm), 63, 64, None, None, None, None, None) == -1
    for fld in ("P", "pdesc", "sP", "eP", "ldesc"):
        bad = (gfpl.KFViewStruct * 1)(k0.s)
        setattr(bad[0], fld, None)
        assert _raw(ctx, bad, one1, 1, prm, 63, 64) == -1, fld
    for fld in ("pl", "pdesc", "le", "ldesc"):
        bad = (gfpl.KFViewStruct * 1)(k1.s)
        setattr(bad[0], fld, None)
        assert _raw(ctx, one0, bad, 1, prm, 63, 64) == -1, fld
    # the arrays the call does not read may be NULL
    ok0, ok1 = (gfpl.KFViewStruct * 1)(k0.s), (gfpl.KFViewStruct * 1)(k1.s)
    for v in (ok0[0], ok1[0]):
        v.pt_sigma2 = None
        v.ls_sigma2 = None
    ok0[0].pl = None
    ok0[0].le = None
    ok1[0].P = None
    ok1[0].sP = None
    ok1[0].eP = None
    assert _raw(ctx, ok0, ok1, 1, prm, 63, 64) == 0
    # a context without a camera
    h = C.c_void_p()
    gfpl.check(ctx.L.gfpl_create(0, C.c_void_p(0), C.byref(h)), "gfpl_create")
    try:
        assert ctx.L.gfpl_kf_loop_closure(h, one0, one1, 0, C.byref(prm), 0, 0, None, None, None, None, None) == -1
    finally:
        gfpl.check(ctx.L.gfpl_destroy(h), "gfpl_destroy")
