"""gfpl_map_fuse_search (k_fuse.hip) against lm_fuse_ref.search.

Bar: equality of loc, the counts and the pair lists with the reference, in order.  The maps come
from tests/fuse_search_cases.py, whose conditions (both branches of the line gate taken, both
gates deciding both ways, a mirrored pair) are asserted on the reference first.
"""
import numpy as np
import pytest

import fuse_search_cases as SC
import gfpl
import lm_fuse_ref as FR

pytestmark = pytest.mark.gpu


class Env:
    def __init__(self):
        cfg = gfpl.default_config()
        self.cam = gfpl.make_camera("vga", cfg)
        self.camd = SC.cam_dict(self.cam)
        SC.assert_not_blunt(self.camd)
        self.ctx = gfpl.Context(self.cam, cfg)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


def _run(env, pt, ls, prm=None):
    """one call over a point map and a line map (desc, X, kf, T) against the reference per kind"""
    fm = gfpl.FuseMap(pt[0], pt[1], pt[2], ls[0], ls[1], ls[2], pt[3], device="cuda")
    rc, got = env.ctx.fuseSearch_rc(fm, gfpl.FuseParams.default(**prm) if prm else None)
    ref_prm = dict(FR.DEFAULT_FUSE_PARAMS, **(prm or {}))
    want = [FR.search(env.camd, d, X, kf, T, ref_prm) for d, X, kf, T in (pt, ls)]
    return rc, got, want


def _same(got, want):
    for k, (loc, pairs, _) in zip(("pt", "ls"), want):
        assert np.array_equal(got[k + "_loc"], loc), k
        assert got[k + "_pairs"].shape == pairs.shape and np.array_equal(got[k + "_pairs"], pairs), k


@pytest.mark.parametrize("n", SC.SIZES)
def test_sizes_both_kinds(env, n):
    pt, ls = SC.make_map(env.camd, n, False, 1), SC.make_map(env.camd, n, True, 1)
    rc, got, want = _run(env, pt, ls)
    assert rc == 0
    _same(got, want)
    if n >= 31:
        assert len(want[0][1]) > 0 and len(want[1][1]) > 0 and len(want[0][0]) < n


def test_kinds_of_different_sizes_and_other_thresholds(env):
    """the kinds are independent: a large point map with no lines, one line with many points, and
    thresholds that move every gate"""
    empty_ls = SC.make_map(env.camd, 0, True, 2)
    rc, got, want = _run(env, SC.make_map(env.camd, 1500, False, 2), empty_ls)
    assert rc == 0 and len(got["ls_loc"]) == 0 and len(got["ls_pairs"]) == 0
    _same(got, want)
    rc, got, want = _run(env, SC.make_map(env.camd, 700, False, 3), SC.make_map(env.camd, 1, True, 3))
    assert rc == 0
    _same(got, want)
    prm = dict(max_point_point_error=0.06, max_point_line_error=0.05, max_dir_line_error=0.2)
    rc, got, want = _run(env, SC.make_map(env.camd, 1100, False, 4), SC.make_map(env.camd, 1100, True, 4), prm)
    assert rc == 0
    _same(got, want)
    base = FR.search(env.camd, *SC.make_map(env.camd, 1100, False, 4))[1]
    assert 0 < len(want[0][1]) < len(base)


def test_repeated_calls_reuse_the_workspace(env):
    big = SC.make_map(env.camd, 2049, False, 5), SC.make_map(env.camd, 1025, True, 5)
    small = SC.make_map(env.camd, 40, False, 6), SC.make_map(env.camd, 33, True, 6)
    for pt, ls in (small, big, small, big):
        rc, got, want = _run(env, pt, ls)
        assert rc == 0
        _same(got, want)


@pytest.mark.parametrize("bad", [-1, SC.N_KF, 2 ** 31 - 1, -2 ** 31])
def test_keyframe_index_out_of_range(env, bad):
    """the row is never used as an index: the call returns GFPL_E_INVALID, and the same map without
    the row's fault still searches"""
    pt, ls = list(SC.make_map(env.camd, 300, False, 7)), list(SC.make_map(env.camd, 300, True, 7))
    for m, at in ((pt, 17), (ls, 299)):
        kf = m[2].copy()
        kf[at] = bad
        broken = list(m)
        broken[2] = kf
        rc, got, want = _run(env, broken if m is pt else pt, broken if m is ls else ls)
        assert rc == FR.E_INVALID and (want[0][2] or want[1][2])
    rc, got, want = _run(env, pt, ls)
    assert rc == 0
    _same(got, want)


def test_arguments(env):
    import ctypes as C
    pt, ls = SC.make_map(env.camd, 64, False, 8), SC.make_map(env.camd, 64, True, 8)
    fm = gfpl.FuseMap(pt[0], pt[1], pt[2], ls[0], ls[1], ls[2], pt[3], device="cuda")
    rc, got = env.ctx.fuseSearch_rc(fm)
    assert rc == 0
    L, prm = env.ctx.L, gfpl.FuseParams.default()
    assert (prm.max_point_point_error, prm.max_point_line_error, prm.max_dir_line_error) == (0.1, 0.1, 0.1)
    import torch
    out = [torch.zeros(128, dtype=torch.int32, device="cuda") for _ in range(4)]
    cnt = [C.c_int(-5) for _ in range(4)]

    def call(ctx=env.ctx.h, m=fm.s, p=prm, skip=None):
        a = [ctx, C.byref(m) if m is not None else None, C.byref(p) if p is not None else None]
        for k in range(4):
            a += [out[k].data_ptr() if skip != ("o", k) else None, C.byref(cnt[k]) if skip != ("c", k) else None]
        torch.cuda.synchronize()
        return L.gfpl_map_fuse_search(*a)
    assert call() == 0 and [c.value for c in cnt] == [len(got["pt_loc"]), len(got["pt_pairs"]), len(got["ls_loc"]), len(got["ls_pairs"])]
    assert call(ctx=None) == FR.E_INVALID and call(m=None) == FR.E_INVALID and call(p=None) == FR.E_INVALID
    for k in range(4):
        assert call(skip=("o", k)) == FR.E_INVALID and call(skip=("c", k)) == FR.E_INVALID
    # a misaligned descriptor pointer of a kind with two or more rows is refused; of a kind with one row it is not read
    for field in ("pdesc", "ldesc"):
        s = gfpl.FuseMapStruct.from_buffer_copy(fm.s)
        setattr(s.map, field, getattr(s.map, field) + 8)
        assert call(m=s) == FR.E_INVALID, field
        setattr(s.map, "n_pt" if field == "pdesc" else "n_ls", 1)
        assert call(m=s) == 0, field
    for field in ("P", "L", "pdesc", "ldesc"):
        s = gfpl.FuseMapStruct.from_buffer_copy(fm.s)
        setattr(s.map, field, None)
        assert call(m=s) == FR.E_INVALID, field
    for field in ("pt_kf", "ls_kf", "T_kf"):
        s = gfpl.FuseMapStruct.from_buffer_copy(fm.s)
        setattr(s, field, None)
        assert call(m=s) == FR.E_INVALID, field
    s = gfpl.FuseMapStruct.from_buffer_copy(fm.s)
    s.map.n_pt = -1
    assert call(m=s) == FR.E_INVALID
    assert call() == 0


def test_context_without_camera(env):
    L = env.ctx.L
    import ctypes as C
    h = C.c_void_p()
    assert L.gfpl_create(0, None, C.byref(h)) == 0
    pt, ls = SC.make_map(env.camd, 8, False, 9), SC.make_map(env.camd, 8, True, 9)
    fm = gfpl.FuseMap(pt[0], pt[1], pt[2], ls[0], ls[1], ls[2], pt[3], device="cuda")
    import torch
    out = [torch.zeros(32, dtype=torch.int32, device="cuda") for _ in range(4)]
    cnt = [C.c_int(0) for _ in range(4)]
    prm = gfpl.FuseParams.default()
    a = [h, C.byref(fm.s), C.byref(prm)]
    for k in range(4):
        a += [out[k].data_ptr(), C.byref(cnt[k])]
    torch.cuda.synchronize()
    assert L.gfpl_map_fuse_search(*a) == FR.E_INVALID
    assert L.gfpl_destroy(h) == 0
