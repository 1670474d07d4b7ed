"""The keyframe match consumers on the GPU against the written cases of kf_match_cases.py:
gfpl_kf_common_matches / gfpl_kf_local_map_matches (k_kf_gate, k_kf_map_filter, the single-sequence k_knn2m)
against the numpy statement where a case has one, and against the oracle always.

Bar: pairs, counts and order are integer results, compared exactly; no tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gfpl
import oracle as O
import kf_match_cases as K

pytestmark = pytest.mark.gpu
SENTINEL = -0x5A5A5A5B


@pytest.fixture(scope="module")
def contexts():
    """one context per (camera, config), shared by every test of the module: a case sees what the last one left"""
    made = {}

    def get(c):
        if (c.cam, c.cfg) not in made:
            made[c.cam, c.cfg] = gfpl.Context(K.camera(c.cam), K.config(c.cfg))
        return made[c.cam, c.cfg]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def reference():
    """(oracle pairs, statement pairs or None) per case, computed once"""
    memo = {}

    def get(c):
        if id(c) not in memo:
            r = c.expected() if c.statement else None
            memo[id(c)] = (c.oracle(O), None if r is None else (r.pp, r.lp))
        return memo[id(c)]
    return get


def _check(c, contexts, reference):
    gp, gl = c.gpu(contexts(c))
    (op, ol), st = reference(c)
    if st is not None:
        np.testing.assert_array_equal(gp, st[0], err_msg="points, statement: " + c.what())
        np.testing.assert_array_equal(gl, st[1], err_msg="lines, statement: " + c.what())
    np.testing.assert_array_equal(gp, op, err_msg="points, oracle: " + c.what())
    np.testing.assert_array_equal(gl, ol, err_msg="lines, oracle: " + c.what())


@pytest.mark.parametrize("family", list(K.FAMILIES))
def test_equality(family, contexts, reference):
    for c in K.cases(family):
        _check(c, contexts, reference)


def test_leftovers(contexts, reference):
    """the whole list forward and then in reverse through the same contexts: no case depends on what the
    previous one left in a context or on the device"""
    for c in K.cases() + K.cases()[::-1]:
        _check(c, contexts, reference)


def _sentinel_cases():
    sizes = {(c.name, c.stage): c for c in K.cases("sizes")}
    six = [sizes[f"{n}x{n}", stage] for n in (2, 1025, 2049) for stage in ("common", "map")]
    few = [sizes[f"{K.FEW[i][0]}{K.FEW[i][1]}", stage] for i in (2, 7, 8) for stage in ("common", "map")]
    return six + few


@pytest.mark.parametrize("k", range(12))
def test_sentinels(k, contexts, reference):
    """the C ABI with caller-owned outputs of 2 n0 + 64 entries: nothing at or beyond 2 * count is written, and
    a kind with fewer than two rows on a side comes back with count 0 and an untouched buffer"""
    c = _sentinel_cases()[k]
    ctx = contexts(c)
    a, k1 = c.a.view("cuda"), c.k1.view("cuda")
    bufs = [torch.full((2 * n + 64,), SENTINEL, dtype=torch.int32, device="cuda") for n in c.n0]
    cnt = [C.c_int(-7), C.c_int(-7)]
    torch.cuda.synchronize()
    if c.stage == "common":
        rc = ctx.L.gfpl_kf_common_matches(ctx.h, C.byref(a.s), C.byref(k1.s), gfpl._ptr(bufs[0]), C.byref(cnt[0]),
                                          gfpl._ptr(bufs[1]), C.byref(cnt[1]))
    else:
        rc = ctx.L.gfpl_kf_local_map_matches(ctx.h, C.byref(a.s), C.byref(k1.s), C.c_double(c.ep[0]), C.c_double(c.ep[1]),
                                             gfpl._ptr(bufs[0]), C.byref(cnt[0]), gfpl._ptr(bufs[1]), C.byref(cnt[1]))
    assert rc == 0
    n1 = (c.k1.n_pt, c.k1.n_ls)
    for kind, ref in enumerate(reference(c)[0]):
        got, n = bufs[kind].cpu().numpy(), cnt[kind].value
        assert n == len(ref), (c.what(), kind)
        np.testing.assert_array_equal(got[:2 * n].reshape(-1, 2), ref, err_msg=c.what())
        assert (got[2 * n:] == SENTINEL).all(), (c.what(), kind, np.flatnonzero(got[2 * n:] != SENTINEL)[:8] + 2 * n)
        if min(c.n0[kind], n1[kind]) < 2:
            assert n == 0


def _knn_sets():
    out = []
    for c in K.cases("ties"):
        if c.stage == "common":
            for lines in (0, 1):
                q, t = c.descs(lines)
                out += [(c.name, q, t), (c.name, t, q)]
    return out


def test_single_sequence_knn(contexts):
    """Context.knn2 (launch_knn2, cell 1) on the tie families' descriptor sets, both directions: indices and
    float distances of the statement's knn-2, nt = 2 included"""
    ctx = contexts(K.cases("ties")[0])
    sets = _knn_sets()
    assert min(len(t) for _, _, t in sets) == 2 and max(len(t) for _, _, t in sets) > 1024
    for name, q, t in sets:
        qd, td = torch.from_numpy(q.copy()).cuda(), torch.from_numpy(t.copy()).cuda()
        idx = torch.full((2 * len(q),), -9, dtype=torch.int32, device="cuda")
        dist = torch.full((2 * len(q),), -9.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert ctx.knn2(qd, len(q), td, len(t), 1, idx, dist) == 0
        ctx.synchronize()
        ei, ed = K.knn2(q, t)
        np.testing.assert_array_equal(idx.cpu().numpy().reshape(-1, 2), ei, err_msg=f"{name} {len(q)}x{len(t)}")
        np.testing.assert_array_equal(dist.cpu().numpy().reshape(-1, 2), ed, err_msg=f"{name} {len(q)}x{len(t)}")


@pytest.mark.parametrize("stage", ["common", "map"])
def test_misaligned_descriptors_are_refused(stage, contexts):
    """include/gfpl.h: pdesc / ldesc are 16-byte aligned.  A descriptor pointer that is not comes back as
    GFPL_E_INVALID from the argument checks: nothing is allocated or launched, counts 0, outputs untouched."""
    c = [c for c in K.cases("align") if c.stage == "map"][0] if stage == "map" else K.cases("poses")[0]
    ctx = contexts(c)
    for side, field in ((0, "pdesc"), (1, "pdesc"), (0, "ldesc"), (1, "ldesc")):
        views = [c.a.view("cuda"), c.k1.view("cuda")]
        setattr(views[side].s, field, getattr(views[side].s, field) + 4)
        bufs = [torch.full((2 * n + 64,), SENTINEL, dtype=torch.int32, device="cuda") for n in c.n0]
        cnt = [C.c_int(-7), C.c_int(-7)]
        torch.cuda.synchronize()
        if stage == "common":
            rc = ctx.L.gfpl_kf_common_matches(ctx.h, C.byref(views[0].s), C.byref(views[1].s), gfpl._ptr(bufs[0]),
                                              C.byref(cnt[0]), gfpl._ptr(bufs[1]), C.byref(cnt[1]))
        else:
            rc = ctx.L.gfpl_kf_local_map_matches(ctx.h, C.byref(views[0].s), C.byref(views[1].s), C.c_double(1.0),
                                                 C.c_double(1.0), gfpl._ptr(bufs[0]), C.byref(cnt[0]), gfpl._ptr(bufs[1]),
                                                 C.byref(cnt[1]))
        assert rc == -1 and cnt[0].value == 0 and cnt[1].value == 0, (stage, side, field, rc)     # GFPL_E_INVALID
        assert all(bool((b == SENTINEL).all()) for b in bufs)
