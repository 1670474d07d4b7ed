"""gfpl_lmstore_fuse (gfpl_lm_fuse_plan.cpp, k_lm.hip) against tests/lm_fuse_ref.py.

Bar: equality of count, med_idx, every list row and the median row with the model, for every
landmark an op names; no tolerance, no case left out.  The descriptors come from the generator of
tests/lm_store_cases.py, whose bar (ties and moved winners) is asserted on the reference first.
"""
import numpy as np
import pytest

import gfpl
import lm_fuse_cases as FC
import lm_fuse_ref as FR
import lm_store_cases as LC
from test_lm_store_gpu import Env, FAMILIES, _same_snapshot

pytestmark = pytest.mark.gpu

LM_CAP, OBS_CAP, MAX_OPS = 512, 64, 1 << 15
A, E, F, M = FR.ADD, FR.ERASE_OBS, FR.FREE, FR.APPEND_LM


@pytest.fixture(scope="module")
def env():
    e = Env()   # asserts the generator's bar
    yield e
    e.ctx.close()


class Harness:
    """a fresh store and its sequential model"""

    def __init__(self, env, lm_cap=LM_CAP, obs_cap=OBS_CAP, max_ops=MAX_OPS):
        self.env = env
        self.store = gfpl.LandmarkStore(env.ctx, lm_cap, obs_cap, max_ops)
        self.model = FR.Model(lm_cap, obs_cap)

    def fill(self, lengths, first_family=0):
        """landmark lm gets lengths[lm] observations of family first_family + lm, through apply"""
        ops = [Env.add(lm, (first_family + lm) % FAMILIES, k) for lm, n in lengths.items() for k in range(n)]
        self.store.apply(ops, self.env.dev)
        self.model.apply(ops, self.env.host)
        return ops

    def fuse(self, ops):
        rc, _, _, _ = self.model.fuse_check(ops, [len(a) for a in self.env.host])
        assert rc == FR.OK
        self.store.fuse(ops, self.env.dev)
        named = self.model.fuse(ops, self.env.host)
        for lm in named:
            self.same(lm)
        return named

    def same(self, lm):
        got, want = self.store.read(lm), self.model.expect(lm)
        assert got["count"] == want["count"], (lm, got["count"], want["count"])
        assert got["med_idx"] == want["med_idx"], (lm, got["med_idx"], want["med_idx"], want["count"])
        assert np.array_equal(got["desc_list"][: want["count"]], want["rows"]), lm
        assert np.array_equal(got["med_desc"], want["med_desc"]), lm

    def snapshot(self):
        rs = [self.store.read(lm) for lm in range(self.store.lm_cap)]
        return (np.array([r["count"] for r in rs]), np.array([r["med_idx"] for r in rs]),
                np.stack([r["desc_list"] for r in rs]), np.stack([r["med_desc"] for r in rs]))

    def close(self):
        self.store.close()


@pytest.fixture()
def h(env):
    x = Harness(env)
    yield x
    x.close()


def _crossed_lengths():
    """(destination, source) lengths from LENGTHS whose sum fits; most change the bucket"""
    return [(d, s) for d in LC.LENGTHS for s in LC.LENGTHS if d + s <= OBS_CAP]


def test_lengths_crossed(h):
    """one append per pair of LENGTHS, the same family on both sides so that the merged list has ties;
    the source kept for the even pairs and freed for the odd ones"""
    pairs = _crossed_lengths()
    assert len(pairs) > 100 and 2 * len(pairs) <= LM_CAP
    bucket = lambda n: max(0, int(np.ceil(np.log2(max(n, 2)))) - 1)
    assert sum(bucket(d + s) != bucket(d) for d, s in pairs) > 60        # the final list changes bucket
    lengths, ops = {}, []
    for i, (d, s) in enumerate(pairs):
        lengths[2 * i], lengths[2 * i + 1] = d, s
    # destination 2i and source 2i + 1 hold different observations of one family
    fill = [Env.add(2 * i, i % FAMILIES, k) for i, (d, s) in enumerate(pairs) for k in range(d)]
    fill += [Env.add(2 * i + 1, i % FAMILIES, d + k) for i, (d, s) in enumerate(pairs) for k in range(s)]
    h.store.apply(fill, h.env.dev)
    h.model.apply(fill, h.env.host)
    for i in range(len(pairs)):
        ops.append((2 * i, M, 2 * i + 1, 0))
        if i % 2:
            ops.append((2 * i + 1, F, 0, 0))
    named = h.fuse(ops)
    assert len(named) == len(pairs) + len(pairs) // 2
    for i in range(0, len(pairs), 2):                                     # a landmark named only as arg is unchanged
        h.same(2 * i + 1)
    assert sum(h.model.expect(2 * i)["med_idx"] >= pairs[i][0] for i in range(len(pairs))) >= 10   # winners among the appended rows


def test_one_wave_of_32_landmarks_with_different_op_counts(h):
    """destinations of 1 row each that gain 1 .. 32 rows: k_lm_apply<64>'s bucket aside, the G = 2 ..
    32 launches carry groups whose op counts differ within a wave"""
    h.fill({lm: 1 for lm in range(32)})
    h.fill({100 + lm: 1 + lm % 7 for lm in range(32)}, first_family=50)
    ops = []
    for step in range(32):
        for lm in range(32):
            if step < lm + 1:
                ops.append(Env.add(lm, lm, 1 + step) if (step + lm) % 3 else (lm, M, 100 + (lm + step) % 32, 0))
    ok = []
    cnt = {lm: 1 for lm in range(32)}
    for op in ops:                                     # keep what fits
        n = 1 if op[1] == A else 1 + (op[2] - 100) % 7
        if cnt[op[0]] + n <= OBS_CAP:
            cnt[op[0]] += n
            ok.append(op)
    named = h.fuse(ok)
    assert len(named) == 32 and len({cnt[lm] for lm in range(32)}) >= 20


def test_chain_ring_and_own_rows_back(h):
    h.fill({0: 3, 1: 2, 2: 4, 10: 2, 11: 3, 20: 5, 21: 1})
    named = h.fuse([
        (1, M, 0, 0), (2, M, 1, 0), (3, A, 7, 0), (3, M, 2, 0),         # a chain of depth 3: 0 -> 1 -> 2 -> 3
        (10, M, 11, 0), (11, M, 10, 0),                                  # a ring, both kept
        (20, M, 21, 0), (21, M, 20, 0), (20, M, 21, 0),                  # 20 receives its own rows from before the call back
    ])
    assert named == [1, 2, 3, 10, 11, 20, 21]
    assert [h.store.read(lm)["count"] for lm in (0, 1, 2, 3)] == [3, 5, 9, 10]
    assert [h.store.read(lm)["count"] for lm in (10, 11)] == [5, 8]
    assert [h.store.read(lm)["count"] for lm in (20, 21)] == [6 + 7, 7]
    h.same(0)
    # and a second call over the merged lists: the store's rows of the first call are origins now
    h.fuse([(0, M, 3, 0), (3, F, 0, 0), (11, M, 21, 0), (21, F, 0, 0)])
    assert h.store.read(0)["count"] == 13 and h.store.read(3)["count"] == 0


def test_source_freed_in_the_same_call_and_added_to_before(h):
    h.fill({0: 4, 1: 6, 2: 33, 3: 31})
    h.fuse([Env.add(1, 60, 0), Env.add(1, 60, 1), (0, M, 1, 0), (1, F, 0, 0), Env.add(0, 61, 3),
            (2, M, 3, 0), (3, F, 0, 0)])
    assert [h.store.read(lm)["count"] for lm in range(4)] == [13, 0, 64, 0]
    r = h.store.read(1)
    assert r["med_idx"] == -1 and not r["med_desc"].any()


@pytest.mark.parametrize("seed", [1, 2])
def test_random_2000_ops_over_64_landmarks(env, seed):
    s = Harness(env, 64, OBS_CAP, 1 << 13)
    rng = np.random.default_rng(seed)
    start = {lm: int(rng.integers(0, 6)) for lm in range(64)}
    s.fill(start)
    rows = [len(a) for a in env.host]
    ops = FC.random_mixed(64, OBS_CAP, rows, 2000, seed, start=[start[lm] for lm in range(64)], max_from=8)
    assert len(ops) == 2000 and sum(o[1] == M for o in ops) >= 100 and sum(o[1] == F for o in ops) >= 10
    s.fuse(ops)
    for lm in range(64):
        s.same(lm)
    s.close()


def test_refused_calls_change_nothing(h, env):
    h.fill({0: 6, 1: 6, 2: 6, 3: 6, 9: OBS_CAP - 3, 10: 4})
    before = h.snapshot()
    lead = [Env.add(0, 40, 0), (1, M, 2, 0), (2, F, 0, 0)]   # valid ops ahead of the one that is refused
    assert h.store.fuse_rc(lead + [(9, M, 10, 0)], env.dev) == FR.E_CAPACITY
    _same_snapshot(before, h.snapshot())
    for bad in ((3, M, 3, 0), (3, M, LM_CAP, 0), (3, M, 2, 0), (2, A, 0, 0), (3, M, 50, 0), (50, M, 3, 0), (3, 4, 0, 0)):
        assert h.store.fuse_rc(lead + [bad], env.dev) == FR.E_INVALID, bad
    _same_snapshot(before, h.snapshot())
    assert h.store.fuse_rc(lead + [(3, E, 0, 0)], env.dev) == FR.E_UNSUPPORTED
    _same_snapshot(before, h.snapshot())
    ptrs = [t.data_ptr() for t in env.dev]
    ptrs[1] += 8
    assert h.store.fuse_rc(lead + [Env.add(3, 31, 0)], env.dev, src_ptrs=ptrs) == FR.E_INVALID   # family 31: source 1
    _same_snapshot(before, h.snapshot())
    small = Harness(env, 16, 8, 5)
    small.fill({0: 2, 1: 2})
    assert small.store.fuse_rc([(0, M, 1, 0), (1, M, 0, 0)], env.dev) == FR.E_CAPACITY   # n_rows 2 + 4 > max_ops 5
    small.same(0), small.same(1)
    small.fuse([(0, M, 1, 0), Env.add(0, 3, 0), (1, F, 0, 0), Env.add(2, 3, 1)])         # n_rows 5
    small.close()
    # the store's counts are what they were: the same ops without the refused one go through
    h.fuse(lead)
    assert h.store.fuse_rc([], env.dev) == FR.OK   # n = 0


def test_apply_and_gather_after_fuse(h):
    h.fill({lm: 1 + lm % 5 for lm in range(40)})
    h.fuse([(lm, M, lm + 20, 0) for lm in range(20)] + [(lm + 20, F, 0, 0) for lm in range(0, 20, 2)])
    ops = [Env.add(lm, 70 + lm, 5) for lm in range(20)] + [(3, E, 0, 0), (21, F, 0, 0), Env.add(20, 90, 0)]
    h.store.apply(ops, h.env.dev)
    for lm in h.model.apply(ops, h.env.host):
        h.same(lm)
    ids = np.array(list(range(20)) + [20, 23], np.int32)
    rows, idx = h.store.gather(ids, with_idx=True)
    want = [h.model.expect(int(i)) for i in ids]
    assert np.array_equal(rows.cpu().numpy(), np.stack([w["med_desc"] for w in want]))
    assert np.array_equal(idx.cpu().numpy(), np.array([w["med_idx"] for w in want]))
    assert max(w["count"] for w in want) >= 10


def _walk_env(env, rng):
    """3 keyframes whose descriptor arrays are the sources; 40 landmarks of 1-3 observations"""
    kf_desc = [np.ascontiguousarray(a[:256]) for a in env.host]
    m = FR.Map(40, kf_desc)
    for lm in range(40):
        m.observe(lm, 0, lm)
        if lm % 2:
            m.observe(lm, 1, lm)
        if lm % 5 == 0:
            m.observe(lm, 2, lm)
    return m


def test_loop_closure_walk_end_to_end(env):
    """loopClosureFuseLandmarks' walk over rows that hit all four cases; its ops through one fuse"""
    from test_lm_fuse_cpu import WALK_ROWS
    import torch
    m = _walk_env(env, np.random.default_rng(3))
    srcs = [torch.from_numpy(d.copy()).cuda() for d in m.kf_desc]
    st = gfpl.LandmarkStore(env.ctx, 64, 16, 256)
    st.apply([(lm, A, row, kf) for lm, l in enumerate(m.lms) for kf, row in l.obs_list], srcs)
    ops, max_idx = FR.loop_closure_fuse_walk(m, 0, 2, WALK_ROWS, 40)
    assert max_idx == 42 and {o[1] for o in ops} == {A, F, M}
    st.fuse(ops, srcs)
    for lm in range(max_idx):
        got = st.read(lm)
        l = [] if m.lms[lm] is None else m.lms[lm].desc_list
        mi = FR.R.med_index(l)
        assert (got["count"], got["med_idx"]) == (len(l), mi), lm
        assert np.array_equal(got["desc_list"][: len(l)], np.array(l, np.uint8).reshape(-1, 32)), lm
        assert np.array_equal(got["med_desc"], l[mi] if l else np.zeros(32, np.uint8)), lm
    st.close()
