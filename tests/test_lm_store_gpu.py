"""gfpl_lmstore_apply / _gather / _read (k_lm.hip) against tests/lm_store_ref.py.

Bar: equality of count, med_idx, every list row and the median row with the reference, for every
landmark a call names; no tolerance, no case left out.  The descriptors come from the generator of
tests/lm_store_cases.py, whose bar (ties and moved winners) is asserted on the reference first.
"""
import ctypes as C

import numpy as np
import pytest

import gfpl
import lm_store_cases as LC
import lm_store_ref as R

pytestmark = pytest.mark.gpu

LM_CAP, OBS_CAP, MAX_OPS = 4096, 64, 1 << 18
FAMILIES = 192   # landmarks' worth of 64 near-duplicate observations each
A, E, F = R.ADD, R.ERASE_OBS, R.FREE


class Env:
    def __init__(self):
        import torch
        LC.assert_adversarial()
        cfg = gfpl.default_config()
        self.cam, self.cfg = gfpl.make_camera("vga", cfg), cfg
        self.ctx = gfpl.Context(self.cam, cfg)
        rng = np.random.default_rng(2024)
        fam = np.stack([LC.near_duplicates(rng, 64) for _ in range(FAMILIES)])
        # family f lives in source f % 3, observation k at row (f // 3) * 64 + k: every call reads three sources
        self.host = [np.ascontiguousarray(fam[s::3].reshape(-1, 32)) for s in range(3)]
        self.dev = [torch.from_numpy(a.copy()).cuda() for a in self.host]

    @staticmethod
    def add(lm, f, k):
        return (lm, A, (f // 3) * 64 + k, f % 3)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


class Harness:
    """a fresh store and its model"""

    def __init__(self, env, lm_cap=LM_CAP, obs_cap=OBS_CAP, max_ops=MAX_OPS):
        self.env = env
        self.store = gfpl.LandmarkStore(env.ctx, lm_cap, obs_cap, max_ops)
        self.model = R.Model(lm_cap, obs_cap)

    def run(self, ops, compare=True):
        self.store.apply(ops, self.env.dev)
        touched = self.model.apply(ops, self.env.host)
        if compare:
            for lm in touched:
                self.same(lm)
        return touched

    def same(self, lm):
        got, want = self.store.read(lm), self.model.expect(lm)
        assert got["count"] == want["count"], (lm, got["count"], want["count"])
        assert got["med_idx"] == want["med_idx"], (lm, got["med_idx"], want["med_idx"], want["count"])
        assert np.array_equal(got["desc_list"][: want["count"]], want["rows"]), lm
        assert np.array_equal(got["med_desc"], want["med_desc"]), lm

    def snapshot(self):
        """every byte the store holds for every landmark"""
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


def _same_snapshot(a, b, keep=None):
    for x, y in zip(a, b):
        if keep is not None:
            x, y = x[keep], y[keep]
        assert np.array_equal(x, y)


def test_lengths_in_one_call(h):
    ops, lm = [], 0
    for n in LC.LENGTHS:
        for rep in range(4):
            ops += [Env.add(lm, (lm * 7) % FAMILIES, k) for k in range(n)]
            lm += 3 if rep % 2 else 1   # neighbours and gaps
    touched = h.run(ops)
    assert len(touched) == 4 * len(LC.LENGTHS)
    assert sum(h.model.expect(t)["med_idx"] > 0 for t in touched) >= 12   # the winners do move


def test_lengths_one_add_per_call(h):
    lms = {100 + 5 * i: n for i, n in enumerate(LC.LENGTHS)}
    for k in range(max(LC.LENGTHS)):
        ops = [Env.add(lm, lm % FAMILIES, k) for lm, n in lms.items() if k < n]
        h.run(ops)   # compares every landmark at every length 1 .. n
    assert [h.store.read(lm)["count"] for lm in lms] == list(LC.LENGTHS)


@pytest.mark.parametrize("n", [5, 9, 17, 64])
def test_erase_first_middle_last(h, n):
    for i, pos in enumerate((0, n // 2, n - 1)):
        h.run([Env.add(10 + i, 20 + i, k) for k in range(n)])
        h.run([(10 + i, E, pos, 0)])
        assert h.store.read(10 + i)["count"] == n - 1


def test_erase_down_to_one_and_none(h):
    h.run([Env.add(7, 3, k) for k in range(4)] + [Env.add(8, 4, k) for k in range(4)])
    h.run([(7, E, 1, 0), (7, E, 2, 0), (7, E, 0, 0)])               # one call, down to one
    r = h.store.read(7)
    assert (r["count"], r["med_idx"]) == (1, 0) and np.array_equal(r["med_desc"], h.env.host[0][64 + 2])
    for pos in (3, 0, 1):                                            # one call each
        h.run([(8, E, pos, 0)])
    assert h.store.read(8)["count"] == 1
    h.run([(8, E, 0, 0)])
    r = h.store.read(8)
    assert (r["count"], r["med_idx"]) == (0, -1) and not r["med_desc"].any()
    h.run([(7, E, 0, 0), (7, F, 0, 0), (7, F, 0, 0)])                # none, then NULL twice
    assert h.store.read(7)["med_idx"] == -1


def test_add_after_free_reuses_the_slot(h):
    h.run([Env.add(50, 9, k) for k in range(5)])
    h.run([(50, F, 0, 0)])
    r = h.store.read(50)
    assert (r["count"], r["med_idx"]) == (0, -1) and not r["med_desc"].any()
    h.run([Env.add(50, 10, k) for k in range(3)])
    # and within one call, with more rows before the FREE than after
    h.run([Env.add(51, 11, k) for k in range(9)] + [(51, F, 0, 0)] + [Env.add(51, 12, k) for k in range(2)])
    assert h.store.read(51)["count"] == 2


def test_add_erase_add_in_one_call(h):
    h.run([Env.add(60, 13, 0), Env.add(60, 13, 1), Env.add(60, 13, 2), (60, E, 1, 0), Env.add(60, 13, 3), (60, E, 0, 0),
           Env.add(60, 13, 4), Env.add(60, 13, 5)])
    assert h.store.read(60)["count"] == 4


def test_peaks_at_64_and_ends_at_3(h):
    rng = np.random.default_rng(5)
    ops = [Env.add(70, 14, k) for k in range(64)]
    ops += [(70, E, int(rng.integers(0, 64 - i)), 0) for i in range(61)]
    h.run(ops + [Env.add(71, 15, 0)])
    assert h.store.read(70)["count"] == 3


def test_all_buckets_and_op_counts_side_by_side(h):
    """landmark 200 + c runs c ops with its list as long as it can get (peaks 1 .. 64), landmark
    300 + c runs c ops that keep its list at 1-2 rows: every bucket in one call, and op counts 1 .. 70
    next to each other in the groups of a wave; the ops of all landmarks interleaved."""
    per = {}
    for c in range(1, 71):
        long = [Env.add(200 + c, c, k) for k in range(min(c, 64))] + [(200 + c, E, (5 * i) % (64 - i), 0) for i in range(c - 64)]
        short = []
        for i in range(c):
            short.append(Env.add(300 + c, 80 + c, i % 64) if i < 2 or i % 2 == 1 else (300 + c, E, (i // 2) % 2, 0))
        per[200 + c], per[300 + c] = long, short
    ops = []
    for i in range(70):
        ops += [l[i] for l in per.values() if i < len(l)]
    touched = h.run(ops)
    assert len(touched) == 140
    peaks = {h.model.expect(200 + c)["count"] for c in range(1, 65)}
    assert peaks == set(range(1, 65))


def test_rows_from_three_sources(h):
    h.run([Env.add(5, f, k) for k in range(3) for f in (30, 31, 32)])   # families 30, 31, 32: sources 0, 1, 2
    assert h.store.read(5)["count"] == 9


@pytest.mark.parametrize("min_lanes", [None, "64"])
def test_obs_cap_below_the_group_width(env, monkeypatch, min_lanes):
    """obs_cap 5: a landmark's rows end inside the 8 lanes of its group, and the next landmark's begin
    there; also with every landmark forced through k_lm_apply<64> (what tools/bench_lm_store.py compares with)"""
    if min_lanes:
        monkeypatch.setenv("GFPL_LM_MIN_LANES", min_lanes)
    s = Harness(env, 67, 5, 1024)
    s.run([Env.add(lm, lm, k) for k in range(5) for lm in range(67) if k < 1 + (lm * 3) % 5])
    s.run([(lm, E, 0, 0) for lm in range(0, 67, 2)] + [Env.add(lm, lm + 67, 9) for lm in range(1, 67, 2) if (lm * 3) % 5 < 4])
    for lm in range(67):
        s.same(lm)
    assert s.store.apply_rc([Env.add(3, 0, 0)], env.dev) == R.E_CAPACITY   # landmark 3 holds 5
    s.close()


def _poisoned(h):
    """every row of every landmark written once, then lists of 0 .. 7 rows left"""
    rng = np.random.default_rng(9)
    h.run([Env.add(lm, (lm * 5 + k) % FAMILIES, k) for lm in range(LM_CAP) for k in range(OBS_CAP)], compare=False)
    ops = []
    for lm in range(LM_CAP):
        keep = int(rng.integers(0, 8))
        ops += [(lm, F, 0, 0)] if keep == 0 else [(lm, E, OBS_CAP - 1 - i, 0) for i in range(OBS_CAP - keep)]
    h.run(ops, compare=False)


def test_untouched_neighbours_keep_their_bytes(h):
    _poisoned(h)
    before = h.snapshot()
    assert before[2].reshape(LM_CAP * OBS_CAP, 32).any(axis=1).all()   # no row was left unwritten
    rng = np.random.default_rng(10)
    touched_want = sorted({0, 1, 63, 64, 65, 4094, 4095} | set(int(v) for v in rng.integers(0, LM_CAP, 300)))
    ops = []
    for lm in touched_want:
        n = h.model.expect(lm)["count"]
        kind = int(rng.integers(0, 4))
        if kind == 0 and n > 0:
            ops.append((lm, E, int(rng.integers(0, n)), 0))
        elif kind == 1:
            ops.append((lm, F, 0, 0))
        else:
            ops += [Env.add(lm, (lm + 17) % FAMILIES, k) for k in range(int(rng.integers(1, 30)))]
    touched = h.run(ops)
    assert sorted(touched) == touched_want
    keep = np.ones(LM_CAP, bool)
    keep[touched] = False
    _same_snapshot(before, h.snapshot(), keep)


def test_refused_call_changes_nothing(h, env):
    good = [Env.add(lm, lm, k) for lm in (0, 1, 2, 3) for k in range(6)]
    h.run(good + [Env.add(9, 9, k) for k in range(OBS_CAP)])
    before = h.snapshot()
    lead = [Env.add(0, 40, 0), (1, E, 0, 0), (2, F, 0, 0)]   # valid ops ahead of the one that is refused
    assert h.store.apply_rc(lead + [Env.add(9, 9, 0)], env.dev) == R.E_CAPACITY
    _same_snapshot(before, h.snapshot())
    assert h.store.apply_rc(lead + [(3, E, 6, 0)], env.dev) == R.E_INVALID
    _same_snapshot(before, h.snapshot())
    ptrs = [t.data_ptr() for t in env.dev]
    ptrs[1] += 8
    assert h.store.apply_rc(lead + [Env.add(3, 31, 0)], env.dev, src_ptrs=ptrs) == R.E_INVALID   # family 31: source 1
    _same_snapshot(before, h.snapshot())
    small = Harness(env, 16, 4, 3)
    assert small.store.apply_rc([Env.add(0, 0, k) for k in range(4)], env.dev) == R.E_CAPACITY    # n > max_ops
    assert small.store.read(0)["count"] == 0
    small.close()
    # the store's counts are what they were: the same ops without the refused one go through
    h.run(lead)
    assert h.store.apply_rc([], env.dev) == R.OK   # n = 0


def test_gather_shuffled_and_repeated(h):
    rng = np.random.default_rng(12)
    lms = [int(v) for v in rng.choice(LM_CAP, 150, replace=False)]
    h.run([Env.add(lm, (lm * 3) % FAMILIES, k) for lm in lms for k in range(1 + lm % 9)])
    ids = np.array(lms + lms[:40] + [lms[0]] * 5, np.int32)
    rng.shuffle(ids)
    rows, idx = h.store.gather(ids, with_idx=True)
    want = [h.model.expect(int(i)) for i in ids]
    assert np.array_equal(rows.cpu().numpy(), np.stack([w["med_desc"] for w in want]))
    assert np.array_equal(idx.cpu().numpy(), np.array([w["med_idx"] for w in want]))
    assert len(h.store.gather([])) == 0


def test_gather_of_a_freed_id_is_refused(h, env):
    import torch
    h.run([Env.add(lm, lm, k) for lm in (1, 2, 3) for k in range(3)])
    h.run([(2, F, 0, 0)])
    out = torch.full((4, 32), 0xAB, dtype=torch.uint8, device="cuda")
    idx = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for ids in ([1, 2, 3], [1, 3, 4], [1, -1], [1, LM_CAP]):   # freed, never created, out of range
        a = np.array(ids, np.int32)
        rc = h.store.L.gfpl_lmstore_gather(h.store.h, a.ctypes.data, len(a), out.data_ptr(), idx.data_ptr())
        assert rc == R.E_INVALID, ids
    assert (out.cpu().numpy() == 0xAB).all() and (idx.cpu().numpy() == 77).all()
    a = np.array([1, 3], np.int32)
    assert h.store.L.gfpl_lmstore_gather(h.store.h, a.ctypes.data, 2, out.data_ptr() + 8, None) == R.E_INVALID
    assert h.store.L.gfpl_lmstore_gather(h.store.h, a.ctypes.data, 2, out.data_ptr(), None) == R.OK
    assert np.array_equal(out.cpu().numpy()[:2], np.stack([h.model.expect(1)["med_desc"], h.model.expect(3)["med_desc"]]))
    assert (out.cpu().numpy()[2:] == 0xAB).all() and (idx.cpu().numpy() == 77).all()


def test_gather_feeds_local_map_matches(env):
    """the local map's descriptors from the store: the pairs equal those from the reference's medians"""
    import torch
    from test_keyframe_matches import known_local_map
    (pdesc, P, ldesc, L), f1, T1, exp_pt, exp_ls = known_local_map(env.cam, 300, 120, 31)
    rng = np.random.default_rng(13)

    def observed(desc):
        """per map row 1-6 near-duplicate observations of its descriptor, the row itself among them"""
        lists = []
        for d in desc:
            obs = LC.near_duplicates(rng, int(rng.integers(1, 7)))
            obs ^= obs[0] ^ d   # the same flips around the map's descriptor
            lists.append(obs)
        return lists
    results = []
    for desc in (pdesc, ldesc):
        lists = observed(np.asarray(desc))
        src = np.concatenate(lists)
        st = gfpl.LandmarkStore(env.ctx, len(lists) + 5, 8, len(src))
        ops, row = [], 0
        for lm, l in enumerate(lists):
            ops += [(lm + 5, A, row + k, 0) for k in range(len(l))]
            row += len(l)
        st.apply(ops, [torch.from_numpy(src).cuda()])
        ids = np.arange(len(lists), dtype=np.int32) + 5
        want = np.stack([l[R.med_index(list(l))] for l in lists])
        got = st.gather(ids)
        assert np.array_equal(got.cpu().numpy(), want)
        results.append((got, want))
        st.close()
    (gp, wp), (gl, wl) = results
    kf1 = gfpl.KeyFrameView(f1, T1, "cuda")
    direct = gfpl.MapView(wp, P, wl, L, device="cuda")
    fed = gfpl.MapView(wp, P, wl, L, device="cuda")
    fed.keep["pdesc"], fed.keep["ldesc"] = gp, gl
    fed.s.pdesc, fed.s.ldesc = gp.data_ptr(), gl.data_ptr()
    a_pt, a_ls = env.ctx.lookForLocalMapMatches(direct, kf1)
    b_pt, b_ls = env.ctx.lookForLocalMapMatches(fed, kf1)
    assert len(a_pt) > 100 and len(a_ls) > 40
    assert np.array_equal(a_pt, b_pt) and np.array_equal(a_ls, b_ls)
