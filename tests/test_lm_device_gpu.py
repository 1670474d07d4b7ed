"""gfpl_lmstore_observe_pairs / _observe_local / _free_ids / _gather_ids / _counts (k_lm_plan.hip, k_lm.hip)
against tests/lm_store_ref.py's Model fed the host-built op list (tests/lm_device_cases.py).

Bar: after every call the WHOLE store (every landmark, touched or not) equals the model byte for byte:
count, med_idx, rows [0, count) and the median row; and equals a second store that was fed the same ops
through gfpl_lmstore_apply.  Rows at and past count are unspecified by the header and not compared with
the model; a refused call is compared on every byte, those rows included.  No tolerance.
"""
import numpy as np
import pytest

import gfpl
import lm_device_cases as DC
import lm_store_cases as LC
import lm_store_ref as R

pytestmark = pytest.mark.gpu

T, B = gfpl.LM_PLAN_TILE, gfpl.LM_BLOCK
POOL = 130 * 64          # rows of either descriptor pool: families of near-duplicates, so medians tie and move
OK, E, CAP = R.OK, R.E_INVALID, R.E_CAPACITY


class Env:
    def __init__(self):
        import torch
        cfg = gfpl.default_config()
        self.cam = gfpl.make_camera("vga", cfg)
        self.ctx = gfpl.Context(self.cam, cfg)
        rng = np.random.default_rng(410)
        self.host = [np.ascontiguousarray(np.concatenate([LC.near_duplicates(rng, 64) for _ in range(POOL // 64)])[rng.permutation(POOL)])
                     for _ in range(2)]
        self.dev = [torch.from_numpy(a.copy()).cuda() for a in self.host]


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


class Duo:
    """a store fed by the device-id calls, a store fed the same ops by gfpl_lmstore_apply, and the model"""

    def __init__(self, env, lm_cap, obs_cap, max_ops):
        self.env = env
        self.a = gfpl.LandmarkStore(env.ctx, lm_cap, obs_cap, max_ops)
        self.b = gfpl.LandmarkStore(env.ctx, lm_cap, obs_cap, max_ops)
        self.model = R.Model(lm_cap, obs_cap)
        self.expect = DC.Expect(self.model)

    def close(self):
        self.a.close()
        self.b.close()

    def check(self, where):
        got = DC.read_all(self.a)
        DC.assert_store_is_model(got, self.expect, where)
        DC.assert_stores_equal(got, DC.read_all(self.b), where)

    def host_route(self, ops, dev, host, where):
        self.b.apply(ops, dev)
        self.expect.touched(self.model.apply(ops, host))
        self.check(where)

    def pairs(self, pairs, lm_out, first_new, where="observe_pairs"):
        p, out = np.array(pairs, np.int32).reshape(-1, 2), np.array(lm_out, np.int32)
        self.a.observe_pairs(self.env.dev[0], self.env.dev[1], p, out, first_new)
        self.host_route(DC.pair_ops(p, out, first_new), self.env.dev, self.env.host, where)

    def local(self, pairs, unm_rows, lm_out, where="observe_local"):
        p, unm, out = np.array(pairs, np.int32).reshape(-1, 2), np.array(unm_rows, np.int32), np.array(lm_out, np.int32)
        self.a.observe_local(self.env.dev[1], p, unm, out)
        self.host_route(DC.local_ops(p, unm, out), self.env.dev[1:], self.env.host[1:], where)

    def free(self, ids, where="free_ids"):
        self.a.free(np.array(ids, np.int32))
        self.host_route(DC.free_ops(ids), [], [], where)

    def create(self, n, row0=0):
        """landmarks [0, n): two rows each, in one call"""
        self.pairs([(row0 + i, (row0 + 3 * i) % POOL) for i in range(n)], list(range(n)), 0, "create")


@pytest.fixture()
def duo(env):
    d = Duo(env, 96, 64, 512)
    yield d
    d.close()


# ------------------------------------------------------------------ base cases
def test_one_created_one_carried_one_skipped_and_none(duo):
    duo.pairs([(3, 5)], [0], 0, "n = 1 created")
    assert duo.a.read(0)["count"] == 2
    duo.pairs([(0, 7)], [0], 1, "n = 1 carried")
    assert duo.a.read(0)["count"] == 3
    before = DC.snapshot(duo.a)
    duo.pairs([(1, 1)], [-1], 1, "the only pair names no landmark")
    assert DC.same_snapshot(before, DC.snapshot(duo.a))
    duo.pairs([], [], 1, "n = 0")
    duo.local([], [], [], "n = 0 local")
    duo.free([], "n = 0 free")
    assert len(duo.a.gather_ids(np.zeros(0, np.int32))) == 0
    assert DC.same_snapshot(before, DC.snapshot(duo.a))


# ------------------------------------------------------------------ one landmark, several pairs
@pytest.mark.parametrize("where", ["adjacent", "workgroups", "scan_tile"])
@pytest.mark.parametrize("k", [2, 3])
def test_one_landmark_several_pairs_in_pair_order(env, where, k):
    at = {"adjacent": [4, 5, 6], "workgroups": [0, B + 3, 2 * B + 1], "scan_tile": [T - 1, T, 2 * T + 1]}[where][:k]
    n = at[-1] + 2
    d = Duo(env, 40, 16, n + 16)
    d.create(8)                                       # (16 ops)
    lm_out = np.full(n, -1, np.int32)
    lm_out[at] = 2
    lm_out[[1, n - 1]] = [5, 7]                       # single carriers around them
    pairs = [(0, (11 * i + 1) % POOL) for i in range(n)]
    d.pairs(pairs, lm_out, 8, f"{k} pairs {where}")
    got = d.a.read(2)
    assert got["count"] == 2 + k
    assert np.array_equal(got["desc_list"][2:2 + k], env.host[1][[pairs[i][1] for i in at]])   # pair order
    d.close()


def test_created_and_carried_side_by_side(duo):
    duo.create(5)
    duo.pairs([(10, 20), (11, 21), (12, 22), (13, 23), (14, 24)], [5, 0, 6, 1, 1], 5, "created beside carried")
    assert [duo.a.read(lm)["count"] for lm in (0, 1, 5, 6)] == [3, 4, 2, 2]


# ------------------------------------------------------------------ buckets
def _grow(duo, targets, first_new):
    """one call: landmark lm receives targets[lm] - its length pairs (a created one its one pair)"""
    pairs, lm_out, row = [], [], 40
    for lm, want in targets.items():
        have = duo.model.counts()[lm]
        for _ in range(1 if have == 0 else want - have):
            pairs.append((row, row + 1))
            lm_out.append(lm)
            row += 2
    order = np.random.default_rng(len(pairs)).permutation(len(pairs))   # the landmarks' pairs interleaved
    duo.pairs([pairs[i] for i in order], [lm_out[i] for i in order], first_new, f"grow to {sorted(targets.values())}")


def test_all_six_buckets_in_one_call_and_the_cap(duo):
    duo.create(7)
    _grow(duo, {3: 8, 4: 10, 5: 32, 6: 40}, 7)
    # lists reach 2 (created), 3, 5, 9, 17, 33 and 64 = obs_cap in ONE call: buckets G = 2, 4, 8, 16, 32, 64, 64
    _grow(duo, {7: 2, 1: 3, 2: 5, 3: 9, 4: 17, 5: 33, 6: 64}, 7)
    assert [duo.a.read(lm)["count"] for lm in (7, 1, 2, 3, 4, 5, 6)] == [2, 3, 5, 9, 17, 33, 64]
    before = DC.snapshot(duo.a)
    assert duo.a.observe_pairs_rc(duo.env.dev[0], duo.env.dev[1], [(0, 0)], [6], 8) == CAP   # 64 + 1
    assert duo.a.observe_pairs_rc(duo.env.dev[0], duo.env.dev[1], [(0, 0), (1, 1), (2, 2)], [5, 0, 6], 8) == CAP
    assert DC.same_snapshot(before, DC.snapshot(duo.a))
    duo.pairs([(0, 0), (1, 1)], [5, 0], 8, "after the refusal")


@pytest.mark.parametrize("min_lanes", [None, "64"])
def test_obs_cap_below_the_group_width(env, monkeypatch, min_lanes):
    """obs_cap 3: a landmark's rows end inside the 4 lanes of its group; also with every landmark through G = 64"""
    if min_lanes:
        monkeypatch.setenv("GFPL_LM_MIN_LANES", min_lanes)
    d = Duo(env, 67, 3, 256)
    d.create(67)
    odd = list(range(1, 67, 2))
    d.pairs([(lm, lm + 100) for lm in odd], odd, 67, "to obs_cap")
    before = DC.snapshot(d.a)
    assert d.a.observe_pairs_rc(env.dev[0], env.dev[1], [(0, 0)], [3], 67) == CAP       # landmark 3 holds 3
    assert d.a.observe_pairs_rc(env.dev[0], env.dev[1], [(0, 0), (1, 1)], [2, 2], 67) == CAP   # 2 + 2
    assert DC.same_snapshot(before, DC.snapshot(d.a))
    d.pairs([(5, 6)], [2], 67, "after the refusal")
    d.close()


# ------------------------------------------------------------------ scan boundaries
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_scan_boundaries(env, n):
    """n touched landmarks, all created (n work items, 2 n ops); then n pairs that carry the even ones and
    create new ones in between, so that op offsets and work offsets differ"""
    d = Duo(env, n + n // 2 + 3, 4, 2 * n)
    d.create(n, row0=17)
    assert int(d.a.counts().sum()) == 2 * n
    lm_out = [i if i % 2 == 0 else n + i // 2 for i in range(n)]
    d.pairs([((5 * i) % POOL, (7 * i + 3) % POOL) for i in range(n)], lm_out, n, "carried and created mixed")
    assert int(d.a.counts().sum()) == 2 * n + (n + 1) // 2 + 2 * (n // 2)
    d.close()


def test_a_tile_whose_leaders_own_more_ops_than_16_bits(env):
    """2048 landmarks of one row each; pairs 0 .. 2047 name them in order and the sequence repeats 33 times: every
    leader sits in tile 0 and bucket G = 64 with 33 ops, 67,584 ops in one tile and bucket, and every later tile
    holds no leader at all"""
    n_lm, reps = T, 33
    d = Duo(env, n_lm, 64, n_lm * reps)
    first = [(lm, R.ADD, lm, 0) for lm in range(n_lm)]
    d.a.apply(first, env.dev)
    d.host_route(first, env.dev, env.host, "one row each")
    lm_out = np.tile(np.arange(n_lm, dtype=np.int32), reps)
    pairs = np.stack([np.zeros(n_lm * reps, np.int32), (np.arange(n_lm * reps, dtype=np.int32) * 5 + 1) % POOL], 1)
    d.pairs(pairs, lm_out, n_lm, "33 pairs per landmark")
    assert (d.a.counts() == 1 + reps).all()
    got = d.a.read(n_lm - 1)["desc_list"]
    assert np.array_equal(got[1:1 + reps], env.host[1][pairs[n_lm - 1::n_lm, 1]])   # the last landmark's rows in pair order
    d.close()


def test_lengths_of_pairs_and_lm_out_must_agree(duo, env):
    with pytest.raises(ValueError):
        duo.a.observe_pairs_rc(env.dev[0], env.dev[1], [(0, 0), (1, 1)], [0], 0)
    with pytest.raises(ValueError):
        duo.a.observe_local_rc(env.dev[1], [(0, 0), (0, 1)], [3, 4], [0, 1, 2])


# ------------------------------------------------------------------ observe_local
def test_observe_local_through_shuffled_unm_rows(duo, env):
    duo.create(12)
    rng = np.random.default_rng(8)
    unm = rng.permutation(300)[:40]                   # kf1's rows without a landmark, shuffled
    cols = rng.permutation(40)[:14]
    lm_out = [0, 1, 2, 3, 3, 5, -1, 7, 8, 3, 10, 11, 0, 1]
    duo.local([(-999 - i, int(c)) for i, c in enumerate(cols)], unm, lm_out, "local")   # column 0 is not read
    assert duo.a.read(3)["count"] == 5
    assert np.array_equal(duo.a.read(3)["desc_list"][2:5], env.host[1][unm[cols[[3, 4, 9]]]])
    before = DC.snapshot(duo.a)
    bad = unm.copy()
    bad[cols[2]] = POOL                               # a row outside n1
    assert duo.a.observe_local_rc(env.dev[1], [(0, int(c)) for c in cols], bad, lm_out) == E
    assert DC.same_snapshot(before, DC.snapshot(duo.a))
    duo.local([(0, int(cols[2]))], unm, [2], "after the refusal")


# ------------------------------------------------------------------ free_ids
def test_free_ids(duo):
    duo.create(10)
    duo.pairs([(1, 2), (3, 4)], [4, 4], 10)
    duo.free([4, 7], "free")
    for lm in (4, 7):
        r = duo.a.read(lm)
        assert (r["count"], r["med_idx"]) == (0, -1) and not r["med_desc"].any()
    assert duo.a.read(4)["desc_list"][:4].any(axis=1).all()       # the rows are left as they are
    duo.free([2, 2, 4, 9, 2], "a repeated id, an empty landmark")
    duo.pairs([(30, 31), (32, 33)], [4, 2], 2, "an add after a free reuses the slot")   # (ids >= 2 count as created)
    assert duo.a.read(4)["count"] == 2


# ------------------------------------------------------------------ gather_ids
def test_gather_ids_equals_the_host_gather(duo):
    duo.create(60)
    duo.pairs([(i, 2 * i) for i in range(45)], [i % 30 for i in range(45)], 60)
    import torch
    rng = np.random.default_rng(12)
    ids = np.array(list(range(60)) + list(range(20)) + [7] * 5, np.int32)
    rng.shuffle(ids)
    rows, idx = duo.a.gather_ids(torch.from_numpy(ids).cuda(), with_idx=True)
    want_rows, want_idx = duo.a.gather(ids, with_idx=True)
    assert np.array_equal(rows.cpu().numpy(), want_rows.cpu().numpy()) and np.array_equal(idx.cpu().numpy(), want_idx.cpu().numpy())
    assert np.array_equal(rows.cpu().numpy(), np.stack([duo.model.expect(int(i))["med_desc"] for i in ids]))
    assert np.array_equal(idx.cpu().numpy(), np.array([duo.model.expect(int(i))["med_idx"] for i in ids]))
    head = duo.a.gather_ids(torch.from_numpy(ids).cuda(), n=9)
    assert np.array_equal(head.cpu().numpy(), want_rows.cpu().numpy()[:9])


def test_gather_ids_of_a_freed_id_is_refused(duo):
    import torch
    duo.create(4)
    duo.free([2])
    out = torch.full((4, 32), 0xAB, dtype=torch.uint8, device="cuda")
    idx = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    L, h = duo.a.L, duo.a.h
    for ids in ([1, 2, 3], [1, 3, 50], [1, -1], [1, 96]):   # freed, never created, out of range
        t = torch.tensor(ids, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert L.gfpl_lmstore_gather_ids(h, t.data_ptr(), len(ids), out.data_ptr(), idx.data_ptr()) == E, ids
    t = torch.tensor([1, 3], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.gfpl_lmstore_gather_ids(h, t.data_ptr(), 2, out.data_ptr() + 8, None) == E
    assert L.gfpl_lmstore_gather_ids(h, None, 2, out.data_ptr(), None) == E
    assert L.gfpl_lmstore_gather_ids(h, t.data_ptr(), -1, out.data_ptr(), None) == E
    assert (out.cpu().numpy() == 0xAB).all() and (idx.cpu().numpy() == 77).all()
    assert L.gfpl_lmstore_gather_ids(h, t.data_ptr(), 2, out.data_ptr(), None) == OK
    assert np.array_equal(out.cpu().numpy()[:2], np.stack([duo.model.expect(1)["med_desc"], duo.model.expect(3)["med_desc"]]))
    assert (out.cpu().numpy()[2:] == 0xAB).all() and (idx.cpu().numpy() == 77).all()


# ------------------------------------------------------------------ refusals change nothing
def test_refusals_change_nothing(env):
    import torch
    d = Duo(env, 24, 4, 64)
    d.create(10)
    d.pairs([(1, 1), (2, 2), (3, 3), (4, 4)], [8, 8, 9, 7], 10)          # 8 holds 4 = obs_cap, 9 and 7 hold 3
    d0, d1 = env.dev
    st, L = d.a, d.a.L
    before = DC.snapshot(st)
    pt = lambda rows: torch.tensor(rows, dtype=torch.int32, device="cuda")
    P1, O1 = pt([[0, 0]]), pt([0])
    torch.cuda.synchronize()
    raw = lambda a0, a1, p, o, n, fn: L.gfpl_lmstore_observe_pairs(st.h, a0, POOL, a1, POOL, p, o, n, fn)
    rawl = lambda a1, p, n, u, nu, o: L.gfpl_lmstore_observe_local(st.h, a1, POOL, p, n, u, nu, o)
    cases = {
        # ---- GFPL_E_INVALID on the host: NULL, n < 0, alignment, first_new
        "desc0 NULL": lambda: raw(None, d1.data_ptr(), P1.data_ptr(), O1.data_ptr(), 1, 10),
        "desc1 NULL": lambda: raw(d0.data_ptr(), None, P1.data_ptr(), O1.data_ptr(), 1, 10),
        "pairs NULL": lambda: raw(d0.data_ptr(), d1.data_ptr(), None, O1.data_ptr(), 1, 10),
        "lm_out NULL": lambda: raw(d0.data_ptr(), d1.data_ptr(), P1.data_ptr(), None, 1, 10),
        "n < 0": lambda: raw(d0.data_ptr(), d1.data_ptr(), P1.data_ptr(), O1.data_ptr(), -1, 10),
        "desc0 misaligned": lambda: raw(d0.data_ptr() + 8, d1.data_ptr(), P1.data_ptr(), O1.data_ptr(), 1, 10),
        "desc1 misaligned": lambda: raw(d0.data_ptr(), d1.data_ptr() + 8, P1.data_ptr(), O1.data_ptr(), 1, 10),
        "first_new < 0": lambda: st.observe_pairs_rc(d0, d1, [(0, 0)], [0], -1),
        "first_new > lm_cap": lambda: st.observe_pairs_rc(d0, d1, [(0, 0)], [0], 25),
        "local desc1 NULL": lambda: rawl(None, P1.data_ptr(), 1, O1.data_ptr(), 1, O1.data_ptr()),
        "local unm NULL": lambda: rawl(d1.data_ptr(), P1.data_ptr(), 1, None, 1, O1.data_ptr()),
        "local n_unm < 0": lambda: rawl(d1.data_ptr(), P1.data_ptr(), 1, O1.data_ptr(), -1, O1.data_ptr()),
        "local desc1 misaligned": lambda: rawl(d1.data_ptr() + 16 + 8, P1.data_ptr(), 1, O1.data_ptr(), 1, O1.data_ptr()),
        "free NULL": lambda: L.gfpl_lmstore_free_ids(st.h, None, 1),
        "free n < 0": lambda: L.gfpl_lmstore_free_ids(st.h, O1.data_ptr(), -1),
        # ---- GFPL_E_INVALID on the device
        "p0 = n0": lambda: st.observe_pairs_rc(d0, d1, [(1, 1), (POOL, 0)], [0, 1], 10),
        "p0 < 0": lambda: st.observe_pairs_rc(d0, d1, [(-1, 0), (1, 1)], [0, 1], 10),
        "p1 = n1": lambda: st.observe_pairs_rc(d0, d1, [(1, 1), (0, POOL)], [0, 1], 10),
        "p1 < 0 of a skipped pair": lambda: st.observe_pairs_rc(d0, d1, [(1, 1), (0, -3)], [0, -1], 10),
        "local p1 = n_unm": lambda: st.observe_local_rc(d1, [(0, 0), (0, 2)], [5, 6], [0, 1]),
        "local p1 < 0": lambda: st.observe_local_rc(d1, [(0, 0), (0, -1)], [5, 6], [0, 1]),
        "unm_rows = n1": lambda: st.observe_local_rc(d1, [(0, 0), (0, 1)], [5, POOL], [0, 1]),
        "unm_rows < 0": lambda: st.observe_local_rc(d1, [(0, 0), (0, 1)], [5, -1], [0, 1]),
        "lm_out = -2": lambda: st.observe_pairs_rc(d0, d1, [(0, 0), (1, 1)], [0, -2], 10),
        "lm_out = lm_cap": lambda: st.observe_pairs_rc(d0, d1, [(0, 0), (1, 1)], [0, 24], 10),
        "local lm_out = lm_cap": lambda: st.observe_local_rc(d1, [(0, 0), (0, 1)], [5, 6], [0, 24]),
        "free id = -1": lambda: st.free_rc([0, -1]),
        "free id = lm_cap": lambda: st.free_rc([0, 24]),
        "created id holds rows": lambda: st.observe_pairs_rc(d0, d1, [(0, 0), (1, 1)], [0, 5], 5),
        "created id twice": lambda: st.observe_pairs_rc(d0, d1, [(0, 0), (1, 1), (2, 2)], [12, 0, 12], 10),
        "carried id is empty": lambda: st.observe_pairs_rc(d0, d1, [(0, 0), (1, 1)], [0, 12], 13),
        "local carried id is empty": lambda: st.observe_local_rc(d1, [(0, 0), (0, 1)], [5, 6], [0, 12]),
        "both kinds are INVALID": lambda: st.observe_pairs_rc(d0, d1, [(0, 0), (1, 1)], [8, -2], 10),
    }
    cap_cases = {
        "a list past obs_cap": lambda: st.observe_pairs_rc(d0, d1, [(0, 0), (1, 1)], [0, 8], 10),
        "two pairs past obs_cap": lambda: st.observe_pairs_rc(d0, d1, [(0, 0), (1, 1), (2, 2)], [9, 0, 9], 10),
        "local past obs_cap": lambda: st.observe_local_rc(d1, [(0, 0), (0, 1)], [5, 6], [0, 8]),
        "n > max_ops": lambda: st.observe_pairs_rc(d0, d1, [(0, 0)] * 65, [-1] * 65, 10),
    }
    named = [0, 1, 5, 8, 9, 12]
    for want, group in ((E, cases), (CAP, cap_cases)):
        for name, call in group.items():
            assert call() == want, name
            assert DC.same_snapshot(before, DC.snapshot(st)), name
            # the scratch was cleared: valid calls on EVERY landmark a refused call names (0, 1, 5, 8, 9, 12) go through
            # and equal the model; a pend word left set on one of them would refuse the create or misplace its rows.
            # They end in the state the cases rely on: 8 holds 4, 9 holds 3, 12 is empty, the others hold 2.
            d.free(named, "after " + name)
            d.pairs([(6 + i, 7 + i) for i in range(len(named))], named, 0, "after " + name)
            d.pairs([(1, 1), (2, 2), (3, 3)], [8, 8, 9], 10, "after " + name)
            d.free([12], "after " + name)
            before = DC.snapshot(st)
    d.close()
    # ops past max_ops, decided on the device: three created pairs are six ops
    s = Duo(env, 8, 4, 5)
    before = DC.snapshot(s.a)
    assert s.a.observe_pairs_rc(d0, d1, [(0, 0), (1, 1), (2, 2)], [0, 1, 2], 0) == CAP
    assert DC.same_snapshot(before, DC.snapshot(s.a))
    s.pairs([(0, 0), (1, 1)], [0, 1], 0, "four ops fit")
    s.pairs([(0, 0), (1, 1), (2, 2)], [0, 1, 0], 2, "three ops fit")
    s.close()


# ------------------------------------------------------------------ the host mirror
def test_mirror_follows_the_device(duo, env):
    duo.create(6)                                                          # device-id call ...
    ops = [(lm, R.ADD, 50 + lm, 1) for lm in (0, 1, 2)] + [(3, R.ERASE_OBS, 0, 0), (4, R.FREE, 0, 0)]
    duo.a.apply(ops, env.dev)                                              # ... then a host apply on the same landmarks
    duo.host_route(ops, env.dev, env.host, "device-id call, then apply")
    duo.pairs([(7, 8), (9, 10), (11, 12)], [0, 3, 4], 4, "apply, then device-id call")   # (4 was freed: created again)
    duo.pairs([(20, 21)], [9], 9, "creates 9")
    rows = duo.a.gather([9, 0])                                            # host-id gather of a landmark the device call created
    assert np.array_equal(rows.cpu().numpy(), np.stack([duo.model.expect(9)["med_desc"], duo.model.expect(0)["med_desc"]]))
    assert np.array_equal(duo.a.counts(), duo.model.counts())
    fuse = [(0, gfpl.LM_APPEND_LM, 9, 0), (9, R.FREE, 0, 0)]               # fuse reads the mirror too
    duo.a.fuse(fuse, env.dev)
    duo.b.fuse(fuse, env.dev)
    duo.model.lists[0] += duo.model.lists[9]
    duo.model.lists[9] = []
    duo.expect.touched([0, 9])
    duo.check("device-id call, then fuse")
    assert np.array_equal(duo.a.counts(), duo.model.counts())


def test_a_store_that_never_uses_them_keeps_its_bytes(env):
    s = gfpl.LandmarkStore(env.ctx, 64, 8, 128)
    n0 = s.nbytes()
    s.apply([(0, R.ADD, 0, 0)], [env.dev[0]])
    assert s.nbytes() == n0
    s.observe_pairs(env.dev[0], env.dev[1], [(1, 1)], [1], 1)
    assert s.nbytes() > n0 and s.last_device_ms() >= 0.0
    s.close()


# ------------------------------------------------------------------ a tick
class DeviceMap:
    """a gfpl.KeyframeMap behind the interface lm_device_cases.tick drives: host lists for the bookkeeping,
    the device tensors beside them for the stores"""

    def __init__(self, ctx, caps):
        self.km = gfpl.KeyframeMap(ctx, *caps)

    def add_keyframe(self, n_pt, n_ls):
        return self.km.add_keyframe(n_pt, n_ls)

    @staticmethod
    def upload(pairs):
        import torch
        return torch.from_numpy(np.array(pairs, np.int32).reshape(-1, 2)).cuda()

    def observe_pairs(self, kind, kf0, kf1, pairs):
        p = self.upload(pairs)
        out, first, new = self.km.observe_pairs(kind, kf0, kf1, p)
        return out.cpu().tolist(), first, new, (p, out)

    def observe_local(self, kind, kf1, pairs, sel, unm, hs, hu):
        p = self.upload(pairs)
        out = self.km.observe_local(kind, kf1, p, hs, hu)
        return out.cpu().tolist(), (p, out)

    def select(self, kind, which, kf1):
        t = self.km.select(kind, which, kf1)
        return t.cpu().tolist(), t

    def unmatched(self, kind, kf):
        t = self.km.unmatched(kind, kf)
        return t.cpu().tolist(), t

    def form_local_map(self, prm):
        self.km.form_local_map(gfpl.KfMapParams.default(**prm))

    def remove_bad(self, prm):
        pt, ls = self.km.remove_bad(gfpl.KfMapParams.default(**prm))
        return [pt.cpu().tolist(), ls.cpu().tolist()], (pt, ls)


class StoreSink:
    """the tick's device arrays into two stores (points, lines); the host-built ops into the models and a second pair of stores"""

    def __init__(self, env, caps, desc):
        import torch
        self.desc = desc
        self.dev = [[torch.from_numpy(d.copy()).cuda() for d in per] for per in desc]
        self.duo = [Duo(env, caps[3], caps[5], 256), Duo(env, caps[4], caps[5], 256)]
        self.gathered = [None, None]

    def pairs(self, kind, kf0, kf1, pairs, lm_out, first, h):
        d = self.duo[kind]
        d.a.observe_pairs(self.dev[kf0][kind], self.dev[kf1][kind], h[0], h[1], first)
        d.host_route(DC.pair_ops(pairs, lm_out, first), [self.dev[kf0][kind], self.dev[kf1][kind]],
                     [self.desc[kf0][kind], self.desc[kf1][kind]], f"tick pairs {kf1}/{kind}")

    def local(self, kind, kf1, pairs, unm, lm_out, h, hu):
        d = self.duo[kind]
        d.a.observe_local(self.dev[kf1][kind], h[0], hu, h[1])
        d.host_route(DC.local_ops(pairs, unm, lm_out), [self.dev[kf1][kind]], [self.desc[kf1][kind]], f"tick local {kf1}/{kind}")

    def free(self, kind, ids, h):
        d = self.duo[kind]
        d.a.free(h)
        d.host_route(DC.free_ops(ids), [], [], f"tick free {kind}")

    def gather(self, kind, kf1, sel, h):
        d = self.duo[kind]
        rows = d.a.gather_ids(h)
        want = np.stack([d.model.expect(j)["med_desc"] for j in sel]) if sel else np.zeros((0, 32), np.uint8)
        assert np.array_equal(rows.cpu().numpy(), want), ("tick gather", kf1, kind)
        self.gathered[kind] = (rows, want)


def test_a_tick(env):
    import mapgeo_cases as MC
    w = MC.World(env.cam, 3, DC.TICK_KFS, 60, 30, 40, 20)
    dm = DeviceMap(env.ctx, DC.TICK_CAPS)
    sink = StoreSink(env, DC.TICK_CAPS, DC.tick_descriptors(w))
    DC.assert_tick_facts(DC.tick(dm, w, sink))
    for kind in (0, 1):
        assert np.array_equal(sink.duo[kind].a.counts(), sink.duo[kind].model.counts())
    # the gathered rows feed gfpl_kf_local_map_matches as the reference's medians do
    from test_keyframe_matches import known_local_map
    (pdesc, P, ldesc, Lm), f1, T1, exp_pt, exp_ls = known_local_map(env.cam, 300, 120, 31)
    import torch
    fed_rows = []
    for desc in (pdesc, ldesc):
        desc = np.ascontiguousarray(np.asarray(desc, np.uint8))
        n = len(desc)
        st = gfpl.LandmarkStore(env.ctx, n, 4, 2 * n)
        src = torch.from_numpy(desc.copy()).cuda()
        ids = torch.arange(n, dtype=torch.int32, device="cuda")
        st.observe_pairs(src, src, torch.stack([ids, ids], 1).contiguous(), ids, 0)   # every row twice: its own median
        fed_rows.append(st.gather_ids(ids))
        assert np.array_equal(fed_rows[-1].cpu().numpy(), desc)
        st.close()
    kf1 = gfpl.KeyFrameView(f1, T1, "cuda")
    direct = gfpl.MapView(np.asarray(pdesc), P, np.asarray(ldesc), Lm, device="cuda")
    fed = gfpl.MapView(np.asarray(pdesc), P, np.asarray(ldesc), Lm, device="cuda")
    fed.keep["pdesc"], fed.keep["ldesc"] = fed_rows
    fed.s.pdesc, fed.s.ldesc = fed_rows[0].data_ptr(), fed_rows[1].data_ptr()
    a_pt, a_ls = env.ctx.lookForLocalMapMatches(direct, kf1)
    b_pt, b_ls = env.ctx.lookForLocalMapMatches(fed, kf1)
    assert len(a_pt) > 100 and len(a_ls) > 40
    assert np.array_equal(a_pt, b_pt) and np.array_equal(a_ls, b_ls)
    for d in sink.duo:
        d.close()
    dm.km.close()
