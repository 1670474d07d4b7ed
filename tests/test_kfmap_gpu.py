"""gfpl.KeyframeMap (k_kfmap.hip, gfpl_kfmap.cpp) against the model of tests/kfmap_ref.py.

Bar: equality of the whole state after every call (every keyframe's rows and flags, every landmark
record, full_graph, the exported lists) and of every returned list and count; no tolerance, no case
left out.  The drivers of tests/kfmap_cases.py compare after each call; each test's situation is
asserted on the model (tests/test_kfmap_cpu.py asserts the same without a GPU).

One refusal of include/gfpl.h cannot be reached through the interface and is not exercised here: a
carried id >= the next id on a keyframe's row (write_keyframe_idx refuses to write one on the host;
the kernel's check stands behind it).
"""
import numpy as np
import pytest

import gfpl
import kfmap_cases as KC
import kfmap_ref as R

pytestmark = pytest.mark.gpu

T = gfpl.KFMAP_TILE


@pytest.fixture(scope="module")
def ctx():
    cfg = gfpl.default_config()
    c = gfpl.Context(gfpl.make_camera("vga", cfg), cfg)
    yield c
    for km in MAPS:            # (a test that failed midway left its map open)
        km.close()
    c.close()


MAPS = []


def make_map(ctx, *caps):
    MAPS.append(gfpl.KeyframeMap(ctx, *caps))
    return MAPS[-1]


def make_pair(ctx, caps):
    return KC.Pair(caps, make_map(ctx, *caps))


def test_sixteen_keyframes(ctx):
    pair = make_pair(ctx, KC.SIXTEEN_CAPS)
    KC.assert_sixteen_facts(KC.sixteen_keyframes(pair))
    assert pair.km.nbytes() == gfpl.kfmap_bytes(gfpl.KfMapCaps(*KC.SIXTEEN_CAPS)) > 0
    assert pair.km.last_device_ms() >= 0.0
    pair.km.close()


@pytest.mark.parametrize("quirk", KC.QUIRKS, ids=[q.__name__ for q in KC.QUIRKS])
def test_pinned_quirks(ctx, quirk):
    pair = make_pair(ctx, KC.QUIRK_CAPS)
    quirk(pair)
    pair.km.close()


# ---------------------------------------------------------------------------- compaction boundaries
def patterns(n):
    z = np.zeros(n, np.uint8)
    out = [("none", z.copy()), ("all", z + 1), ("alternating", (np.arange(n) % 2).astype(np.uint8))]
    first, last = z.copy(), z.copy()
    first[:1] = 1
    last[-1:] = 1
    return out + [("first", first), ("last", last)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_select_boundaries(ctx, n):
    kind = n % 2                                   # both kinds take the same path; alternate them
    caps = (4, 4, 4, 3 * T + 8, 3 * T + 8, 2)
    km = make_map(ctx, *caps)
    assert km.add_keyframe(4, 4) == 0 and km.add_keyframe(4, 4) == 1
    one = np.ones(n, np.uint8)
    owner = np.full(n, -1, np.int32)
    nobs = np.full(n, 2, np.int32)
    seen0 = np.zeros((n, 2), np.int32)             # kf_obs [0, 0]: back() != 1
    for name, f in patterns(n):
        want = np.flatnonzero(f).tolist()
        km.write_landmarks(kind, 0, f, one, one, nobs, owner, seen0)
        assert km.counts()[1 + kind] == n
        assert km.select(kind, gfpl.KFMAP_ALIVE).cpu().tolist() == want, (name, "alive")
        assert km.select(kind, gfpl.KFMAP_LOCAL).cpu().tolist() == want, (name, "alive under local")
        km.write_landmarks(kind, 0, one, f, one, nobs, owner, seen0)
        assert km.select(kind, gfpl.KFMAP_LOCAL).cpu().tolist() == want, (name, "local")
        assert km.select(kind, gfpl.KFMAP_ALIVE).cpu().tolist() == list(range(n)), name
        assert km.select(kind, gfpl.KFMAP_LOCAL_UNSEEN, 1).cpu().tolist() == want, (name, "local, unseen by flag")
        back = seen0.copy()
        back[:, 1] = 1 - f.astype(np.int32)        # kf_obs.back() == kf1 exactly where f is 0
        km.write_landmarks(kind, 0, one, one, one, nobs, owner, back)
        assert km.select(kind, gfpl.KFMAP_LOCAL_UNSEEN, 1).cpu().tolist() == want, (name, "unseen")
        assert km.select(kind, gfpl.KFMAP_LOCAL_UNSEEN, 0).cpu().tolist() == np.flatnonzero(1 - f).tolist(), (name, "unseen 0")
        assert km.select(1 - kind, gfpl.KFMAP_ALIVE).cpu().tolist() == []
    km.close()


def test_unmatched_boundaries(ctx):
    counts = [0, 1, 63, 64, 65, 1025]
    km = make_map(ctx, len(counts), 1025, 1025, 4, 4, 2)
    for k, n in enumerate(counts):
        assert km.add_keyframe(n, counts[-1 - k]) == k
    for kind in (0, 1):
        km.write_landmarks(kind, 0, [1], [0], [1], [1], [-1], np.zeros((1, 2), np.int32))
    for k, n in enumerate(counts):
        for kind, rows in ((0, n), (1, counts[-1 - k])):
            assert km.unmatched(kind, k).cpu().tolist() == list(range(rows))      # a new keyframe: every row
            for name, f in patterns(rows):
                km.write_keyframe_idx(kind, k, 0, f.astype(np.int32) - 1)         # -1 where f is 0, landmark 0 elsewhere
                assert km.unmatched(kind, k).cpu().tolist() == np.flatnonzero(1 - f).tolist(), (k, kind, name)
    km.close()


# ---------------------------------------------------------------------------- one graph word under contention
def test_one_graph_word_under_contention(ctx):
    n = 300
    pair = make_pair(ctx, (4, n, 2, 2 * n, 4, 4))
    for _ in range(3):
        pair.add_keyframe(n, 2)
    rng = np.random.default_rng(11)
    rc, lm_out, first, new = pair.observe_pairs(0, 0, 1, list(zip(rng.permutation(n).tolist(), rng.permutation(n).tolist())))
    assert (rc, first, new) == (R.OK, 0, n)
    rc, lm_out, first, new = pair.observe_pairs(0, 1, 2, list(zip(rng.permutation(n).tolist(), rng.permutation(n).tolist())))
    assert (rc, new) == (R.OK, 0) and sorted(lm_out) == list(range(n))
    g = pair.km.export_graph()["full_graph"]
    assert all(lm.kf_obs_list == [0, 1, 2] for lm in pair.model.map_lms[0])     # every landmark lists keyframe 0
    assert g[2][0] == g[0][2] == n and g[2][1] == g[1][2] == n and g[0][1] == g[1][0] == n
    pair.km.close()


# ---------------------------------------------------------------------------- capacity and refusals
def refusal_map(ctx):
    """tests/kfmap_cases.py's hand-written map, keyframe 5 erased, landmark 3 freed on the device and
    in the model, landmark 0 with a full list (obs_cap 4)"""
    pair = KC.quirk_map(make_pair(ctx, KC.QUIRK_CAPS))
    assert pair.erase_keyframe(5) == R.OK
    assert pair.write_landmarks(0, 3, [0], [0], [0], [0], [-1], [[]]) == R.OK
    assert pair.observe_pairs(0, 1, 2, [(0, 0), (1, 1)])[0] == R.OK
    assert pair.observe_pairs(0, 2, 3, [(0, 0)])[0] == R.OK                    # landmark 0: [0, 1, 2, 3], full
    assert pair.write_keyframe_idx(0, 3, 1, [1]) == R.OK                       # landmark 1: [0, 1, 2], obs_cap - 1
    return pair


OBSERVE_PAIRS = [   # (name, code, kind, kf0, kf1, pairs with valid ones ahead of the bad one, the bad entry's index)
    ("row0_past", R.E_INVALID, 0, 3, 4, [(4, 0), (5, 1), (6, 2)], 2),
    ("row0_negative", R.E_INVALID, 0, 3, 4, [(4, 0), (-1, 1)], 1),
    ("row1_past", R.E_INVALID, 0, 3, 4, [(4, 0), (5, 6)], 1),
    ("row1_negative", R.E_INVALID, 0, 3, 4, [(4, 0), (5, -2)], 1),
    ("column0_twice", R.E_INVALID, 0, 3, 4, [(4, 0), (5, 1), (4, 2)], 2),
    ("column1_twice", R.E_INVALID, 0, 3, 4, [(4, 0), (5, 1), (2, 0)], 2),
    ("list_full", R.E_CAPACITY, 0, 3, 4, [(4, 0), (0, 1)], 1),
    ("invalid_wins", R.E_INVALID, 0, 3, 4, [(0, 1), (4, 0), (5, 9)], 2),
]


@pytest.mark.parametrize("case", OBSERVE_PAIRS, ids=[c[0] for c in OBSERVE_PAIRS])
def test_observe_pairs_refusals(ctx, case):
    name, code, kind, kf0, kf1, pairs, bad = case
    pair = refusal_map(ctx)
    before = KC.raw_snapshot(pair.km)
    assert pair.observe_pairs(kind, kf0, kf1, pairs)[0] == code
    assert KC.same_snapshot(KC.raw_snapshot(pair.km), before), name
    good = pairs[:bad] + pairs[bad + 1:]
    if name == "invalid_wins":
        good = good[1:]                                # (the full list's pair is a refusal of its own)
    rc, lm_out, first, new = pair.observe_pairs(kind, kf0, kf1, good)
    assert rc == R.OK and new >= 1 and not KC.same_snapshot(KC.raw_snapshot(pair.km), before), name
    pair.km.close()


def test_observe_pairs_argument_refusals(ctx):
    pair = refusal_map(ctx)
    before = KC.raw_snapshot(pair.km)
    for kind, kf0, kf1 in ((2, 3, 4), (-1, 3, 4), (0, 3, 3), (0, 5, 4), (0, 4, 5), (0, 13, 4), (0, 3, -1)):
        assert pair.observe_pairs(kind, kf0, kf1, [(4, 0)])[0] == R.E_INVALID, (kind, kf0, kf1)
    assert pair.observe_pairs(0, 3, 4, [(r, r) for r in range(6)] + [(0, 0)])[0] == R.E_INVALID    # more pairs than rows
    assert pair.km.erase_keyframe_rc(5) == pair.km.erase_keyframe_rc(13) == R.E_INVALID
    assert pair.km.add_keyframe_rc(7, 0)[0] == pair.km.add_keyframe_rc(0, 5)[0] == R.E_CAPACITY
    assert pair.km.add_keyframe_rc(-1, 0)[0] == R.E_INVALID
    assert KC.same_snapshot(KC.raw_snapshot(pair.km), before)
    assert pair.observe_pairs(0, 3, 4, [(4, 0)])[0] == R.OK
    pair.km.close()


def test_list_capacity(ctx):
    pair = refusal_map(ctx)
    m = pair.model
    assert len(m.lm(0, 1).kf_obs_list) == KC.QUIRK_CAPS[5] - 1
    rc, lm_out, _, _ = pair.observe_pairs(0, 3, 4, [(1, 1)])                     # obs_cap - 1 takes one more entry
    assert (rc, lm_out) == (R.OK, [1]) and len(m.lm(0, 1).kf_obs_list) == KC.QUIRK_CAPS[5]
    before = KC.raw_snapshot(pair.km)
    sel, unm = [0, 1, 2], pair.model.unmatched(0, 6)
    assert pair.observe_local(0, 6, [(2, 0), (1, 1)], sel, unm)[0] == R.E_CAPACITY   # landmark 1 is full now
    assert KC.same_snapshot(KC.raw_snapshot(pair.km), before)
    # two appends to one list in one call count together: landmark 2 has [0, 1, 7] and room for one
    assert pair.observe_pairs(0, 1, 7, [(2, 0)])[1] == [2]
    assert pair.write_keyframe_idx(0, 4, 2, [2]) == R.OK and pair.write_keyframe_idx(0, 4, 3, [2]) == R.OK
    before = KC.raw_snapshot(pair.km)
    assert pair.observe_pairs(0, 4, 6, [(0, 0), (2, 1), (3, 2)])[0] == R.E_CAPACITY
    assert KC.same_snapshot(KC.raw_snapshot(pair.km), before)
    assert pair.observe_pairs(0, 4, 6, [(0, 0), (2, 1)])[0] == R.OK
    pair.km.close()


def test_id_capacity(ctx):
    caps = (3, 8, 8, 5, 5, 4)
    pair = make_pair(ctx, caps)
    for _ in range(3):
        pair.add_keyframe(8, 8)
    assert pair.observe_pairs(1, 0, 1, [(r, r) for r in range(4)])[0] == R.OK     # 4 of 5 line ids
    before = KC.raw_snapshot(pair.km)
    assert pair.observe_pairs(1, 0, 1, [(4, 4), (5, 5)])[0] == R.E_CAPACITY       # ids past the cap
    assert KC.same_snapshot(KC.raw_snapshot(pair.km), before)
    assert pair.observe_pairs(1, 0, 1, [(4, 4)])[0] == R.OK
    assert pair.observe_pairs(1, 1, 2, [(5, 0)])[0] == R.E_CAPACITY
    assert pair.observe_pairs(0, 1, 2, [(5, 0)])[0] == R.OK                       # the point ids are their own space
    assert pair.add_keyframe(1, 1)[0] == R.E_CAPACITY
    pair.km.close()


OBSERVE_LOCAL = [   # (name, pairs, sel_ids, unm_rows, the bad pair's index or None when a list is bad)
    ("p0_past", [(1, 0), (3, 1)], [0, 1, 2], [0, 1, 2], 1),
    ("p0_negative", [(1, 0), (-1, 1)], [0, 1, 2], [0, 1, 2], 1),
    ("p1_past", [(1, 0), (2, 3)], [0, 1, 2], [0, 1, 2], 1),
    ("column0_twice", [(1, 0), (2, 1), (1, 2)], [0, 1, 2], [0, 1, 2], 2),
    ("column1_twice", [(1, 0), (2, 1), (0, 1)], [0, 1, 2], [0, 1, 2], 2),
    ("sel_freed", [(1, 0), (2, 1)], [0, 1, 3], [0, 1, 2], 1),
    ("sel_past_next", [(1, 0), (2, 1)], [0, 1, 99], [0, 1, 2], 1),
    ("sel_negative", [(1, 0), (2, 1)], [0, 1, -1], [0, 1, 2], 1),
    ("unm_past_rows", [(1, 0), (2, 1)], [0, 1, 2], [0, 77, 2], 1),
    ("unm_negative", [(1, 0), (2, 1)], [0, 1, 2], [0, -3, 2], 1),
    ("unm_row_twice", [(1, 0), (2, 1)], [0, 1, 2], [4, 4, 2], 1),
]


@pytest.mark.parametrize("case", OBSERVE_LOCAL, ids=[c[0] for c in OBSERVE_LOCAL])
def test_observe_local_refusals(ctx, case):
    name, pairs, sel, unm, bad = case
    pair = refusal_map(ctx)
    before = KC.raw_snapshot(pair.km)
    assert pair.observe_local(0, 6, pairs, sel, unm)[0] == R.E_INVALID
    assert KC.same_snapshot(KC.raw_snapshot(pair.km), before), name
    rc, lm_out = pair.observe_local(0, 6, pairs[:bad] + pairs[bad + 1:], sel, unm)
    assert rc == R.OK and len(lm_out) == len(pairs) - 1, name
    assert not KC.same_snapshot(KC.raw_snapshot(pair.km), before)
    pair.km.close()


def test_other_refusals(ctx):
    pair = refusal_map(ctx)
    km = pair.km
    before = KC.raw_snapshot(km)
    for kind, which, kf1 in ((2, 0, 0), (0, 3, 0), (0, -1, 0), (0, gfpl.KFMAP_LOCAL_UNSEEN, 5), (0, gfpl.KFMAP_LOCAL_UNSEEN, 13)):
        with pytest.raises(gfpl.GfplError) as e:
            km.select(kind, which, kf1)
        assert e.value.code == R.E_INVALID
    for kind, kf in ((2, 0), (0, 5), (0, 13), (0, -1)):
        with pytest.raises(gfpl.GfplError) as e:
            km.unmatched(kind, kf)
        assert e.value.code == R.E_INVALID
    assert pair.set_inlier(0, [0, 1, 4], 0) == R.E_INVALID          # 4 is the next id: valid ids ahead of it
    assert pair.set_inlier(0, [0, -1], 0) == R.E_INVALID
    assert km.set_inlier_rc(0, np.array([0], np.int32), 2) == R.E_INVALID
    assert pair.observe_local(0, 5, [], [], [])[0] == R.E_INVALID   # an erased keyframe
    assert pair.write_keyframe_idx(0, 3, 5, [0, 0]) == R.E_INVALID  # past the keyframe's rows
    assert pair.write_keyframe_idx(0, 3, 0, [5]) == R.E_INVALID     # an id that does not exist
    assert pair.write_keyframe_idx(0, 5, 0, [0]) == R.E_INVALID
    assert pair.write_landmarks(0, 0, [1], [0], [1], [5], [-1], [[0, 1, 2, 3, 4]]) == R.E_INVALID    # n_obs > obs_cap
    assert pair.write_landmarks(0, 0, [1], [0], [1], [0], [-1], [[]]) == R.E_INVALID                # alive without an observation
    assert pair.write_landmarks(0, 0, [1], [0], [1], [1], [-1], [[13]]) == R.E_INVALID              # a keyframe that does not exist
    assert pair.write_landmarks(0, 0, [1], [0], [1], [1], [13], [[0]]) == R.E_INVALID
    assert pair.write_landmarks(0, 32, [1], [0], [1], [1], [-1], [[0]]) == R.E_INVALID              # past the cap
    assert KC.same_snapshot(KC.raw_snapshot(km), before)
    assert pair.set_inlier(0, [0, 1, 3], 0) == R.OK                 # (3 is freed: passed over)
    assert [lm.inlier for lm in pair.model.map_lms[0][:3]] == [False, False, True]
    km.close()


# ---------------------------------------------------------------------------- feeding the existing consumers
def test_feeds_landmark_store_and_pose_graph(ctx):
    import torch
    caps = (6, 32, 8, 256, 64, 8)
    pair = make_pair(ctx, caps)
    rng = np.random.default_rng(5)
    store = gfpl.LandmarkStore(ctx, caps[3], caps[5], 1024)
    desc = rng.integers(0, 256, (6, 32, 32), dtype=np.uint8)      # keyframe, row, byte
    dev = [torch.from_numpy(desc[k].copy()).cuda() for k in range(6)]
    prm = dict(min_lm_cov_graph=30, min_kf_local_map=2, min_lm_obs=2, cull_age=10)
    med = {}
    for t in range(6):
        pair.add_keyframe(32, 8)
        if t > 0:
            k0, k1 = rng.permutation(32)[:20].tolist(), rng.permutation(32)[:20].tolist()
            rc, lm_out, first, new = pair.observe_pairs(0, t - 1, t, list(zip(k0, k1)))
            assert rc == R.OK
            # the caller's gfpl_lm_ops from lm_out: a created landmark takes both rows, an existing one kf1's
            ops = []
            for (r0, r1), j in zip(zip(k0, k1), lm_out):
                if j >= first:
                    ops.append((j, gfpl.LM_ADD, r0, t - 1))
                ops.append((j, gfpl.LM_ADD, r1, t))
            store.apply(ops, dev)
            assert pair.observe_pairs(1, t - 1, t, [(r, r) for r in range(4)])[0] == R.OK
        pair.form_local_map(prm)
    ids, want = pair.select(0, gfpl.KFMAP_LOCAL_UNSEEN, 5)
    assert len(want) >= 5
    rows, idx = store.gather(ids.cpu().numpy(), with_idx=True)
    rows, idx = rows.cpu().numpy(), idx.cpu().numpy()
    for i, j in enumerate(want):
        got = store.read(j)
        assert got["count"] == len(pair.model.lm(0, j).kf_obs_list)         # the two halves of the map agree on the lists
        assert idx[i] == got["med_idx"] and np.array_equal(rows[i], got["med_desc"])
    store.close()

    g = pair.km.export_graph()
    m = pair.model
    n_kf = m.n_kf
    T_kf = np.tile(np.eye(4), (n_kf, 1, 1))
    common = dict(lc=[(0, n_kf - 1, 1)], lc_pose=np.zeros((1, 6)), T_kf=T_kf, pt=np.zeros((m.max_idx[0], 3)),
                  ls=np.zeros((m.max_idx[1], 6)))

    def lists(start, idx):
        return [idx[start[k]:start[k + 1]].tolist() for k in range(n_kf)]
    from_dev = gfpl.PoseGraphProblem(g["alive"], g["full_graph"], pt_own=lists(g["pt_kf_start"], g["pt_kf_idx"]),
                                     ls_own=lists(g["ls_kf_start"], g["ls_kf_idx"]), pt_freed=g["pt_freed"],
                                     ls_freed=g["ls_freed"], **common)
    from_model = gfpl.PoseGraphProblem([kf is not None for kf in m.map_keyframes], m.full_graph,
                                       pt_own=[m.kf_lists[0][k] for k in range(n_kf)],
                                       ls_own=[m.kf_lists[1][k] for k in range(n_kf)],
                                       pt_freed=[lm is None for lm in m.map_lms[0]], ls_freed=[lm is None for lm in m.map_lms[1]],
                                       **common)
    prm_g = gfpl.PoseGraphParams.default()
    prm_g.min_lm_cov_graph = 10
    (rc_d, cnt_d), (rc_m, cnt_m) = from_dev.check(prm_g), from_model.check(prm_g)
    assert rc_d == rc_m == 0
    fields = [f for f, _ in gfpl.PgoCounts._fields_]
    assert [getattr(cnt_d, f) for f in fields] == [getattr(cnt_m, f) for f in fields]
    assert cnt_d.n_pt == m.max_idx[0] and cnt_d.n_ls == m.max_idx[1] and cnt_d.n_edge >= n_kf - 1
    pair.km.close()
