"""gfpl.MapGeometry (k_mapgeo.hip, gfpl_mapgeo.cpp) against the model of tests/mapgeo_ref.py, beside a
gfpl.KeyframeMap driven through the model of tests/kfmap_ref.py.

Bar: after every call the whole geometry state equals the model's bit for bit (every pose, every 3D
geometry, every list entry up to n_obs, every count) and n_obs equals the keyframe map's; an assembled
problem equals the model's gather element for element; gfpl_mapgeo_lba leaves the store and the result
record bitwise equal to Context.localBundleAdjustment on the model's host-gathered problem.  No
tolerance anywhere.  The drivers of tests/mapgeo_cases.py compare after each call.
"""
import ctypes as C

import numpy as np
import pytest

import gfpl
import kfmap_ref as K
import mapgeo_cases as MC
import mapgeo_ref as G
import pgo_cases as PC

pytestmark = pytest.mark.gpu

T = gfpl.KFMAP_TILE
bits = MC.bits
OPEN = []


@pytest.fixture(scope="module")
def ctx():
    cfg = gfpl.default_config()
    c = gfpl.Context(gfpl.make_camera("vga", cfg), cfg)
    yield c
    for o in OPEN:             # (a test that failed midway left its objects open)
        if o is not None:
            o.close()
    c.close()


def make_solver(ctx, caps):
    kf, _, _, pl, ll, oc = caps
    s = gfpl.LbaSolver(ctx, (gfpl.LBA_MAX_KFS, kf, pl, ll, pl * oc, ll * oc), 1)
    OPEN.append(s)
    return s


def record(r):
    return (r.iters, r.stop, r.status, r.hmax, bits([r.lambda_, r.err, r.err_prev]))


def lba_both(ctx, trio, solver, prm=None):
    """gfpl_mapgeo_lba on the device objects and the parent's route on the model: 1 when a solve ran"""
    rc, d = trio.model.assemble(K.LOCAL)
    assert rc == G.OK
    want = trio.model.lba_code(d)
    grc, res, cnt = trio.geo.lba_rc(trio.km, solver, prm)
    assert tuple(getattr(cnt, f) for f, _ in gfpl.LbaCounts._fields_) == d["n"]
    if want is not None:
        assert grc == want
        trio.check("lba refused or empty", force=True)
        return 0
    assert grc == G.OK
    ref = ctx.localBundleAdjustment(MC.host_problem(d), prm)
    assert record(res) == record(ref["result"]), (record(res), record(ref["result"]))
    trio.model.write_back(d, ref["T_kf"], ref["pt"], ref["ls"])
    trio.check("lba", force=True)
    got = trio.geo.read_assembled(trio.geo.assemble(trio.km, K.LOCAL, host_lists=False)[0])
    assert bits(got["T_kf"]) == bits(ref["T_kf"]) and bits(got["pt"]) == bits(ref["pt"]) and bits(got["ls"]) == bits(ref["ls"])
    return 1


def test_tick_sequence(ctx):
    trio = MC.Trio(MC.TICK_CAPS, ctx, OPEN)
    solver = make_solver(ctx, MC.TICK_CAPS)
    f = MC.tick_sequence(trio, ctx.cam, solve=lambda t: lba_both(ctx, t, solver))
    MC.assert_tick_facts(f)
    assert f["solves"] == 5
    assert trio.geo.nbytes() == gfpl.mapgeo_bytes(gfpl.KfMapCaps(*MC.TICK_CAPS)) > 0
    assert trio.geo.last_device_ms() >= 0.0
    solver.close()
    trio.close()


def test_repeated_landmark_takes_pair_order(ctx):
    """three kf0 rows (pair indices 0, 300, 700 of 1024: three workgroups) carry one landmark: it receives
    kf1's rows in pair order; every other pair creates"""
    n = 1024
    caps = (3, n, 2, 2 * n, 4, 8)
    trio = MC.Trio(caps, ctx, OPEN, quiet=True)
    rng = np.random.default_rng(5)
    for k in range(3):
        v = G.View(P=rng.normal(0, 1, (n, 3)) + [0, 0, 6], pl=rng.uniform(0, 600, (n, 2)))
        trio.add_keyframe(v, MC.shifted(0.25 * k), np.full(6, 0.5 * k))
    trio.observe_pairs(0, 0, 1, [(0, 0)])
    for row in (300, 700):
        trio.pair.write_keyframe_idx(0, 1, row, [0])
    perm = rng.permutation(n)
    pairs = [(r, int(perm[r])) for r in range(n)]
    lm_out, first, new = trio.observe_pairs(0, 1, 2, pairs)
    assert [lm_out[i] for i in (0, 300, 700)] == [0, 0, 0] and (first, new) == (1, n - 3)
    trio.check("repeated", force=True)
    v2 = trio.views[2][0]
    d = trio.geo.read_landmarks(0, 0, 1)
    assert d["n_obs"][0] == 5 and bits(d["obs"][0, 2:5]) == bits([v2.pl[perm[0]], v2.pl[perm[300]], v2.pl[perm[700]]])
    trio.close()


def test_two_rows_in_one_wave_and_a_skipped_pair(ctx):
    trio = MC.hand_map(4, ctx, OPEN)
    trio.observe_pairs(0, 0, 1, [(0, 0), (1, 1), (2, 2)])            # landmarks 0, 1, 2 on rows 0, 1, 2 of keyframe 1
    trio.write_landmark(0, 1, [0, 0, 0], [], [], [])                  # landmark 1 freed: its pair does nothing (:308)
    trio.pair.write_keyframe_idx(0, 1, 3, [0])                        # row 3 carries landmark 0 too
    lm_out, first, new = trio.observe_pairs(0, 1, 2, [(0, 3), (1, 1), (2, 0), (3, 2)])
    assert lm_out == [0, -1, 2, 0] and new == 0
    v2 = trio.views[2][0]
    assert trio.model.lms[0][0].obs_list[2:] == [list(v2.pl[3]), list(v2.pl[2])]
    assert len(trio.model.lms[0][2].obs_list) == 3 and 1 not in trio.model.lms[0]
    trio.close()


def test_assembled_problem_equals_the_gather(ctx):
    """a fixed keyframe that is not keyframe 0, keyframe 0 observed, an erased keyframe's observations
    dropped, a landmark dropped for having none left; LOCAL and ALIVE"""
    trio = MC.gather_map(ctx, OPEN)
    rc, d, p, lists = trio.assemble(K.LOCAL)
    assert rc == G.OK and d["fix_list"] == [0, 2] and d["pt_list"] == [0, 1, 2] and d["n"] == (2, 2, 3, 3, 6, 6)
    assert gfpl.hiplib().gfpl_lba_check(C.byref(p)) == G.OK           # the struct runs on the existing entry points as it is
    rc, d, p, lists = trio.assemble(K.ALIVE)
    assert rc == G.OK and d["kf_list"] == [2, 3, 4] and d["fix_list"] == [0]
    cnt = gfpl.GbaCounts()
    assert gfpl.hiplib().gfpl_gba_check(C.byref(p), C.byref(cnt)) == G.OK
    trio.close()


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_scan_boundaries(ctx, n):
    """n selected points around the tile, n_obs cycling 1 .. obs_cap, an unselected landmark every 7th id"""
    oc = 4
    ids, selected = [], 0
    while selected < n:
        selected += len(ids) % 7 != 3
        ids.append(len(ids))
    skip = {j for j in ids if j % 7 == 3}
    cap = len(ids)
    caps = (3, 4, 3, cap, 8, oc)
    trio = MC.Trio(caps, ctx, OPEN, quiet=True)
    for k in range(3):
        trio.add_keyframe(MC.hand_view(100.0 * k), MC.shifted(0.5 * k), np.full(6, 0.01 * k))
    trio.pair.form_local_map(dict(min_lm_cov_graph=1000000, min_kf_local_map=3))
    rng = np.random.default_rng(n)
    n_obs = np.array([1 + j % oc for j in ids], np.int32)
    kf_obs = [[(j + i) % 3 for i in range(n_obs[j])] for j in ids]
    local = np.array([0 if j in skip else 1 for j in ids], np.uint8)
    one = np.ones(cap, np.uint8)
    assert trio.pair.model.write_landmarks(0, 0, one, local, one, n_obs, [-1] * cap, kf_obs) == K.OK
    kf_arr = np.zeros((cap, oc), np.int32)
    for j in ids:
        kf_arr[j, : n_obs[j]] = kf_obs[j]
    trio.km.write_landmarks(0, 0, one, local, one, n_obs, np.full(cap, -1, np.int32), kf_arr)
    lm3d, obs, sig = rng.normal(0, 1, (cap, 3)), rng.normal(0, 1, (cap, oc, 2)), rng.uniform(0.5, 2, (cap, oc))
    trio.geo.write_landmarks(0, 0, lm3d, n_obs, obs, sig)
    for j in ids:
        trio.model.write_landmark(0, j, lm3d[j], obs[j, : n_obs[j]], sig[j, : n_obs[j]])
    trio.write_landmark(1, 5, np.arange(6.0), [[1.0, 2.0, 3.0]], [1.5], [2])
    rc, d, p, lists = trio.assemble(K.LOCAL)
    assert rc == G.OK and d["n"][2] == n and d["n"][3] == 1 and d["kf_list"] == [1, 2] and d["fix_list"] == [0]
    assert d["n"][4] == int(n_obs[local == 1].sum())
    trio.close()


def solved_map(ctx, n_local, seed):
    """a map of n_local + 2 keyframes whose last n_local are local"""
    caps = (n_local + 2, 40, 20, 1024, 512, n_local + 4)
    trio = MC.Trio(caps, ctx, OPEN, quiet=True)
    MC.tick_sequence(trio, ctx.cam, n_kf=n_local + 2, seed=seed)
    trio.pair.form_local_map(dict(min_lm_cov_graph=1000000, min_kf_local_map=n_local - 1))
    trio.check("map", force=True)
    return trio, caps


@pytest.mark.parametrize("n_local", [3, gfpl.LBA_MAX_KFS])
def test_lba_equals_the_host_route(ctx, n_local):
    trio, caps = solved_map(ctx, n_local, 11 + n_local)
    solver = make_solver(ctx, caps)
    assert trio.model.assemble(K.LOCAL)[1]["n"][0] == n_local
    assert lba_both(ctx, trio, solver) == 1
    # a second tick's solve starts from the first one's poses and landmarks
    assert lba_both(ctx, trio, solver, gfpl.LbaParams.default(max_iters=3)) == 1
    solver.close()
    trio.close()


def test_gba_on_an_alive_assembly(ctx):
    trio, caps = solved_map(ctx, 3, 21)
    assert trio.pair.model.n_kf == 5
    rc, d, p, lists = trio.assemble(K.ALIVE)
    assert rc == G.OK and d["n"][0] == 4 and d["fix_list"] == [0]
    ref = ctx.globalBundleAdjustment(MC.host_problem(d))
    cnt = gfpl.GbaCounts()
    L = gfpl.hiplib()
    assert L.gfpl_gba_check(C.byref(p), C.byref(cnt)) == G.OK
    gba = gfpl.GbaSolver(ctx, cnt, 1)
    OPEN.append(gba)
    prm, res = gfpl.LbaParams.default(), gfpl.LbaResult()
    assert L.gfpl_gba_solve(gba.h, C.byref(p), 1, C.byref(prm), C.byref(res)) == G.OK
    assert record(res) == record(ref["result"])
    got = trio.geo.read_assembled(p)
    assert bits(got["T_kf"]) == bits(ref["T_kf"]) and bits(got["pt"]) == bits(ref["pt"]) and bits(got["ls"]) == bits(ref["ls"])
    gba.close()
    trio.close()


def refusal_map(ctx):
    trio = MC.hand_map(4, ctx, OPEN)
    trio.observe_pairs(0, 0, 1, [(0, 0), (1, 1)])
    trio.observe_pairs(1, 0, 1, [(0, 0)])
    return trio


def test_refusals_change_nothing(ctx):
    trio = refusal_map(ctx)
    geo, m = trio.geo, trio.model
    v0, v1 = trio.views[0][0], trio.views[1][0]
    before = MC.device_snapshot(geo)
    # the device refusals, each through both (the driver compares the codes)
    E, CAP = G.E_INVALID, G.E_CAPACITY
    assert trio.geo_observe_pairs(0, 0, 1, [(4, 0)], [2], 2) == E           # a kf0 row outside its view
    assert trio.geo_observe_pairs(0, 0, 1, [(2, -1)], [2], 2) == E          # a kf1 row outside its view
    assert trio.geo_observe_pairs(0, 0, 1, [(2, 2)], [8], 2) == E           # an id outside [-1, cap)
    assert trio.geo_observe_pairs(0, 0, 1, [(2, 2)], [-2], 2) == E
    assert trio.geo_observe_pairs(0, 0, 1, [(2, 2)], [0], 0) == E           # a created id that holds a list
    assert trio.geo_observe_pairs(0, 0, 1, [(2, 2)], [2], 3) == E           # a carried id without one
    assert trio.geo_observe_pairs(0, 0, 1, [(2, 2), (3, 3)], [2, 2], 2) == E    # a created id twice
    assert trio.geo_observe_pairs(1, 0, 1, [(3, 0)], [1], 1) == E           # a line row outside its view
    assert trio.geo_observe_local(0, 1, [(0, 2)], [2, 3], [1]) == E         # outside n_unm
    assert trio.geo_observe_local(0, 1, [(0, 0)], [2], [5]) == E            # a carried id without a list
    assert trio.geo_observe_local(0, 1, [(0, 0), (1, 1)], [2, 3], [1, 9]) == E
    # the host refusals
    assert trio.geo_observe_pairs(0, 0, 1, [(0, 0)] * 5, [0] * 5, 2) == E   # n above the views' rows
    assert trio.geo_observe_pairs(0, 5, 1, [], [], 0) == E                  # kf0 without a pose
    assert trio.geo_observe_pairs(0, 1, 1, [], [], 0) == E
    assert trio.geo_observe_pairs(0, 0, 6, [], [], 0) == E
    assert trio.geo_observe_pairs(0, 0, 1, [], [], 9) == E                  # first_new beyond the cap
    assert trio.geo_observe_local(0, 1, [(0, 0)], [4], [1]) == E            # an unm_rows entry outside the view
    assert trio.geo_observe_local(0, 1, [(0, 0), (1, 1)], [2], [0, 1]) == E     # n above n_unm
    d0, d1 = trio.views[0][1], trio.views[1][1]
    p, out = np.array([[2, 2]], np.int32), np.array([2], np.int32)
    assert geo.observe_pairs_rc(2, 0, 1, d0, d1, p, out, 2) == E
    bad = geo.view(P=v0.P, pl=v0.pl)
    bad.s.pl = bad.s.pl + 4                                                   # a misaligned array of the kind that is read
    assert geo.observe_pairs_rc(0, 0, 1, bad, d1, p, out, 2) == E
    bad.s.pl = None
    assert geo.observe_pairs_rc(0, 0, 1, bad, d1, p, out, 2) == E
    assert geo.observe_pairs_rc(1, 0, 1, bad, d1, p, out, 2) == E           # no line arrays in this view
    assert geo.free_rc(0, np.array([1, 8], np.int32)) == E and m.free(0, [1, 8]) == E
    assert geo.free_rc(2, np.array([1], np.int32)) == E
    assert geo.set_keyframe_rc(6, np.eye(4), np.zeros(6)) == E
    z = np.zeros
    assert geo.write_landmarks_rc(0, 7, z((2, 3)), [1, 1], z((2, 4, 2)), z((2, 4))) == E      # beyond the cap
    assert geo.write_landmarks_rc(0, 0, z((1, 3)), [5], z((1, 4, 2)), z((1, 4))) == E         # n_obs beyond obs_cap
    assert MC.same_snapshot(before, MC.device_snapshot(geo))
    # capacity: a list at obs_cap - 1 takes one more entry, a full one refuses; INVALID wins over CAPACITY
    trio.observe_pairs(0, 1, 2, [(0, 0)])
    trio.observe_pairs(0, 2, 3, [(0, 0)])
    assert len(m.lms[0][0].obs_list) == 4 == MC.HAND_CAPS[5]
    before = MC.device_snapshot(geo)
    assert trio.geo_observe_local(0, 3, [(0, 1), (1, 2)], [0, 1, 2], [1, 0]) == CAP
    assert trio.geo_observe_local(0, 3, [(0, 1), (1, 2)], [0, 1, 2], [9, 0]) == E
    assert MC.same_snapshot(before, MC.device_snapshot(geo))
    # the two objects' lists out of step: the assembly is refused
    trio.pair.form_local_map(dict(min_lm_cov_graph=1000000, min_kf_local_map=3))
    geo.free(0, np.array([1], np.int32))
    m.free(0, [1])
    assert trio.assemble(K.LOCAL)[0] == E
    other = gfpl.KeyframeMap(ctx, 6, 4, 3, 8, 8, 5)
    OPEN.append(other)
    assert geo.assemble_rc(other, K.LOCAL)[0] == E                            # a keyframe map of other caps
    assert geo.assemble_rc(trio.km, gfpl.KFMAP_LOCAL_UNSEEN)[0] == E
    other.close()
    trio.close()


def test_seventeen_local_keyframes_are_refused(ctx):
    n = gfpl.LBA_MAX_KFS + 1
    caps = (n + 1, 4, 3, 8, 8, 4)
    trio = MC.Trio(caps, ctx, OPEN, quiet=True)
    for k in range(n + 1):
        trio.add_keyframe(MC.hand_view(100.0 * k), MC.shifted(0.1 * k), np.full(6, 0.01 * k))
    trio.observe_pairs(0, n - 1, n, [(0, 0), (1, 1)])
    trio.observe_pairs(1, n - 1, n, [(0, 0)])
    trio.pair.form_local_map(dict(min_lm_cov_graph=1000000, min_kf_local_map=n))
    solver = make_solver(ctx, caps)
    before = MC.device_snapshot(trio.geo)
    rc, res, cnt = trio.geo.lba_rc(trio.km, solver)
    assert rc == G.E_CAPACITY and cnt.n_kf == n and cnt.n_pt == 2
    assert MC.same_snapshot(before, MC.device_snapshot(trio.geo))
    # counts above the solver's caps, and a solver of another context's kind of refusal: nothing written
    small = gfpl.LbaSolver(ctx, (gfpl.LBA_MAX_KFS, 2, 1, 1, 2, 2), 1)
    OPEN.append(small)
    trio.pair.form_local_map(dict(min_lm_cov_graph=1000000, min_kf_local_map=2))
    rc, res, cnt = trio.geo.lba_rc(trio.km, small)
    assert rc == G.E_CAPACITY and cnt.n_kf == 3 and cnt.n_pt == 2
    assert MC.same_snapshot(before, MC.device_snapshot(trio.geo))
    # no observation at all: nothing is solved
    empty = MC.hand_map(3, ctx, OPEN)
    empty.pair.form_local_map(dict(min_lm_cov_graph=1000000, min_kf_local_map=3))
    assert lba_both(ctx, empty, solver) == 0
    for o in (small, solver, empty, trio):
        o.close()


class RawDev:
    """a device array by its address, for the structs that take tensors"""

    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n

    def data_ptr(self):
        return self.ptr

    def __len__(self):
        return self.n


def test_pose_graph_in_place(ctx):
    """gfpl_pgo_solve on gfpl_mapgeo_arrays changes the store as the same problem on copied arrays does"""
    c = PC.make("in_place", 7, [(1, 5)], seed=31, dirs=False)
    prob, prm = PC.problem(c), PC.params(c)
    rc, cnt = prob.check(prm)
    assert rc == 0
    pg = gfpl.PoseGraph(ctx, [cnt], 1)
    OPEN.append(pg)
    ref = pg.solve([prob], prm)[0]
    n_pt, n_ls = len(c["pt"]), len(c["ls"])
    geo = gfpl.MapGeometry(ctx, 7, 4, 4, n_pt, n_ls, 2)
    OPEN.append(geo)
    for k in range(7):
        geo.set_keyframe(k, c["T_kf"][k], np.full(6, np.nan))
    z = np.zeros
    geo.write_landmarks(0, 0, c["pt"], z(n_pt, np.int32), z((n_pt, 2, 2)), z((n_pt, 2)))
    geo.write_landmarks(1, 0, c["ls"], z(n_ls, np.int32), z((n_ls, 2, 3)), z((n_ls, 2)))
    a = geo.arrays()
    dev = dict(T_kf=RawDev(a["T_kf"], 7), x_kf=RawDev(a["x_kf"], 7), pt=RawDev(a["point3D"], n_pt), ls=RawDev(a["line3D"], n_ls))
    s = prob.struct(dev)
    out = gfpl.PgoResult()
    assert gfpl.hiplib().gfpl_pgo_solve(pg.h, C.byref(s), 1, C.byref(prm), C.byref(out)) == 0
    assert (out.iters, out.stop, out.status, bits([out.chi2])) == (ref["result"].iters, ref["result"].stop, ref["result"].status,
                                                                   bits([ref["result"].chi2]))
    moved = 0
    for k in range(7):
        Tk, xk = geo.read_keyframe(k)
        assert bits(Tk) == bits(ref["T_kf"][k]) and bits(xk) == bits(ref["x_kf"][k]), k
        moved += bits(Tk) != bits(c["T_kf"][k])
    assert moved >= 3
    assert bits(geo.read_landmarks(0, 0, n_pt)["lm3d"]) == bits(ref["pt"])
    assert bits(geo.read_landmarks(1, 0, n_ls)["lm3d"]) == bits(ref["ls"])
    geo.close()
    pg.close()
