"""Generators and drivers for the keyframe-map tests (tests/test_kfmap_cpu.py, tests/test_kfmap_gpu.py).

A `Pair` runs every call on the model of tests/kfmap_ref.py and, when it has one, on a gfpl.KeyframeMap,
compares what the two return, and after every call compares the whole state.  Without a device it
is the model alone, so a test's situation can be asserted on the CPU.
"""
import numpy as np

import kfmap_ref as R


def device_state(km):
    """a KeyframeMap's state in the shape of R.Model.state()"""
    nkf, _, _ = km.counts()
    kfs = []
    for k in range(nkf):
        r = km.read_keyframe(k)
        kfs.append(dict(local=int(r["local"]), pt_idx=r["pt_idx"].tolist(), ls_idx=r["ls_idx"].tolist()) if r["alive"] else None)
    g = km.export_graph()
    lms, csr = [], []
    for kind, name in ((0, "pt"), (1, "ls")):
        d = km.read_landmarks(kind)
        recs = []
        for j in range(len(d["alive"])):
            if d["alive"][j]:
                recs.append(dict(owner=int(d["owner"][j]), local=int(d["local"][j]), inlier=int(d["inlier"][j]),
                                 kf_obs=d["kf_obs"][j, : d["n_obs"][j]].tolist()))
            else:
                recs.append(dict(owner=int(d["owner"][j])))
        lms.append(recs)
        csr.append(dict(start=g[name + "_kf_start"].tolist(), idx=g[name + "_kf_idx"].tolist(), freed=g[name + "_freed"].tolist()))
    return dict(kfs=kfs, lms=lms, graph=g["full_graph"].tolist(), csr=csr, alive=g["alive"].tolist())


def raw_snapshot(km):
    """every array the read calls return, as they are (freed landmarks' bytes and erased keyframes' rows too)"""
    nkf, _, _ = km.counts()
    snap = {"counts": np.array(km.counts())}
    for k in range(nkf):
        for name, v in km.read_keyframe(k).items():
            snap[f"kf{k}_{name}"] = np.array(v)
    for kind in (0, 1):
        for name, v in km.read_landmarks(kind).items():
            snap[f"lm{kind}_{name}"] = v
    for name, v in km.export_graph().items():
        snap["graph_" + name] = v
    return snap


def same_snapshot(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def assert_same_state(got, want, where=""):
    for key in ("alive", "graph", "kfs", "csr"):
        assert got[key] == want[key], (where, key, got[key], want[key])
    for kind in (0, 1):
        assert len(got["lms"][kind]) == len(want["lms"][kind]), (where, kind)
        for j, (g, w) in enumerate(zip(got["lms"][kind], want["lms"][kind])):
            assert g == w, (where, kind, j, g, w)


class Pair:
    """the model and (optionally) the device object, driven together"""

    def __init__(self, caps, km=None):
        self.caps = caps
        self.model = R.Model(*caps)
        self.km = km
        self.calls = 0

    def check(self, where):
        self.calls += 1
        if self.km is not None:
            assert_same_state(device_state(self.km), self.model.state(), f"{where} (call {self.calls})")

    def add_keyframe(self, n_pt, n_ls):
        rc, kf = self.model.add_keyframe(n_pt, n_ls)
        if self.km is not None:
            got = self.km.add_keyframe_rc(n_pt, n_ls)
            assert got == (rc, kf), (got, rc, kf)
        self.check("add_keyframe")
        return rc, kf

    def observe_pairs(self, kind, kf0, kf1, pairs):
        rc, lm_out, first, new = self.model.observe_pairs(kind, kf0, kf1, pairs)
        if self.km is not None:
            grc, gout, gfirst, gnew = self.km.observe_pairs_rc(kind, kf0, kf1, np.array(pairs, np.int32).reshape(-1, 2))
            assert grc == rc, ("observe_pairs", grc, rc)
            if rc == R.OK:
                assert (gout.cpu().tolist(), gfirst, gnew) == (lm_out, first, new), ("observe_pairs", gfirst, gnew, first, new)
        self.check("observe_pairs")
        return rc, lm_out, first, new

    def observe_local(self, kind, kf1, pairs, sel_ids, unm_rows, sel_dev=None, unm_dev=None):
        """sel_dev / unm_dev: the two lists as the device calls returned them (else the host lists are uploaded)"""
        rc, lm_out = self.model.observe_local(kind, kf1, pairs, sel_ids, unm_rows)
        if self.km is not None:
            grc, gout = self.km.observe_local_rc(kind, kf1, np.array(pairs, np.int32).reshape(-1, 2),
                                                 sel_ids if sel_dev is None else sel_dev, unm_rows if unm_dev is None else unm_dev)
            assert grc == rc, ("observe_local", grc, rc)
            if rc == R.OK:
                assert gout.cpu().tolist() == lm_out
        self.check("observe_local")
        return rc, lm_out

    def select(self, kind, which, kf1=0):
        want = self.model.select(kind, which, kf1)
        if self.km is not None:
            got = self.km.select(kind, which, kf1)
            assert got.cpu().tolist() == want, ("select", kind, which)
            return got, want
        return want, want

    def unmatched(self, kind, kf):
        want = self.model.unmatched(kind, kf)
        if self.km is not None:
            got = self.km.unmatched(kind, kf)
            assert got.cpu().tolist() == want, ("unmatched", kind, kf)
            return got, want
        return want, want

    def form_local_map(self, prm):
        import gfpl
        rc = self.model.form_local_map(**prm)
        assert rc == R.OK
        if self.km is not None:
            self.km.form_local_map(gfpl.KfMapParams.default(**prm))
            assert self.km.local_keyframes().tolist() == self.model.local_keyframes()
        self.check("form_local_map")

    def remove_bad(self, prm):
        import gfpl
        removed = self.model.remove_bad(**prm)
        if self.km is not None:
            pt, ls = self.km.remove_bad(gfpl.KfMapParams.default(**prm))
            assert [pt.cpu().tolist(), ls.cpu().tolist()] == removed, "remove_bad"
        self.check("remove_bad")
        return removed

    def set_inlier(self, kind, ids, value):
        rc = self.model.set_inlier(kind, ids, value)
        if self.km is not None:
            assert self.km.set_inlier_rc(kind, np.array(ids, np.int32), value) == rc
        self.check("set_inlier")
        return rc

    def erase_keyframe(self, kf):
        rc = self.model.erase_keyframe(kf)
        if self.km is not None:
            assert self.km.erase_keyframe_rc(kf) == rc
        self.check("erase_keyframe")
        return rc

    def write_keyframe_idx(self, kind, kf, row0, idx):
        rc = self.model.write_keyframe_idx(kind, kf, row0, idx)
        if self.km is not None:
            assert self.km.write_keyframe_idx_rc(kind, kf, row0, idx) == rc
        self.check("write_keyframe_idx")
        return rc

    def write_landmarks(self, kind, id0, alive, local, inlier, n_obs, owner, kf_obs):
        """kf_obs: one list per landmark"""
        rc = self.model.write_landmarks(kind, id0, alive, local, inlier, n_obs, owner, kf_obs)
        if self.km is not None:
            arr = np.full((len(alive), self.caps[5]), -1, np.int32)
            for i, l in enumerate(kf_obs):
                arr[i, : min(len(l), self.caps[5])] = l[: self.caps[5]]
            assert self.km.write_landmarks_rc(kind, id0, alive, local, inlier, n_obs, owner, arr) == rc
        self.check("write_landmarks")
        return rc


# ---------------------------------------------------------------------------- sixteen keyframes
SIXTEEN_CAPS = (16, 96, 40, 2048, 1024, 16)       # kf_cap, pt_rows, ls_rows, pt_lm_cap, ls_lm_cap, obs_cap
SIXTEEN_PRM = dict(min_lm_cov_graph=30, min_kf_local_map=2, min_lm_obs=3, cull_age=10)


def _pair_rows(rng, n_rows, n, forced=()):
    rest = [r for r in range(n_rows) if r not in forced]
    picked = list(forced) + [int(v) for v in rng.choice(rest, size=max(0, min(n, n_rows) - len(forced)), replace=False)]
    return picked


def sixteen_keyframes(pair, seed=7):
    """The addKeyFrame order over 16 ticks (add, observe pairs, select + unmatched, observe local, form
    local map, remove bad), both kinds.  Returns the facts the test is named for, taken from the model."""
    rng = np.random.default_rng(seed)
    m = pair.model
    rows = (SIXTEEN_CAPS[1], SIXTEEN_CAPS[2])
    facts = dict(culled=0, freed_pair=0, twice=0, two_rows=None, last=None)
    culled_pt = []
    watch = None                                   # (landmark, lower row, upper row) on keyframe 0
    for t in range(16):
        rc, kf = pair.add_keyframe(*rows)
        assert (rc, kf) == (R.OK, t)
        if t > 0:
            for kind in (0, 1):
                n_pairs = (40, 15)[kind] if t <= 12 else 3
                forced = []
                idx0 = m.map_keyframes[t - 1].idx[kind]
                if kind == 0 and t == 6:
                    # two rows of kf0 carry one alive landmark: it receives kf1 twice in this call
                    a = next(r for r, v in enumerate(idx0) if v != -1 and m.lm(0, v) is not None)
                    b = next(r for r, v in enumerate(idx0) if v == -1)
                    assert pair.write_keyframe_idx(0, t - 1, b, [idx0[a]]) == R.OK
                    forced = [a, b]
                if kind == 0 and t == 12:
                    # a row of kf0 names a landmark that the culling freed (a loop-closure walk's leftover)
                    assert culled_pt
                    b = next(r for r, v in enumerate(idx0) if v == -1)
                    assert pair.write_keyframe_idx(0, t - 1, b, [culled_pt[0]]) == R.OK
                    forced = [b]
                k0 = _pair_rows(rng, rows[kind], n_pairs, forced)
                k1 = _pair_rows(rng, rows[kind], n_pairs)
                rc, lm_out, first, new = pair.observe_pairs(kind, t - 1, t, list(zip(k0, k1)))
                assert rc == R.OK
                facts["freed_pair"] += lm_out.count(-1)
                facts["twice"] += sum(lm_out.count(j) == 2 for j in set(lm_out) if j >= 0)
                sel_dev, sel = pair.select(kind, R.LOCAL_UNSEEN, t)
                unm_dev, unm = pair.unmatched(kind, t)
                n_loc = ((10, 5)[kind] if 2 <= t <= 12 else 0) if t < 15 else (30, 10)[kind]
                n_loc = min(n_loc, len(sel), len(unm))
                p0 = [int(v) for v in rng.choice(len(sel), size=n_loc, replace=False)] if n_loc else []
                p1 = [int(v) for v in rng.choice(len(unm), size=n_loc, replace=False)] if n_loc else []
                rc, _ = pair.observe_local(kind, t, list(zip(p0, p1)), sel, unm, sel_dev, unm_dev)
                assert rc == R.OK
        if t == 8:
            # an outlier with many observations is culled as well once it is old and not local
            old = [lm.idx for lm in m.map_lms[0] if lm is not None and lm.kf_obs_list[0] <= 1 and len(lm.kf_obs_list) >= 3][:5]
            assert len(old) >= 1 and pair.set_inlier(0, old, 0) == R.OK
        if t == 10:
            # a landmark that the next tick culls, on a second row of its first keyframe
            lm = next(lm for lm in m.map_lms[0] if lm is not None and lm.kf_obs_list == [0, 1] and not lm.local)
            idx0 = m.map_keyframes[0].idx[0]
            a = idx0.index(lm.idx)
            b = next(r for r in range(len(idx0) - 1, -1, -1) if r != a and idx0[r] == -1)
            assert pair.write_keyframe_idx(0, 0, b, [lm.idx]) == R.OK
            watch = (lm.idx, min(a, b), max(a, b))
        prm = dict(SIXTEEN_PRM)
        if t == 15:
            g = m.full_graph[15]
            prm["min_lm_cov_graph"] = max(g[:13])
        pair.form_local_map(prm)
        removed = pair.remove_bad(prm)
        facts["culled"] += len(removed[0]) + len(removed[1])
        culled_pt += removed[0]
        if watch is not None and watch[0] in removed[0]:
            idx0 = m.map_keyframes[0].idx[0]
            facts["two_rows"] = (idx0[watch[1]], idx0[watch[2]] == watch[0])
            watch = None
        if t == 15:
            g, cov, near = m.full_graph[15], prm["min_lm_cov_graph"], prm["min_kf_local_map"]
            loc = [m.map_keyframes[i].local for i in range(16)]
            facts["last"] = dict(
                cov_only=[i for i in range(15) if loc[i] and g[i] >= cov and 15 - i > near],
                dist_only=[i for i in range(15) if loc[i] and g[i] < cov and 15 - i <= near],
                not_local=[i for i in range(15) if not loc[i]])
    facts["max_obs"] = max(len(lm.kf_obs_list) for kind in (0, 1) for lm in m.map_lms[kind] if lm is not None)
    return facts


def assert_sixteen_facts(f):
    assert f["last"]["cov_only"] and f["last"]["dist_only"] and f["last"]["not_local"], f["last"]
    assert f["culled"] >= 10, f["culled"]
    assert f["two_rows"] == (-1, True), f["two_rows"]      # the lower row cleared, the upper keeps the id
    assert f["freed_pair"] >= 1 and f["twice"] >= 1 and f["max_obs"] >= 5, f


# ---------------------------------------------------------------------------- hand-written maps (the pinned quirks)
QUIRK_CAPS = (16, 6, 4, 32, 16, 4)


def quirk_map(pair, n_kf=13):
    """13 keyframes of 6 point rows; landmarks 0-3 created between keyframes 0 and 1 on rows 0-3"""
    for _ in range(n_kf):
        assert pair.add_keyframe(6, 4)[0] == R.OK
    rc, lm_out, first, new = pair.observe_pairs(0, 0, 1, [(0, 0), (1, 1), (2, 2), (3, 3)])
    assert (rc, lm_out, first, new) == (R.OK, [0, 1, 2, 3], 0, 4)
    return pair


CULL = dict(min_lm_obs=3, cull_age=10)
FLM = dict(min_lm_cov_graph=30, min_kf_local_map=3)


def quirk_km1(pair):
    """formLocalMap passes over an erased keyframe within minKFLocalMap of the newest"""
    m = quirk_map(pair).model
    assert pair.erase_keyframe(11) == R.OK
    pair.form_local_map(FLM)
    assert m.local_keyframes() == [9, 10, 12] and m.map_keyframes[11] is None


def quirk_km2(pair):
    """removeBadMapLandmarks passes over a landmark whose first keyframe is erased"""
    m = quirk_map(pair).model
    pair.form_local_map(FLM)
    assert pair.erase_keyframe(0) == R.OK
    assert pair.remove_bad(CULL) == [[], []]
    assert all(m.lm(0, j) is not None for j in range(4))


def quirk_km3_km5(pair):
    """the ownership lists in ascending id; the culled ids stay on the other keyframe's rows"""
    m = quirk_map(pair).model
    assert m.state()["csr"][0]["start"][:3] == [0, 4, 4] and m.state()["csr"][0]["idx"] == [0, 1, 2, 3]
    pair.form_local_map(FLM)
    assert pair.remove_bad(CULL) == [[0, 1, 2, 3], []]
    assert m.state()["csr"][0]["idx"] == [] and m.state()["csr"][0]["freed"] == [1, 1, 1, 1]
    assert m.map_keyframes[0].idx[0][:4] == [-1] * 4 and m.map_keyframes[1].idx[0][:4] == [0, 1, 2, 3]


def quirk_km4(pair):
    """min_lm_obs counts kf_obs_list: three observations stay at 3 and go at 4"""
    m = quirk_map(pair).model
    assert pair.observe_pairs(0, 1, 2, [(0, 0)])[1] == [0]
    pair.form_local_map(FLM)
    assert pair.remove_bad(CULL) == [[1, 2, 3], []]
    assert pair.remove_bad(dict(min_lm_obs=4, cull_age=10)) == [[0], []]
    assert m.map_keyframes[2].idx[0][0] == 0


def quirk_km6(pair):
    """a pair whose kf0 row names a freed landmark does nothing"""
    m = quirk_map(pair).model
    pair.form_local_map(FLM)
    assert pair.remove_bad(CULL)[0] == [0, 1, 2, 3]
    rc, lm_out, first, new = pair.observe_pairs(0, 1, 2, [(0, 0), (5, 1)])
    assert (rc, lm_out, first, new) == (R.OK, [-1, 4], 4, 1)
    assert m.map_keyframes[2].idx[0][:2] == [-1, 4]


def quirk_km7(pair):
    """max_kf_idx - kf_obs[0] > cull_age: 10 stays, 11 goes"""
    quirk_map(pair, n_kf=11)
    pair.form_local_map(FLM)
    assert pair.remove_bad(CULL) == [[], []]
    assert pair.add_keyframe(6, 4)[1] == 11
    pair.form_local_map(FLM)
    assert pair.remove_bad(CULL) == [[0, 1, 2, 3], []]


def quirk_km8(pair):
    """a value twice in a column of pairs is refused, in either column, and nothing changes"""
    m = quirk_map(pair).model
    before = m.state()
    assert pair.observe_pairs(0, 1, 2, [(4, 0), (0, 1), (0, 2)])[0] == R.E_INVALID
    assert pair.observe_pairs(0, 1, 2, [(4, 0), (0, 1), (1, 1)])[0] == R.E_INVALID
    assert m.state() == before
    assert pair.observe_pairs(0, 1, 2, [(4, 0), (0, 1), (1, 2)])[0] == R.OK


def quirk_km9_km10(pair):
    """a new landmark is not local, a new keyframe is; erasing leaves the newest keyframe's graph words"""
    m = quirk_map(pair, n_kf=3).model
    assert [lm.local for lm in m.map_lms[0]] == [False] * 4 and all(kf.local for kf in m.map_keyframes)
    assert pair.observe_pairs(0, 1, 2, [(0, 0), (1, 1)])[0] == R.OK
    assert m.full_graph[1] == [4, 0, 2] and m.full_graph[2] == [2, 2, 0]
    assert pair.erase_keyframe(1) == R.OK
    assert m.full_graph[1] == [0, 0, 2] and m.full_graph[2] == [2, 2, 0] and m.full_graph[0] == [0, 0, 2]


def quirk_first_row(pair):
    """a culled landmark on two rows of its first keyframe: the lower row is cleared, the upper keeps the id"""
    m = quirk_map(pair).model
    assert pair.write_keyframe_idx(0, 0, 5, [2]) == R.OK
    pair.form_local_map(FLM)
    assert pair.remove_bad(CULL)[0] == [0, 1, 2, 3]
    assert m.map_keyframes[0].idx[0] == [-1, -1, -1, -1, -1, 2]


def quirk_two_rows(pair):
    """two kf0 rows carry one landmark: kf1 is appended twice, each graph update counts the old entries only"""
    m = quirk_map(pair).model
    assert pair.write_keyframe_idx(0, 1, 4, [0]) == R.OK
    rc, lm_out, first, new = pair.observe_pairs(0, 1, 2, [(0, 0), (4, 1)])
    assert (rc, lm_out, new) == (R.OK, [0, 0], 0)
    assert m.lm(0, 0).kf_obs_list == [0, 1, 2, 2] and m.full_graph[2][:2] == [2, 2] and m.full_graph[0][2] == 2


def quirk_local_stage(pair):
    """the local-map stage appends through the two selections; an outlier is culled whatever its length"""
    m = quirk_map(pair).model
    pair.form_local_map(dict(min_lm_cov_graph=1, min_kf_local_map=0))
    assert m.local_keyframes() == [12] and m.select(0, R.LOCAL, 0) == []
    assert pair.observe_pairs(0, 1, 12, [(0, 0), (1, 1)])[0] == R.OK
    pair.form_local_map(dict(min_lm_cov_graph=2, min_kf_local_map=0))
    assert m.local_keyframes() == [1, 12]                      # keyframe 1 by covisibility alone
    sel_dev, sel = pair.select(0, R.LOCAL_UNSEEN, 12)
    unm_dev, unm = pair.unmatched(0, 12)
    assert sel == [2, 3] and unm == [2, 3, 4, 5] and m.select(0, R.LOCAL, 0) == [0, 1, 2, 3]
    assert pair.observe_local(0, 12, [(1, 0), (0, 3)], sel, unm, sel_dev, unm_dev) == (R.OK, [3, 2])
    assert m.map_keyframes[12].idx[0] == [0, 1, 3, -1, -1, 2] and m.full_graph[12][:2] == [4, 4]
    assert pair.set_inlier(0, [3], 0) == R.OK
    pair.form_local_map(dict(min_lm_cov_graph=99, min_kf_local_map=0))
    assert pair.remove_bad(dict(min_lm_obs=2, cull_age=10)) == [[], []]      # on the newest keyframe's rows: local
    assert pair.write_keyframe_idx(0, 12, 2, [-1]) == R.OK
    pair.form_local_map(dict(min_lm_cov_graph=99, min_kf_local_map=0))
    assert pair.remove_bad(dict(min_lm_obs=2, cull_age=10)) == [[3], []]


QUIRKS = [quirk_km1, quirk_km2, quirk_km3_km5, quirk_km4, quirk_km6, quirk_km7, quirk_km8, quirk_km9_km10, quirk_first_row,
          quirk_two_rows, quirk_local_stage]
