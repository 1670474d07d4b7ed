"""Generators and drivers for the map-geometry tests (tests/test_mapgeo_cpu.py, tests/test_mapgeo_gpu.py).

A `Trio` runs every call on the two models (tests/kfmap_ref.py, tests/mapgeo_ref.py) and, when it has a
context, on a gfpl.KeyframeMap and a gfpl.MapGeometry, compares the codes, and after every call compares
the whole geometry state bit for bit (the index state is compared by kfmap_cases.Pair).  Without a
device it is the models alone, so a test's situation can be asserted on the CPU.

A `World` is a small synthetic scene: points and segments 4 to 10 m in front of keyframes that move
sideways; row r of keyframe k observes world feature world[k][kind][r], so two rows match when they
observe the same feature.
"""
import numpy as np

import gfpl
import kfmap_cases as KC
import kfmap_ref as K
import loop_closure_ref as LR
import mapgeo_ref as G
import oracle as O


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).tobytes()


class World:
    def __init__(self, cam, seed, n_kf, n_pt_world, n_ls_world, n_pt_rows, n_ls_rows):
        rng = np.random.default_rng(seed)
        self.cam = cam
        P = np.stack([rng.uniform(-2, 2, n_pt_world), rng.uniform(-1.5, 1.5, n_pt_world), rng.uniform(4, 10, n_pt_world)], 1)
        A = np.stack([rng.uniform(-2, 2, n_ls_world), rng.uniform(-1.5, 1.5, n_ls_world), rng.uniform(4, 10, n_ls_world)], 1)
        B = A + rng.uniform(-0.8, 0.8, (n_ls_world, 3))
        self.T, self.x, self.views, self.world = [], [], [], []
        for k in range(n_kf):
            T_true = O.expmap_se3(np.concatenate([[0.15 * k, 0.0, 0.0] + rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.03, 0.03, 3)]))
            Ti = O.inverse_se3(T_true)
            T_est = T_true @ O.expmap_se3(rng.uniform(-0.01, 0.01, 6))
            self.T.append(np.array(T_est, np.float64).reshape(16))
            self.x.append(np.array(LR.logmap_se3(T_est), np.float64).reshape(6))
            wp = rng.permutation(n_pt_world)[:n_pt_rows]
            wl = rng.permutation(n_ls_world)[:n_ls_rows]
            cam_of = lambda X: (Ti[:3, :3] @ X.T).T + Ti[:3, 3]
            Pc = cam_of(P[wp]) + 0.02 * rng.standard_normal((len(wp), 3))
            pl = np.stack([cam.cx + cam.fx * Pc[:, 0] / Pc[:, 2], cam.cy + cam.fy * Pc[:, 1] / Pc[:, 2]], 1)
            pl = pl + 0.5 * rng.standard_normal(pl.shape)
            sP = cam_of(A[wl]) + 0.02 * rng.standard_normal((len(wl), 3))
            eP = cam_of(B[wl]) + 0.02 * rng.standard_normal((len(wl), 3))
            le = []
            for s, e in zip(sP, eP):
                p = np.array([cam.cx + cam.fx * s[0] / s[2], cam.cy + cam.fy * s[1] / s[2], 1.0])
                q = np.array([cam.cx + cam.fx * e[0] / e[2], cam.cy + cam.fy * e[1] / e[2], 1.0])
                l = np.cross(p, q)
                l = l / np.sqrt(l[0] * l[0] + l[1] * l[1])
                l[2] += 0.5 * rng.standard_normal()
                le.append(l)
            self.views.append(G.View(P=Pc, pl=pl, sP=sP, eP=eP, le=np.array(le).reshape(-1, 3)))
            self.world.append((wp.tolist(), wl.tolist()))

    def common(self, kind, kf0, kf1):
        """(kf0 row, kf1 row) of the features both keyframes observe, in kf0 row order"""
        at = {w: r for r, w in enumerate(self.world[kf1][kind])}
        return [(r, at[w]) for r, w in enumerate(self.world[kf0][kind]) if w in at]


def device_snapshot(geo, n_kf_read=None):
    """every array the read calls return, as they are"""
    caps = geo.caps
    snap = {}
    for k in range(caps.kf_cap if n_kf_read is None else n_kf_read):
        T, x = geo.read_keyframe(k)
        snap[f"kf{k}"] = np.concatenate([T.reshape(16), x])
    for kind, cap in ((0, caps.pt_lm_cap), (1, caps.ls_lm_cap)):
        for name, v in geo.read_landmarks(kind, 0, cap).items():
            snap[f"lm{kind}_{name}"] = v
    return snap


def same_snapshot(a, b):
    return a.keys() == b.keys() and all(bits(a[k]) == bits(b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]) for k in a)


def assert_geo_state(geo, model, km=None, where=""):
    """the device's geometry against the model's, bit for bit; n_obs against the kfmap's"""
    for kf in model.T_kf_w:
        T, x = geo.read_keyframe(kf)
        assert (bits(T), bits(x)) == (bits(model.T_kf_w[kf]), bits(model.x_kf_w[kf])), (where, "keyframe", kf)
    for kind, cap in ((0, geo.caps.pt_lm_cap), (1, geo.caps.ls_lm_cap)):
        d = geo.read_landmarks(kind, 0, cap)
        kn = km.read_landmarks(kind, 0, cap) if km is not None else None
        for j in range(cap):
            lm = model.lms[kind].get(j)
            n = int(d["n_obs"][j])
            if lm is None:
                assert n == 0, (where, kind, j, n)
                if j in model.stale[kind]:
                    assert bits(d["lm3d"][j]) == bits(model.stale[kind][j]), (where, kind, j, "stale")
                continue
            assert n == len(lm.obs_list) == len(lm.sigma_list), (where, kind, j, n, len(lm.obs_list))
            assert bits(d["lm3d"][j]) == bits(lm.geo3d), (where, kind, j, "3D", d["lm3d"][j], lm.geo3d)
            assert bits(d["obs"][j, :n]) == bits(lm.obs_list), (where, kind, j, "obs", d["obs"][j, :n], lm.obs_list)
            assert bits(d["sigma"][j, :n]) == bits(lm.sigma_list), (where, kind, j, "sigma")
            if kn is not None and kn["alive"][j]:
                assert int(kn["n_obs"][j]) == n, (where, kind, j, "kfmap n_obs", kn["n_obs"][j], n)


class Trio:
    """the two models and (optionally) the two device objects, driven together"""

    def __init__(self, caps, ctx=None, maps=None, quiet=False):
        """quiet: the state is compared only where the test asks (check(..., force=True))"""
        self.caps, self.quiet = caps, quiet
        km = gfpl.KeyframeMap(ctx, *caps) if ctx is not None else None
        self.geo = gfpl.MapGeometry(ctx, *caps) if ctx is not None else None
        if maps is not None:
            maps += [km, self.geo]
        self.pair = KC.Pair(caps, km)
        if quiet:
            self.pair.check = lambda where: None
        self.km = km
        self.model = G.GeoModel(self.pair.model)
        self.views = {}      # kf -> (model view, device view)
        self.calls = 0

    def close(self):
        for o in (self.geo, self.km):
            if o is not None:
                o.close()

    def check(self, where, force=False):
        self.calls += 1
        if self.geo is not None and (force or not self.quiet):
            assert_geo_state(self.geo, self.model, self.km, f"{where} (call {self.calls})")

    def dev_view(self, view):
        return self.geo.view(**view.arrays()) if self.geo is not None else None

    def add_keyframe(self, view, T, x):
        rc, kf = self.pair.add_keyframe(view.rows(0), view.rows(1))
        assert rc == K.OK
        self.views[kf] = (view, self.dev_view(view))
        assert self.model.set_keyframe(kf, T, x) == K.OK
        if self.geo is not None:
            self.geo.set_keyframe(kf, T, x)
        self.check("add_keyframe")
        return kf

    def geo_observe_pairs(self, kind, kf0, kf1, pairs, lm_out, first_new, v0=None, v1=None):
        """the geometry call alone, on both; returns the code"""
        m0, d0 = self.views.get(kf0, self.views[0]) if v0 is None else (v0, self.dev_view(v0))   # (a keyframe the map lacks: any view)
        m1, d1 = self.views.get(kf1, self.views[0]) if v1 is None else (v1, self.dev_view(v1))
        rc = self.model.observe_pairs(kind, kf0, kf1, m0, m1, pairs, lm_out, first_new)
        if self.geo is not None:
            grc = self.geo.observe_pairs_rc(kind, kf0, kf1, d0, d1, np.array(pairs, np.int32).reshape(-1, 2),
                                            np.array(lm_out, np.int32), first_new)
            assert grc == rc, ("geo observe_pairs", grc, rc)
        self.check("observe_pairs")
        return rc

    def observe_pairs(self, kind, kf0, kf1, pairs):
        rc, lm_out, first, new = self.pair.observe_pairs(kind, kf0, kf1, pairs)
        assert rc == K.OK, rc
        assert self.geo_observe_pairs(kind, kf0, kf1, pairs, lm_out, first) == K.OK
        return lm_out, first, new

    def geo_observe_local(self, kind, kf1, pairs, unm_rows, lm_out, v1=None):
        m1, d1 = self.views[kf1] if v1 is None else (v1, self.dev_view(v1))
        rc = self.model.observe_local(kind, kf1, m1, pairs, unm_rows, lm_out)
        if self.geo is not None:
            grc = self.geo.observe_local_rc(kind, kf1, d1, np.array(pairs, np.int32).reshape(-1, 2), np.array(unm_rows, np.int32),
                                            np.array(lm_out, np.int32))
            assert grc == rc, ("geo observe_local", grc, rc)
        self.check("observe_local")
        return rc

    def observe_local(self, kind, kf1, pairs, sel_ids, unm_rows):
        rc, lm_out = self.pair.observe_local(kind, kf1, pairs, sel_ids, unm_rows)
        assert rc == K.OK, rc
        assert self.geo_observe_local(kind, kf1, pairs, unm_rows, lm_out) == K.OK
        return lm_out

    def remove_bad_and_free(self, prm):
        removed = self.pair.remove_bad(prm)
        for kind in (0, 1):
            assert self.model.free(kind, removed[kind]) == K.OK
            if self.geo is not None:
                assert self.geo.free_rc(kind, np.array(removed[kind], np.int32)) == K.OK
        self.check("free")
        return removed

    def write_landmark(self, kind, j, geo3d, obs_list, sigma_list, kf_obs, local=1):
        """a landmark with these lists in both objects (the test's way to any state)"""
        n = len(kf_obs)
        self.pair.write_landmarks(kind, j, [1 if n else 0], [local if n else 0], [1], [n], [kf_obs[0] if n else -1], [kf_obs])
        self.model.write_landmark(kind, j, geo3d, obs_list, sigma_list)
        if self.geo is not None:
            oc, w = self.caps[5], G.OBS_W[kind]
            obs, sig = np.zeros((1, oc, w)), np.zeros((1, oc))
            obs[0, :n] = np.array(obs_list, np.float64).reshape(n, w)
            sig[0, :n] = sigma_list
            self.geo.write_landmarks(kind, j, np.array(geo3d, np.float64).reshape(1, -1), [n], obs, sig)
        self.check("write_landmark")

    def assemble(self, which):
        """the model's gather and the device's, compared element for element; returns (code, model dict, struct, lists)"""
        rc, want = self.model.assemble(which)
        if self.geo is None:
            return rc, want, None, None
        grc, p, lists = self.geo.assemble_rc(self.km, which)
        assert grc == rc, ("assemble", grc, rc)
        if rc != K.OK:
            return rc, want, p, lists
        n = p.n
        assert (n.n_kf, n.n_fix, n.n_pt, n.n_ls, n.n_pt_obs, n.n_ls_obs) == want["n"], ("assemble counts", want["n"])
        got = self.geo.read_assembled(p)
        for k in ("kf_list", "fix_list", "pt_list", "ls_list"):
            assert got[k].tolist() == want[k], ("assemble", k, got[k].tolist(), want[k])
        for k in gfpl.LBA_INDICES:
            assert lists[k].tolist() == want[k].tolist(), ("assemble", k, lists[k].tolist(), want[k].tolist())
        for k, _ in gfpl.LBA_DOUBLES:
            assert bits(got[k]) == bits(want[k]), ("assemble", k)
        self.check("assemble")      # only workspace was written
        return rc, want, p, lists


def host_problem(d):
    """the model's gather as a gfpl.LbaProblem: the parent route's input"""
    return gfpl.LbaProblem(d["x_kf"], d["T_kf"], d["T_fix"], d["pt"], d["ls"], d["pt_obs_lm"], d["pt_obs_kf"], d["pt_obs"],
                           d["pt_sigma"], d["ls_obs_lm"], d["ls_obs_kf"], d["ls_obs"], d["ls_sigma"])


HAND_CAPS = (6, 4, 3, 8, 8, 4)


def shifted(dx):
    T = np.eye(4)
    T[0, 3] = dx
    return T.reshape(16)


def hand_view(base):
    """rows whose every double names its keyframe, row and field"""
    r = np.arange(4, dtype=np.float64)[:, None]
    return G.View(P=base + r * 10 + np.array([0.25, 0.5, 4.0]), pl=base + r * 10 + np.array([1.0, 2.0]),
                  sP=base + r[:3] * 10 + np.array([0.1, 0.2, 5.0]), eP=base + r[:3] * 10 + np.array([0.3, 0.4, 6.0]),
                  le=base + r[:3] * 10 + np.array([0.6, 0.8, 7.0]))


def hand_map(n_kf=4, ctx=None, maps=None):
    trio = Trio(HAND_CAPS, ctx, maps)
    for k in range(n_kf):
        trio.add_keyframe(hand_view(100.0 * k), shifted(0.5 * k), np.full(6, 0.01 * k))
    return trio


def gather_map(ctx=None, maps=None):
    """keyframes 0..4 of which 3 and 4 are local, keyframe 1 erased; local landmarks written by hand"""
    trio = hand_map(5, ctx, maps)
    trio.pair.form_local_map(dict(min_lm_cov_graph=1000000, min_kf_local_map=1))
    for kind, w3, wo in ((0, 3, 2), (1, 6, 3)):
        mk = lambda j, kfs: trio.write_landmark(kind, j, np.arange(w3) + 10.0 * j + kind, [np.arange(wo) + 100.0 * j + kf for kf in kfs],
                                                [1.0 + 0.25 * i for i in range(len(kfs))], kfs)
        mk(0, [0, 3])          # keyframe 0 observed: a fixed pose
        mk(1, [2, 3, 4])       # keyframe 2 alive, outside the list: fixed, and not keyframe 0
        mk(2, [1, 4])          # keyframe 1 is erased below: the observation is dropped
        mk(3, [1])             # left with nothing: dropped
    trio.pair.erase_keyframe(1)
    return trio


TICK_CAPS = (8, 48, 24, 512, 256, 8)      # kf_cap, pt_rows, ls_rows, pt_lm_cap, ls_lm_cap, obs_cap
TICK_PRM = dict(min_lm_cov_graph=1000, min_kf_local_map=1, min_lm_obs=3, cull_age=1)


def tick_sequence(trio, cam, solve=None, n_kf=6, seed=3):
    """n_kf keyframes in addKeyFrame's order: pairs with the previous keyframe, the local map, formLocalMap,
    the LBA (solve(trio) when given) and removeBadMapLandmarks + free.  Returns facts for assertions."""
    w = World(cam, seed, n_kf, 60, 30, 40, 20)
    lm_world = [{}, {}]
    facts = dict(created=0, carried=0, local_appends=0, removed=0, solves=0)
    for k in range(n_kf):
        kf = trio.add_keyframe(w.views[k], w.T[k], w.x[k])
        assert kf == k
        if k == 0:
            continue
        for kind in (0, 1):                                            # the keyframe-pair stage
            pairs = w.common(kind, k - 1, k)
            lm_out, first, new = trio.observe_pairs(kind, k - 1, k, pairs)
            for (r0, _), j in zip(pairs, lm_out):
                if j >= 0:
                    lm_world[kind][j] = w.world[k - 1][kind][r0]
            facts["created"] += new
            facts["carried"] += sum(0 <= j < first for j in lm_out)
        trio.pair.form_local_map(dict(TICK_PRM, min_kf_local_map=2))   # (the flags the local stage reads: one keyframe further back)
        for kind in (0, 1):                                            # the local-map stage
            _, sel = trio.pair.select(kind, K.LOCAL_UNSEEN, k)
            _, unm = trio.pair.unmatched(kind, k)
            at = {w.world[k][kind][r]: i for i, r in enumerate(unm)}
            pairs = [(a, at[lm_world[kind][j]]) for a, j in enumerate(sel) if lm_world[kind].get(j) in at]
            seen, uniq = set(), []
            for a, b in pairs:                                         # one pair per kf1 row
                if b not in seen:
                    seen.add(b)
                    uniq.append((a, b))
            trio.observe_local(kind, k, uniq, sel, unm)
            facts["local_appends"] += len(uniq)
        trio.pair.form_local_map(TICK_PRM)
        if solve is not None:
            facts["solves"] += solve(trio)
        removed = trio.remove_bad_and_free(dict(min_lm_obs=TICK_PRM["min_lm_obs"], cull_age=TICK_PRM["cull_age"]))
        facts["removed"] += len(removed[0]) + len(removed[1])
    return facts


def assert_tick_facts(f):
    assert f["created"] > 50 and f["carried"] > 50 and f["local_appends"] > 5 and f["removed"] >= 2, f
