"""The map's geometry half as the reference keeps it: obs_list, sigma_list and point3D / line3D of
MapPoint / MapLine and T_kf_w / x_kf_w of KeyFrame over plain Python lists of float64, one statement per
reference line (src/mapHandler.cpp, line numbers in the comments), driven together with the index model
of tests/kfmap_ref.py (kf_obs_list, the local flags and the keyframes are read from it, never copied).

Nothing here knows how the device stores any of it.  R P + t is spelled in se3_apply's order
(gfpl_device.hpp: ((T0 P0 + T1 P1) + T2 P2) + T3, no contraction).  Where the reference would crash
or is silent the model follows the ledger entries MG1-MG7 of DESIGN.md §3; the refusals are those
include/gfpl.h states.
"""
import numpy as np

import kfmap_ref as K

OK, E_INVALID, E_CAPACITY = K.OK, K.E_INVALID, K.E_CAPACITY
LM_W, OBS_W = (3, 6), (2, 3)
LBA_MAX_KFS = 16


def se3_apply(T, P):
    T = np.asarray(T, np.float64).reshape(4, 4)
    P = [np.float64(v) for v in P]
    return [((T[i, 0] * P[0] + T[i, 1] * P[1]) + T[i, 2] * P[2]) + T[i, 3] for i in range(3)]


class Landmark:
    """what MapPoint / MapLine hold of the geometry half (include/mapFeatures.h)"""

    def __init__(self, geo3d, obs0, obs1):
        self.geo3d = [np.float64(v) for v in geo3d]                 # point3D / line3D
        self.obs_list = [list(obs0), list(obs1)]                   # the constructor's obs, then :287 / :429
        self.sigma_list = [np.float64(1.0), np.float64(1.0)]       # the default argument at both places (MG2)


class View:
    """a keyframe's stereo features as numpy arrays: P, pl (points), sP, eP, le (lines)"""

    def __init__(self, P=None, pl=None, sP=None, eP=None, le=None):
        z3, z2 = np.zeros((0, 3)), np.zeros((0, 2))
        self.P = np.asarray(P if P is not None else z3, np.float64).reshape(-1, 3)
        self.pl = np.asarray(pl if pl is not None else z2, np.float64).reshape(-1, 2)
        self.sP = np.asarray(sP if sP is not None else z3, np.float64).reshape(-1, 3)
        self.eP = np.asarray(eP if eP is not None else z3, np.float64).reshape(-1, 3)
        self.le = np.asarray(le if le is not None else z3, np.float64).reshape(-1, 3)

    def rows(self, kind):
        return len(self.le) if kind else len(self.pl)

    def obs(self, kind, row):
        return [np.float64(v) for v in (self.le if kind else self.pl)[row]]

    def arrays(self):
        return dict(P=self.P, pl=self.pl, sP=self.sP, eP=self.eP, le=self.le)


class GeoModel:
    def __init__(self, kmodel):
        self.k = kmodel
        self.kf_cap, self.rows, self.lm_cap, self.obs_cap = kmodel.kf_cap, kmodel.rows, kmodel.lm_cap, kmodel.obs_cap
        self.T_kf_w, self.x_kf_w = {}, {}
        self.lms = [{}, {}]                                        # id -> Landmark (a freed id: absent)
        self.stale = [{}, {}]                                      # id -> the geo3d a freed landmark leaves behind

    # ------------------------------------------------------------------ keyframes
    def set_keyframe(self, kf, T, x):
        if not (0 <= kf < self.kf_cap):
            return E_INVALID
        self.T_kf_w[kf] = np.array(T, np.float64).reshape(16)
        self.x_kf_w[kf] = np.array(x, np.float64).reshape(6)
        return OK

    # ------------------------------------------------------------------ lookForCommonMatches
    def _place_checks(self, kind, lm_out, created):
        """the refusals that look at the landmarks: (invalid, capacity)"""
        invalid = capacity = False
        seen = {}
        for i, j in enumerate(lm_out):
            if j < -1 or j >= self.lm_cap[kind]:
                invalid = True
                continue
            if j == -1:
                continue
            seen[j] = seen.get(j, 0) + 1
            if created[i]:
                invalid = invalid or j in self.lms[kind] or seen[j] > 1
            elif j not in self.lms[kind]:
                invalid = True
        for j, cnt in seen.items():
            if j in self.lms[kind] and len(self.lms[kind][j].obs_list) + cnt > self.obs_cap:
                capacity = True
        return invalid, capacity

    def observe_pairs(self, kind, kf0, kf1, v0, v1, pairs, lm_out, first_new):
        pairs = [tuple(int(v) for v in p) for p in pairs]
        lm_out = [int(v) for v in lm_out]
        if kind not in (0, 1) or not (0 <= kf0 < self.kf_cap) or not (0 <= kf1 < self.kf_cap) or kf0 == kf1:
            return E_INVALID
        if kf0 not in self.T_kf_w or not (0 <= first_new <= self.lm_cap[kind]):
            return E_INVALID
        n = len(pairs)
        if n > min(v0.rows(kind), v1.rows(kind)) or n > self.rows[kind]:
            return E_INVALID
        invalid = any(not (0 <= a < v0.rows(kind) and 0 <= b < v1.rows(kind)) for a, b in pairs)
        created = [j >= first_new for j in lm_out]
        inv2, capacity = self._place_checks(kind, lm_out, created)
        if invalid or inv2:
            return E_INVALID
        if capacity:
            return E_CAPACITY
        T = self.T_kf_w[kf0]
        for (lr_qdx, lr_tdx), j, new in zip(pairs, lm_out, created):   # pair order
            if j == -1:                                                # :308
                continue
            if new:                                                    # :270-289, :407-431
                if kind == 0:
                    geo3d = se3_apply(T, v0.P[lr_qdx])                 # :276-277
                else:
                    geo3d = se3_apply(T, v0.sP[lr_qdx]) + se3_apply(T, v0.eP[lr_qdx])   # :413-417
                self.lms[kind][j] = Landmark(geo3d, v0.obs(kind, lr_qdx), v1.obs(kind, lr_tdx))
            else:                                                      # :312, :440
                lm = self.lms[kind][j]
                lm.obs_list.append(v1.obs(kind, lr_tdx))
                lm.sigma_list.append(np.float64(1.0))
        return OK

    def observe_local(self, kind, kf1, v1, pairs, unm_rows, lm_out):
        pairs = [tuple(int(v) for v in p) for p in pairs]
        unm_rows, lm_out = [int(v) for v in unm_rows], [int(v) for v in lm_out]
        if kind not in (0, 1) or not (0 <= kf1 < self.kf_cap):
            return E_INVALID
        if len(unm_rows) > v1.rows(kind) or len(pairs) > len(unm_rows) or len(pairs) > self.rows[kind]:
            return E_INVALID
        invalid = any(not (0 <= b < len(unm_rows)) or not (0 <= unm_rows[b] < v1.rows(kind)) for a, b in pairs)
        inv2, capacity = self._place_checks(kind, lm_out, [False] * len(lm_out))
        if invalid or inv2:
            return E_INVALID
        if capacity:
            return E_CAPACITY
        for (_, b), j in zip(pairs, lm_out):                          # :609-615, :745-764
            if j == -1:
                continue
            lm = self.lms[kind][j]
            lm.obs_list.append(v1.obs(kind, unm_rows[b]))
            lm.sigma_list.append(np.float64(1.0))
        return OK

    def free(self, kind, ids):
        ids = [int(v) for v in ids]
        if kind not in (0, 1) or len(ids) > self.lm_cap[kind] or any(not (0 <= j < self.lm_cap[kind]) for j in ids):
            return E_INVALID
        for j in ids:                                                  # :2585 delete map_points[j]
            if j in self.lms[kind]:
                self.stale[kind][j] = self.lms[kind].pop(j).geo3d
        return OK

    def write_landmark(self, kind, j, geo3d, obs_list, sigma_list):
        """the loop-closure walk's store of a merged landmark; an empty obs_list frees it"""
        if len(obs_list) == 0:
            self.lms[kind].pop(j, None)
            self.stale[kind][j] = [np.float64(v) for v in geo3d]
            return
        lm = Landmark(geo3d, obs_list[0], obs_list[0])
        lm.obs_list = [[np.float64(v) for v in o] for o in obs_list]
        lm.sigma_list = [np.float64(s) for s in sigma_list]
        self.lms[kind][j] = lm

    # ------------------------------------------------------------------ the gathering loops
    def assemble(self, which):
        """localBundleAdjustment :1113-1209 (which = LOCAL) / globalBundleAdjustment :1851-1939 (ALIVE) as a
        gfpl_lba_problem: (code, dict)"""
        k = self.k
        alive = [kf is not None for kf in k.map_keyframes]
        kf_list = [kf.kf_idx for kf in k.map_keyframes                 # :1115-1127, :1853-1863
                   if kf is not None and kf.kf_idx != 0 and (which == K.ALIVE or kf.local)]
        sel = [[], []]
        fixed = set()
        for kind in (0, 1):
            for lm in k.map_lms[kind]:                                 # map order (:1133, :1174)
                if lm is None or not (which == K.ALIVE or lm.local):
                    continue
                mine = self.lms[kind].get(lm.idx)
                if (len(mine.obs_list) if mine else 0) != len(lm.kf_obs_list):
                    return E_INVALID, None
                kept = [i for i, kf in enumerate(lm.kf_obs_list) if alive[kf]]   # :1981; MG5 for the LBA
                if not kept:
                    continue
                sel[kind].append((lm.idx, kept))
                fixed |= {lm.kf_obs_list[i] for i in kept if lm.kf_obs_list[i] not in kf_list}
        fix_list = sorted(fixed)                                       # MG4
        slot = {kf: j for j, kf in enumerate(kf_list)}                 # :1153-1160
        slot.update({kf: -1 - j for j, kf in enumerate(fix_list)})
        d = dict(kf_list=kf_list, fix_list=fix_list, pt_list=[j for j, _ in sel[0]], ls_list=[j for j, _ in sel[1]])
        d["x_kf"] = np.array([self.x_kf_w[kf] for kf in kf_list], np.float64).reshape(-1, 6)      # :1121
        d["T_kf"] = np.array([self.T_kf_w[kf] for kf in kf_list], np.float64).reshape(-1, 16)
        d["T_fix"] = np.array([self.T_kf_w[kf] for kf in fix_list], np.float64).reshape(-1, 16)
        for kind, name in ((0, "pt"), (1, "ls")):
            geo, obs, sig, olm, okf = [], [], [], [], []
            for local_idx, (j, kept) in enumerate(sel[kind]):
                lm, klm = self.lms[kind][j], k.map_lms[kind][j]
                geo.append(lm.geo3d)                                   # :1139, :1180
                for i in kept:                                         # :1143-1162 in list order
                    obs.append(lm.obs_list[i])
                    sig.append(lm.sigma_list[i])
                    olm.append(local_idx)
                    okf.append(slot[klm.kf_obs_list[i]])
            d[name] = np.array(geo, np.float64).reshape(-1, LM_W[kind])
            d[name + "_obs"] = np.array(obs, np.float64).reshape(-1, OBS_W[kind])
            d[name + "_sigma"] = np.array(sig, np.float64).reshape(-1, 1)
            d[name + "_obs_lm"] = np.array(olm, np.int32)
            d[name + "_obs_kf"] = np.array(okf, np.int32)
        d["n"] = (len(kf_list), len(fix_list), len(sel[0]), len(sel[1]), len(d["pt_obs_lm"]), len(d["ls_obs_lm"]))
        return OK, d

    def write_back(self, d, T_kf, pt, ls):
        """:1688-1712 (x_kf_w is not refreshed: BA1)"""
        for i, kf in enumerate(d["kf_list"]):
            self.T_kf_w[kf] = np.array(T_kf[i], np.float64).reshape(16)
        for i, j in enumerate(d["pt_list"]):
            self.lms[0][j].geo3d = [np.float64(v) for v in pt[i]]
        for i, j in enumerate(d["ls_list"]):
            self.lms[1][j].geo3d = [np.float64(v) for v in ls[i]]

    def lba_code(self, d, caps=None):
        """what gfpl_mapgeo_lba answers for the LOCAL assembly d before it solves: None when it solves"""
        n = d["n"]
        if n[4] + n[5] == 0:
            return OK                                                  # :1212
        if n[0] < 1:
            return E_INVALID                                           # MG6
        if n[0] > LBA_MAX_KFS:
            return E_CAPACITY
        if caps is not None and any(a > b for a, b in zip((n[0], n[2], n[3], n[4], n[5]), (caps[0], caps[2], caps[3], caps[4], caps[5]))):
            return E_CAPACITY
        return None

    # ------------------------------------------------------------------ the state, for comparison
    def state(self):
        out = dict(kfs={kf: (self.T_kf_w[kf].tobytes(), self.x_kf_w[kf].tobytes()) for kf in self.T_kf_w}, lms=[{}, {}], stale=[{}, {}])
        for kind in (0, 1):
            for j, lm in self.lms[kind].items():
                out["lms"][kind][j] = (np.array(lm.geo3d, np.float64).tobytes(), np.array(lm.obs_list, np.float64).tobytes(),
                                       np.array(lm.sigma_list, np.float64).tobytes(), len(lm.obs_list))
            for j, g in self.stale[kind].items():
                if j not in self.lms[kind]:
                    out["stale"][kind][j] = np.array(g, np.float64).tobytes()
        return out
