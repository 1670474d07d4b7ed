"""The map's index half as the reference keeps it: MapHandler's integer bookkeeping restated over plain
Python lists, one statement per reference line (src/mapHandler.cpp, line numbers in the comments).

The model holds what the reference holds: every keyframe's idx arrays, map_points / map_lines entries
or None, real map_points_kf_idx / map_lines_kf_idx lists, and full_graph as a list of lists.  Nothing
here knows how the device stores any of it.  Where the reference would crash or is silent the model
follows the ledger entries KM1-KM10 of DESIGN.md §3; the refusals are those include/gfpl.h states.
"""
import bisect

OK, E_INVALID, E_CAPACITY, E_STATE = 0, -1, -5, -6
POINTS, LINES = 0, 1
LOCAL, LOCAL_UNSEEN, ALIVE = 0, 1, 2
DEFAULT_PARAMS = dict(min_lm_cov_graph=30, min_kf_local_map=3, min_lm_obs=2, cull_age=10)   # src/config.cpp:40, 51, 53; :2558


class Landmark:
    """what MapPoint / MapLine hold of the index half (include/mapFeatures.h)"""

    def __init__(self, idx, kf_obs_list, local=False, inlier=True):
        self.idx = idx
        self.kf_obs_list = list(kf_obs_list)
        self.local = local        # KM9: the constructor leaves it unset; false until the tick's formLocalMap
        self.inlier = inlier      # src/mapFeatures.cpp:29, :97


class KeyFrame:
    def __init__(self, kf_idx, n_pt, n_ls):
        self.kf_idx = kf_idx
        self.local = True                              # :123 (KM9: also for initialize's keyframe)
        self.idx = [[-1] * n_pt, [-1] * n_ls]          # stereo_pt[i]->idx, stereo_ls[i]->idx  (:64-67, :131-134)


class Model:
    def __init__(self, kf_cap, pt_rows, ls_rows, pt_lm_cap, ls_lm_cap, obs_cap):
        self.kf_cap, self.rows, self.lm_cap, self.obs_cap = kf_cap, (pt_rows, ls_rows), (pt_lm_cap, ls_lm_cap), obs_cap
        # initialize (:42-58)
        self.map_keyframes = []
        self.map_lms = [[], []]                        # map_points, map_lines
        self.kf_lists = [{}, {}]                       # map_points_kf_idx, map_lines_kf_idx
        self.full_graph = []
        self.max_idx = [0, 0]                          # max_pt_idx, max_ls_idx

    # ------------------------------------------------------------------ helpers
    @property
    def n_kf(self):
        return len(self.map_keyframes)

    def kf_ok(self, kf):
        return 0 <= kf < self.n_kf and self.map_keyframes[kf] is not None

    def lm(self, kind, j):
        return self.map_lms[kind][j]

    # ------------------------------------------------------------------ keyframes
    def add_keyframe(self, n_pt, n_ls):
        if n_pt < 0 or n_ls < 0:
            return E_INVALID, -1
        if self.n_kf >= self.kf_cap or n_pt > self.rows[0] or n_ls > self.rows[1]:
            return E_CAPACITY, -1
        # expandGraphs (:116) / initialize's 1 x 1 graph (:56-58)
        for row in self.full_graph:
            row.append(0)
        self.full_graph.append([0] * (self.n_kf + 1))
        kf = KeyFrame(self.n_kf, n_pt, n_ls)           # max_kf_idx++ (:121), the index reset (:131-134)
        self.map_keyframes.append(kf)                  # :90, :148
        self.kf_lists[0][kf.kf_idx] = []               # :91-92, :149-150
        self.kf_lists[1][kf.kf_idx] = []
        return OK, kf.kf_idx

    def erase_keyframe(self, kf_idx):
        if not self.kf_ok(kf_idx):
            return E_INVALID
        for k in range(len(self.full_graph) - 1):      # :2777 (as written: the last index is left, KM10)
            self.full_graph[kf_idx][k] = 0
            self.full_graph[k][kf_idx] = 0
        self.map_keyframes[kf_idx] = None              # :2784
        return OK

    # ------------------------------------------------------------------ lookForCommonMatches
    def _append(self, kind, lm_idx, kf1_idx):
        """addMap*Observation's kf_obs_list.push_back and the graph loop (:315-324, :615-624)"""
        lm = self.lm(kind, lm_idx)
        lm.kf_obs_list.append(kf1_idx)
        for obs in lm.kf_obs_list:
            if obs != kf1_idx:
                self.full_graph[kf1_idx][obs] += 1
                self.full_graph[obs][kf1_idx] += 1

    @staticmethod
    def _column_repeats(pairs, col):
        vals = [p[col] for p in pairs]
        return len(set(vals)) != len(vals)

    def _capacity(self, kind, appended, n_created):
        """GFPL_E_CAPACITY: a list beyond obs_cap, an id beyond the landmark cap"""
        for lm_idx in set(appended):
            if len(self.lm(kind, lm_idx).kf_obs_list) + appended.count(lm_idx) > self.obs_cap:
                return True
        return self.max_idx[kind] + n_created > self.lm_cap[kind]

    def observe_pairs(self, kind, kf0_idx, kf1_idx, pairs):
        """returns (code, lm_out, first_new, n_new); a refused call changes nothing"""
        pairs = [tuple(int(v) for v in p) for p in pairs]
        if kind not in (0, 1) or not self.kf_ok(kf0_idx) or not self.kf_ok(kf1_idx) or kf0_idx == kf1_idx:
            return E_INVALID, None, None, None
        kf0, kf1 = self.map_keyframes[kf0_idx], self.map_keyframes[kf1_idx]
        idx0, idx1 = kf0.idx[kind], kf1.idx[kind]
        bad = self._column_repeats(pairs, 0) or self._column_repeats(pairs, 1)            # KM8
        bad = bad or any(not (0 <= a < len(idx0) and 0 <= b < len(idx1)) for a, b in pairs)
        bad = bad or any(idx0[a] < -1 or idx0[a] >= self.max_idx[kind] for a, b in pairs if 0 <= a < len(idx0))
        if bad:
            return E_INVALID, None, None, None
        appended = [idx0[a] for a, b in pairs if idx0[a] != -1 and self.lm(kind, idx0[a]) is not None]
        if self._capacity(kind, appended, sum(idx0[a] == -1 for a, b in pairs)):
            return E_CAPACITY, None, None, None
        first_new, lm_out = self.max_idx[kind], []
        for lr_qdx, lr_tdx in pairs:                   # the loop body with its gates passed (:266-336, :404-485)
            if idx0[lr_qdx] == -1:                     # :270 new 3D landmark
                idx0[lr_qdx] = self.max_idx[kind]      # :273
                idx1[lr_tdx] = self.max_idx[kind]      # :274
                lm = Landmark(self.max_idx[kind], [kf0_idx])                      # :280
                self.kf_lists[kind][kf0_idx].append(self.max_idx[kind])          # :282
                lm.kf_obs_list.append(kf1_idx)         # :287
                self.map_lms[kind].append(lm)          # :289
                self.max_idx[kind] += 1                # :290
                self.full_graph[kf1_idx][kf0_idx] += 1                           # :292
                self.full_graph[kf0_idx][kf1_idx] += 1                           # :293
                lm_out.append(lm.idx)
            else:
                lm_idx = idx0[lr_qdx]                  # :307
                if self.lm(kind, lm_idx) is not None:  # :308
                    idx1[lr_tdx] = lm_idx              # :310
                    self._append(kind, lm_idx, kf1_idx)                          # :315-324
                    lm_out.append(lm_idx)
                else:
                    lm_out.append(-1)                  # KM6: the pair of a freed landmark does nothing
        return OK, lm_out, first_new, self.max_idx[kind] - first_new

    def observe_local(self, kind, kf1_idx, pairs, sel_ids, unm_rows):
        """returns (code, lm_out)"""
        pairs = [tuple(int(v) for v in p) for p in pairs]
        sel_ids, unm_rows = [int(v) for v in sel_ids], [int(v) for v in unm_rows]
        if kind not in (0, 1) or not self.kf_ok(kf1_idx):
            return E_INVALID, None
        idx1 = self.map_keyframes[kf1_idx].idx[kind]
        if len(sel_ids) > self.max_idx[kind] or len(unm_rows) > len(idx1) or len(pairs) > min(len(sel_ids), len(unm_rows)):
            return E_INVALID, None
        bad = self._column_repeats(pairs, 0) or self._column_repeats(pairs, 1)
        bad = bad or any(not (0 <= a < len(sel_ids) and 0 <= b < len(unm_rows)) for a, b in pairs)
        if bad:
            return E_INVALID, None
        lms = [sel_ids[a] for a, b in pairs]
        rows = [unm_rows[b] for a, b in pairs]
        if any(not (0 <= j < self.max_idx[kind]) or self.lm(kind, j) is None for j in lms):
            return E_INVALID, None
        if any(not (0 <= r < len(idx1)) for r in rows) or len(set(rows)) != len(rows):
            return E_INVALID, None
        if self._capacity(kind, lms, 0):
            return E_CAPACITY, None
        for lm_idx, row in zip(lms, rows):
            idx1[row] = lm_idx                         # :611-612
            self._append(kind, lm_idx, kf1_idx)        # :615-624
        return OK, lms

    # ------------------------------------------------------------------ formLocalMap (:789-857)
    def form_local_map(self, min_lm_cov_graph, min_kf_local_map, **_):
        if self.n_kf < 1 or self.map_keyframes[-1] is None:
            return E_STATE
        for kf in self.map_keyframes:                  # :793-797
            if kf is not None:
                kf.local = False
        for kind in (0, 1):                            # :798-807
            for lm in self.map_lms[kind]:
                if lm is not None:
                    lm.local = False

        def mark(kf):
            for kind in (0, 1):
                for lm_idx in kf.idx[kind]:
                    if lm_idx != -1 and self.lm(kind, lm_idx) is not None:      # :817, :844
                        self.lm(kind, lm_idx).local = True
        self.map_keyframes[-1].local = True            # :810
        mark(self.map_keyframes[-1])                   # :811-830
        g_size = len(self.full_graph) - 1              # :833
        for i in range(g_size):
            if self.full_graph[g_size][i] >= min_lm_cov_graph or abs(g_size - i) <= min_kf_local_map:   # :836
                if self.map_keyframes[i] is None:      # KM1: :838 dereferences it unchecked
                    continue
                self.map_keyframes[i].local = True     # :838
                mark(self.map_keyframes[i])            # :840-853
        return OK

    # ------------------------------------------------------------------ the selections
    def select(self, kind, which, kf1_idx=0):
        out = []
        for lm in self.map_lms[kind]:                  # map order
            if lm is None:
                continue
            if which == ALIVE:
                out.append(lm.idx)
            elif which == LOCAL and lm.local:          # :1133-1166
                out.append(lm.idx)
            elif which == LOCAL_UNSEEN and lm.local and lm.kf_obs_list[-1] != kf1_idx:   # :520, :642
                out.append(lm.idx)
        return out

    def unmatched(self, kind, kf_idx):
        return [it for it, v in enumerate(self.map_keyframes[kf_idx].idx[kind]) if v == -1]   # :539-546, :666-673

    def local_keyframes(self):
        return [kf.kf_idx for kf in self.map_keyframes if kf is not None and kf.local and kf.kf_idx != 0]   # :1115-1127

    # ------------------------------------------------------------------ removeBadMapLandmarks (:2550-2630)
    def remove_bad(self, min_lm_obs, cull_age, **_):
        max_kf_idx = self.n_kf - 1
        removed = [[], []]
        for kind in (0, 1):
            for j, lm in enumerate(self.map_lms[kind]):
                if lm is None:
                    continue
                if lm.local is False and max_kf_idx - lm.kf_obs_list[0] > cull_age:          # :2558 (KM7)
                    if lm.inlier is False or len(lm.kf_obs_list) < min_lm_obs:                # :2560 (KM4)
                        kf_obs = lm.kf_obs_list[0]     # :2562
                        if self.map_keyframes[kf_obs] is None:                                # KM2: :2565 dereferences it
                            continue
                        rows = self.map_keyframes[kf_obs].idx[kind]
                        for r in range(len(rows)):     # :2565-2573: the first carrying row, then the loop ends
                            if rows[r] == lm.idx:
                                rows[r] = -1
                                break
                        lst = self.kf_lists[kind][kf_obs]
                        if lm.idx in lst:              # :2576-2583
                            lst.remove(lm.idx)
                        self.map_lms[kind][j] = None   # :2585
                        removed[kind].append(j)
        return removed

    def set_inlier(self, kind, ids, value):
        ids = [int(v) for v in ids]
        if kind not in (0, 1) or value not in (0, 1) or any(not (0 <= j < self.max_idx[kind]) for j in ids):
            return E_INVALID
        for j in ids:
            if self.lm(kind, j) is not None:
                self.lm(kind, j).inlier = bool(value)
        return OK

    # ------------------------------------------------------------------ the patch calls
    def write_keyframe_idx(self, kind, kf_idx, row0, idx):
        idx = [int(v) for v in idx]
        if kind not in (0, 1) or not self.kf_ok(kf_idx) or row0 < 0:
            return E_INVALID
        rows = self.map_keyframes[kf_idx].idx[kind]
        if row0 + len(idx) > len(rows) or any(v < -1 or v >= self.max_idx[kind] for v in idx):
            return E_INVALID
        rows[row0:row0 + len(idx)] = idx
        return OK

    def write_landmarks(self, kind, id0, alive, local, inlier, n_obs, owner, kf_obs):
        """kf_obs: one list per landmark (its first n_obs entries count)"""
        n = len(alive)
        if kind not in (0, 1) or id0 < 0 or id0 + n > self.lm_cap[kind]:
            return E_INVALID
        for i in range(n):
            if alive[i] not in (0, 1) or local[i] not in (0, 1) or inlier[i] not in (0, 1):
                return E_INVALID
            if not ((1 if alive[i] else 0) <= n_obs[i] <= self.obs_cap) or not (-1 <= owner[i] < self.n_kf):
                return E_INVALID
            if any(not (0 <= k < self.n_kf) for k in kf_obs[i][:n_obs[i]]):
                return E_INVALID
        while self.max_idx[kind] < id0 + n:            # the ids between are freed landmarks
            self.map_lms[kind].append(None)
            self.max_idx[kind] += 1
        for i in range(n):
            j = id0 + i
            self.map_lms[kind][j] = (Landmark(j, kf_obs[i][:n_obs[i]], bool(local[i]), bool(inlier[i])) if alive[i] else None)
            for lst in self.kf_lists[kind].values():
                if j in lst:
                    lst.remove(j)
            if owner[i] >= 0:
                bisect.insort(self.kf_lists[kind][int(owner[i])], j)              # KM3: a list is its landmarks in ascending id
        return OK

    # ------------------------------------------------------------------ the state, for comparison
    def owner_of(self, kind):
        own = [-1] * self.max_idx[kind]
        for k, lst in self.kf_lists[kind].items():
            for j in lst:
                own[j] = k
        return own

    def state(self):
        """every keyframe's rows and flags, every landmark record, full_graph, and the lists as
        gfpl_pgo_problem takes them"""
        kfs = []
        for kf in self.map_keyframes:
            kfs.append(None if kf is None else dict(local=int(kf.local), pt_idx=list(kf.idx[0]), ls_idx=list(kf.idx[1])))
        lms, csr = [], []
        for kind in (0, 1):
            own = self.owner_of(kind)
            recs = []
            for j, lm in enumerate(self.map_lms[kind]):
                recs.append(dict(owner=own[j]) if lm is None else
                            dict(owner=own[j], local=int(lm.local), inlier=int(lm.inlier), kf_obs=list(lm.kf_obs_list)))
            lms.append(recs)
            assert all(lst == sorted(lst) for lst in self.kf_lists[kind].values())    # KM3 holds on every path taken
            start, idx = [0], []
            for k in range(self.n_kf):
                idx += self.kf_lists[kind][k]
                start.append(len(idx))
            csr.append(dict(start=start, idx=idx, freed=[int(lm is None) for lm in self.map_lms[kind]]))
        return dict(kfs=kfs, lms=lms, graph=[list(r) for r in self.full_graph], csr=csr,
                    alive=[int(kf is not None) for kf in self.map_keyframes])
