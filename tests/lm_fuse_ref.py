"""Landmark fusion's reference (include/gfpl.h "ops that cross landmarks"):
lm_store_ref.Model extended with GFPL_LM_APPEND_LM and the sequential semantics of
gfpl_lmstore_fuse, the rules of gfpl_lm_fuse_check, the origin of every element of a final list,
and MapHandler::loopClosureFuseLandmarks' walk (src/mapHandler.cpp:4425 ff.) over a small
pure-Python map that emits the ops of one gfpl_lmstore_fuse per kind.
"""
import numpy as np

import lm_store_ref as R

ADD, ERASE_OBS, FREE, APPEND_LM = R.ADD, R.ERASE_OBS, R.FREE, 3
OK, E_INVALID, E_CAPACITY, E_UNSUPPORTED = R.OK, R.E_INVALID, R.E_CAPACITY, -7


def _rows(ops):
    return np.asarray(ops, np.int64).reshape(-1, 4).tolist()


class Model(R.Model):
    """The ops one after another over the whole list, as gfpl_lmstore_fuse runs them."""

    def fuse_check(self, ops, src_rows, counts=None):
        """(code, counts after, n_rows, origins): the rules of gfpl_lm_fuse_check, the first failing
        op decides.  origins: {lm: list of (src, row)} for every landmark named as lm, over its
        final list: src >= 0 a source row, src < 0 row `row` of landmark -1 - src before the call.
        A refused list returns the counts as they were, n_rows 0 and no origins."""
        before = np.array(self.counts() if counts is None else counts, np.int32)
        refused = lambda code: (code, before.copy(), 0, {})
        lists, freed, named, n_rows = {}, set(), [], 0

        def cur(lm):   # the list of a landmark as origins, None when its count is not a count
            if lm not in lists:
                if not 0 <= before[lm] <= self.obs_cap:
                    return None
                lists[lm] = [(-1 - lm, p) for p in range(int(before[lm]))]
            return lists[lm]
        for lm, kind, arg, src in _rows(ops):
            if not 0 <= lm < self.lm_cap or cur(lm) is None or lm in freed:
                return refused(E_INVALID)
            if lm not in named:
                named.append(lm)
            if kind == ADD:
                if not 0 <= src < len(src_rows) or not 0 <= arg < src_rows[src]:
                    return refused(E_INVALID)
                if len(lists[lm]) >= self.obs_cap:
                    return refused(E_CAPACITY)
                lists[lm].append((src, arg))
                n_rows += 1
            elif kind == ERASE_OBS:
                return refused(E_UNSUPPORTED)
            elif kind == FREE:
                lists[lm] = []
                freed.add(lm)
                n_rows += 1
            elif kind == APPEND_LM:
                if not 0 <= arg < self.lm_cap or arg == lm or arg in freed or cur(arg) is None:
                    return refused(E_INVALID)
                if not lists[arg] or not lists[lm]:        # the reference merges two landmarks that are != NULL
                    return refused(E_INVALID)
                if len(lists[lm]) + len(lists[arg]) > self.obs_cap:
                    return refused(E_CAPACITY)
                lists[lm] += list(lists[arg])              # desc_list.push_back over the source's list, in order
                n_rows += len(lists[arg])
            else:
                return refused(E_INVALID)
        after = before.copy()
        for lm in named:
            after[lm] = len(lists[lm])
        return OK, after, n_rows, {lm: lists[lm] for lm in named}

    def fuse(self, ops, srcs):
        """The ops in array order (a valid list); returns the landmarks named as lm, by first touch."""
        named = {}
        for lm, kind, arg, src in _rows(ops):
            named[lm] = True
            if kind == ADD:
                self.lists[lm].append(np.array(srcs[src][arg], np.uint8))
            elif kind == FREE:
                self.lists[lm] = []
            else:
                assert kind == APPEND_LM and arg != lm
                self.lists[lm] = self.lists[lm] + [r.copy() for r in self.lists[arg]]
        return list(named)


# ---- loopClosureFuseLandmarks (src/mapHandler.cpp:4425 ff.), the desc_list half of one kind -----
class Landmark:
    """What the walk touches of a MapPoint / MapLine: desc_list and the lists the caller keeps in
    parallel (obs_list stands for kf_obs_list / obs_list / dir_list / pts_list: one entry per row)."""

    def __init__(self, idx):
        self.idx, self.desc_list, self.obs_list = idx, [], []


class Map:
    """map_points (or map_lines) as a list with None for NULL, and per keyframe the features'
    landmark index (-1: none) and descriptors."""

    def __init__(self, n_lm, kf_desc):
        self.lms = [None] * n_lm
        self.kf_desc = [np.asarray(d, np.uint8) for d in kf_desc]        # [kf][rows][32]
        self.kf_idx = [[-1] * len(d) for d in self.kf_desc]              # features' idx

    def observe(self, lm, kf, row):
        if self.lms[lm] is None:
            self.lms[lm] = Landmark(lm)
        self.lms[lm].desc_list.append(self.kf_desc[kf][row].copy())
        self.lms[lm].obs_list.append((kf, row))
        self.kf_idx[kf][row] = lm


def loop_closure_fuse_walk(m: Map, kf_prev: int, kf_curr: int, lc_idxs, max_idx: int):
    """The four cases of loopClosureFuseLandmarks over lc_idxs rows (lm_idx0, lm_ldx0, lm_idx1,
    lm_ldx1) as the reference records them: the landmark indices are the row's, not the features'
    current idx.  Runs on the Python map and emits the same as ops for one gfpl_lmstore_fuse whose
    sources are the keyframes' descriptor arrays (source k = keyframe k).  max_idx: the reference's
    max_pt_idx / max_ls_idx, the slot of the next new landmark (len(m.lms) grows with it).
    Returns (ops, max_idx).  The features are never NULL here (stereo_pt[...] != NULL)."""
    ops = []
    for lm0, r_prev, lm1, r_curr in lc_idxs:
        if lm0 == -1 and lm1 != -1:            # the landmark exists once: the previous keyframe's feature joins it
            if m.lms[lm1] is not None:
                m.observe(lm1, kf_prev, r_prev)
                ops.append((lm1, ADD, r_prev, kf_prev))
        if lm0 != -1 and lm1 == -1:
            if m.lms[lm0] is not None:
                m.observe(lm0, kf_curr, r_curr)
                ops.append((lm0, ADD, r_curr, kf_curr))
        if lm0 == -1 and lm1 == -1:            # a new landmark from both features (created by its first ADD)
            while len(m.lms) <= max_idx:
                m.lms.append(None)
            m.observe(max_idx, kf_prev, r_prev)
            m.observe(max_idx, kf_curr, r_curr)
            ops += [(max_idx, ADD, r_prev, kf_prev), (max_idx, ADD, r_curr, kf_curr)]
            max_idx += 1
        if lm0 != -1 and lm1 != -1:            # two landmarks: the current one is merged into the previous one
            # lm0 == lm1: the reference pushes onto the list it iterates (undefined); nothing to merge, skipped here
            if lm0 != lm1 and m.lms[lm0] is not None and m.lms[lm1] is not None:
                a, b = m.lms[lm0], m.lms[lm1]
                for d, o in zip(b.desc_list, b.obs_list):
                    a.desc_list.append(d.copy())
                    a.obs_list.append(o)
                m.kf_idx[kf_curr][r_curr] = lm0    # (only this feature's idx changes, :4534)
                m.lms[lm1] = None
                ops += [(lm0, APPEND_LM, lm1, 0), (lm1, FREE, 0, 0)]
    return ops, max_idx



def fuse_local_map_walk(m: Map, local_idx, pairs, as_written=True):
    """The fuse loop of fuseLandmarksFromLocalMap (src/mapHandler.cpp:926-952 points; the line loop,
    :1060-1099, first orders the pair by length) over the pairs of gfpl_map_fuse_search.  local_idx
    [j]: the landmark index of selected row j (map_local_points_idx); the loop works on the pointers
    taken at selection time (map_local_points), which it never nulls.
    as_written: `map_points[map_local_points_idx[k]] = NULL` with k the position in the fuse list
    (ledger FU10), so the k-th selected landmark is dropped, whichever was merged; the ops it emits
    can name a freed landmark, which gfpl_lmstore_fuse refuses as a whole.  Otherwise the evident
    intent: the merged landmark is dropped, its pointer nulled, and a pair with a NULL side skipped.
    Returns the ops of one gfpl_lmstore_fuse."""
    ptr = [m.lms[i] for i in local_idx]
    ops = []
    for k, (i1, i2) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2).tolist()):
        P1, P2 = ptr[i1], ptr[i2]
        if P1 is None or P2 is None or i1 == i2:
            continue
        for d, o in zip(list(P2.desc_list), list(P2.obs_list)):   # addMapPointObservation per observation of P2
            P1.desc_list.append(d.copy())
            P1.obs_list.append(o)
        ops.append((P1.idx, APPEND_LM, P2.idx, 0))
        gone = local_idx[k] if as_written else P2.idx
        m.lms[gone] = None
        ops.append((gone, FREE, 0, 0))
        if not as_written:
            ptr[i2] = None
    return ops


# ---- fuseLandmarksFromLocalMap's candidate search (src/mapHandler.cpp:859-1056) -----------------
# The statement of gfpl_map_fuse_search, one kind at a time.  Every operation below is one IEEE
# double operation on numpy arrays, written in the order the ledger pins;
# numpy contracts nothing.
def _sum3(a0, a1, a2):
    """FU3: a size-3 sum as Eigen 3.3's unvectorised fixed-size reduction takes it."""
    return a0 + (a1 + a2)


def _norm3(v):
    return np.sqrt(_sum3(v[..., 0] * v[..., 0], v[..., 1] * v[..., 1], v[..., 2] * v[..., 2]))


def _dot3(a, b):
    return _sum3(a[..., 0] * b[..., 0], a[..., 1] * b[..., 1], a[..., 2] * b[..., 2])


def in_image(cam, T, X):
    """FU1 / FU2: Pf = R X + t with T taken as written (T_kf_w, not inverted), pf = projection(Pf);
    0 < pf.x < width, 0 < pf.y < height, Pf.z > 0, all strict.  T [n][16], X [n][3]."""
    with np.errstate(all="ignore"):
        Pf = [((T[:, 4 * i] * X[:, 0] + T[:, 4 * i + 1] * X[:, 1]) + T[:, 4 * i + 2] * X[:, 2]) + T[:, 4 * i + 3] for i in range(3)]
        u = cam["cx"] + (cam["fx"] * Pf[0]) / Pf[2]
        v = cam["cy"] + (cam["fy"] * Pf[1]) / Pf[2]
        return (u > 0) & (u < cam["width"]) & (v > 0) & (v < cam["height"]) & (Pf[2] > 0.0)


def knn2_self(desc):
    """[n][2] neighbours of every row among all rows, its own included: ascending (distance, index),
    the tie rule of gfpl_knn2_hamming."""
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8), axis=1).astype(np.float32)
    ones = bits.sum(1)
    d = (ones[:, None] + ones[None, :] - 2.0 * (bits @ bits.T)).astype(np.int64)   # exact: integers below 2^24
    key = d * len(desc) + np.arange(len(desc))[None, :]
    return np.argsort(key, axis=1, kind="stable")[:, :2]


def point_gate(P, i, t, prm):
    """FU4: |P_t - P_i| < max_point_point_error."""
    return _norm3(P[t] - P[i]) < prm["max_point_point_error"]


def line_gate(L, i, t, prm, branch=None):
    """FU5-FU7 over pairs (i, t) of rows of L [n][6]; branch (a list) receives d1.norm() > d2.norm()."""
    with np.errstate(all="ignore"):
        L1, L2 = L[i], L[t]
        v1, v2 = L1[:, 3:] - L1[:, :3], L2[:, 3:] - L2[:, :3]
        d1, d2 = v1 / _norm3(v1)[:, None], v2 / _norm3(v2)[:, None]       # a zero-length line: 0 / 0 = NaN
        Ld = _norm3(d1 - d2)
        first = _norm3(d1) > _norm3(d2)                                      # two numbers within an ulp of 1, as written

        def dist(p, x, d):                                                   # |(p - x) - ((p - x) . d) d|
            w = p - x
            return _norm3(w - _dot3(w, d)[:, None] * d)
        dP = np.where(first, dist(L2[:, :3], L1[:, :3], d1), dist(L1[:, :3], L2[:, :3], d2))
        dQ = np.where(first, dist(L2[:, 3:], L1[:, :3], d1), dist(L1[:, 3:], L2[:, :3], d2))
        if branch is not None:
            branch.extend(first.tolist())
        return (Ld < prm["max_dir_line_error"]) & (dP < prm["max_point_line_error"]) & (dQ < prm["max_point_line_error"])


DEFAULT_FUSE_PARAMS = dict(max_point_point_error=0.1, max_point_line_error=0.1, max_dir_line_error=0.1)   # src/config.cpp:46-48


def search(cam, desc, X, kf, T_kf, prm=None, stats=None):
    """One kind of gfpl_map_fuse_search.  X [n][3] points or [n][6] lines, kf [n] = kf_obs_list[0],
    T_kf [n_kf][16].  Returns (loc, pairs [m][2], bad_kf): loc the map rows selected, in order;
    pairs (i, t) over the selected list in ascending i; bad_kf whether some kf lies outside
    [0, n_kf) (such a row is not selected and the call returns GFPL_E_INVALID).  stats (a dict)
    receives the pairs that reached the gate, the accepted ones and the lines' branches."""
    prm = prm or DEFAULT_FUSE_PARAMS
    desc, X = np.asarray(desc, np.uint8).reshape(-1, 32), np.asarray(X, np.float64)
    n = len(desc)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros((0, 2), np.int32), False
    X = X.reshape(n, -1)
    kf, T_kf = np.asarray(kf, np.int64).reshape(-1), np.asarray(T_kf, np.float64).reshape(-1, 16)
    good_kf = (kf >= 0) & (kf < len(T_kf))
    sel = np.zeros(n, bool)
    if good_kf.any():
        g = np.nonzero(good_kf)[0]
        keep = in_image(cam, T_kf[kf[g]], X[g, :3])
        if X.shape[1] == 6:
            keep &= in_image(cam, T_kf[kf[g]], X[g, 3:])
        sel[g] = keep
    loc = np.nonzero(sel)[0].astype(np.int32)
    pairs = np.zeros((0, 2), np.int32)
    if len(loc) > 1:
        second = knn2_self(desc[loc])[:, 1]
        i = np.nonzero(second != np.arange(len(loc)))[0]          # lr_qdx != lr_tdx
        t = second[i]
        branch = []
        ok = point_gate(X[loc], i, t, prm) if X.shape[1] == 3 else line_gate(X[loc], i, t, prm, branch)
        pairs = np.stack([i[ok], t[ok]], axis=1).astype(np.int32)
        if stats is not None:
            stats.update(reached=len(i), accepted=int(ok.sum()), branch=branch)
    return loc, pairs, bool((~good_kf).any())
