"""Hand-made line descriptor sets for the in-kernel line matching (k_stereo_lines, k_cross_lines) and a
plain numpy statement of the matching stage they are compared with.

Three parts:
  * the reference: Hamming / 2-bit-cell distances through a 256-entry table, the forward knn-2, the
    reverse knn-1 and the acceptance rules of the stereo and the cross-frame line matching, in integer
    numpy.  It calls neither the oracle nor the library.  Every rule can be altered (`Rules`) so a test
    can show that the descriptor families notice the fault an alteration stands for;
  * the descriptor families, each aimed at one way knn2_mfma (gfpl_knn.hpp) can go wrong, over the grid
    of tile-edge line counts;
  * keylines that make every (left i, right j) pair pass the triangulation gates and let the pair be
    read back from the output row, and the frame builders for the GPU handler and the oracle.
"""
from collections import namedtuple

import numpy as np

import gfpl   # struct definitions and the synthetic frame container only
from test_knn_fp4_gpu import _POP1, _POP2

# ------------------------------------------------------------------------------------- reference --
_TAB = {1: _POP1.astype(np.uint8), 2: _POP2.astype(np.uint8)}   # (a byte holds at most 8 bits / 4 cells)
BIG = 1000   # a distance above every real one (256): a candidate that is not there


def distances(q, t, cell):
    """D[i, j]: set bits (cell 1) / differing 2-bit cells (cell 2) of q[i] ^ t[j], per byte by table."""
    tab = _TAB[cell]
    D = np.empty((len(q), len(t)), np.int64)
    for i0 in range(0, len(q), 128):   # (chunks: the 2048 x 2048 x 32 byte cube does not fit comfortably)
        D[i0:i0 + 128] = tab[q[i0:i0 + 128, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int64)
    return D


# The matching rules, and the faults of knn2_mfma they can be altered into (test_families_are_sensitive):
#   fwd_tie_high  the forward knn keeps the HIGHER train index among equal distances
#   rev_tie_high  the reverse knn keeps the HIGHER query index among equal distances
#   pad_trains    the zero rows that fill the last train tile count as candidates (at the distance a zero
#                 row has: the row's set bits / non-zero cells)
#   pad_queries   the zero columns that fill the last query tile count as reverse candidates
#   pad_dist0     both kinds of padding count as candidates at distance 0
#   drop_last     the last train row of a partial tile is not a candidate (forward and reverse)
#   ge            the nn12 test is >= instead of >
Rules = namedtuple("Rules", "fwd_tie_high rev_tie_high pad_trains pad_queries pad_dist0 drop_last ge",
                   defaults=(False,) * 7)
EXACT = Rules()
ALTERATIONS = {"rev_tie_high": Rules(rev_tie_high=True), "fwd_tie_high": Rules(fwd_tie_high=True),
               "pad_trains": Rules(pad_trains=True), "pad_queries": Rules(pad_queries=True),
               "pad_dist0": Rules(pad_dist0=True),
               "drop_last": Rules(drop_last=True), "ge": Rules(ge=True)}


def _zero_dist(rows, cell):
    return _TAB[cell][rows].sum(axis=1, dtype=np.int64)


def knn(D, q, t, cell, rules=EXACT):
    """(lr, d0, d1, rl): per query the two lexicographically smallest (D[i, j], j) -> lr, d0, d1; per
    train the lexicographically smallest (D[i, j], i) -> rl.  With altered rules an index can point at
    a padding row (>= the count)."""
    nq, nt = D.shape
    F = D.copy()
    if rules.drop_last and nt % 32:
        F[:, nt - 1] = BIG
    R = F.T.copy()
    if (rules.pad_trains or rules.pad_dist0) and nt % 32:
        pad = np.repeat(_zero_dist(q, cell)[:, None], 32 - nt % 32, axis=1)
        F = np.concatenate([F, 0 * pad if rules.pad_dist0 else pad], axis=1)
    if (rules.pad_queries or rules.pad_dist0) and nq % 32:
        pad = np.repeat(_zero_dist(t, cell)[:, None], 32 - nq % 32, axis=1)
        R = np.concatenate([R, 0 * pad if rules.pad_dist0 else pad], axis=1)

    def keys(M, high):
        idx = np.arange(M.shape[1], dtype=np.int64)
        return M * 65536 + ((65535 - idx) if high else idx)[None, :]

    kf = np.sort(keys(F, rules.fwd_tie_high), axis=1)[:, :2]
    lr = kf[:, 0] & 0xFFFF
    if rules.fwd_tie_high:
        lr = 65535 - lr
    d0, d1 = kf[:, 0] >> 16, kf[:, 1] >> 16
    kr = keys(R, rules.rev_tie_high).min(axis=1)
    rl = kr & 0xFFFF
    if rules.rev_tie_high:
        rl = 65535 - rl
    return lr, d0, d1, rl


def _nn12_th(d0, d1, n, desc_th_l):
    """lineDescriptorMAD's nn12 threshold: 1.4826 * float(sorted(float(d1 - d0))[n / 2]) * desc_th_l."""
    dev = np.sort((d1 - d0).astype(np.float32))
    return (1.4826 * float(dev[n // 2])) * desc_th_l


def _mutual(lr, rl, i):
    return lr[i] < len(rl) and rl[lr[i]] == i


def stereo_pairs(D, q, t, cell, desc_th_l=0.1, rules=EXACT):
    """The ordered (i, lr[i]) list of the stereo line matching (initial frame: cell 1, later: cell 2)."""
    NL, NR = D.shape
    if NL < 2 or NR < 2:
        return np.zeros((0, 2), np.int64)
    lr, d0, d1, rl = knn(D, q, t, cell, rules)
    th = _nn12_th(d0, d1, NL, desc_th_l)
    out = []
    for i in range(min(NL, NR)):
        d12 = float(np.float32(d1[i]) - np.float32(d0[i]))
        if _mutual(lr, rl, i) and (d12 >= th if rules.ge else d12 > th):
            out.append((i, int(lr[i])))
    return np.array(out, np.int64).reshape(-1, 2)


def cross_pairs(D, q, t, desc_th_l=0.1, max_num=300, rules=EXACT):
    """The ordered (i, lr[i]) list of the cross-frame line matching (cell 1), cut at max_num."""
    Sl, Sc = D.shape
    if Sl < 2 or Sc < 2:
        return np.zeros((0, 2), np.int64)
    lr, d0, d1, rl = knn(D, q, t, 1, rules)
    nn12 = _nn12_th(d0, d1, Sl, desc_th_l)
    budget = float(np.sort(d0.astype(np.float32))[min(max_num, Sl) - 1])
    out = []
    for i in range(Sl):
        if float(np.float32(d0[i])) > 1.2 * budget:
            continue
        d12 = float(np.float32(d1[i]) - np.float32(d0[i]))
        if _mutual(lr, rl, i) and (d12 >= nn12 if rules.ge else d12 > nn12):
            out.append((i, int(lr[i])))
        if len(out) >= max_num:
            break
    return np.array(out, np.int64).reshape(-1, 2)


# -------------------------------------------------------------------------------------- families --
GRID = (2, 31, 32, 33, 63, 64, 65, 255, 256)      # partial and full tiles, one to eight tiles per side
GRID_PAIRS = [(nl, nr) for nl in GRID for nr in GRID]
KL_CAP = 256
FAMILIES = ("planted", "reverse_ties", "reverse_near_ties", "forward_dups", "forward_dups_open", "zero_rows",
            "extremes", "all_equal", "edge_bytes")
# forward_dups_open: the forward_dups sets with a negative desc_th_l, so that a pair with d1 - d0 = 0
# passes the nn12 test and the forward tie rule (lower train index) shows in the accepted list — with
# the default threshold (>= 0) a tied best match is never accepted and the rule cannot be observed.
CFG_OVER = {"forward_dups_open": {"desc_th_l": -1.0}}


def desc_th_l(family):
    return CFG_OVER.get(family, {}).get("desc_th_l", 0.1)


def _flip(rng, rows, n, cells=None):
    """rows with n bits flipped per row, each in a distinct 2-bit cell: both norms see distance n."""
    rows = np.atleast_2d(rows)
    pool = np.arange(128) if cells is None else np.asarray(cells)
    m = len(rows)
    pick = pool[np.argsort(rng.random((m, len(pool))), axis=1)[:, :n]]
    bits = 2 * pick + rng.integers(0, 2, (m, n))
    mask = np.zeros((m, 32), np.uint8)
    np.bitwise_xor.at(mask, (np.repeat(np.arange(m), n), (bits >> 3).ravel()),
                      (1 << (bits & 7)).astype(np.uint8).ravel())
    return rows ^ mask


def _planted(rng, nq, nt, flips=16):
    """Train = a permutation of noisy copies of the queries (the rest random): most rows form accepted
    mutual matches at distance `flips`, everything else sits near 128 (cell 1) / 96 (cell 2)."""
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    m = min(nq, nt)
    perm = rng.permutation(nt)[:m]
    t[perm] = _flip(rng, q[:m], flips)
    return q, t, perm


def tie_placements(nq, m):
    """Query pairs a < b for the reverse ties: inside one 16-lane DPP row at each of the reduce-scatter's
    partner distances (p ^ 15, p ^ 7, p ^ 3, p ^ 1), in the other DPP row of a tile, across a column-tile
    edge (31 / 32, 63 / 64: different waves) and from tile 0 to the last tile."""
    cands = [(2, 13), (3, 4), (5, 6), (8, 9), (17, 30), (31, 32), (63, 64), (1, nq - 1), (10, nq - 2)]
    used, out = set(), []
    for a, b in cands:
        if a < b < nq and a < m and a not in used and b not in used:
            out.append((a, b))
            used |= {a, b}
    return out or [(0, 1)]


def dup_placements(nt):
    """Train pairs lo < hi holding the same row: lowest / highest index, and across the tile edges."""
    return [(0, nt - 1)] + [(lo, hi) for lo, hi in ((31, 32), (63, 64)) if hi < nt - 1]


def descriptors(family, nq, nt):
    """(q [nq][32], t [nt][32], facts): facts names what was planted, for the known-answer checks."""
    fam = "forward_dups" if family == "forward_dups_open" else family
    rng = np.random.default_rng([FAMILIES.index(fam), nq, nt])
    q, t, perm = _planted(rng, nq, nt)
    m = min(nq, nt)
    facts = {}
    if fam == "planted":
        pass
    elif fam in ("reverse_ties", "reverse_near_ties"):
        facts["ties"] = []
        for a, b in tie_placements(nq, m):
            T = int(perm[a])
            q[a] = _flip(rng, t[T], 16)[0]
            q[b] = q[a]
            if fam == "reverse_near_ties":   # b one bit closer to t: restore the lowest flipped bit
                diff = q[a] ^ t[T]
                k = int(np.nonzero(diff)[0][0])
                q[b, k] ^= np.uint8(int(diff[k]) & -int(diff[k]))
            facts["ties"].append((a, b, T))
    elif fam == "forward_dups":
        facts["dups"] = []
        for k, (lo, hi) in enumerate(dup_placements(nt)):
            if k < nq:
                t[hi] = t[lo]
                q[k] = t[lo]
                facts["dups"].append((k, lo, hi))
    elif fam == "zero_rows":
        if (nq + nt) % 2 == 0:
            # two all-zero queries and one all-zero train: the zero rows that pad a partial train tile
            # are at distance 0 from them as well (second-best distance, or an index >= nt)
            za, zb, tz = (0, 1, nt // 2) if nq == 2 else (1, min(5, nq - 1), nt // 2)
            q[za] = 0
            q[zb] = 0
            t[tz] = 0
            facts["zero"] = (za, zb, tz)
        else:
            # a train row of three set bits in the last tile with a query at distance 16: the zero
            # columns that pad a partial query tile are at distance 3 from it
            s = nt - 1
            t[s] = 0
            t[s, 0], t[s, 10], t[s, 31] = 0x01, 0x10, 0x80
            q[0] = _flip(rng, t[s], 16)[0]
            facts["sparse"] = (0, s)
    elif fam == "extremes":
        blk = max(1, min(4, nq // 2, nt // 2))
        q[1:1 + blk] = 0x00
        t[nt - blk:] = 0xFF
        facts["extremes"] = (1, nt - blk, blk)
    elif fam == "all_equal":
        q[:] = q[0]
        t[:] = q[0]
    elif fam == "edge_bytes":
        # rows differ from a common row only in bytes 0..3 (even rows) or 28..31 (odd rows): the first
        # and the last k-step of both lane halves, for both cells; planted partners two bits away
        common = q[0].copy()
        for rows in (q, t):
            n = len(rows)
            r = rng.integers(0, 256, (n, 4), dtype=np.uint8)
            rows[:] = common
            rows[0::2, 0:4] = r[0::2]
            rows[1::2, 28:32] = r[1::2]
        ev, od = np.arange(0, m, 2), np.arange(1, m, 2)
        t[perm[ev]] = _flip(rng, q[ev], 2, cells=np.arange(0, 16))
        if len(od):
            t[perm[od]] = _flip(rng, q[od], 2, cells=np.arange(112, 128))
    else:
        raise ValueError(family)
    return q, t, facts


class Case:
    """One sequence's line descriptors: queries q (left / previous frame), trains t (right / current)."""

    def __init__(self, family, q, t, facts=None):
        self.family, self.q, self.t, self.facts = family, q, t, facts or {}
        self.nl, self.nr = len(q), len(t)
        self._D, self._ref = {}, {}

    def D(self, cell):
        if cell not in self._D:
            self._D[cell] = distances(self.q, self.t, cell)
        return self._D[cell]

    def stereo(self, cell, rules=EXACT):
        """reference pairs of the stereo matching (cell 1: initialize, cell 2: stereoLines)"""
        k = ("s", cell, rules)
        if k not in self._ref:
            self._ref[k] = stereo_pairs(self.D(cell), self.q, self.t, cell, desc_th_l(self.family), rules)
        return self._ref[k]

    def cross(self, rules=EXACT, max_num=300):
        k = ("c", rules, max_num)
        if k not in self._ref:
            self._ref[k] = cross_pairs(self.D(1), self.q, self.t, desc_th_l(self.family), max_num, rules)
        return self._ref[k]

    def what(self):
        return f"{self.family} NL {self.nl} NR {self.nr}"


_CASES = {}


def grid_cases(family):
    """The 81 sequences of one family (one per (NL, NR) of the grid), built and referenced once."""
    if family not in _CASES:
        _CASES[family] = [Case(family, *descriptors(family, nl, nr)) for nl, nr in GRID_PAIRS]
    return _CASES[family]


def large_cases():
    """kl_cap 2048: (2048, 2047) and (2047, 2048) as prefixes of one 2048-row reverse_ties set, so the
    distances are computed once: train indices above 1024, the 1024-thread kernels, the largest LDS layout."""
    if "large" not in _CASES:
        q, t, facts = descriptors("reverse_ties", 2048, 2048)
        full = Case("reverse_ties", q, t, facts)
        out = []
        for nl, nr in ((2048, 2047), (2047, 2048)):
            c = Case("reverse_ties", q[:nl], t[:nr])
            c._D = {cell: full.D(cell)[:nl, :nr] for cell in (1, 2)}
            out.append(c)
        _CASES["large"] = out
    return _CASES["large"]


ODD_CAP = 200


def odd_cases():
    """kl_cap 200 (no multiple of the 32-row tile: a view stride that is not tile-aligned), counts 200 / 199."""
    if "odd" not in _CASES:
        _CASES["odd"] = [Case(f, *descriptors(f, nl, nr))
                         for f, (nl, nr) in (("reverse_near_ties", (200, 199)), ("zero_rows", (199, 200)))]
    return _CASES["odd"]


MATCH_CAP_KL = 512


def match_cap_cases():
    """Cross lines only: 512-row sets with more than max_line_match_num (300) mutual matches, every
    seventh planted pair at distance 24 (above 1.2 * budget = 19.2) and, where Sl > Sc, unplanted queries."""
    if "match_cap" not in _CASES:
        out = []
        for nl, nr in ((512, 512), (512, 480), (500, 512)):
            rng = np.random.default_rng([99, nl, nr])
            q, t, perm = _planted(rng, nl, nr)
            far = np.arange(0, min(nl, nr), 7)
            t[perm[far]] = _flip(rng, q[far], 24)
            out.append(Case("match_cap", q, t, {"far": far}))
        _CASES["match_cap"] = out
    return _CASES["match_cap"]


# -------------------------------------------------------------------------------------- geometry --
# Vertical segments with common end rows: left line i at x = XL0 + i dx, right line j at x = XR0 + j dx,
# dx a power of two, every right x at least 64 below every left x.  Then for every (i, j): the overlap
# is 1, |le[0]| is 1 (200 before normalising), both disparities are xl - xr >= 64 exactly, and the
# endpoint covariance gate's largest eigenvalue stays below 1e-3 (line_cov_th 10), so triangulate
# accepts the pair and the output row holds i in spl[0] and j in spl[0] - sdisp.
XL0, XR0, SY, EY = 330.0, 10.0, 100.0, 300.0


def line_dx(cap):
    return min(1.0, 256.0 / (1 << (cap - 1).bit_length()))


def keylines(cap):
    dx = line_dx(cap)
    out = []
    for x0 in (XL0, XR0):
        kl = np.zeros(cap, gfpl.KEYLINE_DT)
        kl["sx"] = kl["ex"] = (x0 + dx * np.arange(cap)).astype(np.float32)
        kl["sy"], kl["ey"] = SY, EY
        kl["angle"] = np.arctan2(np.float32(EY - SY), np.float32(0.0)).astype(np.float32)
        out.append(kl)
    return out


def fill_frames(H, f, cases):
    """Overwrite the line inputs of frame f of a HostFrames with one case per sequence.  Rows past the
    counts hold exact copies of a row of the OTHER side: a read past a count would find a perfect match."""
    cap = H.kl_cap
    kl_l, kl_r = keylines(cap)
    assert len(cases) == H.B
    for b, c in enumerate(cases):
        H.n_kl_l[f, b], H.n_kl_r[f, b] = c.nl, c.nr
        H.kl_l[f, b], H.kl_r[f, b] = kl_l, kl_r
        H.ldesc_l[f, b] = c.t[0]
        H.ldesc_r[f, b] = c.q[0]
        H.ldesc_l[f, b, :c.nl] = c.q
        H.ldesc_r[f, b, :c.nr] = c.t


def stereo_rows(fh, cap):
    """The (i, j) pairs of a frame's stereo lines, decoded from spl[0] and sdisp; None when a row is
    no line of the grid."""
    dx = line_dx(cap)
    x = fh.get("ls_spl")[:, 0]
    i = (x - XL0) / dx
    j = ((x - fh.get("ls_sdisp")) - XR0) / dx
    if not (np.all(i == np.round(i)) and np.all(j == np.round(j))):
        return None
    return np.stack([i, j], axis=1).astype(np.int64).reshape(-1, 2)


def check_stereo(fh, case, cell, initial, cap):
    """[] or the differences of a frame's stereo lines from the reference of `case`."""
    want = case.stereo(cell)
    got = stereo_rows(fh, cap)
    w = f"{case.what()} cell {cell}: "
    if got is None:
        return [w + "an output row is no line of the grid"]
    out = (got < 0).any(axis=1) | (got[:, 0] >= case.nl) | (got[:, 1] >= case.nr)
    if out.any():
        return [w + f"an index out of range: {got[out][0].tolist()}"]
    if len(got) != len(want) or not np.array_equal(got, want):
        return [w + f"{len(got)} pairs, want {len(want)}; first difference {_first_diff(got, want)}"]
    bad = []
    if not np.array_equal(fh.get("ldesc"), case.q[want[:, 0]]):
        bad.append(w + "ldesc rows are not the left rows")
    idx = np.arange(len(want)) if initial else np.full(len(want), -1)
    if not np.array_equal(fh.get("ls_idx"), idx):
        bad.append(w + f"ls_idx {fh.get('ls_idx')[:8].tolist()}.. want {idx[:8].tolist()}..")
    return bad


def _first_diff(got, want):
    for k in range(max(len(got), len(want))):
        g = got[k].tolist() if k < len(got) else None
        w = want[k].tolist() if k < len(want) else None
        if g != w:
            return f"at {k}: got {g} want {w}"
    return "none"


# Cross lines: no geometric gate.  PREV ls_idx = 1000 + i and CURR ls_sdisp = j, so after the stage
# matched_ls holds the accepted i in order, PREV ls_sdisp_obs[i] the partner j, and CURR ls_idx[j]
# the written-back 1000 + i; everything else keeps -1.
def cross_frames(case, kp_cap, cap):
    P, C = gfpl.FrameHost(kp_cap, cap), gfpl.FrameHost(kp_cap, cap)
    for fh, rows, n in ((P, case.q, case.nl), (C, case.t, case.nr)):
        fh.s.n_pt, fh.s.n_ls = 0, n
        fh.arr["ldesc"][:n] = rows
        fh.arr["ls_sdisp_obs"][:] = -1.0
        fh.arr["ls_idx"][:] = -1
        for nme in ("Tfw", "DT"):
            getattr(fh.s, nme)[:] = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    P.arr["ls_idx"][:case.nl] = 1000 + np.arange(case.nl)
    C.arr["ls_sdisp"][:case.nr] = np.arange(case.nr)
    return P, C


def check_cross(prev, curr, track, case, max_num=300):
    """[] or the differences of the state after crossFrameMatchingLines from the reference of `case`."""
    want = case.cross(max_num=max_num)
    w = f"{case.what()} cross: "
    m = np.asarray(track["matched_ls"], np.int64)
    obs = prev.get("ls_sdisp_obs")
    bad = []
    if track["n_inliers_ls"] != len(want):
        bad.append(w + f"n_inliers_ls {track['n_inliers_ls']} want {len(want)}")
    if len(m) and (m.min() < 0 or m.max() >= case.nl):
        return bad + [w + f"a matched index out of range: {m.tolist()[:8]}"]
    got = np.stack([m, obs[m].astype(np.int64)], axis=1).reshape(-1, 2)
    if len(got) != len(want) or not np.array_equal(got, want):
        return bad + [w + f"{len(got)} pairs, want {len(want)}; first difference {_first_diff(got, want)}"]
    e_obs = np.full(case.nl, -1.0)
    e_obs[want[:, 0]] = want[:, 1]
    e_idx = np.full(case.nr, -1, np.int64)
    e_idx[want[:, 1]] = 1000 + want[:, 0]
    if not np.array_equal(obs, e_obs):
        k = int(np.nonzero(obs != e_obs)[0][0])
        bad.append(w + f"PREV ls_sdisp_obs[{k}] = {obs[k]} want {e_obs[k]}")
    if not np.array_equal(curr.get("ls_idx"), e_idx):
        k = int(np.nonzero(curr.get("ls_idx") != e_idx)[0][0])
        bad.append(w + f"CURR ls_idx[{k}] = {curr.get('ls_idx')[k]} want {e_idx[k]}")
    return bad


def host_frames(cam, n_seq, kl_cap, kp_cap=64):
    """One synthetic frame of n_seq sequences with few keypoints: the point inputs and the pyramid stay
    ordinary, the line inputs are overwritten by fill_frames."""
    sp = gfpl.synth_params(n_kp=48, n_kl=8, n_world_pts=80, n_world_lines=16, seed=5)
    return gfpl.HostFrames(cam, sp, n_seq, 1, kp_cap, kl_cap)
