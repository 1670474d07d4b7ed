"""Hand-made keyframes and local maps for the keyframe match consumers (gfpl_kf_common_matches,
gfpl_kf_local_map_matches: k_kf_gate, k_kf_map_filter and the single-sequence k_knn2m launches) and a
plain numpy statement of the two stages they are compared with.

Three parts, as in point_match_cases.py:
  * the statement: common_matches / local_map_matches in integer, float32 and float64 numpy.  It calls
    neither the library nor the oracle.  Every rule can be altered (`Rules`), one alteration per kernel
    fault, so a test can show that the families notice that fault;
  * the families, each aimed at one mechanism of the kernels, at the smallest counts where it turns over;
  * the containers (`KF`, `Map`, `Case`) that hand one case to the oracle or to a Context.

Geometry of the descriptor families (ties, ratio, MAD) is trivial on purpose: identity poses, the exact
camera (fx = fy = 512, cx = 320, cy = 240) and every feature on one spot, so each pairing has error 0 and
the descriptor rules alone decide.  The threshold families use the same camera with Z a power of two, so a
projection is exact under any association; `Case.exact` marks them, every other statement-checked case
must keep its geometric decisions 1e-9 (relative) away from their thresholds (`Res.margin`).  A projection
of exactly the smallest positive double needs cx = cy = 0 (320 + x cannot be that small): the `corner`
camera, where (X, Y, 512) projects to (X, Y).
"""
import math
from collections import namedtuple

import numpy as np

import gfpl   # struct definitions, cameras and the frame container only
from point_match_cases import hamming

# ------------------------------------------------------------------------------------- statement --
# The rules, and the kernel faults they can be altered into (test_families_are_sensitive):
#  knn     knn_tie_high      equal best distances go to the HIGHER train row
#          second_tie_high   equal second distances go to the HIGHER train row
#  tests   no_mutual         the mutual-best test is dropped
#          ratio_lt          d0 / d1 < max_ratio_12_p
#          ratio_double_div  the ratio is a double division
#          mad_median_lo     the MAD median is element (n - 1) / 2
#          mad_ge            d1 - d0 >= threshold
#          mad_over_all_rows (local map) the MAD runs over all map rows, not the compacted ones
#  gates   chi_le            err <= sqrt(7.815)
#          sigma_not_sqrt    err = |e| * sigma2
#          epip_le           (local map) error <= max_kf_epip_p / _l
#          line_abs          (local map) the line residuals are compared by absolute value
#  filter  border_incl_lo / border_incl_hi   pf >= 0 / pf <= width, height
#          no_z_test         no z > 0 test (filter and local-map gate)
#          one_endpoint      a line with one endpoint inside passes the filter
#  output  pair_compact_row  (local map) a pair names the compacted row
#          chunk_offset      the gate's second 1024-chunk starts writing at 0
#          unordered         pairs not in row order
_RULES = ("knn_tie_high second_tie_high no_mutual ratio_lt ratio_double_div mad_median_lo mad_ge mad_over_all_rows "
          "chi_le sigma_not_sqrt epip_le line_abs border_incl_lo border_incl_hi no_z_test one_endpoint "
          "pair_compact_row chunk_offset unordered")
Rules = namedtuple("Rules", _RULES, defaults=(False,) * len(_RULES.split()))
EXACT = Rules()
ALTERATIONS = {n: Rules(**{n: True}) for n in _RULES.split()}
Res = namedtuple("Res", "pp lp margin")
CHI = math.sqrt(7.815)
BLOCK = 1024   # k_kf_gate / k_kf_map_filter compact in chunks of BLOCK rows


def knn2(q, t, rules=EXACT):
    """cv::batchDistance's insertion rule over integer Hamming distances: both neighbours take the lower
    train row among equals.  -> idx [nq][2] int32, dist [nq][2] float32"""
    D = hamming(q, t)
    nq, nt = D.shape
    j, r = np.arange(nt), np.arange(nq)
    k = D * nt + ((nt - 1 - j) if rules.knn_tie_high else j)
    i0 = np.argmin(k, axis=1)
    k = D * nt + ((nt - 1 - j) if rules.second_tie_high else j)
    k[r, i0] = np.iinfo(np.int64).max
    i1 = np.argmin(k, axis=1)
    return (np.stack([i0, i1], 1).astype(np.int32), np.stack([D[r, i0], D[r, i1]], 1).astype(np.float32))


def inverse_se3(T):
    T = np.asarray(T, np.float64).reshape(4, 4).tolist()
    o = [[0.0] * 4 for _ in range(4)]
    for i in range(3):
        for j in range(3):
            o[i][j] = T[j][i]
        o[i][3] = ((-T[0][i]) * T[0][3] + (-T[1][i]) * T[1][3]) + (-T[2][i]) * T[2][3]
    o[3][3] = 1.0
    return o


def mat4_mul(A, B):
    A, B = np.asarray(A, np.float64).reshape(4, 4).tolist(), np.asarray(B, np.float64).reshape(4, 4).tolist()
    return [[((A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]) + A[i][3] * B[3][j] for j in range(4)]
            for i in range(4)]


def _se3(T, X):
    X = np.asarray(X, np.float64).reshape(-1, 3)
    return np.stack([((T[i][0] * X[:, 0] + T[i][1] * X[:, 1]) + T[i][2] * X[:, 2]) + T[i][3] for i in range(3)], 1)


def _project(cam, X):
    return np.stack([cam.cx + (cam.fx * X[:, 0]) / X[:, 2], cam.cy + (cam.fy * X[:, 1]) / X[:, 2]], 1)


class _Margin:
    """the smallest relative distance of a finite geometric value from its threshold (a non-finite value is
    decided by the IEEE comparison rules, not by a rounding)"""

    def __init__(self):
        self.v = math.inf

    def __call__(self, val, th, scale=None):
        val = np.asarray(val, np.float64).ravel()
        r = np.abs(val - th) / (abs(th) if scale is None else scale)
        r = r[np.isfinite(r)]
        if r.size:
            self.v = min(self.v, float(r.min()))


def _knn(cache, key, q, t, rules):
    key = key + (rules.knn_tie_high, rules.second_tie_high)
    if cache is None:
        return knn2(q, t, rules)
    if key not in cache:
        cache[key] = knn2(q, t, rules)
    return cache[key]


def _mad_th(d12, cfg, rules):
    v = np.sort(np.abs(d12[:, 1] - d12[:, 0]))             # float32
    k = (len(v) - 1) // 2 if rules.mad_median_lo else len(v) // 2
    return (1.4826 * float(v[k])) * cfg.desc_th_l


def _desc_test(lines, i12, d12, i21, cfg, rules, th):
    n0 = len(i12)
    t = i12[:, 0]
    ok = (np.arange(n0) == i21[t, 0]) | rules.no_mutual
    d0, d1 = d12[:, 0], d12[:, 1]
    if not lines:
        r = d0.astype(np.float64) / d1.astype(np.float64) if rules.ratio_double_div else (d0 / d1).astype(np.float64)
        ok &= (r < cfg.max_ratio_12_p) if rules.ratio_lt else (r <= cfg.max_ratio_12_p)
    else:
        diff = (d1 - d0).astype(np.float64)
        ok &= (diff >= th) if rules.mad_ge else (diff > th)
    return t, ok


def _compact(t, flag, rules, rows=None):
    sel = np.flatnonzero(flag)
    if rules.chunk_offset and len(flag) > BLOCK:
        sel = sel[sel >= BLOCK]   # the later chunks overwrite the first one's pairs; the count is theirs
    left = sel if rows is None or rules.pair_compact_row else rows[sel]
    p = np.stack([left, t[sel]], 1).astype(np.int32).reshape(-1, 2)
    return p[::-1].copy() if rules.unordered else p


_NONE = np.zeros((0, 2), np.int32)


def common_matches(cam, cfg, kf0, kf1, rules=EXACT, cache=None):
    """MapHandler::lookForCommonMatches, keyframe-pair stage: the accepted (kf0 row, kf1 row) pairs."""
    mg = _Margin()
    DT = mat4_mul(inverse_se3(kf1.T), kf0.T)
    lt = (lambda a, b: a <= b) if rules.chi_le else (lambda a, b: a < b)
    out = []
    with np.errstate(all="ignore"):
        for lines in (0, 1):
            n0, n1 = (kf0.n_ls, kf1.n_ls) if lines else (kf0.n_pt, kf1.n_pt)
            if n0 < 2 or n1 < 2:
                out.append(_NONE)
                continue
            q, t_ = (kf0.ldesc, kf1.ldesc) if lines else (kf0.pdesc, kf1.pdesc)
            i12, d12 = _knn(cache, (lines, 12), q, t_, rules)
            i21, _ = _knn(cache, (lines, 21), t_, q, rules)
            t, ok = _desc_test(lines, i12, d12, i21, cfg, rules, _mad_th(d12, cfg, rules) if lines else None)
            s2 = kf0.sigma2_ls if lines else kf0.sigma2_pt
            s = s2 if rules.sigma_not_sqrt else np.sqrt(s2)
            if not lines:
                uv = _project(cam, _se3(DT, kf0.P))
                ex, ey = uv[:, 0] - kf1.pl[t, 0], uv[:, 1] - kf1.pl[t, 1]
                err = np.sqrt(ex * ex + ey * ey) * s
            else:
                su, eu, l = _project(cam, _se3(DT, kf0.sP)), _project(cam, _se3(DT, kf0.eP)), kf0.le
                e0 = (l[:, 0] * su[:, 0] + l[:, 1] * su[:, 1]) + l[:, 2]
                e1 = (l[:, 0] * eu[:, 0] + l[:, 1] * eu[:, 1]) + l[:, 2]
                err = np.sqrt(e0 * e0 + e1 * e1) * s
            mg(err[ok], CHI)
            out.append(_compact(t, ok & lt(err, CHI), rules))
    return Res(out[0], out[1], mg.v)


def local_map_matches(cam, cfg, mp, kf1, ep_p=1.0, ep_l=1.0, rules=EXACT, cache=None):
    """lookForCommonMatches, local-map stage: the accepted (caller's map row, kf1 row) pairs."""
    mg = _Margin()
    Twf = inverse_se3(kf1.T)
    lt = (lambda a, b: a <= b) if rules.epip_le else (lambda a, b: a < b)

    def inside(X):
        Pf = _se3(Twf, X)
        pf = _project(cam, Pf)
        lo = (pf >= 0).all(1) if rules.border_incl_lo else (pf > 0).all(1)
        hi = ((pf[:, 0] <= cam.width) & (pf[:, 1] <= cam.height) if rules.border_incl_hi else
              (pf[:, 0] < cam.width) & (pf[:, 1] < cam.height))
        for c, size in ((0, cam.width), (1, cam.height)):
            mg(pf[:, c], 0.0, size)
            mg(pf[:, c], float(size))
        mg(Pf[:, 2], 0.0, 1.0)
        return lo & hi & (True if rules.no_z_test else Pf[:, 2] > 0.0)

    out = []
    with np.errstate(all="ignore"):
        for lines in (0, 1):
            n0, n1 = (len(mp.ldesc), kf1.n_ls) if lines else (len(mp.pdesc), kf1.n_pt)
            if n0 < 2 or n1 < 2:      # (the ABI launches nothing for such a kind)
                out.append(_NONE)
                continue
            if lines:
                a, b = inside(mp.L[:, :3]), inside(mp.L[:, 3:])
                loc = np.flatnonzero((a | b) if rules.one_endpoint else (a & b))
            else:
                loc = np.flatnonzero(inside(mp.P))
            if len(loc) < 2:          # ledger U4 on the selected rows
                out.append(_NONE)
                continue
            qa, t_ = (mp.ldesc, kf1.ldesc) if lines else (mp.pdesc, kf1.pdesc)
            h = hash(loc.tobytes())
            i12, d12 = _knn(cache, (lines, 12, h), qa[loc], t_, rules)
            i21, _ = _knn(cache, (lines, 21, h), t_, qa[loc], rules)
            th = None
            if lines:
                th = _mad_th(_knn(cache, (lines, 12, "all"), qa, t_, rules)[1] if rules.mad_over_all_rows else d12,
                          cfg, rules)
            t, ok = _desc_test(lines, i12, d12, i21, cfg, rules, th)
            if not lines:
                Pf = _se3(Twf, mp.P[loc])
                pf = _project(cam, Pf)
                ex, ey = pf[:, 0] - kf1.pl[t, 0], pf[:, 1] - kf1.pl[t, 1]
                err = np.sqrt(ex * ex + ey * ey)
                z = np.ones(len(loc), bool) if rules.no_z_test else Pf[:, 2] > 0.0
                mg(err[ok & z], ep_p)
                geo = z & lt(err, ep_p)
            else:
                sc, ec = _se3(Twf, mp.L[loc, :3]), _se3(Twf, mp.L[loc, 3:])
                su, eu, l = _project(cam, sc), _project(cam, ec), kf1.le[t]
                e0 = (l[:, 0] * su[:, 0] + l[:, 1] * su[:, 1]) + l[:, 2]
                e1 = (l[:, 0] * eu[:, 0] + l[:, 1] * eu[:, 1]) + l[:, 2]
                z = np.ones(len(loc), bool) if rules.no_z_test else (sc[:, 2] > 0.0) & (ec[:, 2] > 0.0)
                if rules.line_abs:
                    e0, e1 = np.abs(e0), np.abs(e1)
                mg(e0[ok & z], ep_l)
                mg(e1[ok & z], ep_l)
                geo = z & lt(e0, ep_l) & lt(e1, ep_l)
            out.append(_compact(t, ok & geo, rules, loc))
    return Res(out[0], out[1], mg.v)


# ------------------------------------------------------------------------------------ containers --
CAMERAS = {"vga": ("vga", {}), "kitti": ("kitti", {}),
           "exact": ("vga", dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)),      # projections of Z = 2^k are exact
           "corner": ("vga", dict(fx=512.0, fy=512.0, cx=0.0, cy=0.0))}        # (X, Y, 512) projects to (X, Y)
CONFIGS = {"default": {}, "r08": dict(max_ratio_12_p=0.8), "r05": dict(max_ratio_12_p=0.5)}
_MEMO = {}


def config(name):
    if ("cfg", name) not in _MEMO:
        _MEMO["cfg", name] = gfpl.default_config(**CONFIGS[name])
    return _MEMO["cfg", name]


def camera(name):
    if ("cam", name) not in _MEMO:
        base, over = CAMERAS[name]
        _MEMO["cam", name] = gfpl.make_camera(base, gfpl.default_config(), **over)
    return _MEMO["cam", name]


class KF:
    """one keyframe's rows: a FrameHost (what KeyFrameView reads) and T_kf_w"""

    def __init__(self, n_pt, n_ls, T=None):
        self.fh = gfpl.FrameHost(max(n_pt, 2), max(n_ls, 2))
        self.fh.s.n_pt, self.fh.s.n_ls = n_pt, n_ls
        self.n_pt, self.n_ls = n_pt, n_ls
        self.T = np.eye(4) if T is None else np.asarray(T, np.float64)
        self.fh.arr["pt_sigma2"][:] = 1.0
        self.fh.arr["ls_sigma2"][:] = 1.0

    def view(self, device=None):
        return gfpl.KeyFrameView(self.fh, self.T, device)


for _a, _f, _pt in (("pdesc", "pdesc", 1), ("P", "pt_P", 1), ("pl", "pt_pl", 1), ("sigma2_pt", "pt_sigma2", 1),
                    ("ldesc", "ldesc", 0), ("sP", "ls_sP", 0), ("eP", "ls_eP", 0), ("le", "ls_le", 0),
                    ("sigma2_ls", "ls_sigma2", 0)):
    setattr(KF, _a, property(lambda s, f=_f, pt=_pt: s.fh.arr[f][:s.n_pt if pt else s.n_ls]))


class Map:
    def __init__(self, n_pt, n_ls):
        self.pdesc, self.P = np.zeros((n_pt, 32), np.uint8), np.zeros((n_pt, 3))
        self.ldesc, self.L = np.zeros((n_ls, 32), np.uint8), np.zeros((n_ls, 6))

    def view(self, device=None):
        return gfpl.MapView(self.pdesc, self.P, self.ldesc, self.L, device=device)


class Case:
    def __init__(self, family, name, stage, cam, a, k1, cfg="default", ep=(1.0, 1.0), statement=True, exact=False,
                 facts=None):
        self.family, self.name, self.stage, self.cam, self.cfg = family, name, stage, cam, cfg
        self.a, self.k1, self.ep, self.statement, self.exact = a, k1, ep, statement, exact
        self.facts = facts or {}
        self._cache = {}

    @property
    def n0(self):
        return (self.a.n_pt, self.a.n_ls) if self.stage == "common" else (len(self.a.pdesc), len(self.a.ldesc))

    def expected(self, rules=EXACT):
        if self.stage == "common":
            return common_matches(camera(self.cam), config(self.cfg), self.a, self.k1, rules, self._cache)
        return local_map_matches(camera(self.cam), config(self.cfg), self.a, self.k1, self.ep[0], self.ep[1], rules,
                                 self._cache)

    def oracle(self, O):
        if self.stage == "common":
            return O.kf_common_matches(camera(self.cam), config(self.cfg), self.a.view(), self.k1.view())
        return O.kf_local_map_matches(camera(self.cam), config(self.cfg), self.a.view(), self.k1.view(), *self.ep)

    def gpu(self, ctx):
        if self.stage == "common":
            return ctx.lookForCommonMatches(self.a.view("cuda"), self.k1.view("cuda"))
        return ctx.lookForLocalMapMatches(self.a.view("cuda"), self.k1.view("cuda"), *self.ep)

    def descs(self, lines):
        """(query rows, train rows) of the 12 direction, before any filter"""
        return (self.a.ldesc, self.k1.ldesc) if lines else (self.a.pdesc, self.k1.pdesc)

    def what(self):
        return f"{self.family}/{self.name} [{self.stage}] rows {self.n0} x {(self.k1.n_pt, self.k1.n_ls)}"


# -------------------------------------------------------------------------------------- builders --
def _pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _inv(T):
    o = np.eye(4)
    o[:3, :3] = T[:3, :3].T
    o[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return o


def _uv(cam, P):
    return np.array([cam.cx + (cam.fx * P[0]) / P[2], cam.cy + (cam.fy * P[1]) / P[2]])


def _flipped(d, bits):
    d = d.copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (int(b) % 8))
    return d


def _line_eq(su, eu):
    le = np.cross([su[0], su[1], 1.0], [eu[0], eu[1], 1.0])
    return le / np.hypot(le[0], le[1])


BOUNDS = (32, 128, 1024, 2048)
T_A = _pose(0.01, -0.02, 0.015, [0.1, -0.05, 0.2])
T_B = _pose(0.03, 0.01, -0.01, [0.35, -0.02, 0.08])     # inverse(T_B) T_A: about 2 degrees and 0.3 m
T_M = _pose(0.02, -0.01, 0.03, [0.4, -0.1, 0.3])


def _rejected(r):
    """rows whose planted geometry fails its gate: every eleventh, and rows b - 2 and b of each boundary b,
    so that rows b - 2 .. b + 1 alternate"""
    return r % 11 == 5 or any(r in (b - 2, b) for b in BOUNDS)


def _out_of_view(r):
    return r % 97 == 3 or r in (1021, 1023)


def planted_common(cam_name, n_pt, n_ls, seed, T0=T_A, T1=T_A, flips=8):
    """kf0 row i < min(n0, n1) has its partner (8 flipped bits) at a random kf1 row; the partner's observation
    is 0.3 px off (accepted) or 12 px / 6 px off (_rejected rows).  n_pt, n_ls: (n0, n1)."""
    cam, rng = camera(cam_name), np.random.default_rng(seed)
    k0, k1 = KF(n_pt[0], n_ls[0], T0), KF(n_pt[1], n_ls[1], T1)
    DT = _inv(T1) @ T0
    for lines, (n0, n1) in enumerate((n_pt, n_ls)):
        d0, d1 = (k0.ldesc, k1.ldesc) if lines else (k0.pdesc, k1.pdesc)
        d0[:] = rng.integers(0, 256, (n0, 32), dtype=np.uint8)
        d1[:] = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
        perm = rng.permutation(n1)
        X = np.stack([rng.uniform(-2, 2, n0), rng.uniform(-1.5, 1.5, n0), rng.uniform(2, 8, n0)], 1)
        if not lines:
            k0.P[:] = X
            k0.sigma2_pt[:] = 1.0 / 1.44 ** rng.integers(1, 4, n0)
            k1.pl[:] = rng.uniform(20, 400, (n1, 2))
        else:
            E = X + rng.uniform(-0.8, 0.8, (n0, 3))
            E[:, 2] = np.maximum(E[:, 2], 1.5)
            k0.sP[:], k0.eP[:] = X, E
        for i in range(n0):
            if i < n1:
                d1[perm[i]] = _flipped(d0[i], rng.choice(256, flips, replace=False))
            if not lines:
                if i < n1:
                    off = 12.0 if _rejected(i) else 0.3
                    k1.pl[perm[i]] = _uv(cam, DT[:3, :3] @ X[i] + DT[:3, 3]) + np.array([off, -0.3 * off])
            else:
                le = _line_eq(_uv(cam, DT[:3, :3] @ X[i] + DT[:3, 3]), _uv(cam, DT[:3, :3] @ E[i] + DT[:3, 3]))
                le[2] += 6.0 if _rejected(i) else 0.3
                k0.le[i] = le
    return k0, k1


def planted_map(cam_name, n_pt, n_ls, seed, T1=T_M, flips=8):
    """a local map seen from kf1: _out_of_view rows project far to the right, _rejected rows are observed
    4 px (points) / +5 (lines) off, every 13th line -5 off, which the signed test accepts"""
    cam, rng = camera(cam_name), np.random.default_rng(seed)
    mp, k1 = Map(n_pt[0], n_ls[0]), KF(n_pt[1], n_ls[1], T1)

    def world(pc):
        return T1[:3, :3] @ pc + T1[:3, 3]

    for lines, (n0, n1) in enumerate((n_pt, n_ls)):
        d0, d1 = (mp.ldesc, k1.ldesc) if lines else (mp.pdesc, k1.pdesc)
        d0[:] = rng.integers(0, 256, (n0, 32), dtype=np.uint8)
        d1[:] = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
        perm = rng.permutation(n1)
        if not lines:
            k1.pl[:] = rng.uniform(20, 400, (n1, 2))
        else:
            k1.le[:] = np.array([0.0, 1.0, -100.0])
        for i in range(n0):
            # (both endpoints inside every camera's image: |X / Z| < 0.48, |Y / Z| < 0.19)
            rx, ry, z = rng.uniform(-0.4, 0.4), rng.uniform(-0.15, 0.15), rng.uniform(2, 8)
            sc = np.array([rx * z, ry * z, z])
            z = z + rng.uniform(-0.5, 0.5)
            ec = np.array([(rx + rng.uniform(-0.08, 0.08)) * z, (ry + rng.uniform(-0.04, 0.04)) * z, z])
            su, eu = _uv(cam, sc), _uv(cam, ec)
            if _out_of_view(i):
                (ec if lines else sc)[0] = (ec if lines else sc)[2] * 3.0
            if i < n1:
                d1[perm[i]] = _flipped(d0[i], rng.choice(256, flips, replace=False))
            if not lines:
                mp.P[i] = world(sc)
                if i < n1:
                    k1.pl[perm[i]] = su + np.array([4.0 if _rejected(i) else 0.3, 0.0])
            else:
                mp.L[i] = np.concatenate([world(sc), world(ec)])
                if i < n1:
                    le = _line_eq(su, eu)
                    le[2] += 5.0 if _rejected(i) else (-5.0 if i % 13 == 7 else 0.3)
                    k1.le[perm[i]] = le
    return mp, k1


class Descs:
    """descriptor rows with chosen Hamming distances: a group is one random row on one side and rows at the
    given distances from it on the other (row k flips bits perm[k : k + d]: equal distances are distinct rows,
    distance 0 a duplicate); fillers are random rows (about 128 from everything)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.q, self.t = [], []
        self.want = []           # (query side 'q' / 't', row, (d0, d1) or d0)

    def base(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def _group(self, one, many, dists):
        b, perm = self.base(), self.rng.permutation(256)
        one.append(b)
        i0 = len(many)
        for k, d in enumerate(dists):
            many.append(_flipped(b, perm[k:k + d]))
        return len(one) - 1, list(range(i0, i0 + len(dists)))

    def group(self, *dists):
        """one kf0 row, kf1 rows at `dists` from it -> (q row, [t rows])"""
        return self._group(self.q, self.t, dists)

    def rgroup(self, *dists):
        """one kf1 row, kf0 rows at `dists` from it -> (t row, [q rows])"""
        return self._group(self.t, self.q, dists)

    def fill(self, side, upto):
        side = self.q if side == "q" else self.t
        while len(side) < upto:
            side.append(self.base())

    def arrays(self):
        return np.array(self.q, np.uint8).reshape(-1, 32), np.array(self.t, np.uint8).reshape(-1, 32)


def desc_case(family, name, pt, ls, stage="common", cfg="default", out_pt=(), out_ls=(), facts=None):
    """a case decided by its descriptors alone (pt, ls: (kf0 rows, kf1 rows) or None): exact camera, identity
    poses, every feature on one spot with error 0; out_*: map rows put behind the camera"""
    (qp, tp), (ql, tl) = [x if x is not None else (np.zeros((0, 32), np.uint8),) * 2 for x in (pt, ls)]
    k1 = KF(len(tp), len(tl))
    k1.pdesc[:], k1.ldesc[:] = tp, tl
    k1.pl[:] = (320.0, 240.0)
    k1.le[:] = (0.0, 1.0, -240.0)
    if stage == "common":
        a = KF(len(qp), len(ql))
        a.pdesc[:], a.ldesc[:] = qp, ql
        a.P[:] = (0.0, 0.0, 4.0)
        a.sP[:], a.eP[:], a.le[:] = (-0.5, 0.0, 4.0), (0.5, 0.0, 4.0), (0.0, 1.0, -240.0)
    else:
        a = Map(len(qp), len(ql))
        a.pdesc[:], a.ldesc[:] = qp, ql
        a.P[:] = (0.0, 0.0, 4.0)
        a.L[:] = (-0.5, 0.0, 4.0, 0.5, 0.0, 4.0)
        for r in out_pt:
            a.P[r, 2] = -4.0
        for r in out_ls:
            a.L[r, 2] = -4.0
    return Case(family, name, stage, "exact", a, k1, cfg=cfg, facts=facts)


# -------------------------------------------------------------------------------------- families --
SIZES = (2, 3, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 2049)
SIZE_PAIRS = [(n, n) for n in SIZES] + [(2, 1025), (1025, 2), (129, 33), (33, 129), (1024, 1025)]
# fewer than two rows on a side: ((pt n0, n1), (ls n0, n1))
FEW = [((0, 5), (20, 20)), ((5, 0), (20, 20)), ((1, 7), (20, 20)), ((7, 1), (20, 20)), ((20, 20), (0, 5)),
       ((20, 20), (5, 0)), ((20, 20), (1, 7)), ((20, 20), (7, 1)), ((1, 5), (5, 1)), ((0, 0), (0, 0)), ((1, 1), (0, 2))]


def _sizes():
    out = []
    for k, (n0, n1) in enumerate(SIZE_PAIRS):
        out.append(Case("sizes", f"{n0}x{n1}", "common", "vga", *planted_common("vga", (n0, n1), (n0, n1), 100 + k)))
        out.append(Case("sizes", f"{n0}x{n1}", "map", "vga", *planted_map("vga", (n0, n1), (n0, n1), 200 + k)))
    for k, (pt, ls) in enumerate(FEW):
        out.append(Case("few", f"{pt}{ls}", "common", "vga", *planted_common("vga", pt, ls, 300 + k)))
        out.append(Case("few", f"{pt}{ls}", "map", "vga", *planted_map("vga", pt, ls, 320 + k)))
    # map counts whose COMPACTED count sits on a boundary
    for k, target in enumerate((32, 33, 128, 129, 1024, 1025)):
        n0 = target
        while sum(not _out_of_view(r) for r in range(n0)) < target:
            n0 += 1
        out.append(Case("sizes", f"compacted{target}", "map", "vga", *planted_map("vga", (n0, target), (n0, target), 340 + k),
                        facts={"compacted": target}))
    return out


def _tie_descs(seed, big):
    """ties in both directions, at train rows (3, 4) — the two lane halves of a tile —, (31, 32) and, big,
    (1023, 1024); -> Descs and the facts"""
    D = Descs(seed)
    f = {"first12": [], "first21": [], "second12": [], "dup_t": [], "dup_q": [], "closer": None}
    spots = [3, 31] + ([1023] if big else [])
    for s in spots:
        D.fill("t", s)
        f["first12"].append(D.group(10, 10))        # q: d0 = d1 = 10 at train rows s, s + 1: ratio 1, difference 0
    D.fill("t", len(D.t) + 5)
    for s in spots:
        D.fill("q", s)
        f["first21"].append(D.rgroup(10, 10))       # t's best is kf0 row s (not s + 1): only s is mutual
    f["second12"].append(D.group(5, 10, 10))        # the second neighbour is tied
    f["second12"].append(D.group(10, 10, 5))        # the best comes last, the tie is for the second
    f["second21"] = [D.rgroup(5, 10, 10), D.rgroup(10, 5, 10)]
    f["dup_t"].append(D.group(8, 8)[0])             # (equal distances, distinct rows)
    f["dup_t"].append(D.group(0, 0)[0])             # duplicates of q itself: 0 / 0
    f["zero"] = D.group(0, 7)[0]                    # ratio 0: accepted
    f["dup_q"].append(D.rgroup(0, 0))               # duplicate kf0 rows: only the lower one is mutual
    f["dup_q"].append(D.rgroup(6, 6))
    t, qs = D.rgroup(12, 6)                         # kf0 row qs[0] prefers t, t prefers qs[1]
    f["closer"] = (t, qs)
    for _ in range(12):
        D.group(8)                                  # ordinary pairs
    n = max(len(D.q), len(D.t)) + 3
    D.fill("q", n)
    D.fill("t", n + 2)
    return D, f


def _ties():
    out = []
    for big in (False, True):
        (Dp, fp), (Dl, fl) = _tie_descs(400 + big, big), _tie_descs(410 + big, big)
        for stage in ("common", "map"):
            out.append(desc_case("ties", "big" if big else "small", Dp.arrays(), Dl.arrays(), stage,
                                 facts={"pt": fp, "ls": fl, "knn": True}))
    # nt = 2, and a tie between the only two train rows
    D = Descs(420)
    D.group(10, 10)
    D.rgroup(10, 10)
    D.group(4)
    for stage in ("common", "map"):
        out.append(desc_case("ties", "two", D.arrays(), D.arrays(), stage, facts={"knn": True}))
    D = Descs(421)
    D.group(3, 9)
    D.fill("q", 5)
    out.append(desc_case("ties", "nt2", D.arrays(), D.arrays(), "common", facts={"knn": True}))
    return out


def _tiny_ratio(d0, d1, seed):
    """kf0 = [q, ~q], kf1 = [q ^ d0 bits, q ^ d1 bits]: q has the distances (d0, d1) whatever they are"""
    rng = np.random.default_rng(seed)
    q, perm = rng.integers(0, 256, 32, dtype=np.uint8), rng.permutation(256)
    return np.stack([q, ~q]), np.stack([_flipped(q, perm[:d0]), _flipped(q, perm[:d1])])


RATIOS = [("default", 9, 10, True), ("default", 45, 50, True), ("default", 91, 100, False), ("default", 0, 7, True),
          ("default", 0, 0, False), ("r08", 4, 5, False), ("r08", 8, 10, False), ("r08", 100, 125, False),
          ("r08", 79, 99, True), ("r05", 5, 10, True), ("r05", 64, 128, True), ("r05", 51, 100, False)]


def _ratio():
    out = []
    for k, (cfg, d0, d1, acc) in enumerate(RATIOS):
        for stage in ("common", "map"):
            out.append(desc_case("ratio", f"{d0}/{d1}@{cfg}", _tiny_ratio(d0, d1, 500 + k), None, stage, cfg=cfg,
                                 facts={"accept": acc}))
    for cfg, groups in (("default", [(9, 10), (45, 50), (46, 50), (10, 10), (0, 7)]), ("r08", [(4, 5), (8, 10), (7, 9), (39, 50)]),
                        ("r05", [(5, 10), (1, 2), (6, 11)])):
        D = Descs(520)
        rows = {g: D.group(*g)[0] for g in groups}
        for _ in range(6):
            D.group(8)
        out.append(desc_case("ratio", f"groups@{cfg}", D.arrays(), None, "common", cfg=cfg, facts={"rows": rows}))
    return out


def _mad_descs(seed, diffs, d0=10):
    D = Descs(seed)
    for d in diffs:
        D.group(d0, d0 + d)
    return D


MADS = {"zero": [0, 0, 0, 0, 1, 1, 1],            # median 0: threshold 0, 0 rejected and 1 accepted
        "even": [2, 2, 2, 30, 30, 30],            # n // 2 -> 30 (2 rejected), (n - 1) // 2 -> 2 (all accepted)
        "odd": [2, 2, 2, 30, 30, 30, 30],
        "two": [3, 40],
        "m20": [2, 2, 3, 20, 25, 30, 35],         # 1.4826 * 20 * 0.1 = 2.9652: 2 rejected, 3 accepted
        "m20even": [2, 3, 3, 19, 20, 25, 30, 35]}


def _mad():
    out = []
    for k, (name, diffs) in enumerate(MADS.items()):
        D = _mad_descs(600 + k, diffs)
        for stage in ("common", "map"):
            out.append(desc_case("mad", name, None, D.arrays(), stage, facts={"diffs": diffs}))
    # one difference of 256: all-zero against all-one rows (the last histogram bin)
    z, o = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    h = z.copy()
    h[:16] = 255
    for stage in ("common", "map"):
        out.append(desc_case("mad", "d256", None, (np.stack([z, o, h]), np.stack([z, o])), stage, facts={"diffs": [256, 256, 0]}))
    # local map: the filtered-out rows (difference 0) would move the median from 30 to 0
    D = _mad_descs(620, [2, 30, 30, 30, 0, 0, 0, 0, 0])
    out.append(desc_case("mad", "filtered", None, D.arrays(), "map", out_ls=range(4, 9), facts={"diffs": [2, 30, 30, 30]}))
    return out


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _solve(f, guess, target):
    """the double x near guess with f(x) == target, f nondecreasing (bisection over the doubles); None if the
    rounding of f steps over target"""
    lo, hi = _bits(guess) - (1 << 24), _bits(guess) + (1 << 24)
    while lo < hi:
        mid = (lo + hi) // 2
        if f(float(np.int64(mid).view(np.float64))) < target:
            lo = mid + 1
        else:
            hi = mid
    x = float(np.int64(lo).view(np.float64))
    return x if f(x) == target else None


CHI_NEIGHBOURS = (("below", float(np.nextafter(CHI, 0.0)), True), ("at", CHI, False),
                  ("above", float(np.nextafter(CHI, 4.0)), False))
# residuals whose norm is exact: (3, 0), (3, 4), and 1.5 * (3, 4) in case the products by 5 step over a target
CHI_POINTS = ((3.0, 0.0), (3.0, 4.0), (4.5, 6.0))
CHI_LINES = ((1.125, 1.5), (0.75, 1.0), (1.5, 0.0))


def _chi():
    """common stage, exact camera, identity poses: err = |(ex, ey)| * sqrt(sigma2) lands on the double below
    sqrt(7.815), on it and above it, sigma2 found by stepping through the doubles"""
    rng = np.random.default_rng(700)
    pts, lns = [], []
    for res, store in ((CHI_POINTS, pts), (CHI_LINES, lns)):
        for ex, ey in res:
            hyp = math.sqrt(ex * ex + ey * ey)
            s2 = [_solve(lambda s: hyp * math.sqrt(s), (CHI / hyp) ** 2, tgt) for _, tgt, _ in CHI_NEIGHBOURS]
            if None not in s2:
                store += [(ex, ey, s, name, acc) for s, (name, _, acc) in zip(s2, CHI_NEIGHBOURS)]
    n_pt, n_ls = len(pts) + 3, len(lns) + 3
    k0, k1 = KF(n_pt, n_ls), KF(n_pt, n_ls)
    facts = {"pt": {}, "ls": {}}
    for lines, n in enumerate((n_pt, n_ls)):
        d0, d1 = (k0.ldesc, k1.ldesc) if lines else (k0.pdesc, k1.pdesc)
        d0[:] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        for i in range(n):
            d1[n - 1 - i] = _flipped(d0[i], rng.choice(256, 8, replace=False))
    k0.P[:] = (0.0, 0.0, 4.0)
    k1.pl[:] = (320.0, 240.0)
    for i, (ex, ey, s, name, acc) in enumerate(pts):
        k1.pl[n_pt - 1 - i] = (320.0 - ex, 240.0 - ey)
        k0.sigma2_pt[i] = s
        facts["pt"][i] = (ex, ey, s, name, acc)
    # lines: le = (0, 1, c), the start point projects to v = 0 and the end point to v = e1 - e0
    k0.sP[:], k0.eP[:], k0.le[:] = (-0.5, 0.0, 4.0), (0.5, 0.0, 4.0), (0.0, 1.0, -240.0)
    for i, (e0, e1, s, name, acc) in enumerate(lns):
        k0.sP[i] = (-0.5, (0.0 - 240.0) / 128.0, 4.0)
        k0.eP[i] = (0.5, ((e1 - e0) - 240.0) / 128.0, 4.0)
        k0.le[i] = (0.0, 1.0, e0)
        k0.sigma2_ls[i] = s
        facts["ls"][i] = (e0, e1, s, name, acc)
    return [Case("chi", "neighbours", "common", "exact", k0, k1, exact=True, facts=facts)]


# point residuals (ex, ey) and the line's le[2]: both endpoints project to v = 8, so its residuals are 8 + le[2]
EPIP = (((3.0, 4.0), -7.25), ((320.0 - 319.7, 240.0 - 239.6), -7.3))
V8 = (8.0 - 240.0) / 128.0     # Y of a point at Z = 4 that projects to v = 8


def _epip():
    """local-map gates, exact camera, identity pose: max_kf_epip_p / _l equal to a row's own error (rejected)
    and the next double above it (accepted); signed line residuals"""
    out = []
    for k, ((ex, ey), l2) in enumerate(EPIP):
        e, c = math.sqrt(ex * ex + ey * ey), 8.0 + l2
        for name, ep in (("at", (e, c)), ("above", (float(np.nextafter(e, 9.0)), float(np.nextafter(c, 9.0))))):
            rng = np.random.default_rng(720 + k)
            n = 5
            mp, k1 = Map(n, n), KF(n, n)
            mp.pdesc[:] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            mp.ldesc[:] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            for i in range(n):
                k1.pdesc[n - 1 - i] = _flipped(mp.pdesc[i], rng.choice(256, 8, replace=False))
                k1.ldesc[n - 1 - i] = _flipped(mp.ldesc[i], rng.choice(256, 8, replace=False))
            mp.P[:] = (0.0, 0.0, 4.0)
            k1.pl[:] = (320.0, 240.0)
            k1.pl[n - 1 - 1] = (320.0 - ex, 240.0 - ey)            # map row 1: error e
            mp.L[:] = (-0.5, V8, 4.0, 0.5, V8, 4.0)                 # both endpoints at v = 8
            k1.le[:] = (0.0, 1.0, -8.0)
            k1.le[n - 1 - 1] = (0.0, 1.0, l2)                      # map row 1: residuals (c, c)
            k1.le[n - 1 - 2] = (0.0, 1.0, -13.0)                   # map row 2: (-5, -5), accepted (signed)
            out.append(Case("epip", f"{name}{k}", "map", "exact", mp, k1, ep=ep, exact=True,
                            facts={"e": e, "c": c, "accept": name == "above"}))
    # (-5, -5) accepted, (-5, +ep_l) rejected at the default ep_l = 1
    rng = np.random.default_rng(730)
    n = 4
    mp, k1 = Map(2, n), KF(2, n)
    mp.ldesc[:] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    k1.ldesc[:] = [_flipped(d, rng.choice(256, 8, replace=False)) for d in mp.ldesc]
    mp.L[:] = (-0.5, V8, 4.0, 0.5, V8, 4.0)
    mp.L[1, 3:] = (0.5, (14.0 - 240.0) / 128.0, 4.0)               # end point at v = 14
    k1.le[:] = (0.0, 1.0, -8.0)
    k1.le[0] = (0.0, 1.0, -13.0)                                   # (-5, -5)
    k1.le[1] = (0.0, 1.0, -13.0)                                   # (-5, +1)
    out.append(Case("epip", "signed", "map", "exact", mp, k1, exact=True, facts={"ls": [(0, 0), (2, 2), (3, 3)]}))
    return out


def _border_case(name, cam, pts, lns, seed):
    """pts: (P, inside); lns: (sP, eP, inside): each row's kf1 partner observes it exactly (error 0), so a row
    is paired exactly when the filter lets it through; two anchors per kind come first"""
    rng = np.random.default_rng(seed)
    c = camera(cam)
    anchor = (1.0, 1.0, 512.0) if cam == "corner" else (0.0, 0.0, 4.0)
    anchor2 = (3.0, 2.0, 512.0) if cam == "corner" else (0.25, 0.25, 4.0)
    pts = [(anchor, True), (anchor2, True)] + list(pts)
    lns = [(anchor, anchor2, True), (anchor2, anchor, True)] + list(lns)
    mp, k1 = Map(len(pts), len(lns)), KF(len(pts), len(lns))
    mp.pdesc[:] = rng.integers(0, 256, (len(pts), 32), dtype=np.uint8)
    mp.ldesc[:] = rng.integers(0, 256, (len(lns), 32), dtype=np.uint8)
    k1.pdesc[:] = [_flipped(d, rng.choice(256, 8, replace=False)) for d in mp.pdesc]
    k1.ldesc[:] = [_flipped(d, rng.choice(256, 8, replace=False)) for d in mp.ldesc]
    with np.errstate(all="ignore"):
        for i, (P, _) in enumerate(pts):
            mp.P[i] = P
            uv = _uv(c, np.array(P, np.float64))
            k1.pl[i] = uv if np.isfinite(uv).all() else (0.0, 0.0)
        for i, (s, e, _) in enumerate(lns):
            mp.L[i] = tuple(s) + tuple(e)
            su, eu = _uv(c, np.array(s, np.float64)), _uv(c, np.array(e, np.float64))
            k1.le[i] = _line_eq(su, eu) if np.isfinite(su).all() and np.isfinite(eu).all() else (0.0, 1.0, 0.0)
    return Case("border", name, "map", cam, mp, k1, exact=True,
                facts={"pt": [i for i, p in enumerate(pts) if p[1]], "ls": [i for i, l in enumerate(lns) if l[2]]})


TINY = 5e-324


def _border():
    out = []
    # exact camera: u = 320 + 128 X, v = 240 + 128 Y at Z = 4
    pts = [((-2.5, 0.0, 4.0), False), ((2.5, 0.0, 4.0), False), ((0.0, -1.875, 4.0), False), ((0.0, 1.875, 4.0), False),
           ((-2.4921875, 0.0, 4.0), True), ((0.5, 0.5, -4.0), False), ((0.0, 0.0, 0.0), False), ((1.0, 1.0, 0.0), False),
           ((0.0, 0.0, TINY), True), ((0.5, 0.25, -TINY), False)]
    ins = (0.5, 0.5, 4.0)
    lns = [((-2.5, 0.0, 4.0), ins, False), (ins, (2.5, 0.0, 4.0), False), (ins, (0.0, 1.875, 4.0), False),
           (ins, (0.5, 0.25, -4.0), False), ((1.0, 0.5, 0.0), ins, False), ((-2.4921875, 0.0, 4.0), ins, True)]
    out.append(_border_case("exact", "exact", pts, lns, 800))
    # corner camera: (X, Y, 512) projects to (X, Y) exactly
    w1, h1 = float(np.nextafter(640.0, 0.0)), float(np.nextafter(480.0, 0.0))
    pts = [((TINY, 1.0, 512.0), True), ((1.0, TINY, 512.0), True), ((w1, 1.0, 512.0), True), ((1.0, h1, 512.0), True),
           ((640.0, 1.0, 512.0), False), ((1.0, 480.0, 512.0), False), ((0.0, 1.0, 512.0), False), ((1.0, 0.0, 512.0), False),
           ((w1, h1, 512.0), True), ((-TINY, 1.0, 512.0), False)]
    ins = (5.0, 7.0, 512.0)
    lns = [((TINY, 1.0, 512.0), ins, True), (ins, (w1, h1, 512.0), True), ((0.0, 1.0, 512.0), ins, False),
           (ins, (640.0, 9.0, 512.0), False), (ins, (9.0, 480.0, 512.0), False)]
    out.append(_border_case("corner", "corner", pts, lns, 801))
    # 0, 1 and 2 survivors, first or last map rows (ledger U4 on the selected rows)
    for k in (0, 1, 2):
        for last in ((False,) if k == 0 else (False, True)):
            n = 6
            keep = set(range(n - k, n)) if last else set(range(k))
            far = (40.0, 0.0, 4.0)
            P = [((0.1 * i, 0.1, 4.0) if i in keep else far, i in keep) for i in range(n)]
            L = [(((0.1 * i, 0.1, 4.0), (0.1 * i, 0.5, 4.0), True) if i in keep else (far, (0.0, 0.0, 4.0), False))
                 for i in range(n)]
            c = _border_case(f"keep{k}{'last' if last else 'first'}", "exact", P, L, 810 + k)
            # _border_case puts two anchors in front: take them out of view too
            c.a.P[:2] = far
            c.a.L[:2, :3] = far
            c.facts = {"pt": sorted(i + 2 for i in keep) if k == 2 else [], "ls": sorted(i + 2 for i in keep) if k == 2 else []}
            out.append(c)
    return out


def _wild():
    """compared with the oracle alone: non-finite and huge inputs, sigma2 < 0, z = 0 in the keyframe-pair stage"""
    out = []
    nan, inf = math.nan, math.inf
    vals = [nan, inf, -inf, 1e300, -1e300]
    for cam in ("vga", "exact"):
        T = (T_A, T_B) if cam == "vga" else (np.eye(4), np.eye(4))
        k0, k1 = planted_common(cam, (60, 60), (40, 40), 900, *T)
        for i, v in enumerate(vals):
            k0.P[i, i % 3] = v
            k0.P[5 + i] = v
            k1.pl[i + 10, i % 2] = v
            k0.sigma2_pt[20 + i] = v
            k0.sP[i, i % 3] = v
            k0.eP[5 + i] = v
            k0.le[10 + i, i % 3] = v
            k0.le[15 + i] = v
            k0.sigma2_ls[20 + i] = v
        k0.sigma2_pt[26:29] = (-1.0, -0.0, 0.0)
        k0.sigma2_ls[26:29] = (-1.0, -0.0, 0.0)
        k0.P[30], k0.P[31], k0.P[32] = (0.5, 0.2, 0.0), (0.0, 0.0, 0.0), (1e300, 1e300, 1e300)
        k0.sP[30], k0.eP[31], k0.sP[32] = (0.5, 0.2, 0.0), (0.0, 0.0, 0.0), (1e300, 1e300, 1e300)
        out.append(Case("wild", f"common_{cam}", "common", cam, k0, k1, statement=False))
        mp, k1 = planted_map(cam, (60, 60), (40, 40), 901, T[1] if cam == "vga" else np.eye(4))
        for i, v in enumerate(vals):
            mp.P[i, i % 3] = v
            mp.P[5 + i] = v
            k1.pl[i + 10, i % 2] = v
            mp.L[i, i % 6] = v
            mp.L[5 + i] = v
            k1.le[10 + i, i % 3] = v
            k1.le[15 + i] = v
        mp.P[30], mp.P[31] = (1e300, 1e300, 1e300), (0.0, 0.0, 0.0)
        mp.L[30], mp.L[31, 3:] = (1e300,) * 6, (0.0, 0.0, 0.0)
        out.append(Case("wild", f"map_{cam}", "map", cam, mp, k1, statement=False))
    return out


def _poses():
    out = []
    for k, n in enumerate((33, 1025)):
        out.append(Case("poses", f"dt{n}", "common", "vga", *planted_common("vga", (n, n), (n, n), 1000 + k, T_A, T_B)))
        out.append(Case("poses", f"dt{n}", "map", "vga", *planted_map("vga", (n, n), (n, n), 1010 + k, T_B)))
    out.append(Case("poses", "kitti129", "common", "kitti", *planted_common("kitti", (129, 129), (129, 129), 1020, T_A, T_B)))
    out.append(Case("poses", "kitti129", "map", "kitti", *planted_map("kitti", (129, 129), (129, 129), 1021, T_B)))
    return out


# (n_pt + n_ls) mod 4 = 0, 1, 2, 3; points only and lines only
ALIGN = [(200, 80), (201, 80), (202, 80), (33, 2), (203, 80), (201, 0), (0, 81), (2, 3), (1025, 34)]


def _align():
    return [Case("align", f"{a}+{b}", "map", "vga", *planted_map("vga", (a, a), (b, b), 1100 + k))
            for k, (a, b) in enumerate(ALIGN)]


FAMILIES = {"sizes": _sizes, "ties": _ties, "ratio": _ratio, "mad": _mad, "chi": _chi, "epip": _epip, "border": _border,
            "wild": _wild, "poses": _poses, "align": _align}


def cases(family=None):
    """every case (built once), or one family's (`few` travels with `sizes`)"""
    if family is None:
        return [c for f in FAMILIES for c in cases(f)]
    if ("cases", family) not in _MEMO:
        _MEMO["cases", family] = FAMILIES[family]()
    return _MEMO["cases", family]
