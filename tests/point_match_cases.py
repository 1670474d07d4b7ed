"""Hand-made keypoints, descriptors and pyramids for the in-kernel point matching (k_stereo_points,
k_init_points behind the batched knn-2, k_cross_points) and a plain numpy statement of the three
stages they are compared with.

Three parts, as in line_match_cases.py:
  * the statement: stereo_points / init_points / cross_points in integer, float32 and float64 numpy.
    It calls neither the library nor the oracle.  Every rule can be altered (`Rules`), one alteration
    per kernel fault, so a test can show that the families notice that fault;
  * the families, each aimed at one mechanism of the kernels, at the counts where it turns over;
  * the builders that put one case per sequence into a HostFrames / FrameHost pair and the decoders
    that read the result back (left keypoints have unique (x, y): pt_pl names iL).

Pyramids are written per level as textures periodic in x: both SAD windows come from the right
pyramid, so the SAD of a left window at column uL against the right window at uR + s is zero exactly
where uR + s = uL (mod period) and the sub-pixel result of a planted pair (uL - uR = period * m + k,
|k| <= 4) is scale * (period * m - deltaR): a candidate with another m gives another disparity.
"""
from collections import namedtuple

import numpy as np

import gfpl   # struct definitions and the synthetic frame container only
from line_match_cases import distances, _flip, _first_diff

# ------------------------------------------------------------------------------------- statement --
# The rules, and the kernel faults they can be altered into (test_families_are_sensitive):
#  band scan  ham_tie_high   equal Hamming distances go to the HIGHER iR
#             band_excl_min  a right keypoint is no candidate of the row minr / (band_excl_max) maxr
#             oct_gate0 / oct_gate2   the octave gate is +-0 / +-2 instead of +-1
#             oct_clamped    the gate compares the clamped octaves (the segment index) not the raw ones
#             u_strict_lo / u_strict_hi   uR > uL - maxD / uR < uL
#             le80           bestDist <= 80 starts a refinement
#  SAD        sad_tie_last   equal SADs go to the LAST shift
#             win_left / win_right / win_top / win_bottom   the window validity test is one pixel
#                            stricter on that side
#             row_twice      the centre row of the window is counted twice (quad lane 3's third row)
#  emission   median_lo      the median is element (nv - 1) / 2
#             emit_le        emission while dist <= thDist
#             unstable       equal distances are emitted in descending iL
#  initial    epip_lt / disp_gt   |dy| < max_dist_epip / disparity > min_disp
#  cross      cross_tie_high equal distances go to the HIGHER q
#             gate_ge        a projection AT the gate distance is rejected
#             radius_lt      a distance AT the radius is rejected
#             first_t        pl_obs of a q chosen by several t comes from the first t
#             beyond_cap     matches beyond max_point_match_num still write idx / pl_obs / inlier
_RULES = ("ham_tie_high band_excl_min band_excl_max oct_gate0 oct_gate2 oct_clamped u_strict_lo u_strict_hi le80 "
          "sad_tie_last win_left win_right win_top win_bottom row_twice median_lo emit_le unstable "
          "epip_lt disp_gt cross_tie_high gate_ge radius_lt first_t beyond_cap")
Rules = namedtuple("Rules", _RULES, defaults=(False,) * len(_RULES.split()))
EXACT = Rules()
ALTERATIONS = {n: Rules(**{n: True}) for n in _RULES.split()}


def hamming(q, t):
    """D[i, j]: set bits of q[i] ^ t[j] (line_match_cases.distances with cell 1; by 64-bit words where
    numpy counts bits itself)"""
    if not hasattr(np, "bitwise_count") or not len(q) or not len(t):
        return distances(q, t, 1)
    a, b = np.ascontiguousarray(q).view(np.uint64), np.ascontiguousarray(t).view(np.uint64)
    D = np.empty((len(q), len(t)), np.int64)
    for i0 in range(0, len(q), 256):
        D[i0:i0 + 256] = np.bitwise_count(a[i0:i0 + 256, None, :] ^ b[None, :, :]).sum(axis=2, dtype=np.int64)
    return D


class CamTab:
    """The camera tables as numpy scalars / arrays."""

    def __init__(self, cam):
        n = self.n = cam.n_levels
        self.cam = cam
        self.W, self.H = cam.width, cam.height
        self.scale = np.array(cam.scale[:n], np.float32)
        self.inv = np.array(cam.inv_scale[:n], np.float32)
        self.cols, self.rows = list(cam.lvl_cols[:n]), list(cam.lvl_rows[:n])
        self.off = list(cam.lvl_offset[:n])
        self.pyr_bytes = cam.pyr_bytes
        self.maxD = np.float32(cam.fx)
        self.mbf = np.float32(cam.fx * cam.b)
        self.fx, self.fy, self.cx, self.cy = cam.fx, cam.fy, cam.cx, cam.cy

    def level(self, pyr, o):
        return pyr[self.off[o]:self.off[o] + self.rows[o] * self.cols[o]].reshape(self.rows[o], self.cols[o])

    def clamp(self, o):
        return np.clip(o, 0, self.n - 1)


def roundf(v):
    """C's roundf (halves away from zero) of float32 values; exact in float64."""
    d = np.asarray(v, np.float64)
    return (np.sign(d) * np.floor(np.abs(d) + 0.5)).astype(np.float32)


def sad_vector(ct, pyr, o, vL, uL, uR, rules=EXACT):
    """The 11 integer SADs (shifts -5..5) of the centre-subtracted 11 x 11 windows at (vL, uL) and
    (vL, uR + s) of level o of the right pyramid."""
    img = ct.level(pyr, o)
    IL = img[vL - 5:vL + 6, uL - 5:uL + 6].astype(np.int64) - int(img[vL, uL])
    strip = img[vL - 5:vL + 6, uR - 10:uR + 11].astype(np.int64)
    out = np.empty(11, np.int64)
    for s in range(11):
        A = np.abs(IL - (strip[:, s:s + 11] - strip[5, s + 5]))
        out[s] = A.sum() + (A[5].sum() if rules.row_twice else 0)
    return out


def sub_pixel(ct, pyr, kpL, kpR, rules=EXACT):
    """The oracle's subPixel: (float32 disparity or None, detail).  None stands for its -1."""
    o = int(ct.clamp(int(kpL["octave"])))
    sf = ct.inv[o]
    suL = roundf(np.float32(kpL["x"]) * sf)
    svL = roundf(np.float32(kpL["y"]) * sf)
    suR = roundf(np.float32(kpR["x"]) * sf)
    cols, rows = ct.cols[o], ct.rows[o]
    det = {"o": o, "uL": int(suL), "vL": int(svL), "uR": int(suR)}
    if suR < 0 or suR + np.float32(11) >= cols:
        return None, det
    vL, uL, uR = int(svL), int(suL), int(suR)
    lo_v, hi_v = (1 if rules.win_top else 0), rows - (1 if rules.win_bottom else 0)
    lo_u, hi_u = (1 if rules.win_left else 0), cols - (1 if rules.win_right else 0)
    if (vL - 5 < lo_v or vL + 5 >= hi_v or uL - 5 < lo_u or uL + 5 >= hi_u or uR - 10 < lo_u or uR + 10 >= cols
            or (rules.win_right and uR + 11 >= hi_u)):
        return None, det
    sad = sad_vector(ct, pyr, o, vL, uL, uR, rules)
    det["sad"] = sad
    best, inc = None, 0
    for s in range(11):
        if best is None or sad[s] < best or (rules.sad_tie_last and sad[s] == best):
            best, inc = sad[s], s - 5
    det["inc"] = inc
    if inc in (-5, 5):
        return None, det
    d1, d2, d3 = (np.float32(sad[5 + inc + k]) for k in (-1, 0, 1))
    delta = (d1 - d3) / (np.float32(2.0) * (d1 + d3 - np.float32(2.0) * d2))
    det["delta"] = delta
    if delta < -1 or delta > 1:
        return None, det
    best_uR = ct.scale[o] * ((suR + np.float32(inc)) + delta)
    return np.float32(kpL["x"]) - best_uR, det


StereoOut = namedtuple("StereoOut", "rows n_subpix detail")   # rows: (iL, float32 disparity, level) in emission order


def stereo_points(kp_l, kp_r, dl, dr, pyr, cam, rules=EXACT, D=None):
    """The point part of the stereo matching of a later frame (the oracle's stereoPoints)."""
    ct = cam if isinstance(cam, CamTab) else CamTab(cam)
    N, Nr = len(kp_l), len(kp_r)
    if N == 0 or Nr == 0:
        return StereoOut([], 0, {})
    if D is None:
        D = hamming(dl, dr)
    octR = kp_r["octave"].astype(np.int64)
    r = np.float32(2.0) * ct.scale[ct.clamp(octR)]
    yR = kp_r["y"].astype(np.float32)
    maxr = np.ceil(yR + r).astype(np.int64)
    minr = np.floor(yR - r).astype(np.int64)
    uR = kp_r["x"].astype(np.float32)
    iR = np.arange(Nr, dtype=np.int64)
    tie = (65535 - iR) if rules.ham_tie_high else iR
    gate = 0 if rules.oct_gate0 else 2 if rules.oct_gate2 else 1
    found, n_subpix, detail = [], 0, {}
    for iL in range(N):
        k = kp_l[iL]
        vL, uL, lev = np.float32(k["y"]), np.float32(k["x"]), int(k["octave"])
        if not (vL >= 0) or int(vL) >= ct.H:
            continue
        row = int(vL)
        minU, maxU = uL - ct.maxD, uL - np.float32(0)
        if maxU < 0:
            continue
        m = ((minr < row) if rules.band_excl_min else (minr <= row)) & ((row < maxr) if rules.band_excl_max else (row <= maxr))
        oR, oL = (ct.clamp(octR), int(ct.clamp(lev))) if rules.oct_clamped else (octR, lev)
        m &= (oR >= oL - gate) & (oR <= oL + gate)
        m &= ((uR > minU) if rules.u_strict_lo else (uR >= minU)) & ((uR < maxU) if rules.u_strict_hi else (uR <= maxU))
        if not m.any():
            continue
        key = int((D[iL][m] * 65536 + tie[m]).min())
        dist = key >> 16
        if dist >= 100:
            continue
        j = (65535 - (key & 0xFFFF)) if rules.ham_tie_high else (key & 0xFFFF)
        if dist < 80 or (rules.le80 and dist == 80):
            n_subpix += 1
            disp, det = sub_pixel(ct, pyr, k, kp_r[j], rules)
            det.update(dist=dist, iR=j, disp=disp)
            detail[iL] = det
            if disp is not None and disp >= 0 and disp < ct.maxD:
                if disp <= 0:
                    disp = np.float32(0.01)
                found.append((dist, iL, ct.mbf / disp))
    if not found:
        return StereoOut([], n_subpix, detail)
    found.sort(key=lambda e: (e[0], -e[1] if rules.unstable else e[1]))
    nv = len(found)
    median = np.float32(found[(nv - 1) // 2 if rules.median_lo else nv // 2][0])
    th = (np.float32(1.5) * np.float32(1.4)) * median
    rows = []
    for dist, iL, depth in found:
        d = np.float32(dist)
        if not (d <= th if rules.emit_le else d < th):
            break
        disp = ct.mbf / depth
        if disp < 0:
            continue
        rows.append((iL, np.float32(disp), int(kp_l[iL]["octave"])))
    return StereoOut(rows, n_subpix, detail)


def init_points(kp_l, kp_r, dl, dr, cfg, rules=EXACT):
    """The point part of the initial frame: the ordered (i, t) pairs."""
    N, Nr = len(kp_l), len(kp_r)
    if N < 2 or Nr < 2:
        return []
    D = hamming(dl, dr)
    # knn-2 left -> right and knn-1 right -> left, ties to the lower index: (distance, index) keys
    kf = D * 65536 + np.arange(Nr)[None, :]
    k0 = kf.min(axis=1)
    lr, d0 = k0 & 0xFFFF, k0 >> 16
    kf[np.arange(N), lr] = 1 << 40
    d1 = kf.min(axis=1) >> 16
    rl = (D.T * 65536 + np.arange(N)[None, :]).min(axis=1) & 0xFFFF
    out = []
    for i in range(N):
        t = int(lr[i])
        if int(rl[t]) != i:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.float32(d0[i]) / np.float32(d1[i]))
        if not ratio <= cfg.max_ratio_12_p:
            continue
        dy = float(np.abs(np.float32(kp_l[i]["y"]) - np.float32(kp_r[t]["y"])))
        if not (dy < cfg.max_dist_epip if rules.epip_lt else dy <= cfg.max_dist_epip):
            continue
        disp = float(np.float32(kp_l[i]["x"]) - np.float32(kp_r[t]["x"]))
        if disp > cfg.min_disp if rules.disp_gt else disp >= cfg.min_disp:
            out.append((i, t))
    return out


CrossOut = namedtuple("CrossOut", "pairs n_found obs_t")   # pairs: accepted (t, q) ascending in t; obs_t[q]: its t or -1


def cross_points(P, pl, dprev, dcurr, cfg, cam, rules=EXACT, D=None):
    """The cross-frame point matching with identity poses and finite P: per current point t the
    lexicographic (d, q) minimum over the previous points q inside both gates, cut at the cap."""
    ct = cam if isinstance(cam, CamTab) else CamTab(cam)
    Sp, Sc = len(P), len(pl)
    if Sp == 0 or Sc == 0:
        return CrossOut([], 0, np.full(Sp, -1, np.int64))
    if D is None:
        D = hamming(dprev, dcurr)
    with np.errstate(all="ignore"):
        u = ct.cx + (ct.fx * P[:, 0]) / P[:, 2]
        v = ct.cy + (ct.fy * P[:, 1]) / P[:, 2]
    radius = np.float32(cfg.point_match_radius)
    q = np.arange(Sp, dtype=np.int64)
    tie = (65535 - q) if rules.cross_tie_high else q
    pairs = []
    for t in range(Sc):
        dx, dy = u - pl[t, 0], v - pl[t, 1]
        n = np.sqrt(dx * dx + dy * dy)
        m = ~((n >= cfg.proj_gate_px) if rules.gate_ge else (n > cfg.proj_gate_px))
        d = D[:, t].astype(np.float32)
        m &= (d < radius) if rules.radius_lt else (d <= radius)
        if m.any():
            key = int((D[:, t][m] * 65536 + tie[m]).min())
            pairs.append((t, (65535 - (key & 0xFFFF)) if rules.cross_tie_high else (key & 0xFFFF)))
    n_found = len(pairs)
    cap = cfg.max_point_match_num
    written = pairs if rules.beyond_cap else pairs[:cap]
    obs_t = np.full(Sp, -1, np.int64)
    for t, qq in (reversed(written) if rules.first_t else written):
        obs_t[qq] = t
    return CrossOut(pairs[:cap], n_found, obs_t) if not rules.beyond_cap else CrossOut(pairs[:cap] + pairs[cap:], n_found, obs_t)


# ----------------------------------------------------------------------------------- cameras ------
# name -> (gfpl camera, config overrides, make_camera overrides)
CAMERAS = {
    "vga": ("vga", {}, {}),
    # maxD = 544 = 16 * 34: a planted pair reaches the disparity gate exactly
    "vga544": ("vga", {}, {"fx": 544.0}),
    # band heights up to 44 rows (above SP_MINR_PAD = 32)
    "vga8": ("vga", {"orb_scale_factor": 1.4, "orb_n_levels": 8}, {}),
    # coordinates near 1919 / 1079 in the job word's 11-bit fields; with kp_cap in 1025..2048 the SEG
    # layout exceeds 54 KB (5 segments x (1080 + 64) bins) and the launch falls through to <512, false>
    "stress": ("stress", {}, {}),
}
_CT = {}


def config(cam_name, **over):
    return gfpl.default_config(**{**CAMERAS[cam_name][1], **over})


def camera(cam_name):
    if cam_name not in _CT:
        base, _, over = CAMERAS[cam_name]
        _CT[cam_name] = CamTab(gfpl.make_camera(base, config(cam_name), **over))
    return _CT[cam_name]


# ---------------------------------------------------------------------------------- pyramids ------
def texture(ct, rng, period=16, palette=None, palin=False, flat=None, axis=None):
    """A right pyramid: every level row y is the row y % 13 of a random [13][period] table repeated along
    x (palette: the values to draw from; palin: every table row reads the same from column 0 in both
    directions, so windows centred on a multiple of the period — plus axis(level) — see d1 == d3;
    flat: one value)."""
    pyr = rng.integers(0, 256, ct.pyr_bytes, dtype=np.uint8)   # (the tail and level joints: noise)
    for o in range(ct.n):
        if flat is not None:
            ct.level(pyr, o)[:] = flat
            continue
        T = rng.integers(0, 256, (13, period), dtype=np.uint8) if palette is None else \
            np.asarray(palette, np.uint8)[rng.integers(0, len(palette), (13, period))]
        if palin:
            T = T[:, np.minimum(np.arange(period), (-np.arange(period)) % period)]
        a = axis(o) if axis else 0
        ct.level(pyr, o)[:] = T[np.arange(ct.rows[o])[:, None] % 13, (np.arange(ct.cols[o])[None, :] - a) % period]
    return pyr


# ------------------------------------------------------------------------------------- builder ----
class SCase:
    """One sequence of the stereo stage."""

    def __init__(self, family, cam_name, kp_l, kp_r, dl, dr, pyr, facts=None):
        self.family, self.cam_name, self.facts = family, cam_name, facts or {}
        self.kp_l, self.kp_r, self.dl, self.dr, self.pyr = kp_l, kp_r, dl, dr, pyr
        self.n, self.nr = len(kp_l), len(kp_r)
        self._D, self._ref = None, {}
        xy = np.stack([kp_l["x"], kp_l["y"]], axis=1)
        assert len(np.unique(xy, axis=0)) == len(xy), f"{family}: left keypoints share (x, y)"
        self.where = {(float(x), float(y)): i for i, (x, y) in enumerate(xy)}

    def D(self):
        if self._D is None:
            self._D = hamming(self.dl, self.dr) if self.n and self.nr else np.zeros((self.n, self.nr), np.int64)
        return self._D

    def stereo(self, rules=EXACT):
        if rules not in self._ref:
            self._ref[rules] = stereo_points(self.kp_l, self.kp_r, self.dl, self.dr, self.pyr, camera(self.cam_name),
                                             rules, self.D())
        return self._ref[rules]

    def what(self):
        return f"{self.family} N {self.n} Nr {self.nr}"


class SBuild:
    """Collects the keypoints of one sequence.  Positions are given in the level's pixel grid (us, vs)
    and turned into level-0 coordinates that round back to them."""

    def __init__(self, cam_name, seed, **tex):
        self.cam_name, self.ct = cam_name, camera(cam_name)
        self.rng = np.random.default_rng(seed)
        self.period = tex.get("period", 16)
        self.pyr = texture(self.ct, self.rng, **tex)
        self.L, self.R, self.dl, self.dr = [], [], [], []

    def coord(self, o, s, frac=0.0):
        """float32 level-0 coordinate whose scaled rounding at level o is s (frac: offset in level pixels)"""
        ct = self.ct
        x = np.float32((s + frac) * float(ct.scale[o]))
        for _ in range(8):
            got = int(roundf(x * ct.inv[o]))
            if got == s:
                return x
            x = np.nextafter(x, np.float32(np.inf if got < s else -np.inf), dtype=np.float32)
        raise AssertionError((o, s))

    def rand_desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def near(self, desc, n):
        return _flip(self.rng, desc, n)[0] if n else desc.copy()

    def left(self, x, y, octave, desc=None):
        self.L.append((np.float32(x), np.float32(y), int(octave)))
        self.dl.append(self.rand_desc() if desc is None else desc)
        return len(self.L) - 1

    def right(self, x, y, octave, desc=None):
        self.R.append((np.float32(x), np.float32(y), int(octave)))
        self.dr.append(self.rand_desc() if desc is None else desc)
        return len(self.R) - 1

    def pair(self, o, us, vs, m=1, k=0, dist=10, octR=None, fy=0.0):
        """Left keypoint at level-o pixel (us, vs), its right partner period * m + k pixels to the left
        with a descriptor at Hamming distance dist: -> (iL, iR)."""
        d = self.rand_desc()
        y = self.coord(o, vs, fy)
        iL = self.left(self.coord(o, us), y, o, d)
        iR = self.right(self.coord(o, us - (self.period * m + k)), y, o if octR is None else octR, self.near(d, dist))
        return iL, iR

    def case(self, family, facts=None):
        kl = np.array(self.L, gfpl.KEYPOINT_DT).reshape(-1)
        kr = np.array(self.R, gfpl.KEYPOINT_DT).reshape(-1)
        dl = np.array(self.dl, np.uint8).reshape(-1, 32)
        dr = np.array(self.dr, np.uint8).reshape(-1, 32)
        return SCase(family, self.cam_name, kl, kr, dl, dr, self.pyr, facts)


def _spread(ct, n, u0=64, du=12, v0=8, dv=12):
    """n distinct (level, us, vs): level pixels whose windows (and those of partners up to 54 px to the
    left) are valid, dealt to the levels in turn as long as a level has room"""
    room = []
    for o in range(ct.n):
        nu = max((ct.cols[o] - 12 - u0) // du + 1, 0)
        nv = max((ct.rows[o] - 6 - v0) // dv + 1, 0)
        room.append([(o, u0 + du * (i % nu), v0 + dv * (i // nu)) for i in range(nu * nv)])
    assert n <= sum(len(r) for r in room), n
    take, i = [0] * ct.n, 0
    while sum(take) < n:
        if take[i % ct.n] < len(room[i % ct.n]):
            take[i % ct.n] += 1
        i += 1
    # evenly over each level's lattice (the whole image, its last rows and columns included), levels in turn
    picks = [[room[o][(k * len(room[o])) // take[o]] for k in range(take[o])] for o in range(ct.n)]
    out, k = [], 0
    while len(out) < n:
        out += [picks[o][k] for o in range(ct.n) if k < take[o]]
        k += 1
    return out[:n]


# ------------------------------------------------------------------------------------ families ----
GRID_PAIRS = [(1, 1), (2, 1), (1, 2), (63, 64), (64, 65), (65, 63), (255, 257), (256, 255), (257, 256),
              (511, 513), (512, 511), (513, 512), (1023, 1025), (1024, 1023), (1025, 1024), (2047, 2048),
              (2048, 2047), (2048, 2048)]


def _planted(cam_name, n, nr, seed, family="grid"):
    """min(n, nr) planted pairs spread over the levels (distances 3..74, shifts -4..4, m 1..3), the rest
    of either side unmatched noise; the right side in a random order."""
    b = SBuild(cam_name, seed)
    ct = b.ct
    lat = _spread(ct, max(n, 1))
    m = min(n, nr)
    for i in range(n):
        o, us, vs = lat[i]
        if i < m:
            b.pair(o, us, vs, m=1 + i % 3, k=(i * 5) % 9 - 4, dist=3 + (i * 7) % 72)
        else:
            b.left(b.coord(o, us), b.coord(o, vs), o)
    for j in range(nr - m):
        o, us, vs = lat[j % len(lat)]
        b.right(b.coord(o, us - 20), b.coord(o, vs, 0.25), o)
    c = b.case(family, {"planted": m})
    perm = b.rng.permutation(c.nr)
    c.kp_r, c.dr = c.kp_r[perm], c.dr[perm]
    return c


def _band_edges(cam_name, o):
    """Right keypoints of level o with left keypoints at the rows minr - 1, minr, maxr, maxr + 1 (whole
    and fractional y); bands cut by the top and the bottom of the image; left y = -0.0, H - 0.5, < 0, H."""
    b = SBuild(cam_name, [2, o])
    ct = b.ct
    sc = float(ct.scale[o])
    facts = {"in": [], "out": []}
    groups = [(ct.H * 0.25, 0.0), (ct.H * 0.4 + 0.3, 0.75), (ct.H * 0.55 + 0.5, 0.5), (ct.H * 0.7 - 0.25, 0.999)]
    for g, (yr, fl) in enumerate(groups):
        yr = np.float32(round(yr / sc) * sc + (yr % 1))
        r = np.float32(2.0) * ct.scale[o]
        minr, maxr = int(np.floor(yr - r)), int(np.ceil(yr + r))
        d = b.rand_desc()
        b.right(b.coord(o, 12), yr, o, b.near(d, 8))     # (the left rows differ: one x serves them all)
        for n, row in enumerate((minr - 1, minr, maxr, maxr + 1)):
            iL = b.left(b.coord(o, 12 + 16 * (1 + g % 2)), np.float32(row + fl), o, b.near(d, n))
            facts["in" if minr <= row <= maxr else "out"].append(iL)
    # top and bottom of the image: the windows are invalid there, so the matches show in n_subpix only
    d = b.rand_desc()
    b.right(np.float32(60.0), np.float32(1.0), o, d)
    b.right(np.float32(60.0), np.float32(ct.H - 1.5), o, d)
    for n, y in enumerate((-0.0, 0.5, ct.H - 0.5, ct.H - 1.0)):
        facts.setdefault("edge", []).append(b.left(np.float32(200 + 16 * n), np.float32(y), o, d))
    for n, y in enumerate((-0.25, -3.0, float(ct.H), ct.H + 2.0)):
        facts.setdefault("outside", []).append(b.left(np.float32(300 + 16 * n), np.float32(y), o, d))
    return b.case("band_edges", facts)


CHUNK_RUNS = (31, 32, 33, 64, 65, 200)


def _chunks(cam_name, run):
    """`run` right keypoints of one (octave, minr) bin, plus shorter runs on two other rows; left keypoints
    of one wave spread over the three rows, of levels 0 and 1 on the same row, whose best candidate is the
    first, the last, entry 31 / 32 of the run; inactive lanes (y < 0, x < 0) between them."""
    b = SBuild(cam_name, [3, run])
    ct = b.ct
    facts = {"best": []}
    for g, (vs, n) in enumerate(((100, run), (160, 33 if run != 33 else 7), (220, 3))):
        base = len(b.R)
        for j in range(n):
            b.right(b.coord(0, 12 + 2 * j), b.coord(0, vs), 0)
        targets = sorted({0, n - 1, min(31, n - 1), min(32, n - 1), n // 2})
        for e, tj in enumerate(targets * 2):
            lev = e % 2                                   # level-1 left keypoints accept octave-0 candidates too
            uR = 12 + 2 * tj
            k, m = (e % 9) - 4, 27 + e % 3
            x = b.coord(0, uR + 16 * m + k)
            if lev == 1:                                  # window at level 1: keep its shift inside -4..4
                x = b.coord(1, int(roundf(b.coord(0, uR) * ct.inv[1])) + 16 * 20 + k)
            iL = b.left(x, b.coord(0, vs, 0.04 * e), lev, b.near(b.dr[base + tj], 6 + e))
            facts["best"].append((iL, base + tj))
            if e % 3 == 1:
                b.left(np.float32(-7.0 - e), b.coord(0, vs), 0, b.dr[base + tj])        # maxU < 0
                b.left(b.coord(0, 500 + e), np.float32(-2.0 - e - 20 * g), 0, b.dr[base + tj])   # y < 0
    return b.case("chunks", facts)


def _octaves(cam_name, extra):
    """Per left level: right keypoints with one descriptor (9 bits from the left one) at octaves
    levelL - 2 .. levelL + 2, the +-2 ones at the lowest iR (they would win the tie).  Out-of-range octaves on both sides; `extra`:
    whether the right side has out-of-range octaves at all (the extra segment empty or not)."""
    b = SBuild(cam_name, [4, extra])
    ct = b.ct
    facts = {"accept": [], "none": []}

    def group(levL, octs, vs, accept):
        o = int(ct.clamp(levL))
        d = b.rand_desc()
        e = b.near(d, 9)
        y = b.coord(o, vs)
        first = None
        for n, oc in enumerate(octs):
            iR = b.right(b.coord(o, 100 - 16 * n + 2), y, oc, e)
            if first is None and abs(oc - levL) <= 1:
                first = iR
        iL = b.left(b.coord(o, 100 + 16 * 8), y, levL, d)
        assert (first is not None) == accept
        (facts["accept"].append((iL, first)) if accept else facts["none"].append(iL))

    vs = 20
    for lev in range(ct.n):
        octs = [oc for oc in (lev - 2, lev + 2, lev - 1, lev, lev + 1) if extra or 0 <= oc < ct.n]
        group(lev, octs, vs, True)
        vs += 30
    if extra:
        n = ct.n
        group(-1, [-3, 1, -2, 0], vs, True); vs += 30            # raw gate: -2 and 0 pass
        group(n + 1, [n - 1, n + 3, n, n + 2], vs, True); vs += 30   # clamped both would be n - 1
        group(200, [198, 202, 201], vs, True); vs += 30          # beyond int8
        group(-200, [-202, -198, -201], vs, True); vs += 30
        group(300, [44, 300 - 65536, 302], vs, False); vs += 30  # 300 & 0xFF = 44: no candidate
        group(n + 1, [n - 1, n - 2], vs, False); vs += 30        # the clamped octaves would pass
    return b.case("octaves", facts)


def _ham(cam_name):
    """ham_ties: equal distances at the lowest and the highest iR and at entries 31 / 32 of a 53-entry bin;
    ham_thresholds: best distance 79 / 80 / 99 / 100, and a left keypoint without any candidate."""
    b = SBuild(cam_name, [5])
    facts = {"ties": [], "th": {}}
    y0 = b.coord(0, 60)
    anchor = b.rand_desc()
    r_first = b.right(b.coord(0, 300 - 16 * 3), y0, 0, b.near(anchor, 12))           # iR 0
    for j in range(1, 32):                               # 31 others of the same bin first: in index order the
        b.right(b.coord(0, 20 + j), b.coord(0, 120), 0)  # tied pair is the bin's entry 31 and 32
    d2 = b.rand_desc()
    r32 = b.right(b.coord(0, 400 - 16 * 2 + 1), b.coord(0, 120), 0, b.near(d2, 9))   # iR 32
    r33 = b.right(b.coord(0, 400 - 16 * 4 + 1), b.coord(0, 120), 0, b.near(d2, 9))   # iR 33
    for j in range(20):
        b.right(b.coord(0, 60 + j), b.coord(0, 120), 0)
    facts["ties"].append((b.left(b.coord(0, 400), b.coord(0, 120), 0, d2), r32, r33))
    for dist, vs in ((79, 180), (80, 210), (99, 240), (100, 270)):
        d = b.rand_desc()
        iR = b.right(b.coord(0, 200 - 16), b.coord(0, vs), 0, b.near(d, dist))
        facts["th"][dist] = (b.left(b.coord(0, 200), b.coord(0, vs), 0, d), iR)
    facts["alone"] = b.left(b.coord(0, 500), b.coord(0, 400), 0, anchor)
    for n in range(6):                                   # filler at distance 70: the median, so 79 is emitted
        b.pair(1, 100 + 20 * n, 200, m=2, k=n - 3, dist=70)
    r_last = b.right(b.coord(0, 300 - 16 * 5), y0, 0, b.near(anchor, 12))            # the highest iR
    facts["ties"].append((b.left(b.coord(0, 300), y0, 0, anchor), r_first, r_last))
    return b.case("ham", facts)


def _sad_shifts(cam_name, kind):
    """Per level, pairs whose SAD minimum sits at each shift -5..5 (+-5: rejected).  kind "p16": random
    texture of period 16; "p8": period 8, so the shifts -4 and 4 are both zero (the first wins);
    "bw": pixels 0 and 255 only (differences up to 510 either way); "flat": one value (all SADs 0)."""
    tex = {"p16": {}, "p8": {"period": 8}, "bw": {"palette": (0, 255)}, "flat": {"flat": 77}}[kind]
    b = SBuild(cam_name, [6, ("p16", "p8", "bw", "flat").index(kind)], **tex)
    ct = b.ct
    facts = {"shift": []}
    for o in range(ct.n):
        for k in range(-5, 6):
            us, vs = 80 + 13 * (k + 5), 12 + 9 * (k + 5) + o
            m = 2 if b.period == 16 else 4
            iL, _ = b.pair(o, us, vs, m=m, k=k, dist=5 + k + 5)
            facts["shift"].append((iL, k))
    return b.case("sad_" + kind, facts)


def _sad_align(cam_name):
    """Per level the sixteen (pl & 3, pr & 3) dword misalignments of the two window rows."""
    b = SBuild(cam_name, [7])
    ct = b.ct
    facts = {"pairs": []}
    for o in (o for o in range(ct.n) if ct.cols[o] >= 250):
        for a in range(4):
            for k in range(4):
                # one window row for all: uL = a, uR = a - k (mod 4) whatever the level's row pitch
                iL, _ = b.pair(o, 120 + a + 20 * k, 30, m=3, k=k, dist=4 + a + k)
                facts["pairs"].append(iL)
    return b.case("sad_align", facts)


def _sad_borders(cam_name):
    """Per level, windows touching the level's sides: accepted at the bound, rejected one beyond, for uR
    (left bound 10, right bound cols - 12), uL (right bound cols - 6) and vL (5, rows - 6).  uL's left
    bound cannot fire on its own: uR <= uL and uR >= 10 hold first."""
    ct = camera(cam_name)
    # palindromic about column cols - 10 of every level: the pair (uL, uR) = (cols - 10, cols - 12) has
    # deltaR = 0 and disparity exactly 0 (-> 0.01f); a window that far right has no room for a larger one
    b = SBuild(cam_name, [8], palin=True, axis=lambda o: (ct.cols[o] - 10) % 16)
    facts = {"at": [], "beyond": []}
    for o in range(ct.n):
        cols, rows = ct.cols[o], ct.rows[o]
        for key, d in (("at", 0), ("beyond", 1)):
            v1, v2, v3 = (rows * n // 4 + 6 * d for n in (1, 2, 3))
            facts[key].append(("uR_left", b.pair(o, 10 - d + 32, v1, m=2, k=0)[0]))
            facts[key].append(("uL_right", b.pair(o, cols - 6 + d, v2, m=2, k=0)[0]))
            facts[key].append(("uR_right", b.pair(o, cols - 10, v3, m=0, k=2 - d)[0]))
            facts[key].append(("vL_top", b.pair(o, 44, 5 - d, m=2, k=1)[0]))
            facts[key].append(("vL_bottom", b.pair(o, 44, rows - 6 + d, m=2, k=-1)[0]))
    return b.case("sad_borders", facts)


def _disparity():
    """Camera vga544 (maxD = 544.0), level 0, palindromic texture (deltaR = 0 on multiples of 16):
    disparity exactly 0 with uR == uL and with a shift, disparity just below / at maxD, uR == uL - maxD,
    and maxU < 0."""
    b = SBuild("vga544", [9], palin=True)
    f = {}

    def put(name, x, xr, vs):
        d = b.rand_desc()
        y = b.coord(0, vs)
        f[name] = b.left(np.float32(x), y, 0, d)
        b.right(np.float32(xr), y, 0, b.near(d, 7))

    put("zero_same", 560.0, 560.0, 40)                 # uR == uL: shift 0, disparity 0 -> 0.01f
    put("zero_shift", 576.0, 573.0, 70)                # shift 3, disparity 0
    put("at_maxD", 592.0, 48.0, 100)                   # disparity 544 = maxD: rejected
    put("below_maxD", np.nextafter(np.float32(592.0), np.float32(0)), 48.0, 130)
    put("u_at_lo", 607.75, 63.75, 160)                 # uR == uL - maxD exactly; disparity 543.75
    put("u_below_lo", 607.75, np.nextafter(np.float32(63.75), np.float32(0)), 190)
    put("small", 624.0, 608.0, 220)                    # disparity 16
    put("neg_maxU", -1.0, -3.0, 250)
    return b.case("disparity", f)


def _median(kind):
    """Hamming distances chosen per kind; every pair refines to a valid disparity."""
    sets = {
        "odd": [10] * 3 + [21] * 2,                    # nv 5: median 10 (element 2), 21 against 2.1f * 10
        "even": [10] * 2 + [20] * 2 + [42, 41],        # nv 6: element 3 = 20 (element 2 = 20 too) -> 42 against 2.1f * 20
        "split": [10, 10, 30, 30],                     # nv 4: element 2 = 30, element 1 = 10: 30 against 21 / 63
        "m30": [30] * 5 + [63, 62, 64],
        "zero": [0, 0, 0, 5, 7],                       # median 0: nothing
        "spread": [d for d in range(80) for _ in range(1 + (d * 7) % 5)],
    }
    if kind in ("equal600", "equal1100"):
        dists = [17] * int(kind[5:])
    else:
        dists = sets[kind]
    b = SBuild("vga", [10, len(dists), dists[0]])
    ct = b.ct
    n = len(dists)
    lat = _spread(ct, n)
    order = b.rng.permutation(n)                       # distances in no particular iL order
    for i in range(n):
        o, us, vs = lat[i]
        b.pair(o, us, vs, m=1 + i % 3, k=i % 9 - 4, dist=dists[order[i]])
    return b.case("median_" + kind, {"dists": [dists[order[i]] for i in range(n)]})


MEDIAN_KINDS = ("odd", "even", "split", "m30", "zero", "spread", "equal600", "equal1100")
SAD_KINDS = ("p16", "p8", "bw", "flat")
_CASES = {}


def _memo(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def grid_cases():
    """kp_cap 2048, camera vga: one sequence per (N, Nr) of GRID_PAIRS."""
    return _memo("grid", lambda: [_planted("vga", n, nr, [1, n, nr]) for n, nr in GRID_PAIRS])


def small_cases():
    """camera vga, at most 256 keypoints a side: every mechanism family, one sequence each."""
    def make():
        out = [_band_edges("vga", o) for o in range(4)]
        out += [_chunks("vga", run) for run in CHUNK_RUNS]
        out += [_octaves("vga", False), _octaves("vga", True), _ham("vga")]
        out += [_sad_shifts("vga", k) for k in SAD_KINDS]
        out += [_sad_align("vga"), _sad_borders("vga")]
        out += [_median(k) for k in MEDIAN_KINDS if not k.startswith("equal") and k != "spread"]
        return out
    return _memo("small", make)


def median_cases():
    """camera vga, kp_cap 2048: the long sorts (one and two rounds of either block size, split ranks)."""
    return _memo("median", lambda: [_median(k) for k in ("spread", "equal600", "equal1100")])


def disparity_cases():
    return _memo("disparity", lambda: [_disparity()])


def tall_cases(cam_name):
    """Other cameras: planted sets, band edges per level, octaves and the window borders."""
    def make():
        ct = camera(cam_name)
        out = [_planted(cam_name, n, nr, [11, n, nr], "grid_" + cam_name) for n, nr in ((255, 257), (65, 63), (513, 512))]
        out += [_band_edges(cam_name, o) for o in range(ct.n)]
        out += [_sad_borders(cam_name), _sad_align(cam_name)] + ([_octaves(cam_name, True)] if ct.cols[-1] >= 250 else [])
        return out
    return _memo("tall_" + cam_name, make)


STEREO_FAMILIES = {"grid": grid_cases, "small": small_cases, "median": median_cases, "disparity": disparity_cases,
                   "vga8": lambda: tall_cases("vga8"), "stress": lambda: tall_cases("stress")}


# --------------------------------------------------------------------- stereo frames and read-back
def host_frames(cam_name, n_seq, kp_cap, kl_cap=32):
    """One synthetic frame of n_seq sequences with few keylines; the point inputs and the pyramid are
    overwritten by fill_stereo."""
    sp = gfpl.synth_params(n_kp=16, n_kl=8, n_world_pts=40, n_world_lines=16, seed=5)
    return gfpl.HostFrames(camera(cam_name).cam, sp, n_seq, 1, kp_cap, kl_cap)


def fill_stereo(H, f, cases):
    """One case per sequence; a sequence beyond the cases gets the first one again.  Rows past the counts
    hold copies of rows of the OTHER side (a read past a count finds a perfect match)."""
    cap = H.kp_cap
    for b in range(H.B):
        c = cases[b] if b < len(cases) else cases[0]
        assert c.n <= cap and c.nr <= cap
        H.n_kp_l[f, b], H.n_kp_r[f, b] = c.n, c.nr
        src_l, src_r = (c.kp_r, c.dr) if c.nr else (c.kp_l, c.dl), (c.kp_l, c.dl) if c.n else (c.kp_r, c.dr)
        if len(src_l[0]):
            H.kp_l[f, b], H.pdesc_l[f, b] = src_l[0][0], src_l[1][0]
            H.kp_r[f, b], H.pdesc_r[f, b] = src_r[0][0], src_r[1][0]
        H.kp_l[f, b, :c.n], H.pdesc_l[f, b, :c.n] = c.kp_l, c.dl
        H.kp_r[f, b, :c.nr], H.pdesc_r[f, b, :c.nr] = c.kp_r, c.dr
        H.pyr_r[f, b] = c.pyr


def check_stereo(fh, case, initial_idx=True):
    """[] or the differences of a frame's points from the statement of `case`: the rows in emission
    order as (iL from pt_pl, the float32 disparity's bits, the level), then idx and the descriptors."""
    want = case.stereo().rows
    w = case.what() + ": "
    pl, disp, lev = fh.get("pt_pl"), fh.get("pt_disp"), fh.get("pt_level")
    got = []
    for k in range(len(pl)):
        iL = case.where.get((float(pl[k, 0]), float(pl[k, 1])))
        if iL is None:
            return [w + f"row {k}: pt_pl {pl[k].tolist()} is no left keypoint"]
        got.append((iL, float(disp[k]), int(lev[k])))
    exp = [(iL, float(d), lv) for iL, d, lv in want]
    if got != exp:
        return [w + f"{len(got)} rows, want {len(exp)}; first difference "
                + _first_diff(np.array(got, object).reshape(-1, 3), np.array(exp, object).reshape(-1, 3))]
    bad = []
    if len(exp) and not np.array_equal(fh.get("pdesc"), case.dl[[e[0] for e in exp]]):
        bad.append(w + "pdesc rows are not the left rows")
    if not np.array_equal(fh.get("pt_idx"), np.arange(len(exp))):
        bad.append(w + "pt_idx is not 0..n-1")
    return bad


# -------------------------------------------------------------------------------------- initial ---
class ICase:
    def __init__(self, kp_l, kp_r, dl, dr, facts=None, name="init"):
        self.family, self.kp_l, self.kp_r, self.dl, self.dr, self.facts = name, kp_l, kp_r, dl, dr, facts or {}
        self.n, self.nr = len(kp_l), len(kp_r)
        self.cam_name = "vga"
        self.pyr = None
        self._ref = {}
        xy = np.stack([kp_l["x"], kp_l["y"]], axis=1)
        assert len(np.unique(xy, axis=0)) == len(xy)
        self.where = {(float(x), float(y)): i for i, (x, y) in enumerate(xy)}

    def init(self, rules=EXACT):
        if rules not in self._ref:
            self._ref[rules] = init_points(self.kp_l, self.kp_r, self.dl, self.dr, config("vga"), rules)
        return self._ref[rules]

    def what(self):
        return f"{self.family} N {self.n} Nr {self.nr}"


INIT_PAIRS = [(0, 5), (5, 0), (1, 7), (7, 1), (2, 2), (2, 300), (63, 65), (64, 64), (65, 33), (255, 256), (257, 31),
              (512, 511), (513, 512), (1024, 1023), (1025, 1026), (2048, 2047), (2047, 2048)]


def _init_case(n, nr, seed):
    """min(n, nr) planted pairs at distance 4..40 (noise near 128); then the gate cases overwrite the first
    rows: d0 / d1 at 9 / 10, 45 / 50, 0 / 0, 0 / 7; |dy| at 2.0 and the next float; disparity at 1.0 and the
    float below; two left rows equally near one right row (the lower is the mutual one)."""
    rng = np.random.default_rng([12, n, nr, seed])
    kl, kr = np.zeros(n, gfpl.KEYPOINT_DT), np.zeros(nr, gfpl.KEYPOINT_DT)
    dl = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    dr = rng.integers(0, 256, (nr, 32), dtype=np.uint8)
    m = min(n, nr)
    kl["x"], kl["y"] = 100.0 + 0.25 * np.arange(n), 50.0 + (np.arange(n) % 97)
    kl["octave"] = np.arange(n) % 6 - 1
    perm = rng.permutation(nr)[:m]
    for i in range(m):
        dr[perm[i]] = _flip(rng, dl[i], 4 + (i * 5) % 37)[0]
    kr["x"], kr["y"] = 30.0, 400.0
    kr["x"][perm], kr["y"][perm] = kl["x"][:m] - 20.0, kl["y"][:m] + ((np.arange(m) % 5) - 2)
    facts = {}
    if m >= 40:
        def second(i, d0, d1, slot):
            """right perm[i] at distance d0 and right perm[slot] (its own left row turned to noise) at d1"""
            dr[perm[i]] = _flip(rng, dl[i], d0)[0] if d0 else dl[i]
            dr[perm[slot]] = _flip(rng, dl[i], d1)[0] if d1 else dl[i]
            dl[slot] = rng.integers(0, 256, 32, dtype=np.uint8)
            kr["x"][perm[slot]] = 900.0

        second(0, 9, 10, 20); second(1, 45, 50, 21); second(2, 0, 0, 22); second(3, 0, 7, 23); second(4, 46, 50, 24)
        facts["ratio"] = {"9/10": 0, "45/50": 1, "0/0": 2, "0/7": 3, "46/50": 4}
        kr["y"][perm[5]] = kl["y"][5] + np.float32(2.0)
        kr["y"][perm[6]] = np.nextafter(kl["y"][6] + np.float32(2.0), np.float32(1e9), dtype=np.float32)
        kr["y"][perm[7]] = kl["y"][7] - np.float32(2.0)
        facts["epip"] = {"at": (5, 7), "beyond": (6,)}
        kr["x"][perm[8]] = kl["x"][8] - np.float32(1.0)
        kr["x"][perm[9]] = np.nextafter(kl["x"][9] - np.float32(1.0), np.float32(1e9), dtype=np.float32)
        facts["disp"] = {"at": 8, "below": 9}
        dl[11] = dl[10]                                  # rows 10 and 11 tie for right perm[10]
        dr[perm[11]] = rng.integers(0, 256, 32, dtype=np.uint8)
        facts["tie"] = (10, 11)
    return ICase(kl, kr, dl, dr, facts)


def init_cases():
    return _memo("init", lambda: [_init_case(n, nr, 0) for n, nr in INIT_PAIRS])


def fill_init(H, f, cases):
    ct = camera("vga")
    noise = np.random.default_rng(77).integers(0, 256, ct.pyr_bytes, dtype=np.uint8)
    for b, c in enumerate(cases):
        H.n_kp_l[f, b], H.n_kp_r[f, b] = c.n, c.nr
        # rows past the counts: copies of the other side's first row
        if c.nr:
            H.kp_l[f, b], H.pdesc_l[f, b] = c.kp_r[0], c.dr[0]
        if c.n:
            H.kp_r[f, b], H.pdesc_r[f, b] = c.kp_l[0], c.dl[0]
        H.kp_l[f, b, :c.n], H.pdesc_l[f, b, :c.n] = c.kp_l, c.dl
        H.kp_r[f, b, :c.nr], H.pdesc_r[f, b, :c.nr] = c.kp_r, c.dr
        H.pyr_r[f, b] = noise


def check_init(fh, case):
    want = case.init()
    w = case.what() + " initial: "
    pl, disp = fh.get("pt_pl"), fh.get("pt_disp")
    got = []
    for k in range(len(pl)):
        i = case.where.get((float(pl[k, 0]), float(pl[k, 1])))
        if i is None:
            return [w + f"row {k}: pt_pl {pl[k].tolist()} is no left keypoint"]
        got.append((i, float(disp[k])))
    exp = [(i, float(np.float32(case.kp_l[i]["x"]) - np.float32(case.kp_r[t]["x"]))) for i, t in want]
    if got != exp:
        return [w + f"{len(got)} rows, want {len(exp)}; first difference "
                + _first_diff(np.array(got, object).reshape(-1, 2), np.array(exp, object).reshape(-1, 2))]
    bad = []
    if len(exp) and not np.array_equal(fh.get("pdesc"), case.dl[[e[0] for e in exp]]):
        bad.append(w + "pdesc rows are not the left rows")
    if not np.array_equal(fh.get("pt_level"), case.kp_l["octave"][[e[0] for e in exp]].astype(np.int32)):
        bad.append(w + "pt_level")
    if not np.array_equal(fh.get("pt_idx"), np.arange(len(exp))):
        bad.append(w + "pt_idx is not 0..n-1")
    return bad


# ---------------------------------------------------------------------------------------- cross ---
class XCase:
    """One sequence of the cross-frame point matching: previous points P with descriptors dp, current
    observations pl with descriptors dc."""

    def __init__(self, name, P, pl, dp, dc, facts=None, cfg_over=None, statement=True):
        self.family, self.P, self.pl, self.dp, self.dc = name, np.asarray(P, np.float64).reshape(-1, 3), \
            np.asarray(pl, np.float64).reshape(-1, 2), np.asarray(dp, np.uint8).reshape(-1, 32), \
            np.asarray(dc, np.uint8).reshape(-1, 32)
        self.facts, self.cfg_over, self.statement = facts or {}, cfg_over or {}, statement
        self.sp, self.sc = len(self.P), len(self.pl)
        self._D, self._ref = None, {}

    def cfg(self):
        return gfpl.default_config(**self.cfg_over)

    def cross(self, rules=EXACT):
        if rules not in self._ref:
            if self._D is None and self.sp and self.sc:
                self._D = hamming(self.dp, self.dc)
            self._ref[rules] = cross_points(self.P, self.pl, self.dp, self.dc, self.cfg(), camera("vga"), rules, self._D)
        return self._ref[rules]

    def what(self):
        return f"{self.family} Sp {self.sp} Sc {self.sc}"


def _point_at(ct, du, dv):
    """P whose projection is (cx + du, cy + dv) exactly, for whole du, dv: Z = fx."""
    P = np.array([float(du), float(dv) * ct.fx / ct.fy, ct.fx])
    assert ct.cx + (ct.fx * P[0]) / P[2] == ct.cx + du and ct.cy + (ct.fy * P[1]) / P[2] == ct.cy + dv
    return P


def _cross_gates():
    """Offsets (6, 8), (10, 0), (10, 2^-40) and 2^-30 beyond; Hamming 50 / 51; ties to the lower q;
    several t choosing one q."""
    ct = camera("vga")
    rng = np.random.default_rng(20)
    P, pl, dp, dc, f = [], [], [], [], {"gate_in": [], "gate_out": [], "tie": [], "multi": None}

    def add(du, dv, off, dist, key, desc=None):
        d = rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc
        q, t = len(P), len(pl)
        P.append(_point_at(ct, du, dv))
        dp.append(d)
        pl.append((ct.cx + du + off[0], ct.cy + dv + off[1]))
        dc.append(_flip(rng, d, dist)[0] if dist else d)
        if key:
            f[key].append((t, q))

    eps = 2.0 ** -30          # (survives the addition to a coordinate near 300; an ulp of 10.0 would not)
    add(-200, -100, (6.0, 8.0), 10, "gate_in")
    add(-150, -100, (10.0, 0.0), 10, "gate_in")
    add(-100, -100, (10.0, 2.0 ** -40), 10, "gate_in")
    add(-50, -100, (0.0, -10.0), 50, "gate_in")            # both gates at their bound
    add(0, -100, (10.0 + eps, 0.0), 10, "gate_out")
    add(50, -100, (6.0, 8.0 + eps), 10, "gate_out")
    add(100, -100, (3.0, 4.0), 51, "gate_out")             # Hamming 51
    # ties: q and q + 1 at the same place and distance from one t
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    for du in (-200, 0):
        q = len(P)
        P += [_point_at(ct, du, 50), _point_at(ct, du + 1, 50)]
        e = _flip(rng, d, 20)[0]
        dp += [e, e.copy()]
        pl.append((ct.cx + du + 0.5, ct.cy + 50.0))
        dc.append(d)
        f["tie"].append((len(pl) - 1, q, q + 1))
        d = rng.integers(0, 256, 32, dtype=np.uint8)
    # three t around one q: pl_obs is the last one's
    q = len(P)
    P.append(_point_at(ct, 100, 100))
    dp.append(d)
    ts = []
    for off in ((1.0, 0.0), (0.0, 2.0), (-3.0, 0.0)):
        ts.append(len(pl))
        pl.append((ct.cx + 100 + off[0], ct.cy + 100 + off[1]))
        dc.append(_flip(rng, d, 5)[0])
    f["multi"] = (q, ts)
    return XCase("cross_gates", P, pl, dp, dc, f)


def _cross_radius():
    """point_match_radius 49.5: Hamming 49 passes, 50 does not."""
    ct = camera("vga")
    rng = np.random.default_rng(21)
    P, pl, dp, dc = [], [], [], []
    for n, dist in enumerate((49, 50, 48, 51)):
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        P.append(_point_at(ct, -100 + 40 * n, 0)); dp.append(d)
        pl.append((ct.cx - 100 + 40 * n + 1.0, ct.cy)); dc.append(_flip(rng, d, dist)[0])
    return XCase("cross_radius", P, pl, dp, dc, {"in": [0, 2], "out": [1, 3]}, {"point_match_radius": 49.5})


def cross_cs(ct, gate=10.0):
    """cross_grid's cell size: the smallest power of two >= 16 that is >= gate + 0.5 and gives <= 2048 cells"""
    cs = 16
    while not (cs >= gate + 0.5 and ((ct.W + cs - 1) // cs) * ((ct.H + cs - 1) // cs) <= 2048):
        cs *= 2
    return cs


def _cross_cells():
    """Projections and observations on both sides of cell borders (3 px apart across the border), in the
    clamped cells outside the image, at negative coordinates, with |pl| just below and at 1e6 (the slow
    path) and near 1e5 (a coarse float pre-filter): the matching pair is 9.9 px apart, a decoy 10.1 px."""
    ct = camera("vga")
    cs = cross_cs(ct)
    rng = np.random.default_rng(22)
    P, pl, dp, dc, f = [], [], [], [], {"match": [], "cs": cs}

    def add(u, v, off, dist=10):
        """previous point projecting to about (u, v); the current one `off` away"""
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        q = len(P)
        Pq = np.array([(u - ct.cx) / ct.fx * 2.0, (v - ct.cy) / ct.fy * 2.0, 2.0])
        pu, pv = ct.cx + (ct.fx * Pq[0]) / Pq[2], ct.cy + (ct.fy * Pq[1]) / Pq[2]
        P.append(Pq); dp.append(d)
        pl.append((pu + off[0], pv + off[1])); dc.append(_flip(rng, d, dist)[0])
        return q, len(pl) - 1

    borders = [(cs * i, cs * j) for i, j in ((1, 1), (5, 3), (ct.W // cs, 4), (7, ct.H // cs))]
    for bx, by in borders:
        for sx, sy in ((-1.5, 0.0), (0.0, -1.5), (-1.5, -1.5), (1.5, 1.5)):
            f["match"].append(add(bx + sx, by + sy, (-2.0 * sx * 2, -2.0 * sy * 2)))
    for u, v in ((-30.0, 100.0), (-5000.0, -7000.0), (ct.W + 400.0, ct.H + 300.0), (100.0, -0.25), (-0.25, -0.25)):
        f["match"].append(add(u, v, (9.9, 0.0)))
        add(u + 200.0 if abs(u) < 2000 else u * 3, v, (10.1, 0.0))
    for u in (1e5, -1e5, 999989.0, 1e6 - 9.8, 1e6 + 20.0, -1e6 - 20.0):
        f["match"].append(add(u, 120.0, (9.9, 0.0)))
        add(u, 520.0, (0.0, 10.1))
    f["slow"] = [t for q, t in f["match"] if abs(pl[t][0]) >= 1e6]
    return XCase("cross_cells", P, pl, dp, dc, f)


def _cross_sizes(sp, sc, name="cross_sizes", cfg_over=None, one_cell=False, wild=0):
    """min(sp, sc) planted pairs (distance 5..45, offset up to 7 px), each previous point at its own place
    (one_cell: all inside one 16 px cell), the current side in a random order; every fifth current point
    has a second previous point in reach that is farther in Hamming distance; `wild` extra previous points
    with Z = 0 (NaN / infinite projections: they are candidates of every t in the oracle and the kernel)."""
    ct = camera("vga")
    rng = np.random.default_rng([23, sp, sc, int(one_cell), wild])
    m = min(sp, sc)
    P = np.zeros((sp, 3)); pl = np.zeros((sc, 2))
    dp = rng.integers(0, 256, (sp, 32), dtype=np.uint8)
    dc = rng.integers(0, 256, (sc, 32), dtype=np.uint8)
    qs = np.arange(sp)
    if one_cell:
        u, v = 322.0 + (qs % 12), 242.0 + (qs // 12) % 12 + (qs // 144) * 0.01
    else:
        u, v = 8.0 + 13.0 * (qs % 48) + 0.37 * (qs // 48 % 3), 6.0 + 10.5 * (qs // 48)
    Z = 1.0 + (qs % 7)
    P[:, 0], P[:, 1], P[:, 2] = (u - ct.cx) / ct.fx * Z, (v - ct.cy) / ct.fy * Z, Z
    perm = rng.permutation(sc)
    for i in range(m):
        t = perm[i]
        pl[t] = (u[i] + (i % 5) - 2.0, v[i] + (i % 3) * 2.5 - 2.0)
        dc[t] = _flip(rng, dp[i], 5 + (i * 3) % 41)[0]
    for t in perm[m:]:
        pl[t] = (700.0 + t % 50, 500.0 + t // 50)        # outside every gate
    if wild:
        P[sp - wild:] = 0.0
        P[sp - wild:, 0] = (np.arange(wild) % 3) - 1.0   # -inf / NaN / +inf projections
        for w in range(wild):                            # near a current descriptor: a rival of its planted partner
            dp[sp - wild + w] = _flip(rng, dc[perm[w % sc]], 3 + w % 40)[0]
    return XCase(name, P, pl, dp, dc, {"planted": m - wild}, cfg_over, statement=not wild)


def _cross_unique(c):
    """pl unique: the pl_obs of a previous point names the t it came from"""
    assert len(np.unique(c.pl, axis=0)) == c.sc, c.what()
    return c


CROSS_SIZES = [(0, 5), (5, 0), (1, 1), (1, 1025), (1023, 1024), (1024, 1023), (1025, 1), (2048, 1025), (1025, 2048),
               (2048, 2048)]


def cross_cases():
    """The default config (cap 500): gates, cells, sizes; 2048 x 2048 has more than 500 matches, so the cap
    falls inside the first round of 1024 current points."""
    def make():
        out = [_cross_gates(), _cross_cells()]
        out += [_cross_sizes(sp, sc) for sp, sc in CROSS_SIZES]
        out += [_cross_sizes(1500, 1400, "cross_one_cell", one_cell=True), _cross_sizes(40, 700, "cross_sparse"),
                _cross_sizes(600, 300, "cross_wild", wild=200)]
        return [_cross_unique(c) for c in out]
    return _memo("cross", make)


def cross_cfg_cases():
    """Contexts of their own: radius 49.5; max_point_match_num 1500 (the cap falls in the second round)."""
    return _memo("cross_cfg", lambda: [_cross_unique(c) for c in (
        _cross_radius(), _cross_sizes(2048, 2048, "cross_cap1500", {"max_point_match_num": 1500}),
        _cross_sizes(2048, 1100, "cross_cap1500", {"max_point_match_num": 1500}))])


def cross_frames(case, kp_cap, kl_cap):
    """PREV idx = 1000 + q, pl_obs = -1, inlier 0; CURR idx = -1: after the stage matched_pt holds the
    accepted q in t order, CURR idx[t] the written-back 1000 + q and PREV pl_obs[q] the pl of its last t.
    Rows past the counts hold the other frame's first descriptor."""
    P, C = gfpl.FrameHost(kp_cap, kl_cap), gfpl.FrameHost(kp_cap, kl_cap)
    for fh, n in ((P, case.sp), (C, case.sc)):
        fh.s.n_pt, fh.s.n_ls = n, 0
        fh.arr["pt_pl_obs"][:] = -1.0
        fh.arr["pt_idx"][:] = -1
        fh.arr["pt_inlier"][:] = 0
        fh.arr["pt_sigma2"][:] = 1.0
        for nme in ("Tfw", "DT"):
            getattr(fh.s, nme)[:] = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    if case.sc:
        P.arr["pdesc"][:] = case.dc[0]
    if case.sp:
        C.arr["pdesc"][:] = case.dp[0]
    P.arr["pt_P"][:case.sp] = case.P
    P.arr["pdesc"][:case.sp] = case.dp
    P.arr["pt_idx"][:case.sp] = 1000 + np.arange(case.sp)
    P.arr["pt_pl"][:case.sp] = 5000.0 + np.arange(case.sp)[:, None]
    C.arr["pt_pl"][:case.sc] = case.pl
    C.arr["pdesc"][:case.sc] = case.dc
    C.arr["pt_P"][:case.sc] = (0.0, 0.0, 1.0)
    return P, C


def check_cross(prev, curr, track, case):
    """[] or the differences of the state after crossFrameMatchingPoints from the statement of `case`."""
    want = case.cross()
    w = case.what() + " cross: "
    tq = np.array(want.pairs, np.int64).reshape(-1, 2)
    bad = []
    m = np.asarray(track["matched_pt"], np.int64)
    if track["n_inliers_pt"] != len(tq):
        bad.append(w + f"n_inliers_pt {track['n_inliers_pt']} want {len(tq)}")
    if not np.array_equal(m, tq[:, 1]):
        return bad + [w + f"matched_pt: {len(m)} entries, want {len(tq)}; first difference {_first_diff(m[:, None], tq[:, 1:])}"]
    e_idx = np.full(case.sc, -1, np.int64)
    e_idx[tq[:, 0]] = 1000 + tq[:, 1]
    e_obs = np.full((case.sp, 2), -1.0)
    has = want.obs_t >= 0
    e_obs[has] = case.pl[want.obs_t[has]]
    for name, got, exp in (("CURR pt_idx", curr.get("pt_idx"), e_idx), ("PREV pt_pl_obs", prev.get("pt_pl_obs"), e_obs),
                           ("PREV pt_inlier", prev.get("pt_inlier"), has.astype(np.uint8)),
                           ("PREV pt_idx", prev.get("pt_idx"), 1000 + np.arange(case.sp))):
        if not np.array_equal(got, exp):
            k = int(np.nonzero(np.asarray(got != exp).reshape(len(exp), -1).any(axis=1))[0][0])
            bad.append(w + f"{name}[{k}] = {np.asarray(got)[k].tolist()} want {np.asarray(exp)[k].tolist()}")
    return bad
