"""MapHandler::isLoopClosure + computeRelativePoseGN (src/mapHandler.cpp:3078-3545) restated in
Python: the reference the device kernel k_loop_closure is compared with, bit for bit.

numpy float64 scalars and arrays are IEEE doubles without contraction; every sum over a list is an
explicit left-to-right chain (np.add.accumulate from 0.0), never np.sum.  The pinned primitives come
from the oracle (knn2, ldlt_solve6, inverse6, eig_sym, expmap_se3, inverse_se3, sin / cos through
expmap); acos (N6), the 3x3 inverse (N7) and logmap_se3 (N8) are restated here.

The keyword arguments of is_loop_closure other than `prm` switch single rules to a plausible wrong
reading; tests/test_loop_closure_cpu.py shows each changes a result.
"""
import struct
from dataclasses import dataclass, field

import numpy as np

import oracle as O

F = np.float64
EPS = F(2.220446049250313e-16)
LC_DEFAULTS = (1.5, 0.01, 0.3, 1.5, 35.0)   # lc_res, lc_unc, lc_inl, lc_trs, lc_rot (src/config.cpp:62-66)
EXIT_BUDGET, EXIT_DE, EXIT_E, EXIT_X = 0, 1, 2, 3


def _words(x):
    u = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return u >> 32, u & 0xFFFFFFFF


def _from_words(hi, lo):
    return F(struct.unpack("<d", struct.pack("<Q", (hi << 32) | lo))[0])


def acos(x):
    """fdlibm e_acos.c (pin N6): + - * / and sqrt."""
    x = F(x)
    pi, pio2_hi, pio2_lo = F(3.14159265358979311600e+00), F(1.57079632679489655800e+00), F(6.12323399573676603587e-17)
    pS = [F(v) for v in (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01,
                         -4.00555345006794114027e-02, 7.91534994289814532176e-04, 3.47933107596021167570e-05)]
    qS = [None] + [F(v) for v in (-2.40339491173441421878e+00, 2.02094576023350569471e+00,
                                  -6.88283971605453293030e-01, 7.70381505559019352791e-02)]
    one = F(1.0)

    def pq(z):
        p = z * (pS[0] + z * (pS[1] + z * (pS[2] + z * (pS[3] + z * (pS[4] + z * pS[5])))))
        q = one + z * (qS[1] + z * (qS[2] + z * (qS[3] + z * qS[4])))
        return p, q

    hx, lx = _words(x)
    neg = hx >> 31
    ix = hx & 0x7FFFFFFF
    if ix >= 0x3FF00000:
        if ((ix - 0x3FF00000) | lx) == 0:
            return F(0.0) if not neg else pi + F(2.0) * pio2_lo
        return F(np.nan)
    if ix < 0x3FE00000:
        if ix <= 0x3C600000:
            return pio2_hi + pio2_lo
        z = x * x
        p, q = pq(z)
        r = p / q
        return pio2_hi - (x - (pio2_lo - r * x))
    if neg:
        z = (one + x) * F(0.5)
        p, q = pq(z)
        s = np.sqrt(z)
        r = p / q
        w = r * s - pio2_lo
        return pi - F(2.0) * (s + w)
    z = (one - x) * F(0.5)
    s = np.sqrt(z)
    df = _from_words(_words(s)[0], 0)
    c = (z - df * df) / (s + df)
    p, q = pq(z)
    r = p / q
    w = r * s + c
    return F(2.0) * (df + w)


def inverse3(m):
    """Matrix3d::inverse(), Eigen 3.3 size-3 path (pin N7)."""
    m = np.asarray(m, F).reshape(3, 3)
    with np.errstate(all="ignore"):
        c = np.zeros((3, 3), F)
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                c[i, j] = m[i1, j1] * m[i2, j2] - m[i1, j2] * m[i2, j1]
        det = (c[0, 0] * m[0, 0] + c[1, 0] * m[1, 0]) + c[2, 0] * m[2, 0]
        invdet = F(1.0) / det
        out = np.zeros((3, 3), F)
        for r in range(3):
            for k in range(3):
                out[r, k] = c[k, r] * invdet
    return out


def _mat3_mul(A, B):
    C = np.zeros((3, 3), F)
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return C


def _skew(v):
    z = F(0.0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], F)


def logmap_se3(T):
    """src/auxiliar.cpp:184-214 as written (pin N8)."""
    T = np.asarray(T, F).reshape(4, 4)
    with np.errstate(all="ignore"):
        R = T[:3, :3]
        Vt = T[:3, 3]
        w = np.zeros(3, F)
        V = np.eye(3, dtype=F)
        cosine = (((R[0, 0] + R[1, 1]) + R[2, 2]) - F(1.0)) / F(2.0)
        if cosine > 1.0:
            cosine = F(1.0)
        elif cosine < -1.0:
            cosine = F(-1.0)
        sine = np.sqrt(F(1.0) - cosine * cosine)
        if sine > 1.0:
            sine = F(1.0)
        elif sine < -1.0:
            sine = F(-1.0)
        theta = acos(cosine)
        if theta > 0.000001:
            two_sine = F(2.0) * sine
            w[0] = (theta * (R[2, 1] - R[1, 2])) / two_sine
            w[1] = (theta * (R[0, 2] - R[2, 0])) / two_sine
            w[2] = (theta * (R[1, 0] - R[0, 1])) / two_sine
            s = _skew(w) / theta
            ss = _mat3_mul(s, s)
            Id = np.eye(3, dtype=F)
            V = (Id + (s * (F(1.0) - cosine)) / theta) + (ss * (theta - sine)) / theta
        Vi = inverse3(V)
        x = np.zeros(6, F)
        for i in range(3):
            x[i] = (Vi[i, 0] * Vt[0] + Vi[i, 1] * Vt[1]) + Vi[i, 2] * Vt[2]
        x[3:] = w
    return x


def _mat4_mul(A, B):
    C = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return C


def _norm(v):
    s = v[0] * v[0]
    for k in range(1, len(v)):
        s = s + v[k] * v[k]
    return np.sqrt(s)


# ------------------------------------------------------------------ matching --
def mutual_pairs(d0, d1):
    """(kf0 row, kf1 row) with i21[i12[i]] == i, in kf0 row order (:3136-3166); fewer than two rows on
    either side: none (ledger U4)."""
    if len(d0) < 2 or len(d1) < 2:
        return np.zeros((0, 2), np.int32)
    rc, i12, _ = O.knn2(d0, d1, 1)
    rc2, i21, _ = O.knn2(d1, d0, 1)
    assert rc == 0 and rc2 == 0
    return np.array([(i, i12[i, 0]) for i in range(len(d0)) if i21[i12[i, 0], 0] == i], np.int32).reshape(-1, 2)


# ------------------------------------------------------------------ entries --
def _apply(T, P):
    return np.stack([((T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]) + T[i, 2] * P[:, 2]) + T[i, 3] for i in range(3)], 1)


def _proj(cam, Pc):
    return np.stack([cam.cx + (cam.fx * Pc[:, 0]) / Pc[:, 2], cam.cy + (cam.fy * Pc[:, 1]) / Pc[:, 2]], 1)


def _jac(cam, homog, g, lx, ly):
    gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
    gz2 = gz * gz
    fgz2 = cam.fx / np.where(homog < gz2, gz2, homog)   # std::max(homogTh, gz2)
    return np.stack([(fgz2 * lx) * gz,
                     (fgz2 * ly) * gz,
                     (-fgz2) * ((gx * lx) + (gy * ly)),
                     (-fgz2) * ((((gx * gy) * lx) + ((gy * gy) * ly)) + ((gz * gz) * ly)),
                     fgz2 * ((((gx * gx) * lx) + ((gz * gz) * lx)) + ((gx * gy) * ly)),
                     fgz2 * (((gx * gz) * ly) - ((gy * gz) * lx))], 1)


def point_err(cam, T, P, obs):
    Pc = _apply(T, P)
    d = _proj(cam, Pc) - obs
    return Pc, d, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def line_err(cam, T, sP, eP, le):
    sc, ec = _apply(T, sP), _apply(T, eP)
    su, eu = _proj(cam, sc), _proj(cam, ec)
    e0 = (le[:, 0] * su[:, 0] + le[:, 1] * su[:, 1]) + le[:, 2]
    e1 = (le[:, 0] * eu[:, 0] + le[:, 1] * eu[:, 1]) + le[:, 2]
    return sc, ec, e0, e1, np.sqrt(e0 * e0 + e1 * e1)


def _rows(J, nrm, homog, s2):
    d = np.where(homog < nrm, nrm, homog)
    J = J / d[:, None]
    w = F(1.0) / (F(1.0) + (nrm * nrm) * s2)
    return J, nrm, w


def _chain(v, pairwise=False):
    """0.0 + v[0] + v[1] + ... left to right (the reference's += over the list)."""
    if pairwise:
        return F(np.sum(v)) if len(v) else F(0.0)
    return np.add.accumulate(np.concatenate([np.zeros(1, F), v]))[-1]


def _sums(J, nrm, w, pairwise):
    H = np.zeros((6, 6), F)
    g = np.zeros(6, F)
    for i in range(6):
        for k in range(6):
            H[i, k] = _chain((J[:, i] * J[:, k]) * w, pairwise)
        g[i] = _chain((J[:, i] * nrm) * w, pairwise)
    return H, g, _chain((nrm * nrm) * w, pairwise)


@dataclass
class LoopResult:
    is_lc: int = 0
    gates: int = 0
    n_pt: int = 0
    n_ls: int = 0
    n_pt_inl: int = 0
    n_ls_inl: int = 0
    iters: int = 0
    e: float = 0.0
    unc: float = 0.0
    ratio_inliers: float = 0.0
    trs: float = 0.0
    rot: float = 0.0
    x_inc: np.ndarray = field(default_factory=lambda: np.zeros(6))
    pose_inc: np.ndarray = field(default_factory=lambda: np.zeros(6))
    T_inc: np.ndarray = field(default_factory=lambda: np.eye(4))
    # the reference only (not in gfpl_loop_result)
    exit: int = EXIT_BUDGET
    pt_pairs: np.ndarray = None
    ls_pairs: np.ndarray = None
    pt_inlier: np.ndarray = None
    ls_inlier: np.ndarray = None


def is_loop_closure(cam, cfg, f0, f1, prm=LC_DEFAULTS, stereo_sigma2=False, pairwise=False, outlier_ge=False,
                    budget_ref=False):
    """f0 / f1: gfpl.FrameHost of kf0 / kf1 (their stereo_pt / stereo_ls rows)."""
    A0, A1 = f0.arr, f1.arr
    pp = mutual_pairs(A0["pdesc"][:f0.n_pt], A1["pdesc"][:f1.n_pt])
    lp = mutual_pairs(A0["ldesc"][:f0.n_ls], A1["ldesc"][:f1.n_ls])
    P = np.asarray(A0["pt_P"], F)[pp[:, 0]].reshape(-1, 3)
    obs = np.asarray(A1["pt_pl"], F)[pp[:, 1]].reshape(-1, 2)
    sP = np.asarray(A0["ls_sP"], F)[lp[:, 0]].reshape(-1, 3)
    eP = np.asarray(A0["ls_eP"], F)[lp[:, 0]].reshape(-1, 3)
    le = np.asarray(A1["ls_le"], F)[lp[:, 1]].reshape(-1, 3)
    # the (P, pl_obs) / (sP, eP, le_obs, ...) constructors leave sigma2 at the class default 1.0
    s2p = np.asarray(A0["pt_sigma2"], F)[pp[:, 0]] if stereo_sigma2 else np.ones(len(pp), F)
    s2l = np.asarray(A0["ls_sigma2"], F)[lp[:, 0]] if stereo_sigma2 else np.ones(len(lp), F)
    homog = F(cfg.homog_th)
    n_p, n_l = len(pp), len(lp)
    r = LoopResult(n_pt=n_p, n_ls=n_l, pt_pairs=pp, ls_pairs=lp)
    T = np.eye(4, dtype=F)
    H = np.zeros((6, 6), F)
    e = F(0.0)
    err_prev = F(999999999.9)
    with np.errstate(all="ignore"):
        for it in range(cfg.max_iters_ref if budget_ref else cfg.max_iters):
            Pc, d, nrm = point_err(cam, T, P, obs)
            Jp, np_, wp = _rows(_jac(cam, homog, Pc, d[:, 0], d[:, 1]), nrm, homog, s2p)
            H_p, g_p, e_p = _sums(Jp, np_, wp, pairwise)
            sc, ec, e0, e1, nrm = line_err(cam, T, sP, eP, le)
            Js, Je = _jac(cam, homog, sc, le[:, 0], le[:, 1]), _jac(cam, homog, ec, le[:, 0], le[:, 1])
            Jl, nl_, wl = _rows(Js * e0[:, None] + Je * e1[:, None], nrm, homog, s2l)
            H_l, g_l, e_l = _sums(Jl, nl_, wl, pairwise)
            H = H_p + H_l
            g = g_p + g_l
            e = (e_p + e_l) / F(n_l + n_p)
            r.iters = it + 1
            if abs(e - err_prev) < EPS:
                r.exit = EXIT_DE
                break
            if e < EPS:
                r.exit = EXIT_E
                break
            x = O.ldlt_solve6(H, g)
            T = _mat4_mul(T, O.inverse_se3(O.expmap_se3(x)))
            if _norm(x) < EPS:
                r.exit = EXIT_X
                break
            err_prev = e
        x_inc = logmap_se3(T)
        chi = np.sqrt(F(7.815))
        _, _, nrm = point_err(cam, T, P, obs)
        v = nrm * np.sqrt(s2p)
        r.pt_inlier = (~((v >= chi) if outlier_ge else (v > chi))).astype(np.uint8)
        _, _, _, _, nrm = line_err(cam, T, sP, eP, le)
        v = nrm * np.sqrt(s2l)
        r.ls_inlier = (~((v >= chi) if outlier_ge else (v > chi))).astype(np.uint8)
        r.n_pt_inl, r.n_ls_inl = int(r.pt_inlier.sum()), int(r.ls_inlier.sum())
        r.e = e
        r.unc = O.eig_sym(O.inverse6(H))[5]
        r.ratio_inliers = F(r.n_pt_inl + r.n_ls_inl) / F(n_p + n_l)
        r.trs = _norm(x_inc[:3])
        r.rot = (_norm(x_inc[3:]) * F(180.0)) / F(3.1415926535897932384626433832795)
        g5 = [r.e < prm[0], r.unc < prm[1], r.ratio_inliers > prm[2], r.trs < prm[3], r.rot < prm[4]]
        r.gates = sum(1 << i for i, ok in enumerate(g5) if ok)
        r.is_lc = int(r.gates == 31)
        r.x_inc, r.T_inc = x_inc, T
        if r.is_lc:
            r.pose_inc = logmap_se3(O.inverse_se3(T))
    return r
