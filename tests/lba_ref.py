"""MapHandler::levMarquardtOptimizationLBA (src/mapHandler.cpp:1217-1713) restated in Python: the
reference the device kernel k_lba is compared with, bit for bit.

numpy float64 arrays are IEEE doubles without contraction.  The linearisation is evaluated for all
observations at once, element by element in the reference's association; H is DENSE, N x N, and every
entry is accumulated with np.add.at over observation-ordered contributions, which adds them one by one
in list order exactly as the reference's `H.block(...) +=` does (test_lba_cpu.py checks that against
an explicit loop).  expmap_se3 / inverse_se3 / inverse6 are the oracle's, logmap_se3 / inverse3 come
from tests/loop_closure_ref.py.

Two solvers take the damped dense H:
  solve_pinned  the elimination the device runs (DESIGN.md ledger BA12): landmark blocks inverted
                (inverse3 / inverse6), S = U - sum_j W_j V_j^-1 W_j^T over the landmarks in ascending
                order, LDL^T of S's lower triangle without pivoting, back-substitution;
  solve_dense   numpy.linalg.solve, the stand-in for the reference's SimplicialLDLT (the same direct
                solve in exact arithmetic).

The keyword arguments of lba() other than `prm` and `solver` switch single rules to a plausible wrong
reading; tests/test_lba_cpu.py shows each changes a result.
"""
from dataclasses import dataclass, field

import numpy as np

import oracle as O
import loop_closure_ref as LR

F = np.float64
EPS = F(2.220446049250313e-16)
LBA_DEFAULTS = (0.001, 10.0, 20)   # lambdaLbaLM, lambdaLbaK, maxItersLba (src/config.cpp:55-57)
STOP_ITERS, STOP_DERR, STOP_ERR, STOP_STEP = 0, 1, 2, 3
SINGULAR, HMAX_RANGE = 1, 2


# ------------------------------------------------------------ linearisation --
def _apply(Ti, P):
    return np.stack([((Ti[:, i, 0] * P[:, 0] + Ti[:, i, 1] * P[:, 1]) + Ti[:, i, 2] * P[:, 2]) + Ti[:, i, 3]
                     for i in range(3)], 1)


def _proj(cam, Pc):
    return np.stack([cam.cx + (cam.fx * Pc[:, 0]) / Pc[:, 2], cam.cy + (cam.fy * Pc[:, 1]) / Pc[:, 2]], 1)


def _max(th, v):
    return np.where(th < v, v, th)   # std::max(th, v)


def _jac(cam, th, g, ex, ey):
    """:1277-1282 — the landmark's three terms (:1286-1288) are the first three"""
    gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
    gz2 = F(1.0) / _max(th, gz * gz)
    a, b = cam.fx * ex, cam.fy * ey
    return np.stack([(gz2 * a) * gz,
                     (gz2 * b) * gz,
                     (-gz2) * (a * gx + b * gy),
                     (-gz2) * (((a * gx) * gy + (b * gy) * gy) + (b * gz) * gz),
                     gz2 * (((a * gx) * gx + (a * gz) * gz) + (b * gx) * gy),
                     gz2 * ((b * gx) * gz - (a * gy) * gz)], 1)


def _jtr(J, Ti):
    return np.stack([(J[:, 0] * Ti[:, 0, j] + J[:, 1] * Ti[:, 1, j]) + J[:, 2] * Ti[:, 2, j] for j in range(3)], 1)


def point_rows(cam, th, Ti, Xw, obs, s2):
    """per point observation: J_pose [n][6], J_landmark [n][3], |err|, w (:1252-1293)"""
    Xc = _apply(Ti, Xw)
    d = obs - _proj(cam, Xc)
    nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    J = _jac(cam, th, Xc, d[:, 0], d[:, 1])
    den = _max(th, nrm)
    return J / den[:, None], _jtr(J, Ti) / den[:, None], nrm, F(1.0) / (F(1.0) + (nrm * nrm) * s2)


def line_rows(cam, th, Ti, PQ, l, s2):
    """per line observation: J_pose [n][6], J_landmark [n][6], |err|, w (:1331-1402)"""
    Pc, Qc = _apply(Ti, PQ[:, :3]), _apply(Ti, PQ[:, 3:])
    pu, qu = _proj(cam, Pc), _proj(cam, Qc)
    e0 = (l[:, 0] * pu[:, 0] + l[:, 1] * pu[:, 1]) + l[:, 2]
    e1 = (l[:, 0] * qu[:, 0] + l[:, 1] * qu[:, 1]) + l[:, 2]
    nrm = np.sqrt(e0 * e0 + e1 * e1)
    JP, JQ = _jac(cam, th, Pc, e0, e1), _jac(cam, th, Qc, e0, e1)
    den = _max(th, nrm)
    JT = (JP * e0[:, None] + JQ * e1[:, None]) / den[:, None]
    JL = np.concatenate([(_jtr(JP, Ti) * e0[:, None]) / den[:, None], (_jtr(JQ, Ti) * e1[:, None]) / den[:, None]], 1)
    return JT, JL, nrm, F(1.0) / (F(1.0) + (nrm * nrm) * s2)


def _chain(v):
    """0.0 + v[0] + v[1] + ... left to right"""
    return np.add.accumulate(np.concatenate([np.zeros(1, F), np.asarray(v, F)]))[-1]


def accumulate(H, g, N, JT, JL, nrm, w, kf, jdx):
    """the reference's `+=` of one observation list (:1295-1315 / :1404-1424) onto dense H and g, in
    list order; kf: slot per observation (< 0: fixed), jdx: first row of the observation's landmark.
    Returns the list's err terms (|err| |err|) w."""
    n, D = JL.shape
    Hf = H.reshape(-1)
    r = jdx[:, None] + np.arange(D)[None, :]                                   # [n][D] landmark rows
    np.add.at(g, r.reshape(-1), ((JL * nrm[:, None]) * w[:, None]).reshape(-1))
    np.add.at(Hf, (r[:, :, None] * N + r[:, None, :]).reshape(-1),
              ((JL[:, :, None] * JL[:, None, :]) * w[:, None, None]).reshape(-1))
    loc = kf >= 0
    if loc.any():
        JTl, JLl, nl, wl = JT[loc], JL[loc], nrm[loc], w[loc]
        c = (6 * kf[loc])[:, None] + np.arange(6)[None, :]                     # [m][6] pose rows
        rl = r[loc]
        np.add.at(g, c.reshape(-1), ((JTl * nl[:, None]) * wl[:, None]).reshape(-1))
        np.add.at(Hf, (c[:, :, None] * N + c[:, None, :]).reshape(-1),
                  ((JTl[:, :, None] * JTl[:, None, :]) * wl[:, None, None]).reshape(-1))
        Haux = ((JLl[:, :, None] * JTl[:, None, :]) * wl[:, None, None]).reshape(-1)   # [m][D][6]
        np.add.at(Hf, (rl[:, :, None] * N + c[:, None, :]).reshape(-1), Haux)
        np.add.at(Hf, (rl[:, :, None] + c[:, None, :] * N).reshape(-1), Haux)
    return (nrm * nrm) * w


# ------------------------------------------------------------------ solvers --
@dataclass
class Layout:
    nkf: int
    npt: int
    nls: int
    masks: list          # per landmark (points first): ascending local keyframes that observe it

    @property
    def N(self):
        return 6 * self.nkf + 3 * self.npt + 6 * self.nls

    def lm(self, j):
        """(first row, rows) of landmark j"""
        if j < self.npt:
            return 6 * self.nkf + 3 * j, 3
        return 6 * self.nkf + 3 * self.npt + 6 * (j - self.npt), 6


def layout_of(a):
    nkf, npt, nls = len(a["x_kf"]), len(a["pt"]), len(a["ls"])
    masks = [set() for _ in range(npt + nls)]
    for lm, kf, off in ((a["pt_obs_lm"], a["pt_obs_kf"], 0), (a["ls_obs_lm"], a["ls_obs_kf"], npt)):
        for j, s in zip(lm, kf):
            if s >= 0:
                masks[off + int(j)].add(int(s))
    return Layout(nkf, npt, nls, [sorted(m) for m in masks])


def _finite(x):
    return bool(np.all(np.isfinite(x)))


def _matmul_seq(A, B):
    """A [D][D] times B [D][k]: each entry A[p,0] B[0,c] + A[p,1] B[1,c] + ... left to right"""
    Y = A[:, 0:1] * B[0:1, :]
    for q in range(1, A.shape[1]):
        Y = Y + A[:, q:q + 1] * B[q:q + 1, :]
    return Y


def ldlt_nopivot(S):
    """LDL^T of the lower triangle of S without pivoting: L (unit lower), D, ok.  Column k:
    v_i = S[i,k] - sum_{m<k} (L[i,m] L[k,m]) D[m] with m ascending; a pivot that is not positive and
    finite stops it."""
    n = S.shape[0]
    Lm, D = np.zeros((n, n), F), np.zeros(n, F)
    for k in range(n):
        v = S[k:, k].copy()
        for m in range(k):
            v = v - (Lm[k:, m] * Lm[k, m]) * D[m]
        if not (v[0] > 0.0 and np.isfinite(v[0])):
            return Lm, D, False
        D[k] = v[0]
        Lm[k, k] = F(1.0)
        Lm[k + 1:, k] = v[1:] / v[0]
    return Lm, D, True


def ldlt_solve(Lm, D, b):
    n = len(b)
    y = np.array(b, F)
    for m in range(n):
        y[m + 1:] = y[m + 1:] - Lm[m + 1:, m] * y[m]
    y = y / D
    for m in range(n - 1, 0, -1):
        y[:m] = y[:m] - Lm[m, :m] * y[m]
    return y


def solve_pinned(Hd, g, lay):
    """(DX, ok, |DX|^2) of the damped dense system by the device's elimination"""
    nkf, n6, nlm = lay.nkf, 6 * lay.nkf, lay.npt + lay.nls
    with np.errstate(all="ignore"):
        Vi, z, W, Y = [], [], [], []
        ok = True
        for j in range(nlm):
            r0, D = lay.lm(j)
            V = Hd[r0:r0 + D, r0:r0 + D]
            dg = np.diag(V)
            ok = ok and bool(np.all(dg > 0.0)) and _finite(dg)
            inv = LR.inverse3(V) if D == 3 else O.inverse6(V)
            ok = ok and _finite(inv)
            Vi.append(inv)
            z.append(_matmul_seq(inv, g[r0:r0 + D, None])[:, 0])
            W.append({s: Hd[r0:r0 + D, 6 * s:6 * s + 6].copy() for s in lay.masks[j]})
            Y.append({s: _matmul_seq(inv, W[j][s]) for s in lay.masks[j]})
        if not ok:
            return np.zeros(lay.N, F), False, F(0.0)
        S = np.zeros((n6, n6), F)
        gr = np.array(g[:n6], F)
        for s in range(nkf):
            S[6 * s:6 * s + 6, 6 * s:6 * s + 6] = Hd[6 * s:6 * s + 6, 6 * s:6 * s + 6]
        for j in range(nlm):
            for sa in lay.masks[j]:
                Wa = W[j][sa]                                     # [D][6]
                gr[6 * sa:6 * sa + 6] = gr[6 * sa:6 * sa + 6] - _matmul_seq(Wa.T, z[j][:, None])[:, 0]
                for sb in lay.masks[j]:
                    if sb > sa:
                        continue
                    blk = S[6 * sa:6 * sa + 6, 6 * sb:6 * sb + 6]
                    blk -= _matmul_seq(Wa.T, Y[j][sb])
        Lm, Dg, ok = ldlt_nopivot(S)
        if not ok:
            return np.zeros(lay.N, F), False, F(0.0)
        DX = np.zeros(lay.N, F)
        DX[:n6] = ldlt_solve(Lm, Dg, gr)
        n2 = _chain(DX[:n6] * DX[:n6])
        for j in range(nlm):
            r0, D = lay.lm(j)
            u = np.array(g[r0:r0 + D], F)
            for s in lay.masks[j]:
                for k in range(6):
                    u = u - W[j][s][:, k] * DX[6 * s + k]
            dj = _matmul_seq(Vi[j], u[:, None])[:, 0]
            DX[r0:r0 + D] = dj
            q = dj[0] * dj[0]
            for p in range(1, D):
                q = q + dj[p] * dj[p]
            n2 = n2 + q
    return DX, True, n2


def solve_dense(Hd, g, lay):
    """numpy.linalg.solve on the damped H (SimplicialLDLT's stand-in)"""
    try:
        with np.errstate(all="ignore"):
            DX = np.linalg.solve(Hd, g)
    except np.linalg.LinAlgError:
        return np.zeros(lay.N, F), False, F(0.0)
    if not _finite(DX):
        return np.zeros(lay.N, F), False, F(0.0)
    return DX, True, _chain(DX * DX)


# ----------------------------------------------------------------- the loop --
@dataclass
class LbaRef:
    iters: int = 1
    stop: int = STOP_ITERS
    status: int = 0
    hmax: int = 0
    lambda_: float = 0.0
    err: float = 0.0
    err_prev: float = 999999999.9
    X: np.ndarray = None
    T_kf: np.ndarray = None
    pt: np.ndarray = None
    ls: np.ndarray = None
    rejected: int = 0                              # iterations that took err > err_prev
    systems: list = field(default_factory=list)    # per evaluated iteration (keep=True): dict H, g, err, lambda, DX


def _inv_poses(Ts):
    return np.array([O.inverse_se3(T) for T in Ts], F).reshape(-1, 4, 4)


def build_system(cam, homog, a, lay, X, it, lines_read_x=False):
    """dense undamped H, g and the err sum of iteration `it` (0: the pre-pass, :1237-1426; else :1460-1649)"""
    nkf, npt = lay.nkf, lay.npt
    N = lay.N
    H, g = np.zeros((N, N), F), np.zeros(N, F)
    Ti_in = _inv_poses(a["T_kf"]) if nkf else np.zeros((0, 4, 4))
    Ti_fix = _inv_poses(a["T_fix"]) if len(a["T_fix"]) else np.zeros((0, 4, 4))
    Ti_x = _inv_poses([O.expmap_se3(X[6 * s:6 * s + 6]) for s in range(nkf)]) if it > 0 else Ti_in

    def poses(kf, local):
        out = np.zeros((len(kf), 4, 4), F)
        for o, s in enumerate(kf):
            out[o] = local[s] if s >= 0 else Ti_fix[-1 - s]
        return out

    terms = []
    with np.errstate(all="ignore"):
        if len(a["pt_obs_lm"]):
            lm, kf = a["pt_obs_lm"].astype(np.int64), a["pt_obs_kf"].astype(np.int64)
            Xw = (X[6 * nkf:6 * nkf + 3 * npt].reshape(-1, 3) if it > 0 else a["pt"])[lm]
            JT, JL, nrm, w = point_rows(cam, F(homog), poses(kf, Ti_x), Xw, a["pt_obs"], a["pt_sigma"][:, 0])
            terms.append(accumulate(H, g, N, JT, JL, nrm, w, kf, 6 * nkf + 3 * lm))
        if len(a["ls_obs_lm"]):
            lm, kf = a["ls_obs_lm"].astype(np.int64), a["ls_obs_kf"].astype(np.int64)
            # the iterations read map_lines[..]->line3D and T_kf_w, not X, with 1e-7 for homogTh (:1555-1618)
            rx = lines_read_x and it > 0
            PQ = (X[6 * nkf + 3 * npt:].reshape(-1, 6) if rx else a["ls"])[lm]
            th = F(homog) if it == 0 else F(0.0000001)
            JT, JL, nrm, w = line_rows(cam, th, poses(kf, Ti_x if rx else Ti_in), PQ, a["ls_obs"], a["ls_sigma"][:, 0])
            terms.append(accumulate(H, g, N, JT, JL, nrm, w, kf, 6 * nkf + 3 * npt + 6 * lm))
        # err is ONE running sum over both lists, points first
        err = _chain(np.concatenate(terms)) if terms else F(0.0)
    return H, g, err


def lba(cam, homog, a, prm=LBA_DEFAULTS, solver=solve_pinned, keep=False, lines_read_x=False, hmax_double=False,
        finite_first=False, apply_on_reject=False, divisor_obs=False, x_from_T=False):
    """a: the arrays of a gfpl.LbaProblem (its .a).  Returns LbaRef."""
    lam0, lam_k, max_iters = F(prm[0]), F(prm[1]), int(prm[2])
    lay = layout_of(a)
    nkf, npt, nls, N = lay.nkf, lay.npt, lay.nls, lay.N
    n6 = 6 * nkf
    x0 = np.array([LR.logmap_se3(T) for T in a["T_kf"]], F).reshape(-1) if x_from_T else a["x_kf"].reshape(-1)
    X = np.concatenate([x0, a["pt"].reshape(-1), a["ls"].reshape(-1)]).astype(F)
    r = LbaRef(lambda_=lam0)
    nobs = len(a["pt_obs_lm"]) + len(a["ls_obs_lm"])
    with np.errstate(all="ignore"):
        it = 0
        while True:
            H, g, esum = build_system(cam, homog, a, lay, X, it, lines_read_x)
            if it == 0:
                # err /= (Npt_obs + Nls_obs): both counters are 0 for good (:1240, :1319, :1427)
                err = esum / F(nobs) if finite_first else esum / F(0.0)
                dg = np.diag(H)
                if hmax_double:
                    hmax = F(np.max(np.abs(dg[~np.isnan(dg)]))) if len(dg) else F(0.0)
                else:
                    hmax = 0                                   # int Hmax = 0.0 (:1429-1434)
                    for d in dg:
                        if d > hmax or d < -hmax:
                            v = abs(d)
                            if not (v < 2147483648.0):         # (int) of it is undefined behaviour
                                r.status |= HMAX_RANGE
                                r.hmax = 0x7FFFFFFF
                                r.err = err
                                r.X, r.T_kf, r.pt, r.ls = X, a["T_kf"].reshape(-1, 4, 4).copy(), a["pt"].copy(), a["ls"].copy()
                                return r
                            hmax = int(v)
                r.hmax = int(hmax)
                r.lambda_ = lam0 * F(hmax)
            else:
                err = esum / F(nobs if divisor_obs else npt + nls)
                r.iters = it
            r.err = err
            if keep:
                r.systems.append(dict(H=H, g=g.copy(), err=err, lambda_=r.lambda_))
            if it > 0:
                if abs(err - r.err_prev) < EPS:
                    r.stop = STOP_DERR
                    break
                if err < EPS:
                    r.stop = STOP_ERR
                    break
            lam = r.lambda_
            Hd = H.copy()
            di = np.arange(N)
            Hd[di, di] = Hd[di, di] + lam * Hd[di, di]          # H(i,i) += lambda * H(i,i)
            DX, ok, n2 = solver(Hd, g, lay)
            if keep:
                r.systems[-1].update(Hd=Hd, DX=DX.copy(), ok=ok)
            accept = True
            if it > 0:
                if err > r.err_prev:
                    r.lambda_ = lam / lam_k
                    r.rejected += 1
                    accept = bool(apply_on_reject)
                else:
                    r.lambda_ = lam * lam_k
            if not ok:                                          # ledger BA13: DX = 0, the update skipped
                accept = False
                r.status |= SINGULAR
                n2 = F(0.0)
            if accept:
                for s in range(nkf):
                    Tc = LR._mat4_mul(O.expmap_se3(X[6 * s:6 * s + 6]), O.inverse_se3(O.expmap_se3(DX[6 * s:6 * s + 6])))
                    X[6 * s:6 * s + 6] = LR.logmap_se3(Tc)
                X[n6:] = X[n6:] + DX[n6:]
            if it > 0 and np.sqrt(n2) < EPS:
                r.stop = STOP_STEP
                r.iters = it
                break
            r.err_prev = err
            r.iters = it + 1
            if it + 1 >= max_iters:
                break
            it += 1
        r.X = X
        r.T_kf = np.array([O.expmap_se3(X[6 * s:6 * s + 6]) for s in range(nkf)], F).reshape(-1, 4, 4)
        r.pt = X[n6:n6 + 3 * npt].reshape(-1, 3).copy()
        r.ls = X[n6 + 3 * npt:].reshape(-1, 6).copy()
    return r


def blocks_of(H, g, lay):
    """the debug hook's view of a dense system: U, V_pt, V_ls, W_pt, W_ls (landmark rows, pose columns)"""
    nkf, npt, nls = lay.nkf, lay.npt, lay.nls
    U = np.array([H[6 * s:6 * s + 6, 6 * s:6 * s + 6] for s in range(nkf)], F).reshape(nkf, 6, 6)
    V_pt, V_ls = np.zeros((npt, 3, 3), F), np.zeros((nls, 6, 6), F)
    W_pt, W_ls = np.zeros((npt, nkf, 3, 6), F), np.zeros((nls, nkf, 6, 6), F)
    for j in range(npt + nls):
        r0, D = lay.lm(j)
        (V_pt if D == 3 else V_ls)[j if D == 3 else j - npt] = H[r0:r0 + D, r0:r0 + D]
        for s in range(nkf):
            (W_pt if D == 3 else W_ls)[j if D == 3 else j - npt, s] = H[r0:r0 + D, 6 * s:6 * s + 6]
    return dict(U=U, g=g.copy(), V_pt=V_pt, V_ls=V_ls, W_pt=W_pt, W_ls=W_ls)
