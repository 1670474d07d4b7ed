"""MapHandler::levMarquardtOptimizationGBA (src/mapHandler.cpp:1950-2544) restated in Python: the
reference the device kernels of k_gba.hip are compared with, bit for bit (DESIGN.md ledger GB1-GB12).

The linearisation (point_rows / line_rows), the dense N x N H with np.add.at in list order and the
helpers are tests/lba_ref.py's: the GBA's text has the same Jacobian forms and the same `+=` order.
What differs from the LBA is gathered in Rules, one field per rule, so that tests/test_gba_cpu.py can
switch each to the LBA's (or another plausible) reading and show that a result changes:

  divisor_zero       every iteration divides err by Npt_obs + Nls_obs, both 0 for good (:2479); the
                     LBA's iterations divide by Npt + Nls
  line_th_homog      the line terms of the iterations keep Config::homogTh() (:2386); the LBA has 1e-7
  prepass_transposed the pre-pass writes a line's coupling block transposed: H(jdx+j, idx+i) += Hij(i,j)
                     with Hij = Jij_Lwj Jij_Tiw^T (:2188-2198)
  lower_triangle     SimplicialLDLT reads the lower triangle of H as written
  any_sign_pivot     a pivot of the reduced system is accepted when finite and non-zero
  err_start          the value the uninitialised `err` (:1964) is pinned to before the pre-pass
  x_from_T           X starts from logmap(T_kf_w) instead of x_kf_w (a wrong reading)
  explicit_inverse   the landmark blocks through inverse3 / inverse6 as in the LBA's pin (BA12) instead of
                     their own LDL^T and substitutions (GB11)

H is built with BOTH triangles exactly as the reference writes them (the iterations write a line's
upper block wrongly, :2472), so the debug hook can be compared against it; the solve reads the lower.
"""
from dataclasses import dataclass, field, replace

import numpy as np

import oracle as O
import loop_closure_ref as LR
import lba_ref as R

F = np.float64
EPS = R.EPS
GBA_DEFAULTS = R.LBA_DEFAULTS      # the GBA reads lambdaLbaLM, lambdaLbaK, maxItersLba too (:1965-1966)
STOP_ITERS, STOP_DERR, STOP_ERR, STOP_STEP = 0, 1, 2, 3
SINGULAR, HMAX_RANGE, INDEFINITE = 1, 2, 4


@dataclass(frozen=True)
class Rules:
    divisor_zero: bool = True
    line_th_homog: bool = True
    prepass_transposed: bool = True
    lower_triangle: bool = True
    any_sign_pivot: bool = True
    err_start: float = 0.0
    x_from_T: bool = False
    explicit_inverse: bool = False


GBA_RULES = Rules()


def accumulate(H, g, N, JT, JL, nrm, w, kf, jdx, coupling):
    """one observation list onto dense H and g in list order (:2023-2074, :2162-2201, :2301-2352,
    :2437-2476).  coupling: 'point' (both triangles right), 'line0' (the pre-pass: both triangles hold
    Hij(i,j) at (idx+i, jdx+j) and (jdx+j, idx+i)), 'line' (the iterations: the lower block right, the
    upper as the pre-pass writes it).  Returns the list's err terms."""
    n, D = JL.shape
    Hf = H.reshape(-1)
    r = jdx[:, None] + np.arange(D)[None, :]
    np.add.at(g, r.reshape(-1), ((JL * nrm[:, None]) * w[:, None]).reshape(-1))
    np.add.at(Hf, (r[:, :, None] * N + r[:, None, :]).reshape(-1),
              ((JL[:, :, None] * JL[:, None, :]) * w[:, None, None]).reshape(-1))
    loc = kf >= 0
    if loc.any():
        JTl, JLl, nl, wl = JT[loc], JL[loc], nrm[loc], w[loc]
        c = (6 * kf[loc])[:, None] + np.arange(6)[None, :]
        rl = r[loc]
        np.add.at(g, c.reshape(-1), ((JTl * nl[:, None]) * wl[:, None]).reshape(-1))
        np.add.at(Hf, (c[:, :, None] * N + c[:, None, :]).reshape(-1),
                  ((JTl[:, :, None] * JTl[:, None, :]) * wl[:, None, None]).reshape(-1))
        Hij = (JLl[:, :, None] * JTl[:, None, :]) * wl[:, None, None]          # [m][D][6]: Hij(i,j) = JL_i JT_j w
        if coupling == "point":
            np.add.at(Hf, (rl[:, :, None] * N + c[:, None, :]).reshape(-1), Hij.reshape(-1))       # H(jdx+i, idx+j)
            np.add.at(Hf, (rl[:, :, None] + c[:, None, :] * N).reshape(-1), Hij.reshape(-1))       # H(idx+j, jdx+i)
        else:
            # H(idx+i, jdx+j) += Hij(i,j): row c_i, column r_j (D = 6)
            np.add.at(Hf, (c[:, :, None] * N + rl[:, None, :]).reshape(-1), Hij.reshape(-1))
            if coupling == "line0":
                # H(jdx+j, idx+i) += Hij(i,j): row r_j, column c_i
                np.add.at(Hf, (c[:, :, None] + rl[:, None, :] * N).reshape(-1), Hij.reshape(-1))
            else:
                # H(jdx+j, idx+i) += Hij(j,i): row r_j, column c_i takes JL_j JT_i w
                np.add.at(Hf, (rl[:, :, None] * N + c[:, None, :]).reshape(-1), Hij.reshape(-1))
    return (nrm * nrm) * w


def build_system(cam, homog, a, lay, X, it, rules=GBA_RULES):
    """dense undamped H (both triangles as written), g and the err sum of iteration `it`
    (0: the pre-pass, :1970-2203; else :2240-2478)"""
    nkf, npt = lay.nkf, lay.npt
    N = lay.N
    H, g = np.zeros((N, N), F), np.zeros(N, F)
    Ti_in = R._inv_poses(a["T_kf"]) if nkf else np.zeros((0, 4, 4))
    Ti_fix = R._inv_poses(a["T_fix"]) if len(a["T_fix"]) else np.zeros((0, 4, 4))
    Ti_x = R._inv_poses([O.expmap_se3(X[6 * s:6 * s + 6]) for s in range(nkf)]) if it > 0 else Ti_in

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
            JT, JL, nrm, w = R.point_rows(cam, F(homog), poses(kf, Ti_x), Xw, a["pt_obs"], a["pt_sigma"][:, 0])
            terms.append(accumulate(H, g, N, JT, JL, nrm, w, kf, 6 * nkf + 3 * lm, "point"))
        if len(a["ls_obs_lm"]):
            lm, kf = a["ls_obs_lm"].astype(np.int64), a["ls_obs_kf"].astype(np.int64)
            # every line term reads map_lines[..]->line3D and T_kf_w, never X (:2091-2094, :2366-2369)
            th = F(homog) if (it == 0 or rules.line_th_homog) else F(0.0000001)
            JT, JL, nrm, w = R.line_rows(cam, th, poses(kf, Ti_in), a["ls"][lm], a["ls_obs"], a["ls_sigma"][:, 0])
            mode = "line0" if it == 0 and rules.prepass_transposed else "line"
            terms.append(accumulate(H, g, N, JT, JL, nrm, w, kf, 6 * nkf + 3 * npt + 6 * lm, mode))
        err = R._chain(np.concatenate(terms)) if terms else F(0.0)
    return H, g, err


def ldlt_any_sign(S, any_sign=True):
    """LDL^T of the lower triangle of S without pivoting, as lba_ref.ldlt_nopivot, but a pivot is
    accepted when it is finite and non-zero (SimplicialLDLT does not need positive pivots).  Returns
    L, D, ok, negative (the number of negative pivots accepted before it stopped)."""
    n = S.shape[0]
    Lm, D = np.zeros((n, n), F), np.zeros(n, F)
    neg = 0
    for k in range(n):
        v = S[k:, k].copy()
        for m in range(k):
            v = v - (Lm[k:, m] * Lm[k, m]) * D[m]
        good = np.isfinite(v[0]) and (v[0] != 0.0 if any_sign else v[0] > 0.0)
        if not good:
            return Lm, D, False, neg
        if v[0] < 0.0:
            neg += 1
        D[k] = v[0]
        Lm[k, k] = F(1.0)
        Lm[k + 1:, k] = v[1:] / v[0]
    return Lm, D, True, neg


def block_ldlt(V):
    """LDL^T of a landmark's damped D x D block (its lower triangle) without pivoting, in
    ldlt_any_sign's order; every pivot must be positive and finite.  Returns (L, d, ok)."""
    Lm, d, ok, _ = ldlt_any_sign(np.array(V, F), any_sign=False)
    return Lm, d, ok


def block_solve(Lm, d, B):
    """V^-1 B for B [D][k] from the block's factor: forward, diagonal and backward substitution, each
    row's terms in index order (lba_ref.ldlt_solve's orders, a column of B at a time)"""
    n = len(d)
    y = np.array(B, F)
    for m in range(n):
        y[m + 1:] = y[m + 1:] - Lm[m + 1:, m:m + 1] * y[m:m + 1]
    y = y / d[:, None]
    for m in range(n - 1, 0, -1):
        y[:m] = y[:m] - Lm[m, :m][:, None] * y[m:m + 1]
    return y


def solve_pinned(Hd, g, lay, rules=GBA_RULES):
    """(DX, ok, |DX|^2, negative pivots) of the damped system by the device's elimination (ledger
    GB11): lba_ref.solve_pinned's orders, the blocks read from the lower triangle of H as written.
    A landmark's block is FACTORISED (block_ldlt) and z_j, Y_j, DX_j come from substitutions, not from
    an explicit inverse3 / inverse6 as in the LBA: with every step applied (GB3) a run can reach blocks
    of condition 1e7 and beyond, where products with an explicit inverse lose the backward-error bound
    (rules.explicit_inverse shows it)."""
    Hl = Hd if rules.lower_triangle else Hd.T
    nkf, n6, nlm = lay.nkf, 6 * lay.nkf, lay.npt + lay.nls
    zero = (np.zeros(lay.N, F), False, F(0.0), 0)
    with np.errstate(all="ignore"):
        Vi, z, W, Y = [], [], [], []
        ok = True
        for j in range(nlm):
            r0, D = lay.lm(j)
            V = Hl[r0:r0 + D, r0:r0 + D]
            dg = np.diag(V)
            ok = ok and bool(np.all(dg > 0.0)) and R._finite(dg)
            W.append({s: Hl[r0:r0 + D, 6 * s:6 * s + 6].copy() for s in lay.masks[j]})
            if rules.explicit_inverse:
                inv = LR.inverse3(V) if D == 3 else O.inverse6(V)
                ok = ok and R._finite(inv)
                apply = (lambda inv: lambda B: R._matmul_seq(inv, B))(inv)
            else:
                Lb, db, okb = block_ldlt(V)
                ok = ok and okb
                apply = (lambda Lb, db: lambda B: block_solve(Lb, db, B))(Lb, db)
            Vi.append(apply)
            z.append(apply(g[r0:r0 + D, None])[:, 0])
            Y.append({s: apply(W[j][s]) for s in lay.masks[j]})
        if not ok:
            return zero
        S = np.zeros((n6, n6), F)
        gr = np.array(g[:n6], F)
        for s in range(nkf):
            S[6 * s:6 * s + 6, 6 * s:6 * s + 6] = Hl[6 * s:6 * s + 6, 6 * s:6 * s + 6]
        for j in range(nlm):
            for sa in lay.masks[j]:
                WaT = W[j][sa].T
                gr[6 * sa:6 * sa + 6] = gr[6 * sa:6 * sa + 6] - R._matmul_seq(WaT, z[j][:, None])[:, 0]
                for sb in lay.masks[j]:
                    if sb > sa:
                        continue
                    blk = S[6 * sa:6 * sa + 6, 6 * sb:6 * sb + 6]
                    blk -= R._matmul_seq(WaT, Y[j][sb])
        Lm, Dg, ok, neg = ldlt_any_sign(S, rules.any_sign_pivot)
        if not ok:
            return zero[:3] + (neg,)
        DX = np.zeros(lay.N, F)
        DX[:n6] = R.ldlt_solve(Lm, Dg, gr)
        n2 = R._chain(DX[:n6] * DX[:n6])
        for j in range(nlm):
            r0, D = lay.lm(j)
            u = np.array(g[r0:r0 + D], F)
            for s in lay.masks[j]:
                for k in range(6):
                    u = u - W[j][s][:, k] * DX[6 * s + k]
            dj = Vi[j](u[:, None])[:, 0]
            DX[r0:r0 + D] = dj
            q = dj[0] * dj[0]
            for p in range(1, D):
                q = q + dj[p] * dj[p]
            n2 = n2 + q
    return DX, True, n2, neg


def solve_dense(Hd, g, lay, rules=GBA_RULES):
    """numpy.linalg.solve on the symmetric matrix rebuilt from the triangle the solver reads"""
    Hl = Hd if rules.lower_triangle else Hd.T
    Hs = np.tril(Hl) + np.tril(Hl, -1).T
    try:
        with np.errstate(all="ignore"):
            DX = np.linalg.solve(Hs, g)
    except np.linalg.LinAlgError:
        return np.zeros(lay.N, F), False, F(0.0), 0
    if not R._finite(DX):
        return np.zeros(lay.N, F), False, F(0.0), 0
    return DX, True, R._chain(DX * DX), 0


@dataclass
class GbaRef:
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
    rejected: int = 0
    negative: list = field(default_factory=list)   # per solved iteration: negative pivots accepted
    systems: list = field(default_factory=list)


def gba(cam, homog, a, prm=GBA_DEFAULTS, solver=solve_pinned, keep=False, rules=GBA_RULES):
    """a: the arrays of a gfpl.LbaProblem (its .a): the keyframe list is every alive keyframe but 0,
    observations by dead keyframes left out, keyframe 0 among the fixed poses.  Returns GbaRef."""
    lam0, lam_k, max_iters = F(prm[0]), F(prm[1]), int(prm[2])
    lay = R.layout_of(a)
    nkf, npt, nls, N = lay.nkf, lay.npt, lay.nls, lay.N
    n6 = 6 * nkf
    x0 = np.array([LR.logmap_se3(T) for T in a["T_kf"]], F).reshape(-1) if rules.x_from_T else a["x_kf"].reshape(-1)
    X = np.concatenate([x0, a["pt"].reshape(-1), a["ls"].reshape(-1)]).astype(F)
    r = GbaRef(lambda_=lam0)
    with np.errstate(all="ignore"):
        it = 0
        while True:
            H, g, esum = build_system(cam, homog, a, lay, X, it, rules)
            if it == 0:
                # `double err` is uninitialised (:1964): pinned to err_start; err /= (Npt_obs + Nls_obs), both 0
                err = (F(rules.err_start) + esum if rules.err_start != 0.0 else esum) / F(0.0)
                dg = np.diag(H)
                hmax = 0
                for d in dg:
                    if d > hmax or d < -hmax:
                        v = abs(d)
                        if not (v < 2147483648.0):
                            r.status |= HMAX_RANGE
                            r.hmax = 0x7FFFFFFF
                            r.err = err
                            r.X, r.T_kf, r.pt, r.ls = X, a["T_kf"].reshape(-1, 4, 4).copy(), a["pt"].copy(), a["ls"].copy()
                            return r
                        hmax = int(v)
                r.hmax = int(hmax)
                r.lambda_ = lam0 * F(hmax)
            else:
                err = esum / (F(0.0) if rules.divisor_zero else F(npt + nls))
                r.iters = it
            r.err = err
            if keep:
                r.systems.append(dict(H=H, g=g.copy(), err=err, lambda_=r.lambda_, it=it))
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
            Hd[di, di] = Hd[di, di] + lam * Hd[di, di]
            DX, ok, n2, neg = solver(Hd, g, lay, rules)
            r.negative.append(neg)
            if neg:
                r.status |= INDEFINITE
            if keep:
                r.systems[-1].update(Hd=Hd, DX=DX.copy(), ok=ok, negative=neg)
            accept = True
            if it > 0:
                if err > r.err_prev:
                    r.lambda_ = lam / lam_k
                    r.rejected += 1
                    accept = False
                else:
                    r.lambda_ = lam * lam_k
            if not ok:
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


def pairs_of(lay):
    """the planner's (landmark, keyframe) pair list: landmarks ascending, each one's keyframes ascending"""
    return [(j, s) for j in range(lay.npt + lay.nls) for s in lay.masks[j]]


def blocks_of(H, g, lay):
    """the debug hook's view of a dense system: U, V_pt, V_ls, and the LOWER coupling blocks (landmark
    rows, pose columns) per pair in the planner's order: W_pt [point pairs][3][6], W_ls [line pairs][6][6]"""
    nkf, npt, nls = lay.nkf, lay.npt, lay.nls
    U = np.array([H[6 * s:6 * s + 6, 6 * s:6 * s + 6] for s in range(nkf)], F).reshape(nkf, 6, 6)
    V_pt = np.array([H[lay.lm(j)[0]:lay.lm(j)[0] + 3, lay.lm(j)[0]:lay.lm(j)[0] + 3] for j in range(npt)], F).reshape(npt, 3, 3)
    V_ls = np.array([H[lay.lm(npt + j)[0]:lay.lm(npt + j)[0] + 6, lay.lm(npt + j)[0]:lay.lm(npt + j)[0] + 6]
                     for j in range(nls)], F).reshape(nls, 6, 6)
    pr = pairs_of(lay)
    W_pt = np.array([H[lay.lm(j)[0]:lay.lm(j)[0] + 3, 6 * s:6 * s + 6] for j, s in pr if j < npt], F).reshape(-1, 3, 6)
    W_ls = np.array([H[lay.lm(j)[0]:lay.lm(j)[0] + 6, 6 * s:6 * s + 6] for j, s in pr if j >= npt], F).reshape(-1, 6, 6)
    return dict(U=U, g=g.copy(), V_pt=V_pt, V_ls=V_ls, W_pt=W_pt, W_ls=W_ls, pairs=np.array(pr, np.int32).reshape(-1, 2))
