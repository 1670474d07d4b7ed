"""The loop-closure pose graph restated in Python: the statement the builder
(gfpl_pgo_plan.cpp) and the kernels (k_pgo.hip) are compared with.

Graph (build_graph): the index work of MapHandler::loopClosureOptimizationCovGraphG2O / EssGraphG2O
(src/mapHandler.cpp:4209-4304, :3973-4066) with explicit loops, the `break` included.
Objective (edge, update): the project's own pin, ledger PG1-PG8 — g2o is not in the reference tree.
Every sum is taken in the pinned order: a vertex's blocks over its incident edges in edge-list order,
chi2 over the edges in order.  expmap_se3 / inverse_se3 are the oracle's, logmap_se3 and the 4 x 4
product come from tests/loop_closure_ref.py.

Two solvers take the damped dense system: solve_dense (numpy.linalg.solve) and solve_envelope (the
LDL^T over the block envelope the device runs, without pivoting).

Keyword arguments named `alt_*` switch single rules to a plausible wrong reading;
tests/test_pgo_cpu.py shows each changes a named case.
"""
from dataclasses import dataclass, field

import numpy as np

import oracle as O
import loop_closure_ref as LR

F = np.float64
EPS = F(2.220446049250313e-16)
COV, ESS = 0, 1
OK, E_INVALID, E_CAPACITY, E_STATE = 0, -1, -5, -6
FIXED, LC_J, LC_I = 1, 2, 4
STOP_ITERS, STOP_STEP, STOP_DCHI2, STOP_REJECT, STOP_NOFREE = 0, 1, 2, 3, 4
SINGULAR = 1
DEFAULTS = dict(ess=100, cov=30, variant=COV, max_iters=100, max_rejects=10, lambda_init=1e-10)


# -------------------------------------------------------------------- graph --
@dataclass
class Graph:
    first: int = 0
    kf_curr: int = -1
    vert: list = field(default_factory=list)        # (keyframe, flags, lc_id or -1, free index or -1)
    edge: list = field(default_factory=list)        # (vertex i, vertex j, loop entry or -1, 0)
    free_vert: list = field(default_factory=list)
    inc: list = field(default_factory=list)         # per free vertex: incident edges, edge-list order
    env_first: list = field(default_factory=list)

    @property
    def n_free(self):
        return len(self.free_vert)

    @property
    def env_blocks(self):
        return sum(r - f + 1 for r, f in enumerate(self.env_first))


def check(alive, full_graph, lc, ess, cov, variant):
    """the refusals of gfpl_pgo_check that concern the graph"""
    if alive is None or full_graph is None or lc is None:
        return E_INVALID
    n_kf = len(alive)
    if n_kf < 1 or len(lc) < 1 or ess < 0 or cov < 0 or variant not in (COV, ESS):
        return E_INVALID
    for a, b, _ in lc:
        if a < 0 or b >= n_kf or a >= b:
            return E_INVALID
        if not alive[a] or not alive[b]:
            return E_INVALID
    if variant == COV and not alive[0]:
        return E_INVALID
    return OK


def build_graph(alive, full_graph, lc, ess=100, cov=30, variant=COV, alt_no_break=False, alt_lc_edges_first=False):
    n_kf = len(alive)
    g = Graph()
    kf_prev, kf_curr = 2 ** 31 - 1, -1
    for a, b, _ in lc:
        if a < kf_prev:
            kf_prev = a
        if b > kf_curr:
            kf_curr = b
    if variant == COV:
        kf_prev = 0
    g.first, g.kf_curr = int(kf_prev), int(kf_curr)
    vertex_of = {}
    for i in range(kf_prev, kf_curr + 1):
        if not alive[i]:
            continue
        is_lc_i = is_lc_j = False
        idx = 0
        for it in lc:
            if it[0] == i:
                is_lc_i = True
                if not alt_no_break:
                    break
            if it[1] == i:
                is_lc_j = True
                if not alt_no_break:
                    break
            idx += 1
        if alt_no_break:
            # the reading without the break: the LAST entry that names i decides, and both flags may be set
            idx = max(k for k, it in enumerate(lc) if i in (it[0], it[1])) if (is_lc_i or is_lc_j) else len(lc)
        if is_lc_j:
            fixed = variant == ESS
        elif variant == COV:
            fixed = i == 0
        else:
            fixed = is_lc_i or i == 0
        flags = (FIXED if fixed else 0) | (LC_J if is_lc_j else 0) | (LC_I if is_lc_i else 0)
        vertex_of[i] = len(g.vert)
        free = -1
        if not fixed:
            free = len(g.free_vert)
            g.free_vert.append(len(g.vert))
        g.vert.append((i, flags, idx if (is_lc_i or is_lc_j) else -1, free))
    kf_edges, lc_edges = [], []
    for i in range(kf_prev, kf_curr + 1):
        for j in range(i + 1, kf_curr + 1):
            if alive[i] and alive[j]:
                c = full_graph[i][j]
                if c >= ess or (variant == COV and c >= cov) or abs(i - j) == 1:
                    kf_edges.append((vertex_of[i], vertex_of[j], -1, 0))
    for l, it in enumerate(lc):
        lc_edges.append((vertex_of[it[0]], vertex_of[it[1]], l, 0))
    g.edge = lc_edges + kf_edges if alt_lc_edges_first else kf_edges + lc_edges
    g.inc = [[] for _ in g.free_vert]
    g.env_first = list(range(len(g.free_vert)))
    for e, (vi, vj, _, _) in enumerate(g.edge):
        ri, rj = g.vert[vi][3], g.vert[vj][3]
        if ri >= 0:
            g.inc[ri].append(e)
        if rj >= 0:
            g.inc[rj].append(e)
        if ri >= 0 and rj >= 0:
            g.env_first[rj] = min(g.env_first[rj], ri)
    return g


# ---------------------------------------------------------------- objective --
def quat(D, alt_no_w_flip=False):
    """(x, y, z, w) of D's rotation: the four-branch rule, normalised, w >= 0"""
    r = D
    tr = (r[0, 0] + r[1, 1]) + r[2, 2]
    if tr > 0.0:
        s = np.sqrt(tr + F(1.0)) * F(2.0)
        w, x, y, z = F(0.25) * s, (r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s
    elif r[0, 0] > r[1, 1] and r[0, 0] > r[2, 2]:
        s = np.sqrt(((F(1.0) + r[0, 0]) - r[1, 1]) - r[2, 2]) * F(2.0)
        w, x, y, z = (r[2, 1] - r[1, 2]) / s, F(0.25) * s, (r[0, 1] + r[1, 0]) / s, (r[0, 2] + r[2, 0]) / s
    elif r[1, 1] > r[2, 2]:
        s = np.sqrt(((F(1.0) + r[1, 1]) - r[0, 0]) - r[2, 2]) * F(2.0)
        w, x, y, z = (r[0, 2] - r[2, 0]) / s, (r[0, 1] + r[1, 0]) / s, F(0.25) * s, (r[1, 2] + r[2, 1]) / s
    else:
        s = np.sqrt(((F(1.0) + r[2, 2]) - r[0, 0]) - r[1, 1]) * F(2.0)
        w, x, y, z = (r[1, 0] - r[0, 1]) / s, (r[0, 2] + r[2, 0]) / s, (r[1, 2] + r[2, 1]) / s, F(0.25) * s
    n = np.sqrt(((x * x + y * y) + z * z) + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    if w < 0.0 and not alt_no_w_flip:
        x, y, z, w = -x, -y, -z, -w
    return np.array([x, y, z, w], F)


def edge(Xi, Xj, Z, jac=True, alt_no_w_flip=False):
    """e [6] and, with jac, J_i and J_j [6][6] of the update X <- X Delta(delta)"""
    Zi = O.inverse_se3(Z)
    M = LR._mat4_mul(O.inverse_se3(Xi), Xj)
    D = LR._mat4_mul(Zi, M)
    q = quat(D, alt_no_w_flip)
    e = np.array([D[0, 3], D[1, 3], D[2, 3], q[0], q[1], q[2]], F)
    if not jac:
        return e
    Q = np.array([[q[3], -q[2], q[1]], [q[2], q[3], -q[0]], [-q[1], q[0], q[3]]], F)
    S = np.array([[0.0, -M[2, 3], M[1, 3]], [M[2, 3], 0.0, -M[0, 3]], [-M[1, 3], M[0, 3], 0.0]], F)
    Ji, Jj = np.zeros((6, 6), F), np.zeros((6, 6), F)
    for a in range(3):
        for b in range(3):
            Jj[a, b] = D[a, b]
            Jj[3 + a, 3 + b] = Q[a, b]
            Ji[a, b] = -Zi[a, b]
            Ji[a, 3 + b] = F(2.0) * ((Zi[a, 0] * S[0, b] + Zi[a, 1] * S[1, b]) + Zi[a, 2] * S[2, b])
            Ji[3 + a, 3 + b] = -((Q[a, 0] * M[b, 0] + Q[a, 1] * M[b, 1]) + Q[a, 2] * M[b, 2])
    return e, Ji, Jj


def delta_matrix(d):
    x, y, z = F(d[3]), F(d[4]), F(d[5])
    n2 = (x * x + y * y) + z * z
    if n2 > 1.0:
        n = np.sqrt(n2)
        x, y, z, w = x / n, y / n, z / n, F(0.0)
    else:
        w = np.sqrt(F(1.0) - n2)
    two, one = F(2.0), F(1.0)
    E = np.zeros((4, 4), F)
    E[0] = [one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w), d[0]]
    E[1] = [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w), d[1]]
    E[2] = [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y), d[2]]
    E[3, 3] = one
    return E


def update(X, d, alt_left=False):
    """X Delta(d); a step that is all zero keeps the pose's bits"""
    if not np.any(np.asarray(d) != 0.0):
        return X.copy()
    return LR._mat4_mul(delta_matrix(d), X) if alt_left else LR._mat4_mul(X, delta_matrix(d))


def start(g, T_kf, lc, lc_pose):
    """X0 [n_vert][4][4] (PG1) and Z [n_edge][4][4] (PG2)"""
    X0 = np.zeros((len(g.vert), 4, 4), F)
    for v, (kf, flags, idx, _) in enumerate(g.vert):
        if flags & LC_J:
            X0[v] = LR._mat4_mul(O.expmap_se3(lc_pose[idx]), T_kf[lc[idx][0]])
        else:
            X0[v] = T_kf[kf]
    Z = np.zeros((len(g.edge), 4, 4), F)
    for e, (vi, vj, l, _) in enumerate(g.edge):
        if l >= 0:
            Z[e] = O.expmap_se3(lc_pose[l])
        else:
            Z[e] = LR._mat4_mul(O.inverse_se3(T_kf[g.vert[vi][0]]), T_kf[g.vert[vj][0]])
    return X0, Z


def _dot6(u, v):
    s = u[0] * v[0]
    for q in range(1, 6):
        s = s + u[q] * v[q]
    return s


def chi2_of(g, X, Z, **alt):
    c = F(0.0)
    for e, (vi, vj, _, _) in enumerate(g.edge):
        r = edge(X[vi], X[vj], Z[e], jac=False, **alt)
        c = c + _dot6(r, r)
    return c


def system(g, X, Z, **alt):
    """dense undamped H (both triangles), b = J^T e and chi2, every sum in the pinned order"""
    nf = g.n_free
    rows = [edge(X[vi], X[vj], Z[e], **alt) for e, (vi, vj, _, _) in enumerate(g.edge)]
    H, b = np.zeros((6 * nf, 6 * nf), F), np.zeros(6 * nf, F)
    for r in range(nf):
        v = g.free_vert[r]
        for e in g.inc[r]:
            vi, vj, _, _ = g.edge[e]
            er, Ji, Jj = rows[e]
            J = Ji if vi == v else Jj
            for a in range(6):
                b[6 * r + a] = b[6 * r + a] + _dot6(J[:, a], er)
                for c in range(6):
                    H[6 * r + a, 6 * r + c] = H[6 * r + a, 6 * r + c] + _dot6(J[:, a], J[:, c])
            if vj == v and g.vert[vi][3] >= 0:
                ci = g.vert[vi][3]
                for a in range(6):
                    for c in range(6):
                        H[6 * r + a, 6 * ci + c] = H[6 * r + a, 6 * ci + c] + _dot6(Jj[:, a], Ji[:, c])
                        H[6 * ci + c, 6 * r + a] = H[6 * r + a, 6 * ci + c]
    chi2 = F(0.0)
    for er, _, _ in rows:
        chi2 = chi2 + _dot6(er, er)
    return H, b, chi2


def gradient(g, X, Z):
    """b = J^T e alone (the GPU test's gradient norm)"""
    return system(g, X, Z)[1]


# ------------------------------------------------------------------ solvers --
def ldlt_envelope(A, env_first):
    """LDL^T of the lower triangle of A over the block envelope, without pivoting: L (unit lower), D,
    ok.  Column k: v_i = A[i,k] - sum_m (L[i,m] L[k,m]) D[m], m ascending from the later of the two
    rows' first columns; a pivot that is not positive and finite stops it."""
    n = A.shape[0]
    lo = np.repeat(6 * np.asarray(env_first, np.int64), 6)
    Lm, D = np.zeros((n, n), F), np.zeros(n, F)
    for k in range(n):
        rows = np.arange(k, n)
        rows = rows[lo[rows] <= (k // 6) * 6]
        v = A[rows, k].copy()
        for m in range(lo[k], k):
            act = lo[rows] <= m
            v[act] = v[act] - (Lm[rows[act], m] * Lm[k, m]) * D[m]
        if not (v[0] > 0.0 and np.isfinite(v[0])):
            return Lm, D, False
        D[k] = v[0]
        Lm[k, k] = F(1.0)
        Lm[rows[1:], k] = v[1:] / v[0]
    return Lm, D, True


def solve_envelope(Hd, rhs, g):
    with np.errstate(all="ignore"):
        Lm, D, ok = ldlt_envelope(Hd, g.env_first)
        if not ok:
            return np.zeros(len(rhs), F), False
        return LR_ldlt_solve(Lm, D, rhs), True


def LR_ldlt_solve(Lm, D, b):
    n = len(b)
    y = np.array(b, F)
    for m in range(n):
        y[m + 1:] = y[m + 1:] - Lm[m + 1:, m] * y[m]
    y = y / D
    for m in range(n - 1, 0, -1):
        y[:m] = y[:m] - Lm[m, :m] * y[m]
    return y


def solve_dense(Hd, rhs, g):
    try:
        with np.errstate(all="ignore"):
            d = np.linalg.solve(Hd, rhs)
    except np.linalg.LinAlgError:
        return np.zeros(len(rhs), F), False
    if not np.all(np.isfinite(d)):
        return np.zeros(len(rhs), F), False
    return d, True


# ----------------------------------------------------------------- the loop --
@dataclass
class PgoRef:
    iters: int = 0
    stop: int = STOP_ITERS
    status: int = 0
    rejects: int = 0
    lambda_: float = 0.0
    chi2_0: float = 0.0
    chi2: float = 0.0
    X: np.ndarray = None
    X0: np.ndarray = None
    Z: np.ndarray = None
    first: dict = None      # iteration 0's H, b, chi2


def _seq_sum(v):
    s = F(0.0)
    for x in v:
        s = s + x
    return s


def solve(g, T_kf, lc, lc_pose, max_iters=100, max_rejects=10, lambda_init=1e-10, solver=solve_envelope,
          alt_left=False, alt_no_w_flip=False):
    """the Levenberg-Marquardt iteration of DESIGN.md §4j (PG3) on graph g"""
    alt = dict(alt_no_w_flip=alt_no_w_flip)
    X0, Z = start(g, T_kf, lc, lc_pose)
    X = X0.copy()
    r = PgoRef(lambda_=F(lambda_init), X0=X0, Z=Z)
    lam, nu = F(lambda_init), F(2.0)
    nf = g.n_free
    with np.errstate(all="ignore"):
        chi2 = chi2_of(g, X, Z, **alt)
        r.chi2_0 = chi2
        prev = chi2
        done = False
        if nf == 0:
            r.stop, done = STOP_NOFREE, True
        elif max_iters < 1:
            done = True
        it = 0
        while not done:
            H, b, _ = system(g, X, Z, **alt)
            if it == 0:
                r.first = dict(H=H, b=b.copy(), chi2=chi2)
            rej_it = 0
            accepted = False
            while True:
                Hd = H.copy()
                di = np.arange(6 * nf)
                Hd[di, di] = Hd[di, di] + lam
                d, ok = solver(Hd, -b, g)
                sing = not ok
                if not sing:
                    dmax = F(0.0)
                    for x in d:
                        a = abs(x)
                        if not (a <= dmax):
                            dmax = a
                    scale = _seq_sum(d * (lam * d - b))
                    if dmax <= F(64.0) * EPS:
                        r.stop, done = STOP_STEP, True
                        break
                    Xt = X.copy()
                    for rr in range(nf):
                        v = g.free_vert[rr]
                        Xt[v] = update(X[v], d[6 * rr:6 * rr + 6], alt_left)
                    chi2t = chi2_of(g, Xt, Z, **alt)
                accept, rho = False, F(0.0)
                if not sing and np.isfinite(chi2t) and scale > 0.0 and np.isfinite(scale):
                    rho = (chi2 - chi2t) / scale
                    accept = bool(rho > 0.0 or chi2t - chi2 <= (F(64.0) * EPS) * chi2)
                if accept:
                    t = F(2.0) * rho - F(1.0)
                    f = F(1.0) - (t * t) * t
                    if f < F(1.0) / F(3.0):
                        f = F(1.0) / F(3.0)
                    lam, nu = lam * f, F(2.0)
                    prev, chi2 = chi2, chi2t
                    X = Xt
                    accepted = True
                    break
                lam, nu = lam * nu, nu * F(2.0)
                r.rejects += 1
                rej_it += 1
                if sing:
                    r.status |= SINGULAR
                if rej_it >= max_rejects:
                    r.stop, done = STOP_REJECT, True
                    break
            if accepted and not done:
                r.iters = it + 1
                if prev - chi2 <= (F(64.0) * EPS) * prev:
                    r.stop, done = STOP_DCHI2, True
                elif it + 1 >= max_iters:
                    done = True
            it += 1
    r.lambda_, r.chi2, r.X = lam, chi2, X
    return r


# ----------------------------------------------------------- map correction --
def _move(C, p):
    return np.array([((C[i, 0] * p[0] + C[i, 1] * p[1]) + C[i, 2] * p[2]) + C[i, 3] for i in range(3)], F)


def correct(g, X, alive, T_kf, pt, ls, pt_own, ls_own, pt_dirs=None, ls_dirs=None, pt_freed=None, ls_freed=None,
            alt_own_corr=False, alt_dir_untranslated=False, T_given=None):
    """the write-back and map correction (:4312-4412, PG4) with explicit loops.  pt_own / ls_own: per
    keyframe the list of landmark ids (< 0: freed); *_dirs: per landmark an [n][3] array, or None.
    Returns new copies: T_kf, x_kf, pt, ls, pt_dirs, ls_dirs.  x_kf rows of keyframes not moved are NaN."""
    T_kf, pt, ls = np.array(T_kf, F).reshape(-1, 4, 4).copy(), np.array(pt, F).reshape(-1, 3).copy(), np.array(ls, F).reshape(-1, 6).copy()
    x_kf = np.full((len(T_kf), 6), np.nan, F)
    pt_dirs = None if pt_dirs is None else [np.array(d, F).reshape(-1, 3).copy() for d in pt_dirs]
    ls_dirs = None if ls_dirs is None else [np.array(d, F).reshape(-1, 3).copy() for d in ls_dirs]

    def move_dir(C, row):
        if alt_dir_untranslated:
            return np.array([(C[i, 0] * row[0] + C[i, 1] * row[1]) + C[i, 2] * row[2] for i in range(3)], F)
        return _move(C, row)

    def landmarks(C, kf):
        for j in pt_own[kf]:
            if j < 0 or (pt_freed is not None and pt_freed[j]):
                continue
            pt[j] = _move(C, pt[j])
            if pt_dirs is not None:
                for k in range(len(pt_dirs[j])):
                    pt_dirs[j][k] = move_dir(C, pt_dirs[j][k])
        for j in ls_own[kf]:
            if j < 0 or (ls_freed is not None and ls_freed[j]):
                continue
            ls[j, :3] = _move(C, ls[j, :3])
            ls[j, 3:] = _move(C, ls[j, 3:])
            if ls_dirs is not None:
                for k in range(len(ls_dirs[j])):
                    ls_dirs[j][k] = move_dir(C, ls_dirs[j][k])

    with np.errstate(all="ignore"):
        C = np.eye(4, dtype=F)
        for v, (kf, _, _, _) in enumerate(g.vert):
            # T_given: the written-back pose of every keyframe as another solve produced it
            T = O.expmap_se3(LR.logmap_se3(X[v])) if T_given is None else np.array(T_given[kf], F)
            Tprev = T_kf[kf].copy()
            T_kf[kf] = T
            x_kf[kf] = LR.logmap_se3(T)
            C = LR._mat4_mul(T, O.inverse_se3(Tprev))
            landmarks(C, kf)
        for i in range(g.kf_curr + 1, len(T_kf)):
            if not alive[i]:
                continue   # (the reference dereferences a NULL keyframe here)
            Ci = C
            if alt_own_corr:
                Ci = np.eye(4, dtype=F)
            T_kf[i] = LR._mat4_mul(Ci, T_kf[i])
            x_kf[i] = LR.logmap_se3(T_kf[i])
            landmarks(Ci, i)
    return T_kf, x_kf, pt, ls, pt_dirs, ls_dirs
