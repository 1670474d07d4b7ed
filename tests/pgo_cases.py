"""Loop-closure pose-graph cases for tests/test_pgo_cpu.py and tests/test_pgo_gpu.py: small maps
whose graphs cross every boundary the builder and k_pgo have (tests/pgo_ref.py is the statement).

The constants the shapes are chosen by (gfpl_layout.hpp): PGO_BLOCK = 256 lanes (an edge per lane, the
chi2 / step sums a chunk of 256 at a time, rows of a column 256 at a time), PGO_RED = 78 reduction
lanes per free vertex (3 free vertices fill 234 of the 256 lanes, 4 need a second pass), PGO_PANEL =
16 block columns of the pivot row staged in LDS at a time.
"""
import numpy as np

import oracle as O
import loop_closure_ref as LR
import pgo_ref as R

F = np.float64
ESS_TH, COV_TH = 100, 30


def trajectory(n_kf, seed):
    """T_kf_w of n_kf keyframes: a drifting walk with rotations of a few degrees a step"""
    rng = np.random.default_rng(seed)
    T = [O.expmap_se3(np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 0.2, 3)]))]
    for _ in range(1, n_kf):
        step = np.concatenate([[0.4, 0.0, 0.05] + rng.normal(0, 0.05, 3), rng.normal(0, 0.06, 3)])
        T.append(LR._mat4_mul(O.expmap_se3(step), T[-1]))
    return np.array(T, F)


def make(name, n_kf, lc, variant=R.COV, dead=(), seed=1, graph=None, dense=False, dirs=True, with_map=True, noise=0.03):
    """One case.  graph: {(i, j): count} entries over the default (120 for |i - j| <= 1, 35 for
    |i - j| == 2, else 5; dense: 120 everywhere).  The keyframes after the largest kf_curr are the
    'rest of frames' of :4368."""
    rng = np.random.default_rng(1000 + seed)
    alive = np.ones(n_kf, np.uint8)
    for d in dead:
        alive[d] = 0
    fg = np.full((n_kf, n_kf), 120 if dense else 5, np.int32)
    if not dense:
        for i in range(n_kf):
            for j in range(n_kf):
                if abs(i - j) <= 1:
                    fg[i, j] = 120
                elif abs(i - j) == 2:
                    fg[i, j] = 35
    for (i, j), c in (graph or {}).items():
        fg[i, j] = fg[j, i] = c
    T = trajectory(n_kf, seed)
    lc = np.array([list(l) + [1] for l in lc], np.int32).reshape(-1, 3)
    lc_pose = np.zeros((len(lc), 6), F)
    for l, (a, b, _) in enumerate(lc):
        rel = LR.logmap_se3(LR._mat4_mul(T[b], O.inverse_se3(T[a])))
        lc_pose[l] = rel + rng.normal(0, noise, 6)
    case = dict(name=name, alive=alive, full_graph=fg, lc=lc, lc_pose=lc_pose, T_kf=T, variant=variant, n_kf=n_kf)
    # the map: keyframe i owns i % 3 points and (i + 1) % 2 lines (so some own none); ids shuffled;
    # one point freed by a negative entry, one line by its mark; dir lists of 0 .. 3 rows
    n_pt = sum(i % 3 for i in range(n_kf)) if with_map else 0
    n_ls = sum((i + 1) % 2 for i in range(n_kf)) if with_map else 0
    pid, lid = list(rng.permutation(n_pt)), list(rng.permutation(n_ls))
    pt_own = [[int(pid.pop()) for _ in range(i % 3 if with_map else 0)] for i in range(n_kf)]
    ls_own = [[int(lid.pop()) for _ in range((i + 1) % 2 if with_map else 0)] for i in range(n_kf)]
    pt_freed, ls_freed = np.zeros(n_pt, np.uint8), np.zeros(n_ls, np.uint8)
    if n_pt > 2:
        k = next(i for i in range(n_kf) if len(pt_own[i]) == 2)
        pt_own[k][1] = -1 - pt_own[k][1]
    if n_ls > 1:
        ls_freed[ls_own[2][0] if ls_own[2] else 0] = 1
    case.update(pt=rng.normal(0, 3, (n_pt, 3)), ls=rng.normal(0, 3, (n_ls, 6)), pt_own=pt_own, ls_own=ls_own,
                pt_freed=pt_freed, ls_freed=ls_freed,
                pt_dirs=[rng.normal(0, 1, (j % 4, 3)) for j in range(n_pt)] if dirs else None,
                ls_dirs=[rng.normal(0, 1, ((j + 1) % 4, 3)) for j in range(n_ls)] if dirs else None)
    return case


def cases():
    c = []
    # free vertices 1, 2, 3 and 4 (3 x 78 lanes fit one pass of the reduction, 4 x 78 do not)
    c.append(make("free1", 2, [(0, 1)], seed=1))
    c.append(make("free2", 3, [(0, 2)], seed=2))
    c.append(make("free3", 4, [(1, 3)], seed=3))
    c.append(make("free4", 5, [(1, 4)], seed=4))
    # builder cases: a dead keyframe inside the range, a dead neighbour that isolates a vertex, shared
    # kf_prev, a kf_curr that is another entry's kf_prev, counts around each threshold, later keyframes
    c.append(make("dead_inside", 7, [(1, 5)], dead=(3,), seed=5))
    c.append(make("isolated", 9, [(0, 6)], dead=(2, 4, 8), seed=6, graph={(3, j): 5 for j in range(9) if j != 3} | {(1, 5): 120}))
    c.append(make("shared_prev", 7, [(1, 4), (1, 6)], seed=7))
    c.append(make("chained_lc", 7, [(0, 3), (3, 6)], seed=8))
    c.append(make("thresholds", 8, [(1, 6)], seed=9,
                  graph={(0, 3): COV_TH - 1, (0, 4): COV_TH, (0, 5): COV_TH + 1, (1, 4): ESS_TH - 1, (1, 5): ESS_TH, (2, 6): ESS_TH + 1}))
    c.append(make("thresholds_ess", 8, [(1, 6)], variant=R.ESS, seed=9,
                  graph={(0, 3): COV_TH - 1, (0, 4): COV_TH, (0, 5): COV_TH + 1, (1, 4): ESS_TH - 1, (1, 5): ESS_TH, (2, 6): ESS_TH + 1}))
    c.append(make("later_kfs", 9, [(1, 5)], dead=(7,), seed=10))
    c.append(make("no_dirs", 6, [(1, 5)], seed=11, dirs=False))
    c.append(make("no_map", 5, [(1, 4)], seed=12, with_map=False))
    # ESS: a chain (envelope width 1 beside the covisibility band), and a graph with no free vertex
    c.append(make("ess_chain", 9, [(0, 8)], variant=R.ESS, seed=13, graph={(i, i + 2): 5 for i in range(7)}))
    c.append(make("ess_nofree", 2, [(0, 1)], variant=R.ESS, seed=14))
    # a COV loop edge from a free kf_prev: the last envelope row spans the whole problem; 15, 16 and 17
    # block columns before its diagonal are one below, at and one above PGO_PANEL
    for nf in (16, 17, 18):
        c.append(make(f"span{nf - 1}", nf + 1, [(1, nf)], seed=20 + nf))
    # 6 n_free = 252 and 258 scalars around PGO_BLOCK (the step sums and the column's rows), chain only
    c.append(make("scalars252", 44, [(0, 43)], variant=R.ESS, seed=40, graph={(i, i + 2): 5 for i in range(42)}, with_map=False))
    c.append(make("scalars258", 45, [(0, 44)], variant=R.ESS, seed=41, graph={(i, i + 2): 5 for i in range(43)}, with_map=False))
    # 255, 256 and 257 edges around PGO_BLOCK: 23 keyframes all connected (253 edges) and 2, 3, 4 loop entries
    for k, lcs in ((255, [(1, 22), (2, 21)]), (256, [(1, 22), (2, 21), (3, 20)]), (257, [(1, 22), (2, 21), (3, 20), (4, 19)])):
        c.append(make(f"edges{k}", 23, lcs, seed=50 + k, dense=True, with_map=False))
    return c


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


def graph_of(c, **alt):
    return R.build_graph(c["alive"], c["full_graph"], [tuple(int(v) for v in l) for l in c["lc"]], ESS_TH, COV_TH, c["variant"], **alt)


_SOLVED = {}


def solved(c, solver="envelope"):
    """the statement's solve of a case, computed once per process: (graph, PgoRef)"""
    key = (c["name"], solver)
    if key not in _SOLVED:
        g = graph_of(c)
        lc = [tuple(int(v) for v in l) for l in c["lc"]]
        T = c["T_kf"].reshape(-1, 4, 4)
        _SOLVED[key] = (g, R.solve(g, T, lc, c["lc_pose"], solver=R.solve_envelope if solver == "envelope" else R.solve_dense))
    return _SOLVED[key]


def corrected(c, g, X, **alt):
    return R.correct(g, X, c["alive"], c["T_kf"], c["pt"], c["ls"], c["pt_own"], c["ls_own"], c["pt_dirs"], c["ls_dirs"],
                     c["pt_freed"], c["ls_freed"], **alt)


def written_back(c, g, X):
    """T_kf_w of the graph's keyframes as the call returns them, [n_vert][4][4]"""
    T = corrected(c, g, X)[0]
    return np.array([T[v[0]] for v in g.vert], F).reshape(-1, 4, 4)


def spread(c):
    """largest difference between the poses the statement's two solvers return for a case"""
    g, a = solved(c, "envelope")
    _, b = solved(c, "dense")
    return float(np.max(np.abs(written_back(c, g, a.X) - written_back(c, g, b.X))))


def problem(c):
    import gfpl
    return gfpl.PoseGraphProblem(c["alive"], c["full_graph"], c["lc"], c["lc_pose"], c["T_kf"], c["pt"], c["ls"], c["pt_own"],
                                 c["ls_own"], c["pt_dirs"], c["ls_dirs"], c["pt_freed"], c["ls_freed"])


def params(c, **over):
    import gfpl
    return gfpl.PoseGraphParams.default(min_lm_ess_graph=ESS_TH, min_lm_cov_graph=COV_TH, variant=c["variant"], **over)
