#!/usr/bin/env python3
"""gfpl_pgo_solve on one MI355X (k_pgo.hip): one JSON line.

--problems loop-closure optimisations (COV) of --n-kf keyframes each, every keyframe alive, a
covisibility band of --band keyframes (full_graph >= minLMEssGraph for |i - j| <= band) and one loop
entry from the last keyframe to keyframe 1 (keyframe 0 is fixed in COV, so the loop edge's row spans
the whole free system); every keyframe owns --pts points and --lines lines.  --distinct generated
problems are repeated over the batch (every copy does the same work).  Each repeat restores the in /
out arrays from pristine device copies outside the timed region, then times ONE gfpl_pgo_solve on the
host clock: the graph builder, the staging and upload of the lists, the two launches, the result
copy and the call's one synchronisation.  The kernels' device times come from events in the library
(gfpl_pgo_debug_ms).  --statement: also the time of tests/pgo_ref.py (Python, not the reference) on one
problem of that size."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gf-pl-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_case(n_kf, band, pts, lines, seed):
    import oracle as O
    import loop_closure_ref as LR
    import pgo_cases as PC
    rng = np.random.default_rng(seed)
    T = PC.trajectory(n_kf, seed)
    i, j = np.meshgrid(np.arange(n_kf), np.arange(n_kf), indexing="ij")
    fg = np.where(np.abs(i - j) <= band, 120, 5).astype(np.int32)
    lc = np.array([[1, n_kf - 1, 1]], np.int32)
    rel = LR.logmap_se3(LR._mat4_mul(T[n_kf - 1], O.inverse_se3(T[1])))
    lc_pose = (rel + rng.normal(0, 0.03, 6)).reshape(1, 6)
    pt_own = [list(range(k * pts, (k + 1) * pts)) for k in range(n_kf)]
    ls_own = [list(range(k * lines, (k + 1) * lines)) for k in range(n_kf)]
    return dict(alive=np.ones(n_kf, np.uint8), full_graph=fg, lc=lc, lc_pose=lc_pose, T_kf=T,
                pt=rng.normal(0, 3, (n_kf * pts, 3)), ls=rng.normal(0, 3, (n_kf * lines, 6)), pt_own=pt_own, ls_own=ls_own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--n-kf", type=int, default=256)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--pts", type=int, default=20)
    ap.add_argument("--lines", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--statement", action="store_true", help="also time the Python statement on one problem")
    ap.add_argument("--out", help="also append the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pgo: no GPU (nothing is measured without one)")
    import gfpl
    cfg = gfpl.default_config()
    ctx = gfpl.Context(gfpl.make_camera("vga", cfg), cfg)
    dev = torch.device("cuda", ctx.device)
    prm = gfpl.PoseGraphParams.default()
    cases = [make_case(a.n_kf, a.band, a.pts, a.lines, 900 + k) for k in range(a.distinct)]
    probs = [gfpl.PoseGraphProblem(c["alive"], c["full_graph"], c["lc"], c["lc_pose"], c["T_kf"], c["pt"], c["ls"], c["pt_own"],
                                   c["ls_own"]) for c in cases]
    counts = []
    for p in probs:
        rc, cnt = p.check(prm)
        gfpl.check(rc, "pgo_check")
        counts.append(cnt)
    pg = gfpl.PoseGraph(ctx, counts, a.problems)
    rc, hbm, lds = gfpl.pgoWorkspace(counts[0])
    structs = (gfpl.PgoProblemStruct * a.problems)()
    pristine, work = [], []
    for i in range(a.problems):
        p = probs[i % a.distinct]
        d = {k: torch.from_numpy(p.a[k].copy()).to(dev) for k in ("T_kf", "pt", "ls")}
        d["x_kf"] = torch.zeros((a.n_kf, 6), dtype=torch.float64, device=dev)
        pristine.append({k: v.clone() for k, v in d.items()})
        work.append(d)
        structs[i] = p.struct(d)
    out = (gfpl.PgoResult * a.problems)()
    call_ms, solve_ms, corr_ms = [], [], []
    for rep in range(a.warmup + a.repeats):
        for d, q in zip(work, pristine):
            for k, v in q.items():
                d[k].copy_(v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gfpl.check(ctx.L.gfpl_pgo_solve(pg.h, structs, a.problems, C.byref(prm), out), "pgo_solve")
        t1 = time.perf_counter()
        if rep >= a.warmup:
            call_ms.append((t1 - t0) * 1e3)
            s, c = pg.ms()
            solve_ms.append(s)
            corr_ms.append(c)
    res = {"bench": "pgo", "device": torch.cuda.get_device_name(0), "problems": a.problems, "n_kf": a.n_kf, "band": a.band,
           "points_per_kf": a.pts, "lines_per_kf": a.lines, "n_free": counts[0].n_free, "n_edge": counts[0].n_edge,
           "env_blocks": counts[0].env_blocks, "workspace_bytes_per_problem": hbm, "lds_bytes": lds,
           "iters": sorted({out[i].iters for i in range(a.problems)}), "stops": sorted({out[i].stop for i in range(a.problems)}),
           "rejects": sorted({out[i].rejects for i in range(a.problems)}), "status": sorted({out[i].status for i in range(a.problems)}),
           "chi2_0": out[0].chi2_0, "chi2": out[0].chi2,
           "call_ms": [round(x, 3) for x in call_ms], "median_call_ms": float(np.median(call_ms)),
           "median_k_pgo_ms": float(np.median(solve_ms)), "median_k_pgo_correct_ms": float(np.median(corr_ms)),
           "k_pgo_share": float(np.median(solve_ms) / np.median(call_ms))}
    pg.close()
    ctx.close()
    if a.statement:
        import pgo_ref as R
        c = cases[0]
        lc = [tuple(int(v) for v in l) for l in c["lc"]]
        t0 = time.perf_counter()
        g = R.build_graph(c["alive"], c["full_graph"], lc, prm.min_lm_ess_graph, prm.min_lm_cov_graph, R.COV)
        r = R.solve(g, c["T_kf"], lc, c["lc_pose"])
        res["statement_python_s_one_problem"] = time.perf_counter() - t0
        res["statement_iters"] = r.iters
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
