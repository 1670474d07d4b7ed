#!/usr/bin/env python3
"""gfpl_gba_solve on one MI355X (k_gba.hip): one JSON line.

One global bundle adjustment of --n-kf keyframes (+ keyframe 0 fixed), --n-pt points and --n-ls lines
with --obs observations per landmark by neighbouring keyframes, resident in HBM.  Each repeat restores
the in / out arrays (T_kf, pt, ls) from pristine device copies outside the timed region, then times ONE
gfpl_gba_solve on the host clock: the planner, the staging and upload of its lists, every launch of
every iteration, the result copy and the call's one synchronisation.  lambda_k defaults to 3 so that the
problem does not meet the stop by step before --max-iters (with the reference's 10 the damping passes
1e17 after some 14 iterations).  --compare-lba runs the same problem (n_kf <= 16) through gfpl_lba_solve
too: different algorithms by the ledger (GB3, GB5, GB7), so a note, not a bar.  The per-phase split is
read from a kernel trace of this script taken in a run of its own, not measured here."""
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


def make_map(gfpl, O, LR, cam, seed, n_kf, n_pt, n_ls, obs):
    """a map like lba_cases.make_problem's, generated with numpy: landmark j is seen by `obs` consecutive
    poses of [fixed keyframe 0, local 0 .. n_kf - 1] starting at a random one"""
    rng = np.random.default_rng(seed)
    pose = lambda r, t: O.expmap_se3(np.concatenate([rng.uniform(-t, t, 3), rng.uniform(-r, r, 3)]))
    T_true = [pose(0.05, 0.5) for _ in range(n_kf + 1)]           # index 0: the fixed keyframe
    T_est = [T @ pose(0.01, 0.01) for T in T_true[1:]]
    Ti = np.array([O.inverse_se3(T) for T in T_true])
    pool = n_kf + 1
    k = min(obs, pool)

    def observers(n):
        first = rng.integers(0, pool - k + 1, n)
        return (first[:, None] + np.arange(k)[None, :]).reshape(-1)          # pool index, ascending per landmark

    def project(P, who):
        Pc = np.einsum("nij,nj->ni", Ti[who][:, :3, :3], P) + Ti[who][:, :3, 3]
        return np.stack([cam.cx + cam.fx * Pc[:, 0] / Pc[:, 2], cam.cy + cam.fy * Pc[:, 1] / Pc[:, 2]], 1)

    P = np.stack([rng.uniform(-2, 2, n_pt), rng.uniform(-1.5, 1.5, n_pt), rng.uniform(4, 10, n_pt)], 1)
    A = np.stack([rng.uniform(-2, 2, n_ls), rng.uniform(-1.5, 1.5, n_ls), rng.uniform(4, 10, n_ls)], 1)
    Lw = np.concatenate([A, A + rng.uniform(-0.8, 0.8, (n_ls, 3))], 1)
    pw, lw = observers(n_pt), observers(n_ls)
    pt_lm, ls_lm = np.repeat(np.arange(n_pt), k), np.repeat(np.arange(n_ls), k)
    pt_obs = project(P[pt_lm], pw) + 0.5 * rng.standard_normal((len(pw), 2))
    p, q = project(Lw[ls_lm, :3], lw), project(Lw[ls_lm, 3:], lw)
    l = np.cross(np.concatenate([p, np.ones((len(p), 1))], 1), np.concatenate([q, np.ones((len(q), 1))], 1))
    l = l / np.sqrt(l[:, 0:1] ** 2 + l[:, 1:2] ** 2)
    l[:, 2] += 0.5 * rng.standard_normal(len(l))
    slot = lambda w: np.where(w == 0, -1, w - 1)
    return gfpl.LbaProblem(np.array([LR.logmap_se3(T) for T in T_est]).reshape(-1, 6), np.array(T_est).reshape(-1, 16),
                           np.array(T_true[0]).reshape(1, 16), P + 0.05 * rng.standard_normal(P.shape),
                           Lw + 0.05 * rng.standard_normal(Lw.shape), pt_lm, slot(pw), pt_obs,
                           rng.uniform(0.5, 2.0, len(pw)), ls_lm, slot(lw), l.reshape(-1, 3), rng.uniform(0.5, 2.0, len(lw)))


def timed(gfpl, torch, ctx, solver, solve, prob, prm, warmup, repeats):
    dev = torch.device("cuda", ctx.device)
    d = {k: torch.from_numpy(prob.a[k].copy()).to(dev) for k, _ in gfpl.LBA_DOUBLES}
    d["x_out"] = d["x_kf"].clone()
    pristine = {k: d[k].clone() for k in ("T_kf", "pt", "ls")}
    structs = (gfpl.LbaProblemStruct * 1)()
    structs[0] = prob.struct(d)
    out = (gfpl.LbaResult * 1)()
    ms = []
    for rep in range(warmup + repeats):
        for k, v in pristine.items():
            d[k].copy_(v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gfpl.check(solve(solver.h, structs, 1, C.byref(prm), out), "solve")
        t1 = time.perf_counter()
        if rep >= warmup:
            ms.append((t1 - t0) * 1e3)
    return ms, out[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-kf", type=int, default=200)
    ap.add_argument("--n-pt", type=int, default=20000)
    ap.add_argument("--n-ls", type=int, default=4000)
    ap.add_argument("--obs", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--lambda-k", type=float, default=3.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--compare-lba", action="store_true")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_gba: no GPU (nothing is measured without one)")
    import gfpl
    import lba_cases as LC
    import loop_closure_ref as LR
    import oracle as O
    cam, cfg = LC.setup()
    ctx = gfpl.Context(cam, cfg)
    prob = make_map(gfpl, O, LR, cam, 900, a.n_kf, a.n_pt, a.n_ls, a.obs)
    rc, cnt = gfpl.gbaCheck(prob)
    gfpl.check(rc, "gba_check")
    prm = gfpl.LbaParams.default(max_iters=a.max_iters, lambda_k=a.lambda_k)
    solver = gfpl.GbaSolver(ctx, cnt, 1)
    ms, r = timed(gfpl, torch, ctx, solver, ctx.L.gfpl_gba_solve, prob, prm, a.warmup, a.repeats)
    solver.close()
    _, hbm, lds = gfpl.gbaWorkspace(cnt)
    med = float(np.median(ms))
    res = {"bench": "gba", "device": torch.cuda.get_device_name(0), "n_kf": a.n_kf, "n_pt": a.n_pt, "n_ls": a.n_ls,
           "obs_per_landmark": a.obs, "pairs": cnt.n_pt_pairs + cnt.n_ls_pairs, "terms": cnt.n_terms, "max_iters": a.max_iters,
           "lambda_k": a.lambda_k, "iters_run": r.iters, "stop": r.stop, "status": r.status, "workspace_bytes": hbm,
           "lds_bytes": lds, "launches_per_iteration": 11 + a.n_kf, "call_ms": [round(x, 3) for x in ms],
           "median_call_ms": med, "ms_per_iteration": med / max(r.iters, 1)}
    if a.compare_lba:
        lsolver = gfpl.LbaSolver(ctx, [getattr(prob.counts, f) for f, _ in gfpl.LbaCounts._fields_], 1)
        lms, lr = timed(gfpl, torch, ctx, lsolver, ctx.L.gfpl_lba_solve, prob, prm, a.warmup, a.repeats)
        lsolver.close()
        res["lba"] = {"call_ms": [round(x, 3) for x in lms], "median_call_ms": float(np.median(lms)), "iters_run": lr.iters,
                      "stop": lr.stop, "status": lr.status}
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
