#!/usr/bin/env python3
"""gfpl_lba_solve on one MI355X (k_lba.hip): one JSON line.

A batch of --problems local bundle adjustments of --n-kf keyframes, --n-pt points and --n-ls lines with
--obs observations per landmark (--distinct generated problems, repeated over the batch; every copy
does the same work), resident in HBM.  Each repeat restores the in / out arrays (T_kf, pt, ls) from
pristine device copies outside the timed region, then times ONE gfpl_lba_solve on the host clock: the
check of the index arrays, their staging and upload, the k_lba launch, the result copy and the call's
one synchronisation.  lambda_k defaults to 3 so that no problem meets a stop test before --max-iters
(with the reference's 10 the damping passes 1e17 after some 14 iterations and |DX| < eps ends the
problem).  The kernel's own time is read from a kernel trace of this script (rocprofv3 --kernel-trace
--stats), not measured here."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--n-kf", type=int, default=8)
    ap.add_argument("--n-pt", type=int, default=1500)
    ap.add_argument("--n-ls", type=int, default=300)
    ap.add_argument("--obs", type=int, default=4)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--lambda-k", type=float, default=3.0)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lba: no GPU (nothing is measured without one)")
    import gfpl
    import lba_cases as LC
    cam, cfg = LC.setup()
    ctx = gfpl.Context(cam, cfg)
    dev = torch.device("cuda", ctx.device)
    probs = [LC.make_problem(cam, 700 + k, a.n_kf, 2, a.n_pt, a.n_ls, obs=a.obs) for k in range(a.distinct)]
    batch = [probs[i % a.distinct] for i in range(a.problems)]
    caps = [max(getattr(p.counts, f) for p in probs) for f, _ in gfpl.LbaCounts._fields_]
    solver = gfpl.LbaSolver(ctx, caps, a.problems)
    pristine, work = [], []
    structs = (gfpl.LbaProblemStruct * a.problems)()
    for i, p in enumerate(batch):
        d = {k: torch.from_numpy(p.a[k].copy()).to(dev) for k, _ in gfpl.LBA_DOUBLES}
        d["x_out"] = d["x_kf"].clone()
        pristine.append({k: d[k].clone() for k in ("T_kf", "pt", "ls")})
        work.append(d)
        structs[i] = p.struct(d)
    prm = gfpl.LbaParams.default(max_iters=a.max_iters, lambda_k=a.lambda_k)
    out = (gfpl.LbaResult * a.problems)()
    hbm, lds = probs[0].workspace()
    ms = []
    for rep in range(a.warmup + a.repeats):
        for d, q in zip(work, pristine):
            for k, v in q.items():
                d[k].copy_(v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gfpl.check(ctx.L.gfpl_lba_solve(solver.h, structs, a.problems, C.byref(prm), out), "lba_solve")
        t1 = time.perf_counter()
        if rep >= a.warmup:
            ms.append((t1 - t0) * 1e3)
    iters = sorted({out[i].iters for i in range(a.problems)})
    stops = sorted({out[i].stop for i in range(a.problems)})
    status = sorted({out[i].status for i in range(a.problems)})
    solver.close()
    ctx.close()
    med = float(np.median(ms))
    res = {"bench": "lba", "device": torch.cuda.get_device_name(0), "problems": a.problems, "n_kf": a.n_kf, "n_pt": a.n_pt,
           "n_ls": a.n_ls, "obs_per_landmark": a.obs, "max_iters": a.max_iters, "lambda_k": a.lambda_k,
           "iters_run": iters, "stops": stops, "status": status, "workspace_bytes_per_problem": hbm, "lds_bytes": lds,
           "call_ms": [round(x, 3) for x in ms], "median_call_ms": med, "problems_per_s": a.problems / (med * 1e-3),
           "ms_per_problem_iteration": med / (a.problems * max(iters))}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
