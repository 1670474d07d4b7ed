#!/usr/bin/env python3
"""gfpl_kf_loop_closure on one MI355X (k_loop.hip): one JSON line.

A batch of --pairs candidate pairs of (--n-pt, --n-ls) features each (--distinct generated pairs,
repeated over the batch; every pair does the same work), resident in HBM.  HIP events on the
context's stream around
  call:  Context.isLoopClosure (per pair 4 knn-2 launches, then ONE k_loop_closure launch, the
         per-call scratch allocation and the result copies),
  knn:   the same 4 x pairs knn-2 launches alone (Context.knn2 on the same descriptors into
         preallocated lists),
  call0: the call with max_iters = 0 (no Gauss-Newton iteration: compaction, outlier pass, gates).
call - knn is k_loop_closure plus the call's allocation and copies; call - call0 is the
Gauss-Newton loop alone."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gf-pl-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--n-pt", type=int, default=2048)
    ap.add_argument("--n-ls", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loop_closure: no GPU (nothing is measured without one)")
    import gfpl
    import loop_closure_cases as LC
    cam, cfg = LC.setup()
    ctx = gfpl.Context(cam, cfg)
    views = []
    for k in range(a.distinct):
        f0, f1 = LC.make_pair(cam, a.n_pt, a.n_ls, seed=500 + k)
        views.append((gfpl.KeyFrameView(f0, np.eye(4), "cuda"), gfpl.KeyFrameView(f1, np.eye(4), "cuda")))
    v0 = [views[i % a.distinct][0] for i in range(a.pairs)]
    v1 = [views[i % a.distinct][1] for i in range(a.pairs)]
    dev = torch.device("cuda", 0)
    idx = torch.zeros(2 * max(a.n_pt, a.n_ls, 1), dtype=torch.int32, device=dev)
    dist = torch.zeros(2 * max(a.n_pt, a.n_ls, 1), dtype=torch.float32, device=dev)

    def knn_only():
        for k0, k1 in zip(v0, v1):
            for d, n in (("pdesc", a.n_pt), ("ldesc", a.n_ls)):
                if n >= 2:
                    ctx.knn2(k0.keep[d], n, k1.keep[d], n, 1, idx, dist)
                    ctx.knn2(k1.keep[d], n, k0.keep[d], n, 1, idx, dist)

    res = {}

    def call():
        res["r"] = ctx.isLoopClosure(v0, v1)

    ms_call = timed(torch, call, a.warmup, a.repeats)
    accepted = sum(r[0].is_lc for r in res["r"])
    iters = sorted({r[0].iters for r in res["r"]})
    ms_knn = timed(torch, knn_only, a.warmup, a.repeats)
    ctx.set_config(gfpl.default_config(max_iters=0))
    ms_call0 = timed(torch, call, a.warmup, a.repeats)
    ctx.close()
    med = lambda v: float(np.median(v))
    out = {"bench": "loop_closure", "device": torch.cuda.get_device_name(0), "pairs": a.pairs, "n_pt": a.n_pt,
           "n_ls": a.n_ls, "max_iters": int(cfg.max_iters), "iters_run": iters, "accepted": accepted,
           "call_ms": [round(x, 3) for x in ms_call], "knn_ms": [round(x, 3) for x in ms_knn],
           "call_max_iters_0_ms": [round(x, 3) for x in ms_call0],
           "median_call_ms": med(ms_call), "median_knn_ms": med(ms_knn),
           "median_call_minus_knn_ms": med(ms_call) - med(ms_knn),
           "median_gauss_newton_ms": med(ms_call) - med(ms_call0),
           "pairs_per_s": a.pairs / (med(ms_call) * 1e-3)}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
