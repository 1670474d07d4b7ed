#!/usr/bin/env python3
"""gfpl_kfmap on one MI355X (k_kfmap.hip): one JSON line.

The map: --keyframes keyframes of --pt-rows / --ls-rows features, --landmarks point landmarks (a
quarter as many lines) with lists of 2..6 keyframes, written through the patch calls; a --local
fraction of the landmarks is local.  Then --ticks keyframe ticks run the calls of addKeyFrame in
order (add, observe pairs with --pairs pairs, select LOCAL_UNSEEN + unmatched, observe local, form
local map, remove bad) and the two other selections.  Every call is timed twice: the host clock
around it (argument checks, launches, the header's copy, the call's one synchronisation) and the
device time between its first and last kernel (gfpl_kfmap_debug_ms); the median over the ticks is
reported.  `empty_call` is a set_inlier of no ids: no kernel, so its host time is what the header
reset, the copy and the synchronisation cost every call.
For the selections `bytes` are what the three launches must move: the flag bytes read by the reduce
and again by the scatter (alive; local too for LOCAL / LOCAL_UNSEEN), for LOCAL_UNSEEN one 4-B length
and one 4-B list entry per alive local landmark in each pass, and 4 B per id written; `hbm_frac` is
bytes / device time over the HBM peak.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gf-pl-slam_amd"))

HBM_PEAK = 8.0e12   # bytes/s, the MI355X's HBM3E specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=256)
    ap.add_argument("--pt-rows", type=int, default=2048)
    ap.add_argument("--ls-rows", type=int, default=512)
    ap.add_argument("--landmarks", type=int, default=1 << 20)
    ap.add_argument("--obs-cap", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--local", type=float, default=0.05)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kfmap: no GPU (nothing is measured without one)")
    import gfpl
    cfg = gfpl.default_config()
    ctx = gfpl.Context(gfpl.make_camera("vga", cfg), cfg)
    rng = np.random.default_rng(1)
    K, N = a.keyframes, (a.landmarks, a.landmarks // 4)
    rows = (a.pt_rows, a.ls_rows)
    slack = a.ticks * a.pairs
    km = gfpl.KeyframeMap(ctx, K, rows[0], rows[1], N[0] + slack, N[1] + slack, a.obs_cap)
    K0 = K - a.ticks
    for _ in range(K0):
        km.add_keyframe(*rows)
    for kind in (0, 1):
        n = N[kind]
        nobs = rng.integers(2, min(6, a.obs_cap - 1) + 1, n).astype(np.int32)
        first = rng.integers(0, K0 - a.obs_cap, n)
        obs = (first[:, None] + np.arange(a.obs_cap)[None, :]).astype(np.int32)      # consecutive keyframes from `first`
        local = (rng.random(n) < a.local).astype(np.uint8)
        km.write_landmarks(kind, 0, np.ones(n, np.uint8), local, np.ones(n, np.uint8), nobs, first.astype(np.int32), obs)
        for k in range(K0):
            idx = rng.integers(0, n, rows[kind]).astype(np.int32)
            idx[rng.random(rows[kind]) < 0.3] = -1
            km.write_keyframe_idx(kind, k, 0, idx)

    times = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        host = (time.perf_counter() - t0) * 1e3
        times.setdefault(name, []).append((host, km.last_device_ms()))
        return r

    prm = gfpl.KfMapParams.default(min_lm_obs=3)   # the first tick culls the old two-observation landmarks
    counts = {}
    for tick in range(a.ticks):
        kf = timed("add_keyframe", lambda: km.add_keyframe(*rows))
        for kind in (0, 1):
            tag = "pt" if kind == 0 else "ls"
            n_pairs = min(a.pairs, rows[kind])
            pairs = np.stack([rng.permutation(rows[kind])[:n_pairs], rng.permutation(rows[kind])[:n_pairs]], 1).astype(np.int32)
            pairs = torch.from_numpy(pairs).cuda()
            out, first, new = timed("observe_pairs_" + tag, lambda: km.observe_pairs(kind, kf - 1, kf, pairs))
            sel = timed("select_local_unseen_" + tag, lambda: km.select(kind, gfpl.KFMAP_LOCAL_UNSEEN, kf))
            unm = timed("unmatched_" + tag, lambda: km.unmatched(kind, kf))
            n_loc = min(a.pairs // 4, len(sel), len(unm))
            lp = np.stack([rng.permutation(len(sel))[:n_loc], rng.permutation(len(unm))[:n_loc]], 1).astype(np.int32)
            lp = torch.from_numpy(lp).cuda()
            timed("observe_local_" + tag, lambda: km.observe_local(kind, kf, lp, sel, unm))
            counts[tag] = dict(pairs=n_pairs, created=new, local_unseen=len(sel), unmatched=len(unm), local_pairs=n_loc)
        timed("form_local_map", lambda: km.form_local_map(prm))
        rem = timed("remove_bad", lambda: km.remove_bad(prm))
        counts["removed"] = [len(rem[0]), len(rem[1])]
        loc = timed("select_local_pt", lambda: km.select(0, gfpl.KFMAP_LOCAL))
        alv = timed("select_alive_pt", lambda: km.select(0, gfpl.KFMAP_ALIVE))
        counts["local_pt"], counts["alive_pt"] = len(loc), len(alv)
        timed("empty_call", lambda: km.set_inlier(0, np.zeros(0, np.int32), 1))
    res = {name: dict(host_ms=round(statistics.median(h for h, _ in v), 4), device_ms=round(statistics.median(d for _, d in v), 4))
           for name, v in times.items()}
    n_pt = km.counts()[1]
    c = counts
    bytes_of = {
        "select_alive_pt": 2 * n_pt + 4 * c["alive_pt"],
        "select_local_pt": 4 * n_pt + 4 * c["local_pt"],
        "select_local_unseen_pt": 4 * n_pt + 16 * c["local_pt"] + 4 * c["pt"]["local_unseen"],
    }
    for name, b in bytes_of.items():
        ms = res[name]["device_ms"]
        res[name].update(bytes=int(b), hbm_frac=round(b / (ms * 1e-3) / HBM_PEAK, 5) if ms > 0 else None)
    line = json.dumps(dict(bench="kfmap", keyframes=K, rows=rows, landmarks=[km.counts()[1], km.counts()[2]], obs_cap=a.obs_cap,
                           ticks=a.ticks, device_bytes=km.nbytes(), counts=counts, calls=res, hbm_peak=HBM_PEAK))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    km.close()
    ctx.close()


if __name__ == "__main__":
    main()
