#!/usr/bin/env python3
"""gfpl_lmstore_apply / _gather on one MI355X (k_lm.hip): one JSON line per workload.

A workload is --landmarks landmarks whose final list lengths are drawn uniformly from
[--len-min, --len-max].  Two applies are timed, each after --warmup untimed rounds, --repeats times,
median reported:
  append : every landmark holds its list less the last observation and one call adds that one
           (a keyframe tick: one ADD per matched landmark); undone by an untimed ERASE_OBS call;
  build  : every landmark is empty and one call adds its whole list; undone by an untimed FREE call;
and one gather of all landmarks' median rows in a shuffled order.  Each timing is given twice: the
host clock around the call (the planner, the staging, the upload, the kernels, the synchronise) and
the device time between the call's first and last kernel (gfpl_lmstore_debug_ms).  `forced64` repeats
the two applies on a store created under GFPL_LM_MIN_LANES=64 (the variable is read when a store is
created), i.e. every landmark through k_lm_apply<64>, the kernel the lane-group buckets are measured
against.  `bytes` of an apply are the descriptor rows the algorithm needs: list rows read, source rows
read, rows written, median rows written (32 B each), over the device time; the peak is HBM's.  What
the kernel moves besides them is given as `list_bytes` and is not in the rate: a 16-B work item and
8 B of count and med_idx per landmark, 16 B per op.  A gather moves 76 B per id: the id, the median row
read and written, med_idx read and written.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gf-pl-slam_amd"))

HBM_PEAK = 8.0e12   # bytes/s, the MI355X's HBM3E specification


def ops_array(lm, kind, arg):
    o = np.zeros((len(lm), 4), np.int32)
    o[:, 0], o[:, 1], o[:, 2] = lm, kind, arg
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=1 << 20)
    ap.add_argument("--len-min", type=int, default=2)
    ap.add_argument("--len-max", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-forced", action="store_true", help="skip the GFPL_LM_MIN_LANES=64 runs")
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_store: no GPU (nothing is measured without one)")
    import gfpl
    cfg = gfpl.default_config()
    ctx = gfpl.Context(gfpl.make_camera("vga", cfg), cfg)
    rng = np.random.default_rng(1)
    N = a.landmarks
    length = rng.integers(a.len_min, a.len_max + 1, N).astype(np.int64)
    total = int(length.sum())
    obs_cap = int(length.max())
    # one source: landmark i's observations are rows first[i] .. first[i] + length[i]
    first = np.concatenate([[0], np.cumsum(length)[:-1]])
    src = torch.randint(0, 256, (total, 32), dtype=torch.uint8, device="cuda")
    lm_of = np.repeat(np.arange(N), length)
    k_of = np.arange(total) - np.repeat(first, length)
    last = k_of == np.repeat(length - 1, length)
    # ops interleaved across the landmarks (observation k of every landmark before k + 1 of any), as
    # keyframes arrive, so that the planner's grouping has work to do
    by_round = np.argsort(k_of, kind="stable")
    build = ops_array(lm_of[by_round], gfpl.LM_ADD, np.arange(total)[by_round])
    head = ops_array(lm_of[by_round][~last[by_round]], gfpl.LM_ADD, np.arange(total)[by_round][~last[by_round]])
    append = ops_array(np.arange(N), gfpl.LM_ADD, first + length - 1)
    un_append = ops_array(np.arange(N), gfpl.LM_ERASE_OBS, length - 1)
    free = ops_array(np.arange(N), gfpl.LM_FREE, 0)

    def timed(ops, undo):
        host, devms = [], []
        for rep in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.apply(ops, [src])
            t1 = time.perf_counter()
            if rep >= a.warmup:
                host.append((t1 - t0) * 1e3)
                devms.append(st.last_device_ms())
            st.apply(undo, [src])
        return float(np.median(host)), float(np.median(devms)), [round(x, 3) for x in devms]

    res = {"bench": "lm_store", "device": torch.cuda.get_device_name(0), "landmarks": N, "len_min": a.len_min,
           "len_max": a.len_max, "observations": total, "obs_cap": obs_cap, "warmup": a.warmup, "repeats": a.repeats}
    # rows read + source rows read + rows written + medians written; the lists the kernel reads beside them
    bytes_append, lists_append = 32 * (int((length - 1).sum()) + N + N + N), (16 + 8 + 16) * N
    bytes_build, lists_build = 32 * (total + total + N), (16 + 8) * N + 16 * total

    def entry(h, d, all_d, nbytes, lists):
        return {"host_ms": h, "device_ms": d, "device_ms_all": all_d, "landmarks_per_s": N / (d * 1e-3), "bytes": nbytes,
                "list_bytes": lists, "bytes_per_s": nbytes / (d * 1e-3), "share_of_hbm_peak": nbytes / (d * 1e-3) / HBM_PEAK}

    st = None
    for tag, env in (("forced64", "64"), ("buckets", None))[1 if a.no_forced else 0:]:
        if st is not None:
            st.close()
        if env is None:
            os.environ.pop("GFPL_LM_MIN_LANES", None)
        else:
            os.environ["GFPL_LM_MIN_LANES"] = env
        st = gfpl.LandmarkStore(ctx, N, obs_cap, total)
        os.environ.pop("GFPL_LM_MIN_LANES", None)
        if len(head):
            st.apply(head, [src])
        res[tag + "_append"] = entry(*timed(append, un_append), bytes_append, lists_append)
        st.apply(free, [src])
        res[tag + "_build"] = entry(*timed(build, free), bytes_build, lists_build)
    res["store_bytes"] = st.nbytes()
    if not a.no_forced:
        res["forced64_over_buckets"] = {"append": res["forced64_append"]["device_ms"] / res["buckets_append"]["device_ms"],
                                        "build": res["forced64_build"]["device_ms"] / res["buckets_build"]["device_ms"]}
    st.apply(build, [src])
    ids = rng.permutation(N).astype(np.int32)
    host, devms = [], []
    for rep in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.gather(ids)
        t1 = time.perf_counter()
        if rep >= a.warmup:
            host.append((t1 - t0) * 1e3)
            devms.append(st.last_device_ms())
    d = float(np.median(devms))
    res["gather"] = {"host_ms": float(np.median(host)), "device_ms": d, "landmarks_per_s": N / (d * 1e-3),
                     "bytes": 76 * N, "bytes_per_s": 76 * N / (d * 1e-3), "share_of_hbm_peak": 76 * N / (d * 1e-3) / HBM_PEAK}
    st.close()
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
