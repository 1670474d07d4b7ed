#!/usr/bin/env python3
"""Landmark fusion on one MI355X (gfpl_lmstore_fuse, gfpl_map_fuse_search): one JSON
line per workload.

--what store : --merges merges of a source landmark into a destination (GFPL_LM_APPEND_LM then
  GFPL_LM_FREE, loopClosureFuseLandmarks' fourth case), list lengths drawn from [--len-min, --len-max].
  `fuse` is one gfpl_lmstore_fuse.  `round_trip` is what a caller had before it, from the entry points
  of gfpl_lmstore_apply's time: gfpl_lmstore_read of every source into one host array, one upload of
  that array, one gfpl_lmstore_apply with an ADD per row and a FREE per source.  Each is given as the
  host clock around it and as the device time of its kernels (gfpl_lmstore_debug_ms).  Between the
  timed rounds an untimed apply puts the lists back.
--what search : one map of --rows rows per kind from the generator of tests/fuse_search_cases.py.
  `call` is the host clock around gfpl_map_fuse_search, `select` / `knn2` / `gate` the device time of
  its launches per kind (gfpl_map_fuse_debug_ms).  `host_gates` is the same search from
  gfpl_knn2_hamming on the selected descriptors plus the select and the gates in numpy on the host
  (tests/lm_fuse_ref.py with the knn-2 replaced), which is what a caller could assemble before.
Every timing is the median of --repeats rounds after --warmup untimed ones.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gf-pl-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def ops_array(lm, kind, arg):
    o = np.zeros((len(lm), 4), np.int32)
    o[:, 0], o[:, 1], o[:, 2] = lm, kind, arg
    return o


def med(v):
    return float(np.median(v))


def bench_store(a, gfpl, ctx, torch):
    rng = np.random.default_rng(1)
    M = a.merges
    dlen = rng.integers(a.len_min, a.len_max + 1, M).astype(np.int64)
    slen = rng.integers(a.len_min, a.len_max + 1, M).astype(np.int64)
    obs_cap = int((dlen + slen).max())
    length = np.stack([dlen, slen], 1).reshape(-1)          # landmark 2i the destination, 2i + 1 the source
    total = int(length.sum())
    first = np.concatenate([[0], np.cumsum(length)[:-1]])
    src = torch.randint(0, 256, (total, 32), dtype=torch.uint8, device="cuda")
    lm_of = np.repeat(np.arange(2 * M), length)
    build = ops_array(lm_of, gfpl.LM_ADD, np.arange(total))
    st = gfpl.LandmarkStore(ctx, 2 * M, obs_cap, 2 * total)
    st.apply(build, [src])
    dst, srcs = 2 * np.arange(M), 2 * np.arange(M) + 1
    fuse = np.zeros((2 * M, 4), np.int32)
    fuse[0::2] = ops_array(dst, gfpl.LM_APPEND_LM, srcs)
    fuse[1::2] = ops_array(srcs, gfpl.LM_FREE, 0)
    # undo: the destinations lose what they gained (from the end), the sources get their rows again
    n_gain = int(slen.sum())
    erase = ops_array(np.repeat(dst, slen), gfpl.LM_ERASE_OBS,
                      np.repeat(dlen + slen, slen) - 1 - (np.arange(n_gain) - np.repeat(np.cumsum(slen) - slen, slen)))
    src_rows = np.repeat(first[srcs], slen) + (np.arange(n_gain) - np.repeat(np.cumsum(slen) - slen, slen))
    refill = ops_array(np.repeat(srcs, slen), gfpl.LM_ADD, src_rows)
    undo = np.concatenate([erase, refill])

    # the round trip's ops: an ADD per source row from the uploaded array (row order = read order), a FREE per source
    rt_ops = np.concatenate([ops_array(np.repeat(dst, slen), gfpl.LM_ADD, np.arange(n_gain)), ops_array(srcs, gfpl.LM_FREE, 0)])
    rows = np.zeros((obs_cap, 32), np.uint8)
    host_rows = np.zeros((n_gain, 32), np.uint8)
    cnt = C.c_int32(0)
    L = st.L

    def round_trip():
        at = 0
        for lm in srcs:
            gfpl.check(L.gfpl_lmstore_read(st.h, int(lm), C.byref(cnt), None, rows.ctypes.data, None), "lmstore_read")
            host_rows[at:at + cnt.value] = rows[:cnt.value]
            at += cnt.value
        up = torch.from_numpy(host_rows).cuda()
        st.apply(rt_ops, [up])

    res = {}
    for tag, fn in (("fuse", lambda: st.fuse(fuse, [src])), ("round_trip", round_trip)):
        host, dev = [], []
        for rep in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if rep >= a.warmup:
                host.append((t1 - t0) * 1e3)
                dev.append(st.last_device_ms())
            st.apply(undo, [src])
        res[tag] = {"host_ms": med(host), "device_ms": med(dev), "host_ms_all": [round(x, 3) for x in host],
                    "device_ms_all": [round(x, 4) for x in dev]}
    res["round_trip_over_fuse_host"] = res["round_trip"]["host_ms"] / res["fuse"]["host_ms"]
    res.update(merges=M, len_min=a.len_min, len_max=a.len_max, rows_moved=n_gain, obs_cap=obs_cap, store_bytes=st.nbytes())
    st.close()
    return res


def bench_search(a, gfpl, ctx, torch, cam):
    import fuse_search_cases as SC
    import lm_fuse_ref as FR
    camd = SC.cam_dict(cam)
    maps = [SC.make_map(camd, a.rows, lines, 1) for lines in (False, True)]
    pt, ls = maps
    fm = gfpl.FuseMap(pt[0], pt[1], pt[2], ls[0], ls[1], ls[2], pt[3], device="cuda")
    host, phases = [], [[], []]
    for rep in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = ctx.fuseSearch(fm)
        t1 = time.perf_counter()
        if rep >= a.warmup:
            host.append((t1 - t0) * 1e3)
            for k in range(2):
                phases[k].append(ctx.fuseSearch_device_ms(k))
    res = {"rows": a.rows, "call_host_ms": med(host), "call_host_ms_all": [round(x, 3) for x in host]}
    for k, tag in enumerate(("points", "lines")):
        p = np.median(np.array(phases[k]), axis=0)
        res[tag] = {"selected": int(len(got[("pt", "ls")[k] + "_loc"])), "pairs": int(len(got[("pt", "ls")[k] + "_pairs"])),
                    "select_ms": float(p[0]), "knn2_ms": float(p[1]), "gate_ms": float(p[2])}

    # the parent's way: select and gates on the host, the knn-2 through gfpl_knn2_hamming
    def host_search(desc, X, kf, T, lines):
        sel = FR.in_image(camd, T[kf], X[:, :3])
        if lines:
            sel &= FR.in_image(camd, T[kf], X[:, 3:])
        loc = np.nonzero(sel)[0]
        d = torch.from_numpy(np.ascontiguousarray(desc[loc])).cuda()
        idx = torch.zeros((len(loc), 2), dtype=torch.int32, device="cuda")
        dist = torch.zeros((len(loc), 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gfpl.check(ctx.knn2(d, len(loc), d, len(loc), 1, idx, dist), "knn2_hamming")
        second = idx.cpu().numpy()[:, 1].astype(np.int64)
        i = np.nonzero(second != np.arange(len(loc)))[0]
        t = second[i]
        ok = FR.line_gate(X[loc], i, t, FR.DEFAULT_FUSE_PARAMS) if lines else FR.point_gate(X[loc], i, t, FR.DEFAULT_FUSE_PARAMS)
        return loc, np.stack([i[ok], t[ok]], 1)
    host = []
    for rep in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [host_search(*m, lines=bool(k)) for k, m in enumerate(maps)]
        t1 = time.perf_counter()
        if rep >= a.warmup:
            host.append((t1 - t0) * 1e3)
    res["host_gates_ms"] = med(host)
    res["host_gates_ms_all"] = [round(x, 3) for x in host]
    res["same_pairs"] = bool(np.array_equal(out[0][1], got["pt_pairs"]) and np.array_equal(out[1][1], got["ls_pairs"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("store", "search"), required=True)
    ap.add_argument("--merges", type=int, default=1 << 10)
    ap.add_argument("--len-min", type=int, default=2)
    ap.add_argument("--len-max", type=int, default=6)
    ap.add_argument("--rows", type=int, default=1 << 10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_fuse: no GPU (nothing is measured without one)")
    import gfpl
    cfg = gfpl.default_config()
    cam = gfpl.make_camera("vga", cfg)
    ctx = gfpl.Context(cam, cfg)
    res = {"bench": "lm_fuse_" + a.what, "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats}
    res.update(bench_store(a, gfpl, ctx, torch) if a.what == "store" else bench_search(a, gfpl, ctx, torch, cam))
    ctx.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
