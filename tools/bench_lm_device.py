#!/usr/bin/env python3
"""gfpl_lmstore_observe_pairs against the host route on one MI355X (k_lm_plan.hip): one
JSON line per size.

A workload is --pairs pairs of one keyframe-pair stage on a map whose landmarks hold lists of
[--len-min, --len-max] - 1 rows: every pair carries its own landmark (one ADD per landmark, §5o's workload),
except a --created share of them, which create theirs (two ADDs).  The arrays pairs / lm_out are on the
device, where gfpl_kfmap_observe_pairs leaves them.  Two routes are timed on two stores of equal content,
alternating, each after --warmup untimed rounds, --repeats times, median and spread reported:
  device : one gfpl_lmstore_observe_pairs;
  host   : what a caller had before it: pairs and lm_out copied to the host, the gfpl_lm_op list built from
           them (vectorised: no Python loop is charged to it), one gfpl_lmstore_apply.
Each is given as the host clock around it (ending in the call's synchronise) and as the device time between
the call's first and last kernel (gfpl_lmstore_debug_ms).  Every round is undone by an untimed host apply
(ERASE_OBS of the added row, FREE of a created landmark).  Before the timing the two stores are compared:
counts and median rows of every landmark must be equal.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gf-pl-slam_amd"))


def ops_array(lm, kind, arg, src=0):
    o = np.zeros((len(lm), 4), np.int32)
    o[:, 0], o[:, 1], o[:, 2], o[:, 3] = lm, kind, arg, src
    return o


def host_ops(pairs, lm_out, first_new, ADD):
    """the op list of include/gfpl.h's observe_pairs from host copies, in pair order (numpy, no Python loop)"""
    live = lm_out >= 0
    created = live & (lm_out >= first_new)
    n_ops = live.astype(np.int64) + created
    at = np.cumsum(n_ops) - n_ops
    o = np.zeros((int(n_ops.sum()), 4), np.int32)
    o[:, 1] = ADD
    c, k = at[created], at[live & ~created]
    o[c, 0], o[c, 2], o[c, 3] = lm_out[created], pairs[created, 0], 0
    o[c + 1, 0], o[c + 1, 2], o[c + 1, 3] = lm_out[created], pairs[created, 1], 1
    o[k, 0], o[k, 2], o[k, 3] = lm_out[live & ~created], pairs[live & ~created, 1], 1
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--len-min", type=int, default=2)
    ap.add_argument("--len-max", type=int, default=6)
    ap.add_argument("--created", type=float, default=0.0, help="share of the pairs that create their landmark")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_device: no GPU (nothing is measured without one)")
    import gfpl
    cfg = gfpl.default_config()
    ctx = gfpl.Context(gfpl.make_camera("vga", cfg), cfg)
    rng = np.random.default_rng(1)
    N = a.pairs
    n_new = int(N * a.created)
    n_old = N - n_new                                   # landmarks [0, n_old) exist, [n_old, N) are created by the call
    length = rng.integers(a.len_min, a.len_max + 1, n_old).astype(np.int64)   # an existing landmark's list after the call
    obs_cap = max(int(length.max()) if n_old else 2, 2)
    desc0 = torch.randint(0, 256, (N, 32), dtype=torch.uint8, device="cuda")
    desc1 = torch.randint(0, 256, (N, 32), dtype=torch.uint8, device="cuda")
    fill = torch.randint(0, 256, (int((length - 1).sum()) + 1, 32), dtype=torch.uint8, device="cuda")
    head = ops_array(np.repeat(np.arange(n_old), length - 1), gfpl.LM_ADD, np.arange(int((length - 1).sum())))
    # pair i: rows (i, perm[i]); the carried landmarks in a shuffled order, the created ids ascending as the kfmap numbers them
    lm_out = np.full(N, -1, np.int32)
    is_new = np.zeros(N, bool)
    is_new[rng.choice(N, n_new, replace=False)] = True
    lm_out[is_new] = n_old + np.arange(n_new)
    lm_out[~is_new] = rng.permutation(n_old)
    pairs = np.stack([np.arange(N), rng.permutation(N)], 1).astype(np.int32)
    d_pairs, d_out = torch.from_numpy(pairs).cuda(), torch.from_numpy(lm_out).cuda()
    undo = np.concatenate([ops_array(np.arange(n_old), gfpl.LM_ERASE_OBS, length - 1), ops_array(n_old + np.arange(n_new), gfpl.LM_FREE, 0)])
    max_ops = max(2 * N, len(head), len(undo))          # (the fill is one apply)
    stores = {k: gfpl.LandmarkStore(ctx, N, obs_cap, max_ops) for k in ("device", "host")}
    for st in stores.values():
        if len(head):
            st.apply(head, [fill])

    def device_route(st):
        st.observe_pairs(desc0, desc1, d_pairs, d_out, n_old)

    def host_route(st):
        p, o = d_pairs.cpu().numpy(), d_out.cpu().numpy()
        st.apply(host_ops(p, o, n_old, gfpl.LM_ADD), [desc0, desc1])

    routes = {"device": device_route, "host": host_route}
    # the two routes leave the same store
    for k, st in stores.items():
        routes[k](st)
    ids = np.arange(N, dtype=np.int32)
    assert np.array_equal(stores["device"].counts(), stores["host"].counts())
    assert torch.equal(stores["device"].gather(ids), stores["host"].gather(ids))
    for st in stores.values():
        st.apply(undo, [])
    wall = {k: [] for k in routes}
    dev = {k: [] for k in routes}
    for rep in range(a.warmup + a.repeats):
        for k in (("device", "host") if rep % 2 == 0 else ("host", "device")):
            st = stores[k]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[k](st)
            t1 = time.perf_counter()
            if rep >= a.warmup:
                wall[k].append((t1 - t0) * 1e3)
                dev[k].append(st.last_device_ms())
            st.apply(undo, [])
    res = {"bench": "lm_device", "gpu": torch.cuda.get_device_name(0), "pairs": N, "created": n_new, "len_min": a.len_min,
           "len_max": a.len_max, "obs_cap": obs_cap, "warmup": a.warmup, "repeats": a.repeats,
           "store_bytes": {k: st.nbytes() for k, st in stores.items()}}
    for k in routes:
        res[k] = {"wall_ms": float(np.median(wall[k])), "wall_ms_all": [round(x, 4) for x in wall[k]],
                  "device_ms": float(np.median(dev[k])), "device_ms_all": [round(x, 4) for x in dev[k]]}
    res["host_over_device_wall"] = res["host"]["wall_ms"] / res["device"]["wall_ms"]
    for st in stores.values():
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
