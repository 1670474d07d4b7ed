#!/usr/bin/env python3
"""gfpl_mapgeo on one MI355X (k_mapgeo.hip): one JSON line.

The map: --keyframes keyframes translating sideways, --landmarks points (a quarter as many segments)
4 to 10 m in front of them, each observed by 3..6 (segments 6..8) consecutive keyframes through projection plus pixel
noise (true poses with small rotations, stored poses a little off them), written through the patch
calls of the two objects; the last --local keyframes are local and so is every landmark one of them
observes.  Measured:

  observe_*   one tick's observe calls on a new keyframe (--pairs pairs per kind, half of them
              creating): device ms between the first and last kernel (gfpl_mapgeo_debug_ms) and the
              host clock around the call.
  assemble    gfpl_mapgeo_assemble(LOCAL) without host lists: device ms, host ms.
  lba         gfpl_mapgeo_lba: host clock around the one call (assembly, solve, write-back).
  parent      the route before this object existed, over the same map and from the same state: the
              index half read to the host (gfpl_kfmap_read_landmarks, local_keyframes), the gather of
              INTEGRATION.md §2c over host-resident geometry (vectorised numpy standing in for the
              caller's walk), the upload, gfpl_lba_solve, the download and the scatter into the host
              arrays.  `same_bits` says the two routes left the same poses and landmarks.
Each of lba / parent is the median of --reps runs; the store is restored between runs.
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--local", type=int, default=8)
    ap.add_argument("--pt-rows", type=int, default=2048)
    ap.add_argument("--ls-rows", type=int, default=512)
    ap.add_argument("--landmarks", type=int, default=16384)
    ap.add_argument("--obs-cap", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mapgeo: no GPU (nothing is measured without one)")
    import gfpl
    import loop_closure_ref as LR
    import oracle as O
    cfg = gfpl.default_config()
    cam = gfpl.make_camera("vga", cfg)
    ctx = gfpl.Context(cam, cfg)
    rng = np.random.default_rng(1)
    K, oc = a.keyframes, a.obs_cap
    N = (a.landmarks, a.landmarks // 4)
    caps = (K + 1, a.pt_rows, a.ls_rows, N[0] + a.pairs, N[1] + a.pairs, oc)
    km, geo = gfpl.KeyframeMap(ctx, *caps), gfpl.MapGeometry(ctx, *caps)

    # ---- the map
    # true poses: sideways motion with small rotations; the stored ones carry a little noise
    T_true = [O.expmap_se3(np.concatenate([[0.1 * k, 0.0, 0.0] + rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.03, 0.03, 3)]))
              for k in range(K + 1)]
    Ti_true = np.stack([O.inverse_se3(T) for T in T_true])
    T_est = [T @ O.expmap_se3(rng.uniform(-0.005, 0.005, 6)) for T in T_true]
    T_host = np.stack([np.asarray(T, np.float64).reshape(16) for T in T_est])
    x_host = np.stack([np.asarray(LR.logmap_se3(T), np.float64).reshape(6) for T in T_est])
    for k in range(K):
        km.add_keyframe(a.pt_rows, a.ls_rows)
        geo.set_keyframe(k, T_host[k], x_host[k])
    km.form_local_map(gfpl.KfMapParams.default(min_lm_cov_graph=1 << 30, min_kf_local_map=a.local - 1))

    def project(X, kf):
        Ti = Ti_true[kf]
        Xc = np.einsum("...ij,...j->...i", Ti[..., :3, :3], np.broadcast_to(X, kf.shape + (3,))) + Ti[..., :3, 3]
        return np.stack([cam.cx + cam.fx * Xc[..., 0] / Xc[..., 2], cam.cy + cam.fy * Xc[..., 1] / Xc[..., 2]], -1)

    host = []
    for kind in (0, 1):
        n = N[kind]
        # an observation is one row of the landmark's block (the residual's norm), so a point needs 3 and a
        # segment 6 of them for a block that is not singular
        nobs = rng.integers(6 if kind else 3, min(8 if kind else 6, oc) + 1, n).astype(np.int32)
        first = rng.integers(0, K - 8, n)
        kf_obs = (first[:, None] + np.arange(oc)[None, :]).astype(np.int32)
        kf_obs[kf_obs >= K] = K - 1
        used = np.arange(oc)[None, :] < nobs[:, None]
        local = ((kf_obs >= K - a.local) & used).any(1).astype(np.uint8)
        X = np.stack([rng.uniform(-2, 2, n) + 0.1 * first, rng.uniform(-1.5, 1.5, n), rng.uniform(4, 10, n)], 1)
        if kind == 0:
            obs = project(X[:, None, :], kf_obs) + rng.normal(0, 0.5, (n, oc, 2))
            lm3d = X + rng.normal(0, 0.05, X.shape)
        else:
            Y = X + rng.uniform(-0.8, 0.8, X.shape)
            p, q = project(X[:, None, :], kf_obs), project(Y[:, None, :], kf_obs)
            l = np.cross(np.concatenate([p, np.ones((n, oc, 1))], -1), np.concatenate([q, np.ones((n, oc, 1))], -1))
            l = l / np.sqrt(l[..., :1] ** 2 + l[..., 1:2] ** 2)
            l[..., 2] += rng.normal(0, 0.5, (n, oc))
            obs = l
            lm3d = np.concatenate([X, Y], 1) + rng.normal(0, 0.05, (n, 6))
        sigma = np.ones((n, oc))
        one = np.ones(n, np.uint8)
        km.write_landmarks(kind, 0, one, local, one, nobs, first.astype(np.int32), kf_obs)
        geo.write_landmarks(kind, 0, lm3d, nobs, obs, sigma)
        host.append(dict(lm3d=lm3d.copy(), obs=obs, sigma=sigma, nobs=nobs))

    def restore():
        for k in range(K):
            geo.set_keyframe(k, T_host[k], x_host[k])
        for kind in (0, 1):
            h = host[kind]
            geo.write_landmarks(kind, 0, h["lm3d"], h["nobs"], h["obs"], h["sigma"])

    lba_caps = (gfpl.LBA_MAX_KFS, K, N[0], N[1], N[0] * 6, N[1] * 8)
    solver = gfpl.LbaSolver(ctx, lba_caps, 1)
    prm = gfpl.LbaParams.default()

    # ---- the parent's route
    def parent():
        t = {}
        t["read_ms"], idx = clock(lambda: ([km.read_landmarks(kind, 0, N[kind]) for kind in (0, 1)], km.local_keyframes()))
        lms, kf_list = idx

        def gather():
            slot = np.full(K + 1, np.iinfo(np.int32).min, np.int64)
            slot[kf_list] = np.arange(len(kf_list))
            parts, fixed = [], np.zeros(K + 1, bool)
            for kind in (0, 1):
                d = lms[kind]
                ids = np.nonzero(d["alive"] & d["local"])[0]
                kfs = d["kf_obs"][ids]
                mask = np.arange(oc)[None, :] < d["n_obs"][ids][:, None]
                cnt = mask.sum(1)
                ids, kfs, mask, cnt = ids[cnt > 0], kfs[cnt > 0], mask[cnt > 0], cnt[cnt > 0]
                fixed[kfs[mask][slot[kfs[mask]] < 0]] = True
                parts.append((ids, kfs[mask], np.repeat(np.arange(len(ids)), cnt), mask))
            fix_list = np.nonzero(fixed)[0]
            slot[fix_list] = -1 - np.arange(len(fix_list))
            h0, h1 = host
            (i0, k0, l0, m0), (i1, k1, l1, m1) = parts
            p = gfpl.LbaProblem(x_host[kf_list], T_now[kf_list], T_now[fix_list], lm_now[0][i0], lm_now[1][i1], l0, slot[k0],
                                h0["obs"][i0][m0], h0["sigma"][i0][m0], l1, slot[k1], h1["obs"][i1][m1], h1["sigma"][i1][m1])
            return p, i0, i1
        t["gather_ms"], (p, i0, i1) = clock(gather)
        t["solve_ms"], r = clock(lambda: solver.solve([p], prm)[0])

        def scatter():
            T_now[kf_list] = r["T_kf"].reshape(-1, 16)
            lm_now[0][i0] = r["pt"]
            lm_now[1][i1] = r["ls"]
        t["scatter_ms"], _ = clock(scatter)
        t["total_ms"] = sum(t.values())
        return t, p.counts, r["result"]

    runs = []
    for _ in range(a.reps + 1):
        T_now, lm_now = T_host.copy(), [host[0]["lm3d"].copy(), host[1]["lm3d"].copy()]
        runs.append(parent())
    runs = runs[1:]                                    # (the first run warms the allocator and the kernels up)
    parent_ms = {k: round(statistics.median(r[0][k] for r in runs), 4) for k in runs[0][0]}
    cnt = runs[0][1]
    counts = {f: getattr(cnt, f) for f, _ in gfpl.LbaCounts._fields_}

    # ---- the one call
    lba_ms, asm_host, asm_dev = [], [], []
    for i in range(a.reps + 1):
        restore()
        ms, (res, got) = clock(lambda: geo.lba(km, solver, prm))
        lba_ms.append(ms)
    lba_ms = lba_ms[1:]
    same = tuple(getattr(got, f) for f, _ in gfpl.LbaCounts._fields_) == tuple(counts.values())
    same = same and all(np.array_equal(geo.read_keyframe(k)[0].reshape(16), T_now[k]) for k in range(K))
    for kind in (0, 1):
        same = same and geo.read_landmarks(kind, 0, N[kind])["lm3d"].tobytes() == lm_now[kind].tobytes()
    ref = runs[0][2]
    same = same and (res.iters, res.stop, res.status, res.err) == (ref.iters, ref.stop, ref.status, ref.err)
    for _ in range(a.reps):
        ms, _p = clock(lambda: geo.assemble(km, gfpl.KFMAP_LOCAL, host_lists=False))
        asm_host.append(ms)
        asm_dev.append(geo.last_device_ms())

    # ---- one tick's observe calls on a new keyframe
    restore()
    kf1 = km.add_keyframe(a.pt_rows, a.ls_rows)
    geo.set_keyframe(kf1, T_host[K], x_host[K])
    obs_calls = {}
    for kind, rows in ((0, a.pt_rows), (1, a.ls_rows)):
        n = min(a.pairs, rows)
        arr = lambda w: rng.normal(0, 1, (rows, w)) + ([0, 0, 6] if w == 3 else 0)
        v0 = geo.view(P=arr(3), pl=arr(2), sP=arr(3), eP=arr(3), le=arr(3))
        v1 = geo.view(P=arr(3), pl=arr(2), sP=arr(3), eP=arr(3), le=arr(3))
        carried = np.nonzero(host[kind]["nobs"] < oc - 1)[0][: n // 2].astype(np.int32)
        idx = np.full(rows, -1, np.int32)
        idx[: len(carried)] = carried
        km.write_keyframe_idx(kind, K - 1, 0, idx)
        pairs = np.stack([np.arange(n), rng.permutation(rows)[:n]], 1).astype(np.int32)
        lm_out, first, new = km.observe_pairs(kind, K - 1, kf1, pairs)
        ms, _r = clock(lambda: geo.observe_pairs(kind, K - 1, kf1, v0, v1, pairs, lm_out, first))
        name = "observe_pairs_" + ("ls" if kind else "pt")
        obs_calls[name] = dict(pairs=n, created=new, host_ms=round(ms, 4), device_ms=round(geo.last_device_ms(), 4))
        sel, unm = km.select(kind, gfpl.KFMAP_LOCAL_UNSEEN, kf1), km.unmatched(kind, kf1)
        m = min(n, int(sel.shape[0]), int(unm.shape[0]))
        keep = (km.read_landmarks(kind, 0, N[kind])["n_obs"] < oc)[sel.cpu().numpy()[:m]]
        lp = np.stack([np.arange(m), np.arange(m)], 1).astype(np.int32)[keep]
        lm_loc = km.observe_local(kind, kf1, lp, sel, unm)
        ms, _r = clock(lambda: geo.observe_local(kind, kf1, v1, lp, unm, lm_loc))
        name = "observe_local_" + ("ls" if kind else "pt")
        obs_calls[name] = dict(pairs=len(lp), host_ms=round(ms, 4), device_ms=round(geo.last_device_ms(), 4))

    out = dict(bench="mapgeo", keyframes=K, local_keyframes=a.local, rows=[a.pt_rows, a.ls_rows], landmarks=list(N), obs_cap=oc,
               reps=a.reps, device_bytes=geo.nbytes(), problem=counts, same_bits=bool(same),
               assemble=dict(host_ms=round(statistics.median(asm_host), 4), device_ms=round(statistics.median(asm_dev), 4)),
               lba_ms=round(statistics.median(lba_ms), 4), parent_ms=parent_ms, calls=obs_calls,
               lba_result=dict(iters=res.iters, stop=res.stop, status=res.status, err=res.err))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    for o in (solver, geo, km):
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
