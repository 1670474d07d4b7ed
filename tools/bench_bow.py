#!/usr/bin/env python3
"""The loop-closure candidate search on one MI355X (k_bow.hip): one JSON line.

A random k = 10, L = 6 vocabulary (1.1 M nodes, 36 MB of node descriptors) built with numpy, and
keyframes of --n-pt point and --n-ls line descriptors.  HIP events on the context's stream around
  transform:  ONE gfpl_bow_transform call over --keyframes point-descriptor sets (k_bow_descend +
              k_bow_finish, the call's scratch allocation and the copy of the counts),
  insert:     ONE BowDatabase.insertKFBowVectorPL against --stored stored keyframes (two transforms of
              one set each, one k_bow_score launch over 2 x (--stored + 1) pairs, the copy of the scores),
  score:      the same pairs through gfpl_bow_score alone.
No target: there is no parent code and no runnable reference for these numbers."""
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


def random_vocab(k, L, seed):
    """a full k-ary tree of depth L, breadth first, random descriptors, idf-like weights"""
    rng = np.random.default_rng(seed)
    n_inner = (k ** L - 1) // (k - 1)
    n = (k ** (L + 1) - 1) // (k - 1)
    child_off = np.zeros(n + 1, np.int64)
    child_off[1:n_inner + 1] = k * np.arange(1, n_inner + 1)
    child_off[n_inner + 1:] = k * n_inner
    child = np.arange(1, n, dtype=np.int32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = np.zeros(n)
    weight[n_inner:] = rng.uniform(0.5, 8.0, n - n_inner)
    word_id = np.full(n, -1, np.int32)
    word_id[n_inner:] = np.arange(n - n_inner)
    return dict(child_off=child_off.astype(np.int32), child=child, desc=desc, weight=weight, word_id=word_id)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=6)
    ap.add_argument("--n-pt", type=int, default=2000)
    ap.add_argument("--n-ls", type=int, default=500)
    ap.add_argument("--keyframes", type=int, default=1024)
    ap.add_argument("--stored", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=1024, help="generated keyframes (repeated beyond)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bow: no GPU (nothing is measured without one)")
    import gfpl
    import loop_closure_cases as LC
    cam, cfg = LC.setup()
    ctx = gfpl.Context(cam, cfg)
    vp, vl = random_vocab(a.k, a.L, 1), random_vocab(a.k, a.L, 2)
    voc_p, voc_l = gfpl.Vocabulary(ctx, **vp), gfpl.Vocabulary(ctx, **vl)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    pts = [torch.randint(0, 256, (a.n_pt, 32), dtype=torch.uint8, device=dev, generator=g) for _ in range(a.distinct)]
    lss = [torch.randint(0, 256, (a.n_ls, 32), dtype=torch.uint8, device=dev, generator=g) for _ in range(a.distinct)]
    sets = [pts[i % a.distinct] for i in range(a.keyframes)]
    # the C call itself, on preallocated outputs (the mirror's result copies are not part of it)
    import ctypes as C
    ptrs = (C.c_void_p * a.keyframes)(*[t.data_ptr() for t in sets])
    cnt = (C.c_int * a.keyframes)(*[a.n_pt] * a.keyframes)
    ids = torch.zeros((a.keyframes, a.n_pt), dtype=torch.int32, device=dev)
    vals = torch.zeros((a.keyframes, a.n_pt), dtype=torch.float64, device=dev)
    nw = (C.c_int * a.keyframes)()
    torch.cuda.synchronize()

    def transform():
        gfpl.check(ctx.L.gfpl_bow_transform(ctx.h, voc_p.h, a.keyframes, ptrs, cnt, a.n_pt, ids.data_ptr(), vals.data_ptr(),
                                            nw), "bow_transform")

    ms_tr = timed(torch, transform, a.warmup, a.repeats)
    words = list(nw[:a.distinct])
    del ids, vals

    def fill(db):
        for i in range(a.stored):
            db.insertKFBowVectorPL(i, stats=stats, pdesc=pts[i % a.distinct], ldesc=lss[i % a.distinct])

    stats = gfpl.bowStats(np.random.default_rng(4).uniform(0, 640, (a.n_pt, 2)), np.zeros((a.n_ls, 2)),
                          np.random.default_rng(5).uniform(0, 640, (a.n_ls, 2)))
    ms_ins = []
    db = gfpl.BowDatabase(ctx, voc_p, voc_l, gfpl.BOW_MODE_PL, a.stored + a.warmup + a.repeats, a.n_pt, a.n_ls)
    fill(db)
    row = np.zeros(a.stored + a.warmup + a.repeats)
    for r in range(a.warmup + a.repeats):   # each insert sees one stored keyframe more than the one before
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        db.insertKFBowVectorPL(a.stored + r, stats=stats, row=row, pdesc=pts[r % a.distinct], ldesc=lss[r % a.distinct])
        e1.record()
        e1.synchronize()
        if r >= a.warmup:
            ms_ins.append(e0.elapsed_time(e1))
    new_p, new_l = db.vector_device(0, a.stored), db.vector_device(1, a.stored)
    va = [new_p] * (a.stored + 1) + [new_l] * (a.stored + 1)
    vb = [db.vector_device(0, i) for i in range(a.stored + 1)] + [db.vector_device(1, i) for i in range(a.stored + 1)]
    n_pairs = len(va)
    ca, cb = (gfpl.BowVec * n_pairs)(*va), (gfpl.BowVec * n_pairs)(*vb)
    sc = torch.zeros(n_pairs, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ms_sc = timed(torch, lambda: gfpl.check(ctx.L.gfpl_bow_score(ctx.h, ca, cb, n_pairs, sc.data_ptr()), "bow_score"),
                  a.warmup, a.repeats)
    db.close()
    voc_p.close()
    voc_l.close()
    ctx.close()
    med = lambda v: float(np.median(v))
    out = {"bench": "bow", "device": torch.cuda.get_device_name(0), "k": a.k, "L": a.L, "nodes": int(len(vp["weight"])),
           "n_pt": a.n_pt, "n_ls": a.n_ls, "keyframes": a.keyframes, "stored": a.stored,
           "words_per_point_vector": [int(min(words)), int(max(words))],
           "transform_ms": [round(x, 3) for x in ms_tr], "insert_ms": [round(x, 3) for x in ms_ins],
           "score_ms": [round(x, 3) for x in ms_sc],
           "median_transform_ms": med(ms_tr), "median_insert_ms": med(ms_ins), "median_score_ms": med(ms_sc),
           "descriptors_per_s": a.keyframes * a.n_pt / (med(ms_tr) * 1e-3),
           "pairs_per_s": 2 * (a.stored + 1) / (med(ms_sc) * 1e-3)}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
