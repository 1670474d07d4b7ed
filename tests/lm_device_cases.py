"""Helpers for the landmark store's device-id calls (tests/test_lm_device_cpu.py, tests/test_lm_device_gpu.py).

The yardstick is the op list a host would build from the same arrays (include/gfpl.h, "the device-id
calls"), run through tests/lm_store_ref.py's Model: pair_ops / local_ops /
free_ops build it from host copies of pairs / lm_out / first_new / unm_rows.  assert_store_is_model
compares a WHOLE store with a Model, every landmark whether a call touched it or not: count, med_idx,
rows [0, count) and the median row, byte for byte.  The one exclusion is the header's: rows at and past
a landmark's count are unspecified ("whatever was last written there"), so they are not compared with
the model; snapshots (a refused call changes nothing) do compare them.
"""
import numpy as np

import lm_store_ref as R

SRC0, SRC1 = 0, 1   # observe_pairs' sources: srcs = [desc0, desc1]; observe_local's srcs = [desc1]


def pair_ops(pairs, lm_out, first_new):
    """gfpl_lmstore_observe_pairs as gfpl_lm_ops over srcs = [desc0, desc1], in pair order"""
    ops = []
    for (p0, p1), lm in zip(np.asarray(pairs, np.int64).reshape(-1, 2).tolist(), np.asarray(lm_out, np.int64).tolist()):
        if lm == -1:
            continue                                   # :308
        if lm >= first_new:                            # a created landmark: kf0's row, then kf1's
            ops += [(lm, R.ADD, p0, SRC0), (lm, R.ADD, p1, SRC1)]
        else:                                          # a carried one
            ops.append((lm, R.ADD, p1, SRC1))
    return ops


def local_ops(pairs, unm_rows, lm_out):
    """gfpl_lmstore_observe_local as gfpl_lm_ops over srcs = [desc1]; column 0 of pairs is not read"""
    unm = np.asarray(unm_rows, np.int64).tolist()
    return [(lm, R.ADD, unm[p1], 0) for (_, p1), lm in zip(np.asarray(pairs, np.int64).reshape(-1, 2).tolist(),
                                                         np.asarray(lm_out, np.int64).tolist()) if lm != -1]


def free_ops(ids):
    return [(int(i), R.FREE, 0, 0) for i in np.asarray(ids, np.int64).tolist()]


def read_all(store):
    """every landmark of a store as gfpl.LandmarkStore.read returns it"""
    return [store.read(lm) for lm in range(store.lm_cap)]


class Expect:
    """Model.expect of every landmark, recomputed only for the landmarks a call named"""

    def __init__(self, model):
        self.model, self.memo = model, {}

    def touched(self, lms):
        for lm in lms:
            self.memo.pop(int(lm), None)

    def of(self, lm):
        if lm not in self.memo:
            self.memo[lm] = self.model.expect(lm)
        return self.memo[lm]


def assert_store_is_model(got, expect, where=""):
    """got: read_all(store); every landmark against the model.  Rows at and past count are not compared
    (unspecified by the header); nothing else is left out."""
    assert len(got) == expect.model.lm_cap
    for lm, g in enumerate(got):
        w = expect.of(lm)
        assert g["count"] == w["count"], (where, lm, "count", g["count"], w["count"])
        assert g["med_idx"] == w["med_idx"], (where, lm, "med_idx", g["med_idx"], w["med_idx"], w["count"])
        assert np.array_equal(g["desc_list"][: w["count"]], w["rows"]), (where, lm, "rows")
        assert np.array_equal(g["med_desc"], w["med_desc"]), (where, lm, "med_desc")


def assert_stores_equal(a, b, where=""):
    """a, b: read_all of two stores fed by the two routes: counts, med_idx, rows below count, median rows"""
    assert len(a) == len(b)
    for lm, (x, y) in enumerate(zip(a, b)):
        assert (x["count"], x["med_idx"]) == (y["count"], y["med_idx"]), (where, lm, x["count"], y["count"], x["med_idx"], y["med_idx"])
        assert np.array_equal(x["desc_list"][: x["count"]], y["desc_list"][: y["count"]]), (where, lm, "rows")
        assert np.array_equal(x["med_desc"], y["med_desc"]), (where, lm, "med_desc")


def snapshot(store):
    """every byte the store holds for every landmark, rows past count included"""
    rs = read_all(store)
    return (np.array([r["count"] for r in rs]), np.array([r["med_idx"] for r in rs]),
            np.stack([r["desc_list"] for r in rs]), np.stack([r["med_desc"] for r in rs]))


def same_snapshot(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- hand-written cases: (name, calls, the lists they must leave), over descriptor pools desc0 / desc1
# whose row r is recognisable.  A call is ("pairs", pairs, lm_out, first_new), ("local", pairs, unm_rows,
# lm_out) or ("free", ids).  Lists name rows as (source, row).
WRITTEN = [
    ("created_then_skipped", [("pairs", [(3, 5), (1, 2), (0, 0)], [4, -1, 5], 4)],
     {4: [(0, 3), (1, 5)], 5: [(0, 0), (1, 0)]}),
    ("carried_in_pair_order", [("pairs", [(3, 5), (0, 0)], [4, 5], 4),
                               ("pairs", [(9, 1), (9, 6), (9, 2)], [4, 5, 4], 6)],
     {4: [(0, 3), (1, 5), (1, 1), (1, 2)], 5: [(0, 0), (1, 0), (1, 6)]}),
    ("created_beside_carried", [("pairs", [(2, 2)], [0], 0),
                                ("pairs", [(7, 8), (4, 3), (6, 1)], [1, 0, 2], 1)],
     {0: [(0, 2), (1, 2), (1, 3)], 1: [(0, 7), (1, 8)], 2: [(0, 6), (1, 1)]}),
    ("local_through_unm_rows", [("pairs", [(3, 5), (0, 0)], [4, 5], 4),
                                ("local", [(77, 1), (-5, 0), (0, 2)], [6, 3, 2], [5, 4, -1])],
     {4: [(0, 3), (1, 5), (1, 6)], 5: [(0, 0), (1, 0), (1, 3)]}),
    ("free_twice_then_reuse", [("pairs", [(3, 5), (0, 0)], [4, 5], 4),
                               ("free", [4, 4]),
                               ("pairs", [(8, 9)], [4], 4)],
     {4: [(0, 8), (1, 9)], 5: [(0, 0), (1, 0)]}),
]


def written_pools(rows=12):
    """desc0 / desc1 [rows][32]: byte 0 names the source, byte 1 the row, the rest is seeded noise"""
    rng = np.random.default_rng(77)
    pools = []
    for s in (0, 1):
        d = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
        d[:, 0], d[:, 1] = s, np.arange(rows)
        pools.append(d)
    return pools


def run_written(model, calls, pools):
    """the calls through the op builders into a Model"""
    for c in calls:
        if c[0] == "pairs":
            model.apply(pair_ops(c[1], c[2], c[3]), pools)
        elif c[0] == "local":
            model.apply(local_ops(c[1], c[2], c[3]), [pools[1]])
        else:
            model.apply(free_ops(c[1]), pools)


# ---- a keyframe tick's arrays (the GPU test feeds them from a gfpl.KeyframeMap, the CPU test from
# tests/kfmap_ref.py's model, so the situation the GPU test relies on is asserted without a device)
TICK_CAPS = (8, 48, 24, 512, 256, 8)      # kf_cap, pt_rows, ls_rows, pt_lm_cap, ls_lm_cap, obs_cap
TICK_PRM = dict(min_lm_cov_graph=1000, min_kf_local_map=0, min_lm_obs=3, cull_age=0)   # local: the last keyframe's landmarks only
TICK_KFS = 3


def tick_descriptors(world, seed=5):
    """desc[k][kind] [rows][32]: every world feature has a descriptor, every observation of it a few flipped bits"""
    rng = np.random.default_rng(seed)
    base = {}
    out = []
    for k in range(len(world.world)):
        per = []
        for kind in (0, 1):
            d = np.zeros((len(world.world[k][kind]), 32), np.uint8)
            for r, w in enumerate(world.world[k][kind]):
                if (kind, w) not in base:
                    base[(kind, w)] = rng.integers(0, 256, 32, dtype=np.uint8)
                d[r] = base[(kind, w)]
                for b in rng.integers(0, 256, 3):
                    d[r, b >> 3] ^= 1 << (b & 7)
            per.append(d)
        out.append(per)
    return out


def tick(kmap, world, sink, n_kf=TICK_KFS):
    """n_kf keyframes in addKeyFrame's order.  kmap: add_keyframe / observe_pairs / observe_local / select /
    unmatched / form_local_map / remove_bad, each returning host lists (and whatever handle the sink wants
    beside them).  The pair stage leaves out every third common pair, as a matcher would, so that the
    local-map stage finds them.  sink.pairs / .local / .free / .gather receive every call's arrays."""
    lm_world = [{}, {}]
    facts = dict(created=0, carried=0, local_appends=0, removed=0, gathered=0)
    for k in range(n_kf):
        assert kmap.add_keyframe(len(world.world[k][0]), len(world.world[k][1])) == k
        if k == 0:
            continue
        for kind in (0, 1):                                            # the keyframe-pair stage
            pairs = [p for i, p in enumerate(world.common(kind, k - 1, k)) if k == 1 or i % 3 != 2]
            lm_out, first, new, h = kmap.observe_pairs(kind, k - 1, k, pairs)
            for (r0, _), j in zip(pairs, lm_out):
                if j >= 0:
                    lm_world[kind][j] = world.world[k - 1][kind][r0]
            facts["created"] += new
            facts["carried"] += sum(0 <= j < first for j in lm_out)
            sink.pairs(kind, k - 1, k, pairs, lm_out, first, h)
        kmap.form_local_map(dict(TICK_PRM, min_kf_local_map=2))
        for kind in (0, 1):                                            # the local-map stage
            sel, hs = kmap.select(kind, 1, k)                          # GFPL_KFMAP_LOCAL_UNSEEN
            unm, hu = kmap.unmatched(kind, k)
            at = {world.world[k][kind][r]: i for i, r in enumerate(unm)}
            seen, uniq = set(), []
            for a, j in enumerate(sel):                                # one pair per kf1 row
                b = at.get(lm_world[kind].get(j))
                if b is not None and b not in seen:
                    seen.add(b)
                    uniq.append((a, b))
            sink.gather(kind, k, sel, hs)                              # the local map's descriptors: select -> gather_ids
            facts["gathered"] += len(sel)
            lm_out, h = kmap.observe_local(kind, k, uniq, sel, unm, hs, hu)
            facts["local_appends"] += len(uniq)
            sink.local(kind, k, uniq, unm, lm_out, h, hu)
        kmap.form_local_map(TICK_PRM)
        removed, hr = kmap.remove_bad(dict(min_lm_obs=TICK_PRM["min_lm_obs"], cull_age=TICK_PRM["cull_age"]))
        for kind in (0, 1):
            sink.free(kind, removed[kind], hr[kind])
            for j in removed[kind]:
                lm_world[kind].pop(j, None)
        facts["removed"] += len(removed[0]) + len(removed[1])
    return facts


def assert_tick_facts(f):
    assert f["created"] > 40 and f["carried"] > 10 and f["local_appends"] > 3 and f["removed"] >= 2 and f["gathered"] > 3, f
