"""The landmark store's device-id calls without a GPU: the declarations and exports, the argument checks
that need no device, and the yardstick of tests/test_lm_device_gpu.py itself: the op builders of
tests/lm_device_cases.py against tests/lm_store_ref.py's Model on hand-written cases, and the tick's
situation (created, carried, local appends, removals) on tests/kfmap_ref.py's model.
"""
import os
import re

import numpy as np
import pytest

import gfpl
import kfmap_ref as K
import lm_device_cases as DC
import lm_store_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gfpl_lmstore_observe_pairs", "gfpl_lmstore_observe_local", "gfpl_lmstore_free_ids", "gfpl_lmstore_gather_ids",
       "gfpl_lmstore_counts")


def test_header_declares_the_calls():
    with open(os.path.join(ROOT, "include", "gfpl.h")) as f:
        h = f.read()
    for n in NEW:
        assert re.search(r"\bint\s+" + n + r"\(gfpl_lmstore\* st\b", h), n
    assert "#define GFPL_ABI_VERSION 6 " in h   # additive: the version stays


def test_exports_and_methods_present():
    L = gfpl.hiplib()
    for n in NEW:
        assert hasattr(L, n), n
    for m in ("observe_pairs", "observe_local", "free", "gather_ids", "counts"):
        assert callable(getattr(gfpl.LandmarkStore, m, None)), m
    assert L.gfpl_abi_version() == 6
    assert (gfpl.LM_BLOCK, gfpl.LM_PLAN_TILE) == (256, 2048)


def test_null_store_is_refused():
    L = gfpl.hiplib()
    assert L.gfpl_lmstore_observe_pairs(None, None, 0, None, 0, None, None, 0, 0) == R.E_INVALID
    assert L.gfpl_lmstore_observe_local(None, None, 0, None, 0, None, 0, None) == R.E_INVALID
    assert L.gfpl_lmstore_free_ids(None, None, 0) == R.E_INVALID
    assert L.gfpl_lmstore_gather_ids(None, None, 0, None, None) == R.E_INVALID
    assert L.gfpl_lmstore_counts(None, None) == R.E_INVALID


@pytest.mark.parametrize("name,calls,want", DC.WRITTEN, ids=[w[0] for w in DC.WRITTEN])
def test_op_builders_against_the_model(name, calls, want):
    pools = DC.written_pools()
    m = R.Model(8, 6)
    DC.run_written(m, calls, pools)
    for lm in range(m.lm_cap):
        rows = [(int(r[0]), int(r[1])) for r in m.lists[lm]]   # (source, row) as the pools mark them
        assert rows == want.get(lm, []), (name, lm, rows)
        e = m.expect(lm)
        assert e["count"] == len(rows) and e["med_idx"] == R.med_index(m.lists[lm])


def test_op_builders_shapes():
    assert DC.pair_ops([(1, 2)], [-1], 0) == []
    assert DC.pair_ops([(1, 2)], [3], 3) == [(3, R.ADD, 1, 0), (3, R.ADD, 2, 1)]
    assert DC.pair_ops([(1, 2)], [3], 4) == [(3, R.ADD, 2, 1)]
    assert DC.local_ops([(9, 1)], [5, 7], [2]) == [(2, R.ADD, 7, 0)]
    assert DC.free_ops([3, 3]) == [(3, R.FREE, 0, 0)] * 2
    # the lists are ones gfpl_lm_ops_check accepts
    rc, cnt = gfpl.lm_ops_check(DC.pair_ops([(1, 2), (0, 0)], [3, 4], 3), np.zeros(6, np.int32), 4, [3, 3])
    assert rc == R.OK and cnt.tolist() == [0, 0, 0, 2, 2, 0]


class ModelMap:
    """tests/kfmap_ref.py's model behind the interface lm_device_cases.tick drives"""

    def __init__(self, caps):
        self.m = K.Model(*caps)

    def add_keyframe(self, n_pt, n_ls):
        rc, kf = self.m.add_keyframe(n_pt, n_ls)
        assert rc == K.OK
        return kf

    def observe_pairs(self, kind, kf0, kf1, pairs):
        rc, lm_out, first, new = self.m.observe_pairs(kind, kf0, kf1, pairs)
        assert rc == K.OK
        return lm_out, first, new, None

    def observe_local(self, kind, kf1, pairs, sel, unm, hs, hu):
        rc, lm_out = self.m.observe_local(kind, kf1, pairs, sel, unm)
        assert rc == K.OK
        return lm_out, None

    def select(self, kind, which, kf1):
        return self.m.select(kind, which, kf1), None

    def unmatched(self, kind, kf):
        return self.m.unmatched(kind, kf), None

    def form_local_map(self, prm):
        assert self.m.form_local_map(**prm) == K.OK

    def remove_bad(self, prm):
        return self.m.remove_bad(**prm), (None, None)


class ModelSink:
    """the tick's calls through the op builders into two Models; every list stays one gfpl_lm_ops_check accepts"""

    def __init__(self, caps, desc):
        self.desc = desc
        self.models = [R.Model(caps[3], caps[5]), R.Model(caps[4], caps[5])]

    def run(self, kind, ops, srcs):
        m = self.models[kind]
        rc, _ = m.check(ops, [len(s) for s in srcs])
        assert rc == R.OK
        m.apply(ops, srcs)

    def pairs(self, kind, kf0, kf1, pairs, lm_out, first, h):
        self.run(kind, DC.pair_ops(pairs, lm_out, first), [self.desc[kf0][kind], self.desc[kf1][kind]])

    def local(self, kind, kf1, pairs, unm, lm_out, h, hu):
        self.run(kind, DC.local_ops(pairs, unm, lm_out), [self.desc[kf1][kind]])

    def free(self, kind, ids, h):
        self.run(kind, DC.free_ops(ids), [])

    def gather(self, kind, kf1, sel, h):
        assert all(len(self.models[kind].lists[j]) > 0 for j in sel)   # gather_ids will accept the list


def test_tick_situation():
    import mapgeo_cases as MC
    cam = gfpl.make_camera("vga", gfpl.default_config())
    w = MC.World(cam, 3, DC.TICK_KFS, 60, 30, 40, 20)
    sink = ModelSink(DC.TICK_CAPS, DC.tick_descriptors(w))
    f = DC.tick(ModelMap(DC.TICK_CAPS), w, sink)
    DC.assert_tick_facts(f)
    # both kinds end with landmarks that hold rows and with freed ones
    for kind in (0, 1):
        lists = sink.models[kind].lists
        assert sum(len(l) > 0 for l in lists) > 5 and max(len(l) for l in lists) >= 3
