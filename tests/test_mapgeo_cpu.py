"""The map geometry without a GPU: the model of tests/mapgeo_ref.py on hand-written cases (place rule,
skipped pair, the gather with a fixed keyframe, keyframe 0, an erased keyframe and a landmark left with
nothing), the tick sequence of the GPU tests on the models alone, the header's declarations against the
library's exports, gfpl_mapgeo_bytes against tests/mapgeo_layout_check.cpp (a stand-alone program under
ASan + UBSan; nothing is preloaded) and the NULL-object refusals.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gfpl
import kfmap_ref as K
import mapgeo_cases as MC
import mapgeo_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
hand_map, gather_map, shifted = MC.hand_map, MC.gather_map, MC.shifted


def test_created_landmarks_take_the_store_pose():
    trio = hand_map()
    lm_out, first, new = trio.observe_pairs(0, 1, 2, [(0, 1), (2, 0)])
    assert (lm_out, first, new) == ([0, 1], 0, 2)
    lm = trio.model.lms[0][1]
    v1, v2 = trio.views[1][0], trio.views[2][0]
    assert lm.geo3d == [v1.P[2][0] + 0.5, v1.P[2][1], v1.P[2][2]]          # T_kf_w(kf0) P0, kf0's pose of the store
    assert lm.obs_list == [list(v1.pl[2]), list(v2.pl[0])] and lm.sigma_list == [1.0, 1.0]
    lm_out, first, new = trio.observe_pairs(1, 1, 2, [(1, 2)])
    ln = trio.model.lms[1][0]
    assert ln.geo3d == [v1.sP[1][0] + 0.5, v1.sP[1][1], v1.sP[1][2], v1.eP[1][0] + 0.5, v1.eP[1][1], v1.eP[1][2]]
    assert ln.obs_list == [list(v1.le[1]), list(v2.le[2])]


def test_place_is_pair_order_and_a_skipped_pair_does_nothing():
    trio = hand_map()
    m = trio.model
    trio.observe_pairs(0, 0, 1, [(0, 0)])                                    # landmark 0 = [kf0 row 0, kf1 row 0]
    v2 = trio.views[2][0]
    before = m.state()
    # three pairs name landmark 0 with different kf1 rows, a skipped pair between them
    assert m.observe_pairs(0, 1, 2, trio.views[1][0], v2, [(0, 3), (1, 1), (2, 0), (3, 2)], [0, -1, 0, 0], 1) == G.E_CAPACITY
    assert m.state() == before                                               # 2 + 3 > obs_cap = 4: nothing changed
    assert m.observe_pairs(0, 1, 2, trio.views[1][0], v2, [(0, 3), (1, 1), (2, 0)], [0, -1, 0], 1) == G.OK
    assert m.lms[0][0].obs_list[2:] == [list(v2.pl[3]), list(v2.pl[0])] and len(m.lms[0][0].sigma_list) == 4


def test_model_refusals_change_nothing():
    trio = hand_map()
    m = trio.model
    trio.observe_pairs(0, 0, 1, [(0, 0), (1, 1)])
    v0, v1 = trio.views[0][0], trio.views[1][0]
    before = m.state()
    assert m.observe_pairs(2, 0, 1, v0, v1, [], [], 0) == G.E_INVALID
    assert m.observe_pairs(0, 0, 0, v0, v0, [], [], 0) == G.E_INVALID
    assert m.observe_pairs(0, 5, 1, v0, v1, [], [], 0) == G.E_INVALID        # no pose stored for keyframe 5
    assert m.observe_pairs(0, 0, 1, v0, v1, [(4, 0)], [2], 2) == G.E_INVALID  # a row outside the view
    assert m.observe_pairs(0, 0, 1, v0, v1, [(2, 2)], [8], 2) == G.E_INVALID  # an id outside the cap
    assert m.observe_pairs(0, 0, 1, v0, v1, [(2, 2)], [0], 0) == G.E_INVALID  # a created id that holds a list
    assert m.observe_pairs(0, 0, 1, v0, v1, [(2, 2)], [2], 3) == G.E_INVALID  # a carried id without one
    assert m.observe_pairs(0, 0, 1, v0, v1, [(2, 2), (3, 3)], [2, 2], 2) == G.E_INVALID   # a created id twice
    assert m.observe_local(0, 1, v1, [(0, 2)], [2, 3], [1]) == G.E_INVALID    # outside n_unm
    assert m.observe_local(0, 1, v1, [(0, 0)], [4], [1]) == G.E_INVALID       # a row outside the view
    assert m.free(0, [8]) == G.E_INVALID
    assert m.state() == before


def test_gather_by_hand():
    trio = gather_map()
    rc, d, _, _ = trio.assemble(K.LOCAL)
    assert rc == G.OK
    assert d["kf_list"] == [3, 4] and d["fix_list"] == [0, 2] and d["pt_list"] == [0, 1, 2] == d["ls_list"]
    assert d["n"] == (2, 2, 3, 3, 6, 6)
    assert d["pt_obs_lm"].tolist() == [0, 0, 1, 1, 1, 2] and d["pt_obs_kf"].tolist() == [-1, 0, -2, 0, 1, 1]
    assert d["pt_sigma"].reshape(-1).tolist() == [1.0, 1.25, 1.0, 1.25, 1.5, 1.25]       # landmark 2 keeps its second entry
    assert d["pt_obs"][5].tolist() == [204.0, 205.0] and d["ls"][1].tolist() == [11.0, 12.0, 13.0, 14.0, 15.0, 16.0]
    assert d["T_fix"][1].tolist() == shifted(1.0).tolist() and d["x_kf"][0].tolist() == [0.01 * 3] * 6
    rc, d, _, _ = trio.assemble(K.ALIVE)
    assert d["kf_list"] == [2, 3, 4] and d["fix_list"] == [0] and d["pt_obs_kf"].tolist() == [-1, 1, 0, 1, 2, 2]
    assert trio.model.lba_code(d) is None
    # a list whose length differs between the two objects is refused
    trio.model.lms[0][1].obs_list.pop()
    assert trio.model.assemble(K.LOCAL)[0] == G.E_INVALID


def test_tick_sequence_reaches_its_situations():
    cam = gfpl.make_camera("vga", gfpl.default_config())
    trio = MC.Trio(MC.TICK_CAPS)
    MC.assert_tick_facts(MC.tick_sequence(trio, cam))
    rc, d, _, _ = trio.assemble(K.LOCAL)
    assert rc == G.OK and d["n"][0] == 2 and d["n"][1] >= 1 and d["n"][4] > 100 and d["n"][5] > 50


def test_header_and_exports():
    with open(os.path.join(ROOT, "include", "gfpl.h")) as f:
        h = f.read()
    assert "#define GFPL_ABI_VERSION 6 " in h
    names = sorted(set(re.findall(r"\b(gfpl_mapgeo_\w+)\s*\(", h)))
    assert names == sorted("gfpl_mapgeo_" + k for k in (
        "bytes", "create", "destroy", "set_keyframe", "read_keyframe", "arrays", "observe_pairs", "observe_local", "free",
        "read_landmarks", "write_landmarks", "assemble", "assembled_ids", "read_assembled", "lba", "debug_ms"))
    L = gfpl.hiplib()
    for n in names:
        assert hasattr(L, n), n
    for n in ("observe_pairs", "observe_local", "free", "assemble", "lba", "set_keyframe", "arrays", "read_landmarks",
              "write_landmarks", "read_keyframe", "last_device_ms"):
        assert hasattr(gfpl.MapGeometry, n), n
    assert C.sizeof(gfpl.MapGeoLists) == 4 * 8 + 8


def test_null_object_is_refused():
    L = gfpl.hiplib()
    caps = gfpl.KfMapCaps(4, 4, 4, 4, 4, 4)
    out, v, f = C.c_void_p(), C.c_int32(0), C.c_float(0)
    d = (C.c_double * 16)()
    view, prob, res, cnt = gfpl.KFViewStruct(), gfpl.LbaProblemStruct(), gfpl.LbaResult(), gfpl.LbaCounts()
    prm = gfpl.LbaParams.default()
    ref = C.byref
    E = G.E_INVALID
    assert L.gfpl_mapgeo_create(None, ref(caps), ref(out)) == E                 # no context without a GPU
    assert L.gfpl_mapgeo_destroy(None) == E
    assert L.gfpl_mapgeo_set_keyframe(None, 0, d, d) == E
    assert L.gfpl_mapgeo_read_keyframe(None, 0, d, d) == E
    assert L.gfpl_mapgeo_arrays(None, ref(out), ref(out), ref(out), ref(out)) == E
    assert L.gfpl_mapgeo_observe_pairs(None, 0, 0, 1, ref(view), ref(view), None, None, 0, 0) == E
    assert L.gfpl_mapgeo_observe_local(None, 0, 1, ref(view), None, 0, None, 0, None) == E
    assert L.gfpl_mapgeo_free(None, 0, None, 0) == E
    assert L.gfpl_mapgeo_read_landmarks(None, 0, 0, 0, None, None, None, None) == E
    assert L.gfpl_mapgeo_write_landmarks(None, 0, 0, 0, None, None, None, None) == E
    assert L.gfpl_mapgeo_assemble(None, None, 0, ref(prob), None) == E
    assert L.gfpl_mapgeo_assembled_ids(None, ref(out), ref(out), ref(out), ref(out)) == E
    assert L.gfpl_mapgeo_read_assembled(None, ref(prob), None, None, None, None) == E
    assert L.gfpl_mapgeo_lba(None, None, None, ref(prm), ref(res), ref(cnt)) == E
    assert L.gfpl_mapgeo_debug_ms(None, ref(f)) == E
    assert L.gfpl_mapgeo_bytes(None) == -1
    for bad in (gfpl.KfMapCaps(0, 4, 4, 4, 4, 4), gfpl.KfMapCaps(4, 4, 4, 4, 4, 65), gfpl.KfMapCaps(4, 4, 4, 4, 4, 1)):
        assert gfpl.mapgeo_bytes(bad) == -1


SHAPES = [(1, 1, 1, 1, 1, 2), (16, 96, 40, 2048, 1024, 16), (7, 1025, 3, 5, 6151, 64), (64, 2048, 512, 1 << 16, 1 << 14, 16)]


@pytest.fixture(scope="module")
def layout_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapgeo_layout") / "mapgeo_layout_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mapgeo_layout_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_bytes_against_the_layout(layout_exe, shape):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([layout_exe] + [str(v) for v in shape], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    end, total, names = 0, None, []
    for line in r.stdout.strip().split("\n"):
        w = line.split()
        if w[1] == "bytes":
            assert w[2] == w[3], line
            total = int(w[2])
        elif w[1] == "consts":
            assert int(w[2]) == gfpl.KFMAP_TILE and int(w[2]) % int(w[3]) == 0   # the tile, the block
        else:
            off, nbytes, align = int(w[2]), int(w[3]), int(w[4])
            assert off % 256 == 0 and off % align == 0 and off >= end, line   # 256-B aligned fields, none overlapping
            end = off + nbytes
            names.append(w[1])
    assert total is not None and end <= total and total % 256 == 0
    assert gfpl.mapgeo_bytes(gfpl.KfMapCaps(*shape)) == total
    kf, pr, lr, pl, ll, oc = shape
    # the state alone is a lower bound: the poses, the 3D geometry, the lists
    assert total >= 8 * (22 * kf + 3 * pl + 6 * ll + 3 * pl * oc + 4 * ll * oc)
    assert len(names) == len(set(names)) == 41
