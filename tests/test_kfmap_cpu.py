"""The keyframe map without a GPU: the model's known answers on hand-written maps for each pinned
quirk (ledger KM1-KM10), the situations of the GPU tests asserted on the model alone, gfpl_kfmap_bytes
against tests/kfmap_layout_check.cpp (a stand-alone program under ASan + UBSan; nothing is preloaded),
the NULL-argument refusals and the default parameters.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gfpl
import kfmap_cases as KC
import kfmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("quirk", KC.QUIRKS, ids=[q.__name__ for q in KC.QUIRKS])
def test_model_known_answers(quirk):
    quirk(KC.Pair(KC.QUIRK_CAPS))


def test_sixteen_keyframes_reach_their_situations():
    pair = KC.Pair(KC.SIXTEEN_CAPS)
    KC.assert_sixteen_facts(KC.sixteen_keyframes(pair))
    assert pair.calls > 100


def test_model_refusals():
    p = KC.quirk_map(KC.Pair(KC.QUIRK_CAPS))
    m = p.model
    before = m.state()
    assert m.observe_pairs(2, 0, 1, [])[0] == R.E_INVALID
    assert m.observe_pairs(0, 0, 0, [])[0] == R.E_INVALID
    assert m.observe_pairs(0, 0, 13, [])[0] == R.E_INVALID
    assert m.observe_pairs(0, 1, 2, [(4, 0), (6, 1)])[0] == R.E_INVALID          # a row past the keyframe's rows
    assert m.observe_pairs(0, 1, 2, [(4, 0), (5, -1)])[0] == R.E_INVALID
    assert m.observe_local(0, 2, [(0, 0), (1, 1)], [0, 9], [0, 1])[0] == R.E_INVALID   # sel_ids names no landmark
    assert m.observe_local(0, 2, [(0, 0), (2, 1)], [0, 1], [0, 1])[0] == R.E_INVALID   # outside n_sel
    assert m.observe_local(0, 2, [(0, 0), (1, 2)], [0, 1], [0, 1])[0] == R.E_INVALID   # outside n_unm
    assert m.set_inlier(0, [0, 4], 0) == R.E_INVALID
    assert m.write_keyframe_idx(0, 1, 0, [4]) == R.E_INVALID
    assert m.add_keyframe(7, 0)[0] == R.E_CAPACITY
    assert m.state() == before
    # a list at obs_cap - 1 takes one more entry, a full one refuses
    assert m.observe_pairs(0, 1, 2, [(0, 0)])[0] == R.OK and m.observe_pairs(0, 2, 3, [(0, 0)])[0] == R.OK
    assert len(m.lm(0, 0).kf_obs_list) == 4 == KC.QUIRK_CAPS[5]
    assert m.observe_pairs(0, 3, 4, [(5, 1), (0, 0)])[0] == R.E_CAPACITY
    assert m.map_keyframes[3].idx[0][5] == -1 and m.max_idx[0] == 4


def test_default_params_and_constants():
    p = gfpl.KfMapParams.default()
    assert (p.min_lm_cov_graph, p.min_kf_local_map, p.min_lm_obs, p.cull_age) == (30, 3, 2, 10)
    assert R.DEFAULT_PARAMS == dict(min_lm_cov_graph=30, min_kf_local_map=3, min_lm_obs=2, cull_age=10)
    assert (gfpl.KFMAP_LOCAL, gfpl.KFMAP_LOCAL_UNSEEN, gfpl.KFMAP_ALIVE) == (R.LOCAL, R.LOCAL_UNSEEN, R.ALIVE) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "gfpl.h")) as f:
        h = f.read()
    assert "#define GFPL_ABI_VERSION 6 " in h and f"#define GFPL_KFMAP_TILE {gfpl.KFMAP_TILE} " in h
    assert gfpl.hiplib().gfpl_abi_version() == 6
    assert hasattr(gfpl.KeyframeMap, "observe_pairs") and hasattr(gfpl.KeyframeMap, "select")


def test_null_arguments_are_refused():
    L = gfpl.hiplib()
    caps = gfpl.KfMapCaps(4, 4, 4, 4, 4, 4)
    out = C.c_void_p()
    v = C.c_int32(0)
    ref = C.byref
    assert L.gfpl_kfmap_create(None, ref(caps), ref(out)) == R.E_INVALID       # no context without a GPU
    assert L.gfpl_kfmap_destroy(None) == R.E_INVALID
    assert L.gfpl_kfmap_counts(None, ref(v), ref(v), ref(v)) == R.E_INVALID
    assert L.gfpl_kfmap_add_keyframe(None, 1, 1, ref(v)) == R.E_INVALID
    assert L.gfpl_kfmap_observe_pairs(None, 0, 0, 1, None, 0, None, ref(v), ref(v)) == R.E_INVALID
    assert L.gfpl_kfmap_observe_local(None, 0, 1, None, 0, None, 0, None, 0, None) == R.E_INVALID
    assert L.gfpl_kfmap_form_local_map(None, ref(gfpl.KfMapParams.default())) == R.E_INVALID
    assert L.gfpl_kfmap_select(None, 0, 0, 0, None, ref(v)) == R.E_INVALID
    assert L.gfpl_kfmap_unmatched(None, 0, 0, None, ref(v)) == R.E_INVALID
    assert L.gfpl_kfmap_local_keyframes(None, None, ref(v)) == R.E_INVALID
    assert L.gfpl_kfmap_remove_bad(None, None, None, ref(v), None, ref(v)) == R.E_INVALID
    assert L.gfpl_kfmap_set_inlier(None, 0, None, 0, 1) == R.E_INVALID
    assert L.gfpl_kfmap_erase_keyframe(None, 0) == R.E_INVALID
    assert L.gfpl_kfmap_read_keyframe(None, 0, None, None, None) == R.E_INVALID
    assert L.gfpl_kfmap_write_keyframe_idx(None, 0, 0, 0, 0, None) == R.E_INVALID
    assert L.gfpl_kfmap_read_landmarks(None, 0, 0, 0, None, None, None, None, None, None) == R.E_INVALID
    assert L.gfpl_kfmap_write_landmarks(None, 0, 0, 0, None, None, None, None, None, None) == R.E_INVALID
    assert L.gfpl_kfmap_export_graph(None, None, None, None, None, None, None, None, None) == R.E_INVALID
    assert L.gfpl_kfmap_debug_ms(None, None) == R.E_INVALID
    assert L.gfpl_kfmap_bytes(None) == -1
    for bad in (gfpl.KfMapCaps(0, 4, 4, 4, 4, 4), gfpl.KfMapCaps(4, 4, 4, 4, 4, 65), gfpl.KfMapCaps(4, 4, 4, 4, 4, 1),
                gfpl.KfMapCaps(4, 0, 4, 4, 4, 4), gfpl.KfMapCaps(4, 4, 4, -1, 4, 4)):
        assert gfpl.kfmap_bytes(bad) == -1


SHAPES = [(1, 1, 1, 1, 1, 2), (16, 96, 40, 2048, 1024, 16), (7, 1025, 3, 5, 6151, 64), (256, 2048, 512, 1 << 20, 1 << 18, 16)]


@pytest.fixture(scope="module")
def layout_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kfmap_layout") / "kfmap_layout_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "kfmap_layout_check.cpp"),
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
    assert gfpl.kfmap_bytes(gfpl.KfMapCaps(*shape)) == total
    kf, pr, lr, pl, ll, oc = shape
    # the state alone is a lower bound: the idx rows, the lists, the graph
    assert total >= 4 * (kf * (pr + lr) + (pl + ll) * oc + kf * kf)
    assert len(names) == len(set(names)) == 27
