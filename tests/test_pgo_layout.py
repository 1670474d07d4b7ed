"""The pose graph's layouts (gfpl_layout.hpp: PgoLds, PgoMem, PgoIdx) through tests/pgo_layout_check.cpp,
a host program built here under ASan + UBSan (stand-alone; nothing is preloaded): every field
naturally aligned, the fields in order without overlap and inside the layout's bytes, the sizing
pass equal to the placing pass, the HBM fields 256-byte aligned, and gfpl_pgo_workspace equal to
the two HBM layouts' sum with PgoLds' bytes.
"""
import os
import subprocess

import pytest

import gfpl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# n_kf n_lc n_vert n_free n_edge env_blocks n_jobs: the smallest graph, one with no free vertex, odd sizes, a large one
SHAPES = [(2, 1, 2, 1, 2, 1, 0), (2, 1, 2, 0, 2, 0, 1), (9, 2, 7, 5, 13, 17, 11), (1024, 3, 1024, 1023, 9200, 10230, 25600)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgo_layout") / "pgo_layout_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pgo_layout_check.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["smallest", "no_free", "odd", "large"])
def test_layouts(exe, shape):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(v) for v in shape], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    fields, total = {}, {}
    for line in r.stdout.strip().split("\n"):
        w = line.split()
        if w[1] == "bytes":
            assert w[2] == w[3], line   # the sizing pass and the placing pass agree
            total[w[0]] = int(w[2])
        else:
            fields.setdefault(w[0], []).append((w[1], int(w[2]), int(w[3]), int(w[4])))
    assert set(fields) == set(total) == {"PgoLds", "PgoMem", "PgoIdx"}
    for lay, fs in fields.items():
        end = 0
        for name, off, nbytes, align in fs:
            assert off % align == 0, (lay, name, off, align)
            assert off >= end, (lay, name, off, end)
            if lay != "PgoLds":
                assert off % 256 == 0, (lay, name, off)
            end = off + nbytes
        assert end <= total[lay], (lay, end, total[lay])
    assert total["PgoLds"] <= 64 * 1024
    n_kf, n_lc, n_vert, n_free, n_edge, env, jobs = shape
    rc, hbm, lds = gfpl.pgoWorkspace(gfpl.PgoCounts(n_kf, n_lc, n_vert, n_free, n_edge, env, jobs, 0))
    assert rc == 0 and hbm == total["PgoMem"] + total["PgoIdx"] and lds == total["PgoLds"]
