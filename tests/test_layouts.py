"""Every dynamic-LDS layout struct (gf-pl-slam_amd/csrc/gfpl_layout.hpp) against the byte formulas
and pointer walks the launchers and kernels held before the structs existed, restated literally
here: the launch totals and every field's offset, over capacities on both sides of each rounding
and kernel switch.  tests/layout_check.cpp (built by make, host code only) prints the structs."""
import json
import os
import re
import subprocess

import pytest

import gfpl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gf-pl-slam_amd", "bin", "layout_check")
RESOURCES = os.path.join(ROOT, "profiles", "layout_carver", "resources_result.md")

KP_CAPS = {2, 66, 2000, 2048, 2050, 8192}
KL_CAPS = {2, 34, 200, 500, 1024, 1026, 2048}
HEIGHTS = sorted({c["height"] for c in gfpl.CAMERAS.values()})
LEVELS = (4, 8)
# the expansion table of the knn MFMA (FP4 operands): dwords per cell size
LUT = {1: 256 * 1, 2: 256 * 2}
SP_CHUNK, SP_MINR_PAD, CH_STRIDE, LSD_RING, KNN_CHUNK = 32, 32, 66, 256, 1024


@pytest.fixture(scope="module")
def rows():
    assert os.path.exists(BIN), "layout_check not built (make all)"
    args = [f"{h}:{n}" for h in HEIGHTS for n in LEVELS]
    p = subprocess.run([BIN] + args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = [json.loads(line) for line in p.stdout.splitlines()]
    for r in out:   # the placing pass announces what the sizing pass did
        assert r["placed"] == r["bytes"], r
    return out


def of(rows, name):
    got = [r for r in rows if r["layout"] == name]
    assert got, name
    return got


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def test_stereo_points(rows):
    got = of(rows, "stereo_points")
    assert {r["kp_cap"] for r in got} == KP_CAPS
    assert {(r["height"], r["levels"]) for r in got} == {(h, n) for h in HEIGHTS for n in LEVELS}
    assert {(r["seg"], r["waves"]) for r in got} == {(0, 8), (0, 16), (1, 8), (1, 16)}
    for r in got:
        KP2 = next_pow2(r["kp_cap"])
        assert r["KP2"] == KP2
        if r["seg"]:   # launch_stereo_points: lds_seg, and lds_seg_w for the 1024-thread form
            nrl = (r["levels"] + 1) * (r["height"] + 2 * SP_MINR_PAD) + 1
            want = KP2 * 18 + ((nrl + 1) & ~1) * 2 + 32 * 4 + 16 + (512 // 64) * SP_CHUNK * 32
            if r["waves"] == 16:
                want += (512 // 64) * SP_CHUNK * 32
        else:
            nrl = r["height"]
            want = KP2 * 18 + ((r["height"] + 1) & ~1) * 2 + 64 * 4
        assert r["bytes"] == want, r
        # k_stereo_points' pointer walk
        rl = (nrl + 1) & ~1
        assert (r["rkey"], r["order"], r["pairs"], r["recx"], r["recm"], r["rowlo"]) == \
            (0, KP2 * 4, KP2 * 8, KP2 * 12, KP2 * 16, KP2 * 18), r
        assert r["misc"] == KP2 * 18 + rl * 2, r
        assert r["depth"] == r["recx"] and r["hr"] == r["rowlo"] and r["offr"] == r["rowlo"], r
        if r["seg"]:
            assert r["stg"] == (KP2 * 18 + rl * 2 + 32 * 4 + 15) & ~15, r
            assert r["hl"] == r["stg"] and r["offl"] == r["stg"], r
            assert r["stg"] + r["waves"] * SP_CHUNK * 32 <= r["bytes"], r


def test_stereo_lines(rows):
    got = of(rows, "stereo_lines")
    assert {r["kl_cap"] for r in got} == KL_CAPS and {r["cell"] for r in got} == {1, 2}
    for r in got:
        cap = r["kl_cap"]
        # stereo_lines_lds(): the table of CELL 2, the larger one, for both instantiations
        assert r["bytes"] == cap * 32 + cap * 16 + 260 * 4 + 64 * 4 + LUT[2] * 4, r
        assert r["lut"] == 0, "knn2_mfma reads the table at LDS address 0"
        tb = LUT[r["cell"]] * 4
        lr_i = tb + cap * 32
        misc = lr_i + 4 * cap * 4 + 260 * 4
        assert (r["tb"], r["lr_i"], r["lr_d0"], r["lr_d1"], r["rl_i"], r["hist"]) == \
            (tb, lr_i, lr_i + cap * 4, lr_i + cap * 8, lr_i + cap * 12, lr_i + cap * 16), r
        assert r["th"] == misc + 8 * 4 and r["scan"] == misc + 16 * 4, r
        assert r["scan"] + 17 * 4 <= r["bytes"], r   # block_exclusive_scan<1024>: 16 wave sums + the total


def test_cross_lines(rows):
    got = of(rows, "cross_lines")
    assert {r["kl_cap"] for r in got} == KL_CAPS
    for r in got:
        cap = r["kl_cap"]
        assert r["bytes"] == cap * 32 + cap * 16 + 520 * 4 + 64 * 4 + LUT[1] * 4, r
        assert r["lut"] == 0, "knn2_mfma reads the table at LDS address 0"
        tb = LUT[1] * 4
        i12 = tb + cap * 32
        h12 = i12 + cap * 16
        misc = h12 + 520 * 4
        assert (r["tb"], r["i12"], r["d012"], r["d112"], r["i21"], r["h12"], r["h0"]) == \
            (tb, i12, i12 + cap * 4, i12 + cap * 8, i12 + cap * 12, h12, h12 + 260 * 4), r
        assert r["scan"] == misc and r["th"] == misc + 16 * 4, r


def test_knn2(rows):
    got = of(rows, "knn2")
    assert {r["cell"] for r in got} == {1, 2}
    for r in got:
        assert r["lut_dwords"] == LUT[r["cell"]] and r["chunk"] == KNN_CHUNK, r
        assert r["lut"] == 0, "knn_tile reads the table at LDS address 0"
        assert r["tb"] == 4 * LUT[r["cell"]], r
        # launch_knn2_as: the table, then one chunk of train rows as views (8 dwords a row), packed
        assert r["bytes"] == 4 * (LUT[r["cell"]] + 8 * KNN_CHUNK), r
        assert r["bytes"] <= 64 * 1024, "k_knn2m launches without raising the dynamic-LDS ceiling"


def test_cross_points(rows):
    got = of(rows, "cross_points")
    assert {r["kp_cap"] for r in got} == KP_CAPS and {r["xl"] for r in got} == {0, 1}
    for r in got:
        cap, nc, xl = r["kp_cap"], r["ncell"], r["xl"]
        # cross_points_lds()
        assert r["bytes"] == 32 * 8 + (nc + 2) * 8 + cap * (32 if xl else 16) + 64 * 4, r
        cnt = 256 + (cap * 16 if xl else 0)
        sq = cnt + 2 * (nc + 2) * 4
        assert (r["prevT"], r["Tinv"], r["spxy"]) == (0, 128, 256 if xl else -1), r
        assert (r["cnt"], r["start"], r["sq"], r["spx"], r["spy"], r["lastT"], r["misc"]) == \
            (cnt, cnt + (nc + 2) * 4, sq, sq + cap * 4, sq + cap * 8, sq + cap * 12, sq + cap * 16), r


def test_pose(rows):
    got = of(rows, "pose")
    assert {r["W"] for r in got} == {1, 4, 8}
    assert {(r["mpt_cap"], r["mls_cap"]) for r in got} == {(500, 300), (2048, 1024)}   # GFPL_MAX_MATCHED_PT / _LS
    for r in got:
        assert r["NP2"] == next_pow2(max(r["mpt_cap"], r["mls_cap"]))
        region = max(r["W"] * 16 * CH_STRIDE, r["NP2"])   # launch_pose
        assert r["bytes"] == region * 8 + ((r["mpt_cap"] + r["mls_cap"] + 15) & ~15) + 16, r
        assert (r["cp"], r["cl"], r["buf"], r["act"]) == (0, 8 * CH_STRIDE * 8, 0, region * 8), r


def test_orb_cell_and_lsd_grow(rows):
    for r in of(rows, "orb_cell"):
        pc = r["patch_cap"]
        assert r["bytes"] == 4 * pc * r["waves"], r   # gfpl_orb_extract_async's launch
        P = r["wave"] * 4 * pc                          # k_orb_cellfast: csm + wave * 4 * patch_cap
        assert (r["P"], r["Sc"], r["cand"]) == (P, P + pc, P + 2 * pc), r
    for r in of(rows, "lsd_grow"):
        assert r["bytes"] == r["cid_cap"] // 8 + 4 * LSD_RING, r   # gfpl_lsd_create
        assert (r["ring"], r["used"]) == (0, 4 * LSD_RING), r      # k_lsd_grow_lds: lds, lds + LSD_RING


def static_lds():
    """Static LDS bytes per kernel of the committed resource table (the compiler's remarks)."""
    out = {}
    with open(RESOURCES) as f:
        for line in f:
            m = re.match(r"\| \S+ \| `(?:void )?([^`]+)` \|(.*)\|\s*$", line)
            if m:
                out[m.group(1)] = int(m.group(2).split("|")[6])
    return out


def test_capacity_limits_fit_a_cu(rows):
    """At the ABI's capacity limits (kp_cap 8192, kl_cap 2048, the matched-list maxima) every layout a
    launcher can choose fits a CU's 160 KB less the kernel's static LDS.  The SEG and XL forms are
    chosen for kp_cap <= 2048 only (launch_stereo_points, launch_cross_points): their limit is 2048."""
    st = static_lds()
    cu = 160 * 1024
    checked = 0
    for r in rows:
        name = r["layout"]
        if name == "stereo_points":
            if r["kp_cap"] != (2048 if r["seg"] else 8192):
                continue
            kernel = f"k_stereo_points<{64 * r['waves']}, {'true' if r['seg'] else 'false'}>"
        elif name == "cross_points":
            if r["kp_cap"] != (2048 if r["xl"] else 8192):
                continue
            kernel = f"k_cross_points<{'true' if r['xl'] else 'false'}>"
        elif name == "stereo_lines":
            if r["kl_cap"] != 2048:
                continue
            kernel = "k_stereo_lines<2, false, 1024>" if r["cell"] == 2 else "k_stereo_lines<1, true, 1024>"
        elif name == "cross_lines":
            if r["kl_cap"] != 2048:
                continue
            kernel = "k_cross_lines<1024>"
        elif name == "pose":
            if r["mpt_cap"] != 2048:
                continue
            kernel = f"k_pose<{r['W']}>"
        else:
            continue
        assert kernel in st, kernel
        assert r["bytes"] <= cu - st[kernel], (kernel, r["bytes"], st[kernel])
        checked += 1
    assert checked >= 5 * len(HEIGHTS)
