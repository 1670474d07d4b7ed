"""k_stereo_points (all four forms), k_init_points behind the batched knn-2 and k_cross_points (both forms)
on hand-made keypoints, descriptors and pyramids, against plain numpy.

The point stages are otherwise reached only through frameStep on synthetic frames, whose descriptors never
tie or land on a threshold, whose keypoints never sit on a band, cell or window edge and whose pyramids
never make two SAD shifts equal.  Here each stage runs on its own through its entry point (initialize,
stereoPoints, crossFrameMatchingPoints on written frames), one case per sequence in one batch, the
families of point_match_cases.py one after the other through the same handler (whatever a family leaves in
the slots and in the scratch is what the next one starts from).  Every assertion is equality with the
numpy statement there — indices, levels and float32 disparity bits — and, for P / sigma2 / idx / pdesc,
bit equality with the oracle through compare_core (test_point_match_cpu.py pins the statement to the
oracle and to hand-checked answers and shows that the families notice the faults they aim at).

Which k_stereo_points form runs follows launch_stereo_points: the SEG layout needs
18 * KP2 + 2 * (((levels + 1) * (height + 64) + 2) & ~1) + 144 + 1024 * waves bytes of LDS (StereoPointsLds);
B <= GFPL_SP_WIDE_MAX_B (256 when unset), kp_cap <= 2048 and that sum <= 64 KB with 16 waves -> <1024, true>; else kp_cap > 2048
-> <1024, false>; else that sum <= 54 KB with 8 waves -> <512, true>; else <512, false>.  n_subpix (the
M_o of last_step_counts) is written by k_step_bytes, which only frameStep launches: no stage call reaches it.
"""
import numpy as np
import pytest

import gfpl
import oracle as O
import point_match_cases as M
from parity import compare_core, diff_fields, PT_MATCHED

pytestmark = pytest.mark.gpu

KL = 32
POINT_BUFS = (0, 1, 2, 3, 4, 5, 12)   # n_kp_l, n_kp_r, kp_l, kp_r, pdesc_l, pdesc_r, pyr_r in HostFrames.arrays()
_ORACLE = {}


class Rig:
    """One synthetic input frame of B sequences in HBM whose point inputs and pyramids are replaced per
    family (the line inputs stay: a few ordinary keylines), and one handler."""

    def __init__(self, cam_name, B, kp_cap):
        import torch
        self.torch = torch
        self.cam_name, self.B, self.cap = cam_name, B, kp_cap
        self.cam, self.cfg = M.camera(cam_name).cam, M.config(cam_name)
        self.H = M.host_frames(cam_name, B, kp_cap, KL)
        self.D = gfpl.DeviceFrames(self.H)
        self.ctx = gfpl.Context(self.cam, self.cfg)
        self.g = gfpl.StereoFrameHandler(self.ctx, B, kp_cap, KL)

    def frames(self, fill, cases):
        assert len(cases) <= self.B
        fill(self.H, 0, cases)
        arrs = self.H.arrays()
        for k in POINT_BUFS:
            a = arrs[k]
            self.D.bufs[k].copy_(self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)))
        return self.D.frames(0)

    def oracle(self, key, cases, stage):
        """the oracle's frame per case, computed once per (inputs, capacity) and left unchanged"""
        k = (key, self.cam_name, self.cap, stage)
        if k not in _ORACLE:
            fr, out = self.H.frames(0), []
            for b in range(len(cases)):
                o = O.OracleHandler(self.cam, self.cfg, self.cap, KL)
                o.initialize(fr, b)
                if stage == "stereo":
                    o.begin_frame(fr, b)
                    o.stereoPoints()
                    o.stereoLines()
                out.append(o.read_frame(gfpl.CURR if stage == "stereo" else gfpl.PREV))
            _ORACLE[k] = out
        return _ORACLE[k]


_RIGS = {}


def rig(cam_name, B, kp_cap):
    k = (cam_name, B, kp_cap)
    if k not in _RIGS:
        _RIGS[k] = Rig(cam_name, B, kp_cap)
    return _RIGS[k]


def _wide(monkeypatch, wide):
    if wide is None:
        monkeypatch.delenv("GFPL_SP_WIDE_MAX_B", raising=False)
    else:
        monkeypatch.setenv("GFPL_SP_WIDE_MAX_B", wide)


def _stereo(r, key, cases):
    fr = r.frames(M.fill_stereo, cases)
    r.g.initialize(fr)
    r.g.stereoPoints(fr)
    r.g.stereoLines(fr)
    ref = r.oracle(key, cases, "stereo")
    bad = []
    for b, c in enumerate(cases):
        fh = r.g.read_frame(gfpl.CURR, b)
        bad += M.check_stereo(fh, c)
        bad += compare_core(fh, ref[b], c.what() + " vs oracle: ")
    return bad


VGA_B = 24


@pytest.mark.parametrize("wide", ["0", None])
def test_stereo_points_vga(monkeypatch, wide):
    """VGA, kp_cap 2048, 24 sequences: the size grid, the mechanism families (band edges, chunks, octaves,
    Hamming ties and thresholds, SAD shifts / alignments / borders, medians) and the long sorts.  SEG LDS =
    36864 + 5444 + 144 + 8192 = 50644 B with 8 waves, 58836 B with 16: GFPL_SP_WIDE_MAX_B=0 runs
    k_stereo_points<512, true>, unset (24 <= 256) runs k_stereo_points<1024, true>."""
    _wide(monkeypatch, wide)
    r = rig("vga", VGA_B, 2048)
    bad = []
    for key in ("grid", "small", "median"):
        bad += _stereo(r, key, M.STEREO_FAMILIES[key]())
    assert not bad, "\n".join(bad[:30])


def test_stereo_points_large_capacity(monkeypatch):
    """The same families at kp_cap 2050: above 2048 every batch size runs k_stereo_points<1024, false> (the
    sorted single list, bitonic sorts, KP2 = 4096)."""
    _wide(monkeypatch, None)
    r = rig("vga", VGA_B, 2050)
    bad = []
    for key in ("grid", "small", "median"):
        bad += _stereo(r, key, M.STEREO_FAMILIES[key]())
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("wide", ["0", None])
def test_stereo_points_tall_image(monkeypatch, wide):
    """The 1920 x 1080 camera at kp_cap 2048: SEG LDS = 36864 + 11444 + 144 + 8192 = 56644 B with 8 waves (above
    54 KB) and 64836 B with 16 (below 64 KB): GFPL_SP_WIDE_MAX_B=0 falls through to k_stereo_points<512, false>
    at a capacity <= 2048, unset runs k_stereo_points<1024, true> with 1144 bins a segment.  The window borders
    put 1914 / 1074 into the job word's 11-bit fields."""
    _wide(monkeypatch, wide)
    cases = M.tall_cases("stress")
    bad = _stereo(rig("stress", len(cases), 2048), "stress", cases)
    assert not bad, "\n".join(bad[:30])


def test_stereo_points_tall_image_small_capacity(monkeypatch):
    """The 1920 x 1080 camera at kp_cap 520 (KP2 1024): 18432 + 11444 + 144 + 8192 = 38212 B with 8 waves:
    GFPL_SP_WIDE_MAX_B=0 runs k_stereo_points<512, true> on 1080 rows."""
    _wide(monkeypatch, "0")
    cases = M.tall_cases("stress")
    bad = _stereo(rig("stress", len(cases), 520), "stress", cases)
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("wide", ["0", None])
def test_stereo_points_eight_levels(monkeypatch, wide):
    """orb_scale_factor 1.4 with 8 levels at kp_cap 520: band heights up to 44 rows (above SP_MINR_PAD), nine
    segments, octave 7 in the job word.  k_stereo_points<512, true> ("0") / <1024, true> (unset)."""
    _wide(monkeypatch, wide)
    cases = M.tall_cases("vga8")
    bad = _stereo(rig("vga8", len(cases), 520), "vga8", cases)
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("wide", ["0", None])
def test_stereo_points_disparity_gates(monkeypatch, wide):
    """fx = 544 (maxD = 16 * 34): disparity exactly 0 (-> 0.01f and the mbf round trip), just below and at maxD,
    uR == uL and uR == uL - maxD, maxU < 0.  kp_cap 64: k_stereo_points<512, true> / <1024, true>."""
    _wide(monkeypatch, wide)
    cases = M.disparity_cases()
    bad = _stereo(rig("vga544", len(cases), 64), "disparity", cases)
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("kp_cap", [2048, 2050])
def test_initial_points(monkeypatch, kp_cap):
    """initialize: launch_knn2_batched both ways (blockIdx.y = the sequence, ragged counts from 0 to the
    capacity) and k_init_points: mutual best with ties, the ratio 9/10, 45/50, 0/0, 0/7, |dy| at 2.0 and the
    next float, disparity at 1.0 and the float below."""
    _wide(monkeypatch, None)
    cases = M.init_cases()
    r = rig("vga", VGA_B, kp_cap)
    r.g.initialize(r.frames(M.fill_init, cases))
    ref = r.oracle("init", cases, "init")
    bad = []
    for b, c in enumerate(cases):
        fh = r.g.read_frame(gfpl.PREV, b)
        bad += M.check_init(fh, c)
        bad += compare_core(fh, ref[b], c.what() + " vs oracle: ")
    assert not bad, "\n".join(bad[:30])


def _oracle_cross(c, cap):
    k = ("cross", id(c), cap)
    if k not in _ORACLE:
        o = O.OracleHandler(M.camera("vga").cam, c.cfg(), cap, KL)
        P, C = M.cross_frames(c, cap, KL)
        o.write_frame(gfpl.PREV, P)
        o.write_frame(gfpl.CURR, C)
        o.crossFrameMatchingPoints()
        _ORACLE[k] = (o.read_frame(gfpl.PREV), o.read_frame(gfpl.CURR), o.read_track())
    return _ORACLE[k]


def _cross(g, cases, cap):
    for b, c in enumerate(cases):
        P, C = M.cross_frames(c, cap, KL)
        g.write_frame(gfpl.PREV, b, P)
        g.write_frame(gfpl.CURR, b, C)
    g.crossFrameMatchingPoints()
    bad = []
    for b, c in enumerate(cases):
        prev, curr, track = g.read_frame(gfpl.PREV, b), g.read_frame(gfpl.CURR, b), g.read_track(b)
        if c.statement:
            bad += M.check_cross(prev, curr, track, c)
        op, oc, ot = _oracle_cross(c, cap)
        w = c.what() + " vs oracle: "
        if not np.array_equal(track["matched_pt"], ot["matched_pt"]) or track["n_inliers_pt"] != ot["n_inliers_pt"]:
            bad.append(w + f"matched_pt: {len(track['matched_pt'])} entries, oracle {len(ot['matched_pt'])}")
            continue
        bad += diff_fields(prev, op, PT_MATCHED + ["pt_idx"], what=w + "PREV ")
        bad += compare_core(curr, oc, w + "CURR ")
    return bad


@pytest.mark.parametrize("kp_cap", [2048, 2050])
def test_cross_points(kp_cap):
    """crossFrameMatchingPoints on written frames: the gate at exactly 10 px, Hamming 50 / 51, ties, several t
    for one q, cell borders and clamped cells, |pl| around 1e6 (the slow path) and 1e5, one crowded cell, an
    almost empty grid, a wild bucket of Z = 0 points (against the oracle alone), the sizes 0 .. 2048 and the
    cap of 500 inside the first round; nothing beyond the cap writes idx, pl_obs or inlier.  kp_cap 2048 runs
    k_cross_points<true> (XL: 256 + 1202 * 8 + 2048 * 32 + 256 B <= 80 KB), kp_cap 2050 k_cross_points<false>."""
    cases = M.cross_cases()
    ctx = gfpl.Context(M.camera("vga").cam, gfpl.default_config())
    g = gfpl.StereoFrameHandler(ctx, len(cases), kp_cap, KL)
    bad = _cross(g, cases, kp_cap)
    bad += _cross(g, cases[::-1], kp_cap)      # again in the slots the other cases left
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("kp_cap", [2048, 2050])
def test_cross_points_other_configs(kp_cap):
    """Contexts of their own: point_match_radius 49.5 (Hamming 49 passes, 50 does not) and
    max_point_match_num 1500 (the cap falls in the second round of 1024 current points; a 1100-point frame stays
    below it).  k_cross_points<true> / <false> by capacity as above."""
    bad = []
    groups = {}
    for c in M.cross_cfg_cases():
        groups.setdefault(tuple(sorted(c.cfg_over.items())), []).append(c)
    for over, cases in groups.items():
        ctx = gfpl.Context(M.camera("vga").cam, gfpl.default_config(**dict(over)))
        g = gfpl.StereoFrameHandler(ctx, len(cases), kp_cap, KL)
        bad += _cross(g, cases, kp_cap)
    assert not bad, "\n".join(bad[:30])
