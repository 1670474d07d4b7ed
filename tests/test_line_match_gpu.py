"""k_stereo_lines (both cells) and k_cross_lines on hand-made line descriptors, against plain numpy.

The kernels' knn pass (knn2_mfma<CELL>, gfpl_knn.hpp: train views, table reads at
LDS address 0, the accumulator block kept across tiles, top-2 by v_med3_u32, the reverse direction by a
DPP reduce-scatter and one atomicMin per lane, masked partial tiles) is otherwise reached only through
frameStep on synthetic frames, whose descriptors never tie, never repeat, are never zero and land on a
tile edge only by luck.  Here each stage runs on its own through its entry point, one sequence per
(NL, NR) of the tile-edge grid in one batch (neighbouring workgroups always differ in shape), on the
descriptor families of line_match_cases.py; every assertion is integer equality with the numpy
statement there (test_line_match_cpu.py pins that statement to the oracle and to hand-checked answers,
and shows that the families notice the faults they aim at).

The keylines make every pair pass triangulate and carry the pair in the output row (line_match_cases:
geometry), so the stereo kernels' accepted (i, j) lists can be read back; the cross kernel is fed and
read through write_frame / read_frame / read_track.
"""
import numpy as np
import pytest

import gfpl
import line_match_cases as L

pytestmark = pytest.mark.gpu

KP = 64
LINE_BUFS = range(6, 12)   # n_kl_l, n_kl_r, kl_l, kl_r, ldesc_l, ldesc_r in HostFrames.arrays()


class Rig:
    """One synthetic input frame of B sequences in HBM whose line inputs are replaced per family, and a
    context per config (forward_dups_open runs with a negative desc_th_l)."""

    def __init__(self, B, kl_cap):
        self.B, self.cap = B, kl_cap
        self.cam = gfpl.make_camera("vga", gfpl.default_config())
        self.H = L.host_frames(self.cam, B, kl_cap, KP)
        self.D = gfpl.DeviceFrames(self.H)
        self._ctx = {}

    def ctx(self, family):
        over = L.CFG_OVER.get(family, {})
        k = tuple(sorted(over.items()))
        if k not in self._ctx:
            self._ctx[k] = gfpl.Context(self.cam, gfpl.default_config(**over))
        return self._ctx[k]

    def handler(self, family):
        return gfpl.StereoFrameHandler(self.ctx(family), self.B, KP, self.cap)

    def frames(self, cases):
        import torch
        L.fill_frames(self.H, 0, cases)
        arrs = self.H.arrays()
        for k in LINE_BUFS:
            a = arrs[k]
            self.D.bufs[k].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)))
        return self.D.frames(0)


@pytest.fixture(scope="module")
def rig():
    return Rig(len(L.GRID_PAIRS), L.KL_CAP)


def _stereo_initial(rig, g, cases):
    g.initialize(rig.frames(cases))
    bad = []
    for b, c in enumerate(cases):
        bad += L.check_stereo(g.read_frame(gfpl.PREV, b), c, 1, True, rig.cap)
    return bad


def _stereo_frame(rig, g, cases):
    fr = rig.frames(cases)
    g.initialize(fr)
    g.stereoLines(fr)
    bad = []
    for b, c in enumerate(cases):
        bad += L.check_stereo(g.read_frame(gfpl.CURR, b), c, 2, False, rig.cap)
    return bad


def _cross(g, cases, cap):
    for b, c in enumerate(cases):
        P, C = L.cross_frames(c, KP, cap)
        g.write_frame(gfpl.PREV, b, P)
        g.write_frame(gfpl.CURR, b, C)
    g.crossFrameMatchingLines()
    bad = []
    for b, c in enumerate(cases):
        bad += L.check_cross(g.read_frame(gfpl.PREV, b), g.read_frame(gfpl.CURR, b), g.read_track(b), c)
    return bad


def _handlers(rig):
    """family -> handler, one handler per context (the families run through it one after the other, so
    whatever a family leaves in the slots and in the scratch is what the next one starts from)"""
    hs = {}
    for fam in L.FAMILIES:
        k = id(rig.ctx(fam))
        if k not in hs:
            hs[k] = rig.handler(fam)
        yield fam, hs[k]


@pytest.mark.parametrize("wide", ["0", "4096"])
def test_stereo_lines_initial_adversarial(monkeypatch, rig, wide):
    """initialize: k_stereo_lines<1, true, 512> (NORM_HAMMING, INITIAL), 81 sequences per family.  The
    initial kernel's block size follows the capacity alone (1024 threads above kl_cap 1024:
    test_line_match_large_and_odd_caps), so both settings run the same kernel here."""
    monkeypatch.setenv("GFPL_SP_WIDE_MAX_B", wide)
    bad = []
    for fam, g in _handlers(rig):
        bad += _stereo_initial(rig, g, L.grid_cases(fam))
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("wide", ["0", "4096"])
def test_stereo_lines_frame_adversarial(monkeypatch, rig, wide):
    """stereoLines after an initialize: k_stereo_lines<2, false, 512 | 1024> (NORM_HAMMING2)."""
    monkeypatch.setenv("GFPL_SP_WIDE_MAX_B", wide)
    bad = []
    for fam, g in _handlers(rig):
        bad += _stereo_frame(rig, g, L.grid_cases(fam))
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("wide", ["0", "4096"])
def test_cross_lines_adversarial(monkeypatch, rig, wide):
    """crossFrameMatchingLines on written frames: k_cross_lines<512 | 1024>; and the match cap (512-row
    sets with more than max_line_match_num mutual matches and rows above 1.2 * budget)."""
    monkeypatch.setenv("GFPL_SP_WIDE_MAX_B", wide)
    bad = []
    for fam, g in _handlers(rig):
        bad += _cross(g, L.grid_cases(fam), rig.cap)
    cases = L.match_cap_cases()
    g = gfpl.StereoFrameHandler(rig.ctx("match_cap"), len(cases), KP, L.MATCH_CAP_KL)
    bad += _cross(g, cases, L.MATCH_CAP_KL)
    assert not bad, "\n".join(bad[:30])


def test_line_match_large_and_odd_caps(monkeypatch):
    """kl_cap 2048 with (NL, NR) = (2048, 2047) and (2047, 2048): train indices above 1024, the
    1024-thread kernels forced by the capacity, the largest LDS layout; kl_cap 200 with 200 / 199 rows:
    a train-view stride that is no multiple of the 32-row tile, under both workgroup layouts."""
    bad = []
    for cases, cap, wides in ((L.large_cases(), 2048, ("0",)), (L.odd_cases(), L.ODD_CAP, ("0", "4096"))):
        r = Rig(len(cases), cap)
        try:
            g = r.handler("planted")
        except gfpl.GfplError as e:     # a capacity the library refuses: it must say so, nothing else to run
            assert e.code == -1 and cap == L.ODD_CAP
            continue
        for wide in wides:
            monkeypatch.setenv("GFPL_SP_WIDE_MAX_B", wide)
            bad += _stereo_initial(r, g, cases)
            bad += _stereo_frame(r, g, cases)
            bad += _cross(g, cases, cap)
    assert not bad, "\n".join(bad[:30])
