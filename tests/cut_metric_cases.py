"""Inputs and references shared by the CPU and GPU tests of the min-eigenvalue line cut
(cut_with_max_vol = 0): oracle states after crossFrameMatchingLines, and the reference cut
(tests/cut_metric_ref.py) of each, computed once per process.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import gfpl
import oracle as O
from cut_metric_ref import CutRef, logdet, min_eig, oracle_to_cross

# ---- per-stage inputs (gfpl_line_cut from oracle state): small frames, M_l ~ 25 per sequence
KP, KL = 256, 64
N_SEQ = 17                      # a lone group, a full wave, a wave + 1, two waves + 1: B = 1, 8, 9, 17
SYNTH = dict(n_kp=150, n_kl=30, n_world_pts=200, n_world_lines=40, seed=13)
WIDE = (-0.5, 1.5)
STEP_B, STEP_F = 3, 3            # whole steps: frameStep over 3 frames, B = 3 (the batch's first sequences)
CUT_FIELDS = ["ls_cut", "ls_invcov", "ls_sP", "ls_eP", "ls_spl", "ls_epl", "ls_sdisp", "ls_edisp"]


def config(rng=(0.0, 1.0), **over) -> gfpl.Config:
    cfg = gfpl.default_config(**over)
    cfg.cut_rng[0], cfg.cut_rng[1] = rng
    return cfg


def camera() -> gfpl.Camera:
    return gfpl.make_camera("vga", gfpl.default_config())


@functools.lru_cache(maxsize=None)
def host_frames() -> gfpl.HostFrames:
    return gfpl.HostFrames(camera(), gfpl.synth_params(**SYNTH), N_SEQ, 1 + STEP_F, KP, KL)


class State:
    """One sequence after crossFrameMatchingLines: PREV, CURR and the track, as read from the oracle."""

    def __init__(self, prev: gfpl.FrameHost, curr: gfpl.FrameHost, track: dict):
        self.prev, self.curr, self.track = prev, curr, track

    def copy(self) -> "State":
        return State(_copy_frame(self.prev), _copy_frame(self.curr),
                     {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.track.items()})


def _copy_frame(f: gfpl.FrameHost) -> gfpl.FrameHost:
    o = gfpl.FrameHost(f.kp_cap, f.kl_cap)
    ptrs = {n: getattr(o.s, n) for n in o.arr}
    C.memmove(C.byref(o.s), C.byref(f.s), C.sizeof(o.s))   # the counts and the pose block
    for n, v in ptrs.items():
        setattr(o.s, n, v)
        o.arr[n][...] = f.arr[n]
    return o


def _state(b: int) -> State:
    """Sequence b of the synthetic batch: one full oracle step (frame 1), then frame 2 up to the cut."""
    H = host_frames()
    cam, cfg = camera(), gfpl.default_config()
    o = O.OracleHandler(cam, cfg, KP, KL)
    o.initialize(H.frames(0), b)
    o.insertStereoPair(H.frames(1), b)
    o.optimizePose()
    o.updateFrame()
    oracle_to_cross(o, H.frames(2), b)
    return State(o.read_frame(gfpl.PREV), o.read_frame(gfpl.CURR), o.read_track())


@functools.lru_cache(maxsize=None)
def base_states() -> tuple:
    return tuple(_state(b) for b in range(N_SEQ))


def _cut_list(st: State, n: int) -> State:
    st = st.copy()
    st.track["matched_ls"] = st.track["matched_ls"][:n].copy()
    return st


def _no_points(st: State) -> State:
    st = st.copy()
    st.track["matched_pt"] = st.track["matched_pt"][:0].copy()
    return st


def _zero_cov(st: State) -> State:
    """The second matched line's start covariance zeroed: vs = 0 at r = (0, 0), so its info and with it
    invCov_sum are not finite from the first sum on (no metric is ever greater: no line moves)."""
    st = st.copy()
    st.prev.arr["ls_covS"][int(st.track["matched_ls"][1])] = 0.0
    return st


ZERO_COV_SLOT = 5


@functools.lru_cache(maxsize=None)
def batch9_states() -> tuple:
    """The batch of 9: in the first wave, matched-line lists cut to 0, 1 and 2 entries, a sequence
    without matched points and one with a zero-covariance line, beside full ones."""
    s = base_states()
    return (s[0], _cut_list(s[1], 0), _cut_list(s[2], 1), _cut_list(s[3], 2), _no_points(s[4]), _zero_cov(s[5]),
            s[6], s[7], s[8])


def states(name: str) -> tuple:
    return batch9_states() if name == "batch9" else base_states()


@functools.lru_cache(maxsize=None)
def reference(name: str, idx: int, rng=(0.0, 1.0), metric: str = "min_eig"):
    """(PREV after the reference cut, its step count) of sequence idx of states(name)."""
    st = states(name)[idx].copy()
    ref = CutRef(camera(), config(rng), min_eig if metric == "min_eig" else logdet)
    steps = ref.line_cut(st.prev, st.curr, st.track)
    return st.prev, steps


def ratios(prev: gfpl.FrameHost, track: dict) -> np.ndarray:
    return prev.arr["ls_cut"][np.asarray(track["matched_ls"], np.int64)].copy()


@functools.lru_cache(maxsize=None)
def step_reference(b: int) -> dict:
    """Sequence b over STEP_F whole steps of the oracle with the min-eig reference cut substituted
    (cut_metric_ref.substituted_insert).  "cuts": per step (the state before the cut, PREV after it);
    "steps": per step dict(old = PREV after optimizePose, track = the track then, new = PREV after
    updateFrame, n = the cut's step count)."""
    H = host_frames()
    cam, cfg = camera(), config()
    ref = CutRef(cam, cfg, min_eig)
    o = O.OracleHandler(cam, cfg, KP, KL)
    o.initialize(H.frames(0), b)
    out = {"cuts": [], "steps": []}
    for k in range(1, 1 + STEP_F):
        oracle_to_cross(o, H.frames(k), b)
        st = State(o.read_frame(gfpl.PREV), o.read_frame(gfpl.CURR), o.read_track())
        prev = _copy_frame(st.prev)
        n = ref.line_cut(prev, st.curr, st.track)
        o.write_frame(gfpl.PREV, prev)
        out["cuts"].append((st, prev))
        o.optimizePose()
        old, track = o.read_frame(gfpl.PREV), o.read_track()
        o.updateFrame()
        out["steps"].append(dict(old=old, track=track, new=o.read_frame(gfpl.PREV), n=n))
    return out
