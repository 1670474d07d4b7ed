"""Written problems for the log-det line cut (cut_with_max_vol = 1, k_cut.hip), shared by
test_line_cut_cases_cpu.py and test_line_cut_cases_gpu.py.

A case is a State (PREV, CURR and the track after crossFrameMatchingLines, cut_metric_cases.State), a
cut_step, a cut_rng and a name.  Every case is a pure function of its arguments and is built once per
process.  Expected values come from the C++ oracle (oracle_result): the state written into an
OracleHandler with the case's config, then estimateProjUncertainty_submodular.  trace() runs an
instrumented copy of CutRef.search on the case and describes it: per line its steps, the moves that take
a ratio back, the smallest gap between the winning metric and every other compared value (the centre
included), the step and the runner-up of that gap, and the pivot ratios of the sum the line meets.

Every state is held at one capacity (KP, KL), so that any mix of cases fits one batch: the small states
of cut_metric_cases (KL 64) are copied into frames of the long-list state's capacity.

Families:
  ties        one line's ls_covE scaled to within a wanted gap of a switch between two final ratios
  steps       the same states under other cut_step / cut_rng, written lines that meet the camera plane
  lists       list lengths on the 16 / 64 / 128 boundaries of k_cut_prep, k_cut_verify and k_cut_vref
  degenerate  rank-deficient and nearly rank-deficient sums, NaN / Inf / zero covariances, a zero-length line
  proof       the capacities of the proven mode (detail list, step record, the off-table list)
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np

import gfpl
import oracle as O
import cut_metric_cases as K
from cut_metric_ref import CutRef, _div, _mat4_mul, logdet, oracle_to_cross

KP, KL = 256, 160
LONG_SYNTH = dict(n_kp=200, n_kl=158, n_world_pts=260, n_world_lines=210, seed=13)
WIDE = K.WIDE
CUT_FIELDS = K.CUT_FIELDS
HOMOG = 1e-7                      # Config::homog_th of default_config (asserted by the CPU test)
CUT_MIN_PIVOT = 1e-2              # k_cut.hip
N_KEYS, CUT_PATH, CUT_DTL = 22, 64, 4   # gfpl_records.hpp: CUT_KS, CUT_PATH, CUT_DTL
STEP_CAP = 4000                   # the >= variant's step cap per line (it can loop between equal metrics)


def canon(f: gfpl.FrameHost) -> gfpl.FrameHost:
    """NaNs to one bit pattern: the sign of a NaN an operation creates is the processor's choice,
    negative on x86 and positive on the GPU."""
    for a in f.arr.values():
        if a.dtype.kind == "f":
            a[np.isnan(a)] = np.nan
    return f


def camera() -> gfpl.Camera:
    return K.camera()


def config(step=0.05, rng=(0.0, 1.0), **over) -> gfpl.Config:
    return K.config(rng, cut_step=step, **over)


# ------------------------------------------------------------------ states --
def widen(f: gfpl.FrameHost) -> gfpl.FrameHost:
    """f in a frame of capacity (KP, KL): the counts, the pose block and every feature row, indices kept."""
    o = gfpl.FrameHost(KP, KL)
    ptrs = {n: getattr(o.s, n) for n in o.arr}
    C.memmove(C.byref(o.s), C.byref(f.s), C.sizeof(o.s))
    for n, v in ptrs.items():
        setattr(o.s, n, v)
        o.arr[n][:len(f.arr[n])] = f.arr[n]
    return o


def _wide_state(st: K.State) -> K.State:
    return K.State(widen(st.prev), widen(st.curr),
                   {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.track.items()})


@functools.lru_cache(maxsize=None)
def small(b: int) -> K.State:
    """Sequence b of cut_metric_cases.base_states() (about 25 matched lines) at capacity (KP, KL)."""
    return _wide_state(K.base_states()[b])


@functools.lru_cache(maxsize=None)
def small9(b: int) -> K.State:
    return _wide_state(K.batch9_states()[b])


@functools.lru_cache(maxsize=None)
def long_state() -> K.State:
    """One sequence with at least 129 matched lines and 130 matched points (the CPU test asserts both)."""
    cam, cfg = camera(), gfpl.default_config()
    H = gfpl.HostFrames(cam, gfpl.synth_params(**LONG_SYNTH), 1, 3, KP, KL)
    o = O.OracleHandler(cam, cfg, KP, KL)
    o.initialize(H.frames(0), 0)
    o.insertStereoPair(H.frames(1), 0)
    o.optimizePose()
    o.updateFrame()
    oracle_to_cross(o, H.frames(2), 0)
    return K.State(o.read_frame(gfpl.PREV), o.read_frame(gfpl.CURR), o.read_track())


def lists(st: K.State, n_ls=None, n_pt=None) -> K.State:
    """st with its matched lists truncated to n_ls lines / n_pt points (None: as they are)."""
    st = st.copy()
    if n_ls is not None:
        st.track["matched_ls"] = st.track["matched_ls"][:n_ls].copy()
    if n_pt is not None:
        st.track["matched_pt"] = st.track["matched_pt"][:n_pt].copy()
    return st


def dt_inv(st: K.State) -> np.ndarray:
    return (O.inverse4(st.curr.get("Tfw")) @ st.prev.get("Tfw")).reshape(4, 4)


def line_row(st: K.State, pos: int) -> int:
    return int(st.track["matched_ls"][pos])


def with_line_depths(st: K.State, pos: int, z0: float, z1: float) -> K.State:
    """Matched line pos rewritten so that its endpoints have depths z0 and z1 in the CURRENT frame
    (their bearings kept): the segment's extension meets the camera plane at t = z0 / (z0 - z1)."""
    st = st.copy()
    li = line_row(st, pos)
    D = dt_inv(st)
    Di = np.linalg.inv(D)
    for f, z in (("ls_sP", z0), ("ls_eP", z1)):
        g = D[:3, :3] @ st.prev.arr[f][li] + D[:3, 3]
        g = g * (z / g[2])
        st.prev.arr[f][li] = Di[:3, :3] @ g + Di[:3, 3]
    return st


def flat_cov(st: K.State, pos: int, c: float, eps: float) -> K.State:
    """Matched line pos with both endpoint covariances diag(c, c, eps) in the CURRENT frame's axes: with eps tiny
    the depth variance at a ratio on the camera plane is tiny, and a search that does not clamp fgz2 there sees
    a large information where the reference, which clamps, sees none."""
    st = st.copy()
    li = line_row(st, pos)
    R = dt_inv(st)[:3, :3]
    Cv = (R.T @ np.diag([c, c, eps]) @ R).reshape(9)
    st.prev.arr["ls_covS"][li] = Cv
    st.prev.arr["ls_covE"][li] = Cv
    return st


def scaled(st: K.State, pos: int, field: str, s: float) -> K.State:
    st = st.copy()
    li = line_row(st, pos)
    st.prev.arr[field][li] = st.prev.arr[field][li] * s
    return st


# ------------------------------------------------------------------- cases --
class Case:
    def __init__(self, name: str, family: str, state: K.State, step=0.05, rng=(0.0, 1.0), tau=None, **tags):
        self.name, self.family, self.state = name, family, state
        self.step, self.rng = float(step), (float(rng[0]), float(rng[1]))
        self.tau = tau            # ties: the cut_certify the rung's bracket is relative to
        self.tags = tags          # what the name promises (the CPU test asserts it on the trace)

    def key(self):
        return (self.step, self.rng)

    def cfg(self, **over) -> gfpl.Config:
        return config(self.step, self.rng, **over)

    @property
    def n_ls(self) -> int:
        return len(self.state.track["matched_ls"])

    @property
    def n_pt(self) -> int:
        return len(self.state.track["matched_pt"])

    def __repr__(self):
        return f"[{self.family}/{self.name} step {self.step} rng {self.rng} {self.n_ls} lines {self.n_pt} points]"


_ORACLE = {}


def oracle_result(c: Case):
    """(PREV after the oracle's estimateProjUncertainty_submodular, NaNs canonical; its step count)."""
    if id(c) not in _ORACLE:
        o = O.OracleHandler(camera(), c.cfg(), KP, KL)
        o.write_frame(gfpl.PREV, c.state.prev)
        o.write_frame(gfpl.CURR, c.state.curr)
        o.write_track(gfpl.track_from_dict(c.state.track))
        o.estimateProjUncertainty_submodular()
        _ORACLE[id(c)] = (canon(o.read_frame(gfpl.PREV)), o.line_cut_steps())
    return _ORACLE[id(c)]


# ------------------------------------------------- the instrumented search --
def pivot_ratio(M) -> float:
    """Smallest ratio of an LLT pivot of the 6x6 M (36 entries) to its diagonal entry (what k_cut.hip
    holds against CUT_MIN_PIVOT); NaN once a pivot is not positive."""
    A = np.array(M, np.float64).reshape(6, 6)
    Lm = np.zeros((6, 6))
    worst = math.inf
    for k in range(6):
        x = A[k, k] - float(Lm[k, :k] @ Lm[k, :k])
        if not x > 0.0 or not math.isfinite(x):
            return math.nan
        worst = min(worst, x / A[k, k])
        Lm[k, k] = math.sqrt(x)
        for i in range(k + 1, 6):
            Lm[i, k] = (A[i, k] - float(Lm[i, :k] @ Lm[k, :k])) / Lm[k, k]
    return worst


class TracedCut(CutRef):
    """CutRef with metric = logdet, its search instrumented, and the deliberately wrong variants the CPU
    test separates the families from:
      last_max     the last maximum among equal neighbour metrics instead of the first
      ge_centre    >= for > against the centre (with a step cap: it can loop)
      unclamped    fgz2 = fx / gz^2 without max(homog_th, .)
      points_first invCov_sum taken in points-then-lines order
    (the range test before the r0 + r1 > 1 test is no variant: all three tests skip the neighbour, so their
    order cannot change a result)."""

    def __init__(self, cam, cfg, variant=None):
        super().__init__(cam, cfg, logdet)
        self.variant = variant
        self.lines = []

    def _pose_jac(self, g, lx, ly):
        if self.variant != "unclamped":
            return super()._pose_jac(g, lx, ly)
        h, self.homog = self.homog, -math.inf
        try:
            return super()._pose_jac(g, lx, ly)
        finally:
            self.homog = h

    def search(self, D, lines, mls, tot):
        s = self.step
        nb = [(s, 0.0), (-s, 0.0), (0.0, s), (0.0, -s), (s, s), (s, -s), (-s, s), (-s, -s)]
        lo, hi = self.rng
        steps = 0
        for li in mls:
            L = lines[li]
            cut = L["cut"]
            metric_back = self.metric(tot)
            rec = dict(row=li, steps=0, back=0, gap=math.inf, gap_step=-1, gap_vs="", nan=False,
                       pivot=pivot_ratio(tot), path=[], m0=metric_back)
            tot = [tot[i] - L["inv"][i] for i in range(36)]
            rec["pivot"] = min(rec["pivot"], pivot_ratio(tot)) if rec["pivot"] == rec["pivot"] else math.nan
            while cut[0] + cut[1] <= 1.0:
                steps += 1
                rec["steps"] += 1
                if self.variant == "ge_centre" and rec["steps"] > STEP_CAP:
                    break
                hit, cand, cand_info = False, None, None
                metric_init = metric_back
                vals = []
                for j in range(8):
                    rt = (cut[0] + nb[j][0], cut[1] + nb[j][1])
                    if rt[0] + rt[1] > 1.0:
                        continue
                    if rt[0] < lo or rt[0] > hi:
                        continue
                    if rt[1] < lo or rt[1] > hi:
                        continue
                    tmp = self.pose_info_on_line(D, L["Jl"], L["sP"], L["eP"], L["covS"], L["covE"], rt[0], rt[1])
                    m = self.metric([tmp[i] + tot[i] for i in range(36)])
                    vals.append(m)
                    if self.variant == "last_max":
                        better = m > metric_init or (hit and m == metric_init)
                    elif self.variant == "ge_centre":
                        better = m > metric_init or (not hit and m == metric_init)
                    else:
                        better = m > metric_init
                    if better:
                        metric_init, cand, cand_info, hit = m, rt, tmp, True
                        win = len(vals) - 1
                # the gaps the decision rests on: the winner against every other value and the centre
                others = [("centre", metric_back)] if hit else []
                others += [("neighbour", v) for k, v in enumerate(vals) if not (hit and k == win)]
                top = metric_init
                if top != top or any(v != v for _, v in others):
                    rec["nan"] = True
                for kind, v in others:
                    g = abs(top - v)
                    if g < rec["gap"]:
                        rec["gap"], rec["gap_step"], rec["gap_vs"] = g, rec["steps"] - 1, kind
                if not hit:
                    break
                if cand[0] < cut[0] or cand[1] < cut[1]:
                    rec["back"] += 1
                cut[0], cut[1] = cand
                rec["path"].append(cand)
                L["inv"] = cand_info
                metric_back = metric_init
            if not (abs(cut[0]) < 0.0001 and abs(cut[1]) < 0.0001):
                if abs(cut[0]) > 0.0001:
                    L["sP"] = [(1 - cut[0]) * L["sP"][k] + cut[0] * L["eP"][k] for k in range(3)]
                    L["spl"] = self._projection(L["sP"])
                    L["sdisp"] = _div(self.fx * self.b, L["sP"][2])
                if abs(cut[1]) > 0.0001:
                    L["eP"] = [(1 - cut[1]) * L["eP"][k] + cut[1] * L["sP"][k] for k in range(3)]
                    L["epl"] = self._projection(L["eP"])
                    L["edisp"] = _div(self.fx * self.b, L["eP"][2])
            tot = [tot[i] + L["inv"][i] for i in range(36)]
            rec["cut"] = (cut[0], cut[1])
            self.lines.append(rec)
        return steps

    def line_cut(self, prev, curr, track):
        if self.variant != "points_first":
            return super().line_cut(prev, curr, track)
        # (line_cut of CutRef with the two sums exchanged)
        mls = [int(x) for x in track["matched_ls"]]
        mpt = [int(x) for x in track["matched_pt"]]
        if not mls:
            return 0
        a = prev.arr
        Tinv = O.inverse4(curr.get("Tfw")).reshape(16).tolist()
        D = _mat4_mul(Tinv, prev.get("Tfw").reshape(16).tolist())
        lines = {li: dict(Jl=a["ls_le_obs"][li, :2].tolist(), sP=a["ls_sP"][li].tolist(), eP=a["ls_eP"][li].tolist(),
                          covS=a["ls_covS"][li].tolist(), covE=a["ls_covE"][li].tolist()) for li in set(mls)}
        tot = [0.0] * 36
        for pi in mpt:
            tmp = self.pose_info_point(D, a["pt_P"][pi].tolist(), a["pt_pl_obs"][pi].tolist())
            tot = [tot[i] + tmp[i] for i in range(36)]
        for li in mls:
            L = lines[li]
            L["cut"] = [0.0, 0.0]
            L["inv"] = self.pose_info_on_line(D, L["Jl"], L["sP"], L["eP"], L["covS"], L["covE"], 0.0, 0.0)
            tot = [tot[i] + L["inv"][i] for i in range(36)]
        steps = self.search(D, lines, mls, tot)
        for li, L in lines.items():
            a["ls_cut"][li] = L["cut"]
            a["ls_invcov"][li] = L["inv"]
            for f, k in (("ls_sP", "sP"), ("ls_eP", "eP"), ("ls_spl", "spl"), ("ls_epl", "epl"),
                         ("ls_sdisp", "sdisp"), ("ls_edisp", "edisp")):
                if k in L:
                    a[f][li] = L[k]
        return steps


class Trace:
    """What the (variant of the) Python search did on one state."""

    def __init__(self, st: K.State, step, rng, variant=None):
        st = st.copy()
        ref = TracedCut(camera(), config(step, rng), variant)
        self.steps = ref.line_cut(st.prev, st.curr, st.track)
        self.prev = canon(st.prev)
        self.lines = ref.lines
        self.ratios = K.ratios(st.prev, st.track)

    @property
    def gap(self):
        return min((r["gap"] for r in self.lines), default=math.inf)

    @property
    def back(self):
        return sum(r["back"] for r in self.lines)

    @property
    def max_steps(self):
        return max((r["steps"] for r in self.lines), default=0)


_TRACE = {}


def trace(c: Case, variant=None) -> Trace:
    k = (id(c), variant)
    if k not in _TRACE:
        _TRACE[k] = Trace(c.state, c.step, c.rng, variant)
    return _TRACE[k]


def same_cut(a: gfpl.FrameHost, b: gfpl.FrameHost) -> bool:
    """CUT_FIELDS of two (canonical) frames equal bit for bit."""
    return all(a.arr[f].tobytes() == b.arr[f].tobytes() for f in CUT_FIELDS)


# -------------------------------------------------------------------- ties --
class Switch:
    """A scalar s* of one line's ls_covE scale at which the line's final ratios switch: bisected between lo and
    hi down to adjacent doubles (a < b, the line ending at other ratios at a than at b).  Every evaluation is
    kept as (s, the line's final ratios, the state's smallest gap)."""

    def __init__(self, base: K.State, pos: int, lo: float, hi: float, step=0.05, rng=(0.0, 1.0), field="ls_covE",
                 first=False):
        self.base, self.pos, self.step, self.rng, self.field = base, pos, step, rng, field
        self.first = first      # the switch of the line's first move instead of its final ratios
        self.evals = {}
        a, b = lo, hi
        fa, fb = self.at(a)[0], self.at(b)[0]
        assert fa != fb, (fa, fb)
        while True:
            m = 0.5 * (a + b)
            if not a < m < b:
                break
            fm = self.at(m)[0]
            if fm == fa:
                a = m
            else:           # (a third outcome: the switch nearest a)
                b, fb = m, fm
        self.a, self.b, self.fa, self.fb = a, b, fa, fb

    def state(self, s: float) -> K.State:
        return scaled(self.base, self.pos, self.field, s)

    def at(self, s: float):
        if s not in self.evals:
            t = Trace(self.state(s), self.step, self.rng)
            r = t.lines[self.pos]
            self.evals[s] = (tuple(r["path"][:1]) if self.first else r["cut"], r["gap"], r["gap_step"], r["gap_vs"], t.gap)
        return self.evals[s]

    def side(self, s: float) -> int:
        return 0 if s <= self.a else 1

    def reach(self, side: int, lo: float, hi: float):
        """A scalar on `side` of the switch whose gap lies in [lo, hi] and whose line ends at that side's
        ratios: among the bisection's evaluations, else by stepping along the (locally linear) gap."""
        want = self.fa if side == 0 else self.fb
        edge = self.a if side == 0 else self.b
        ok = lambda s: self.at(s)[0] == want and lo <= self.at(s)[4] <= hi and self.side(s) == side
        have = sorted((abs(s - edge), s) for s in list(self.evals) if ok(s))
        if have:
            return have[0][1]
        # slope from the evaluation of this side nearest the target
        tgt = math.sqrt(lo * hi) if lo > 0 else 0.5 * hi
        pts = [(s, self.at(s)[4]) for s in self.evals if self.side(s) == side and self.at(s)[0] == want and s != edge
               and self.at(s)[4] > 0]
        pts.sort(key=lambda p: abs(math.log(p[1] / tgt)))
        s0, g0 = pts[0]
        for _ in range(12):
            s = edge + (s0 - edge) * (tgt / g0)
            if ok(s):
                return s
            g = self.at(s)[4]
            if self.at(s)[0] != want or not g > 0:
                break
            s0, g0 = s, g
        raise AssertionError(f"no scalar with a gap in [{lo}, {hi}] on side {side} of {self.a!r}")


TAUS = (1e-9, 1e-10)
# rung -> the gap's bracket in units of tau (the far / lastbit rungs are absolute)
RUNGS = {"clear": (4.0, 64.0), "above": (1.0, 2.0), "below": (0.0, 0.25)}


def _ladder(name: str, sw: Switch) -> list:
    out = []
    for tau in TAUS:
        for rung, (lo, hi) in RUNGS.items():
            for side in (0, 1):
                s = sw.reach(side, lo * tau * (1 + 1e-6) if lo else 0.0, hi * tau)
                out.append(Case(f"{name}_tau{tau:g}_{rung}_{'lo' if side == 0 else 'hi'}", "ties", sw.state(s), sw.step,
                                sw.rng, tau=tau, rung=rung, bracket=(lo * tau, hi * tau), pos=sw.pos))
    for side in (0, 1):
        s = sw.reach(side, 0.0, 1e-12)
        out.append(Case(f"{name}_far_{'lo' if side == 0 else 'hi'}", "ties", sw.state(s), sw.step, sw.rng, tau=1e-10,
                        rung="far", bracket=(0.0, 1e-12), pos=sw.pos))
    for side, s in ((0, sw.a), (1, sw.b)):
        out.append(Case(f"{name}_lastbit_{'lo' if side == 0 else 'hi'}", "ties", sw.state(s), sw.step, sw.rng, tau=1e-10,
                        rung="lastbit", bracket=(0.0, 1e-12), pos=sw.pos, pair=(sw.a, sw.b)))
    return out


# (state, list length = line position + 1, scale lo, scale hi): found by scanning on the CPU; the CPU test asserts
# what each is (the step and the runner-up of its tie)
TIE_MID = (0, 4, 1.0, 6.0)        # a later step of the line, one neighbour against another


@functools.lru_cache(maxsize=None)
def switch(which: str) -> Switch:
    b, n, lo, hi = {"mid": TIE_MID, "centre": TIE_CENTRE, "first": TIE_FIRST}[which]
    return Switch(lists(small(b), n), n - 1, lo, hi, first=(which == "first"))
TIE_CENTRE = (0, 1, 0.5, 1.0)     # the line's stop: the best neighbour against the centre
TIE_FIRST = (0, 1, 20.0, 100.0)   # the line's first step: (s, s) against (0, s) from (0, 0)


@functools.lru_cache(maxsize=None)
def _ties() -> tuple:
    out = _ladder("mid", switch("mid"))
    # the centre and first-step ties: the rungs of tau = 1e-9 and the absolute ones
    for which in ("centre", "first"):
        out += [c for c in _ladder(which, switch(which)) if "tau1e-10" not in c.name]
    return tuple(out)


# -------------------------------------------------------- steps and ranges --
STEPS = (0.02, 0.01, 0.005, 0.07, 0.125, 0.3, 1.0, 2.0)
RANGES = (WIDE, (0.1, 0.1), (0.0, 0.0), (0.25, 0.5), (0.0, 0.5))
STEP_STATES = {0.01: (0, 4), 0.005: (0, 1)}   # (sequence 4 has a line of 65 steps at 0.01; others: 0 and 1)
STEP_LINES = {0.005: 5}                       # (a list length that keeps the 0.005 cases' Python trace short)
PD_EDGE = math.sqrt(2.0 * HOMOG)          # |gz| at which PD_OK flips


@functools.lru_cache(maxsize=None)
def _steps() -> tuple:
    out = []
    for s in STEPS:
        for b in STEP_STATES.get(s, (0, 1)):
            st = lists(small(b), STEP_LINES.get(s))
            out.append(Case(f"step{s:g}_s{b}", "steps", st, step=s, back=(s == 0.02), past_keys=(s in (0.02, 0.01, 0.005)),
                            over_path=(s == 0.005 or (s, b) == (0.01, 4)), one_step=(s == 2.0)))
    for r in RANGES:
        for b in (0, 2):
            out.append(Case(f"rng{r[0]:g}_{r[1]:g}_s{b}", "steps", small(b), rng=r, in_range=r))
    # written lines whose extension meets the camera plane at a grid ratio of the wide range: depths in the current
    # frame 1 -> 21 (the start side at t = -0.05), 21 -> 1 (the end side) and 1 -> 3 (t = -0.5, the range's end)
    for z0, z1 in ((1.0, 21.0), (21.0, 1.0), (1.0, 3.0)):
        st = with_line_depths(lists(small(0), 6), 2, z0, z1)
        out.append(Case(f"plane{z0:g}_{z1:g}_wide", "steps", st, rng=WIDE, negative=True, written=2))
        out.append(Case(f"plane{z0:g}_{z1:g}", "steps", st, written=2))
    # the same lines with a flat covariance (depth variance 1e-12): here the clamp decides.  Without it the ratio on
    # the camera plane wins a step; the reference, which clamps, never takes it
    for npt, cv, z0, z1 in ((None, 1e-4, 1.0, 21.0), (None, 1e-4, 21.0, 1.0), (None, 1e-4, 1.0, 3.0),
                            (None, 1e-4, 0.5, 10.5), (0, 1e-4, 1.0, 21.0), (6, 1e-2, 0.5, 10.5)):
        st = flat_cov(with_line_depths(lists(small(0), 6, npt), 2, z0, z1), 2, cv, 1e-12)
        out.append(Case(f"flat{z0:g}_{z1:g}_{'all' if npt is None else npt}p_wide", "steps", st, rng=WIDE, negative=True,
                        written=2, clamp_decides=True))
    # |gz| of one end just above / just below sqrt(2 homog_th): the PD_OK boundary
    for tag, f in (("above", 1.0 + 1e-6), ("below", 1.0 - 1e-6)):
        st = with_line_depths(lists(small(0), 6), 2, PD_EDGE * f, 2.0)
        out.append(Case(f"pd_edge_{tag}", "steps", st, written=2, pd_edge=f))
        out.append(Case(f"pd_edge_{tag}_wide", "steps", st, rng=WIDE, written=2, pd_edge=f))
    # gz^2 of the start below homog_th at r = 0: the clamp of fgz2 is in the line's own info
    st = with_line_depths(lists(small(0), 6), 2, 2e-4, 2.0)
    out.append(Case("clamp_start", "steps", st, written=2, clamped=True))
    out.append(Case("clamp_start_wide", "steps", st, rng=WIDE, written=2, clamped=True))
    return tuple(out)


# ------------------------------------------------------------------- lists --
LIST_LS = (15, 16, 17, 63, 64, 65, 128, 129)
LIST_PT = (0, 1, 63, 64, 130)
LIST_EXTRA = ((64, 64), (64, 63), (65, 130), (129, 130), (128, 0), (16, 0), (63, 1))


@functools.lru_cache(maxsize=None)
def _lists() -> tuple:
    out = []
    pairs = [(n, LIST_PT[i % len(LIST_PT)]) for i, n in enumerate(LIST_LS)] + list(LIST_EXTRA)
    for n, m in pairs:
        out.append(Case(f"long_{n}l_{m}p", "lists", lists(long_state(), n, m), n_ls=n, n_pt=m))
    names = ["full0", "empty", "one_line", "two_lines", "no_points", "zero_cov", "full6", "full7", "full8"]
    for b, nm in enumerate(names):   # cut_metric_cases.batch9_states() as it stands
        out.append(Case(f"batch9_{nm}", "lists", small9(b)))
    return tuple(out)


# -------------------------------------------------------------- degenerate --
# (sequence, points, lines) of the short lists.  2 x lines + points < 6 leaves the sum rank-deficient, but in no
# list of the generator's does the reference's LLT meet a non-positive pivot: the last pivots are rounding noise
# that happens to be positive, the metrics are finite and the lines move on that noise.  The null_dir lists are
# written so that the pivot is exactly zero: le_obs = (1, 0) leaves row and column 1 of every info exactly zero,
# no metric is finite and nothing moves.
SHORT = [(0, 0, 1), (0, 0, 2), (0, 0, 3), (1, 0, 1), (1, 0, 2), (1, 0, 3), (2, 0, 3), (2, 1, 1), (0, 1, 5), (0, 2, 4)]
PIVOT = [(1, 6, 1, "above"), (0, 4, 1, "above"), (2, 3, 4, "below"), (0, 4, 3, "below"), (0, 6, 2, "below")]


def _poke(st: K.State, pos: int, field: str, idx: int, v: float) -> K.State:
    st = st.copy()
    st.prev.arr[field][line_row(st, pos), idx] = v
    return st


@functools.lru_cache(maxsize=None)
def _degenerate() -> tuple:
    out = []
    for b, m, n in SHORT:
        out.append(Case(f"short_s{b}_{m}p_{n}l", "degenerate", lists(small(b), n, m), n_ls=n, n_pt=m,
                        rank_deficient=(2 * n + m < 6)))
    for n in (1, 2, 3):
        st = lists(small(0), n, 0)
        for pos in range(n):
            st.prev.arr["ls_le_obs"][line_row(st, pos), :2] = (1.0, 0.0)
        out.append(Case(f"null_dir_{n}l", "degenerate", st, n_ls=n, n_pt=0, stays=True))
    for b, m, n, side in PIVOT:
        out.append(Case(f"pivot_{side}_s{b}_{m}p_{n}l", "degenerate", lists(small(b), n, m), n_ls=n, n_pt=m, pivot=side))
    st = lists(small(3), 6)
    out.append(Case("nan_covS", "degenerate", _poke(st, 1, "ls_covS", 0, math.nan), nonfinite=True))
    out.append(Case("inf_covS", "degenerate", _poke(st, 1, "ls_covS", 4, math.inf), nonfinite=True))
    z = st.copy()
    z.prev.arr["ls_eP"][line_row(z, 2)] = z.prev.arr["ls_sP"][line_row(z, 2)]
    out.append(Case("zero_length", "degenerate", z, written=2))
    return tuple(out)


# ------------------------------------------------------------------- proof --
BACK_LINES = (1, (4, 10, 13, 14, 15, 21))   # small(1) at step 0.02: every one of these lines moves a ratio back


@functools.lru_cache(maxsize=None)
def _proof() -> tuple:
    out = []
    # under a range outside [0, 1] the proven mode bounds no line (verify_line_bound): every line with a margined
    # step is left to the per-step replay.  6 lines overflow the detail list at B = 1 (CUT_DTL x B = 4) and fit
    # it at B = 9 beside empty lists
    out.append(Case("detail6_wide", "proof", lists(small(0), 6), rng=WIDE, detail=6))
    st = small(BACK_LINES[0]).copy()
    st.track["matched_ls"] = st.track["matched_ls"][list(BACK_LINES[1])].copy()
    out.append(Case("all_back", "proof", st, step=0.02, all_back=True, back=True, past_keys=True))
    out.append(Case("clear", "proof", small(4), clear=True))
    out += [c for c in _steps() if c.tags.get("over_path")]
    return tuple(out)


FAMILIES = {"ties": _ties, "steps": _steps, "lists": _lists, "degenerate": _degenerate, "proof": _proof}


def family(name: str) -> tuple:
    return FAMILIES[name]()


def all_cases() -> list:
    seen, out = set(), []
    for f in FAMILIES:
        for c in family(f):
            if id(c) not in seen:
                seen.add(id(c))
                out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def empty_case() -> Case:
    return Case("empty", "lists", lists(small(0), 0, 0))


def last_key(step: float) -> float:
    """cut_keys[21] of the proven search for a range reaching past it: 21 additions of the step."""
    t = 0.0
    for _ in range(N_KEYS - 1):
        t = t + step
    return t
