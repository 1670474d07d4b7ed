"""estimateProjUncertainty_submodular with the metric as a parameter (CPU reference).

A plain restatement of the oracle's lineCut() (oracle/gfpl_oracle.cpp, itself
src/stereoFrameHandler.cpp:1618-1764 with getPoseInfoOnLine :1342-1411,
getPoseInfoPoint :1414-1447 and updateEndPointByRatio :1451-1470), operation for
operation, on the oracle's PREV / CURR FrameHost and track as they stand after
crossFrameMatchingLines.  Python floats are IEEE doubles and nothing here is fused, so
with metric = logdet it gives gfplo_line_cut's bits (tests/test_cut_metric_cpu.py pins
that); with metric = min_eig it is the reference of cut_with_max_vol = 0 (DESIGN.md §3
N5), which the oracle does not run.

The matrix primitives are the oracle's own: inverse4, logdet6, eig_sym.
"""
from __future__ import annotations

import numpy as np

import gfpl
import oracle as O


def _div(a: float, b: float) -> float:
    """a / b as IEEE gives it (a Python float raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def _ref_max(a, b):
    return b if a < b else a


def _se3_apply(T, P):
    return [((T[i * 4 + 0] * P[0] + T[i * 4 + 1] * P[1]) + T[i * 4 + 2] * P[2]) + T[i * 4 + 3] for i in range(3)]


def _mat4_mul(A, B):
    return [((A[i * 4 + 0] * B[0 * 4 + j] + A[i * 4 + 1] * B[1 * 4 + j]) + A[i * 4 + 2] * B[2 * 4 + j])
            + A[i * 4 + 3] * B[3 * 4 + j] for i in range(4) for j in range(4)]


# ---- metrics: 36 row-major entries of info + invCov_sum -> float
def logdet(M) -> float:
    """logdet (include/linespec.h:43-56), the cut_with_max_vol = 1 metric."""
    return O.logdet6(np.array(M, np.float64).reshape(6, 6))


def mirror_lower(M) -> np.ndarray:
    A = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            A[i, j] = M[i * 6 + j]
            A[j, i] = M[i * 6 + j]
    return A


def min_eig(M) -> float:
    """getMinEigenValue (src/linespec.cpp:53-66), pinned to element 0 of eig_sym of the matrix
    whose lower triangle is M's, mirrored."""
    return float(O.eig_sym(mirror_lower(M))[0])


class CutRef:
    def __init__(self, cam: gfpl.Camera, cfg: gfpl.Config, metric=min_eig):
        self.fx, self.fy, self.cx, self.cy, self.b = cam.fx, cam.fy, cam.cx, cam.cy, cam.b
        self.homog = cfg.homog_th
        self.step = cfg.cut_step
        self.rng = (cfg.cut_rng[0], cfg.cut_rng[1])
        self.metric = metric

    # getJacob3D_2D (src/stereoFrame.cpp:1394-1412)
    def _jacob3D_2D(self, px, py, pz):
        f, b, pz_2 = self.fx, self.b, pz * pz
        J = [0.0] * 9
        J[0] = _div(f, pz)
        J[4] = _div(f, pz)
        J[2] = _div((-f) * px, pz_2)
        J[5] = _div((-f) * py, pz_2)
        J[8] = _div((-f) * b, pz_2)
        return J

    def _pose_jac(self, g, lx, ly):
        gx, gy, gz = g
        gz2 = gz * gz
        fgz2 = _div(self.fx, _ref_max(self.homog, gz2))
        return [(fgz2 * lx) * gz,
                (fgz2 * ly) * gz,
                (-fgz2) * ((gx * lx) + (gy * ly)),
                (-fgz2) * ((((gx * gy) * lx) + ((gy * gy) * ly)) + ((gz * gz) * ly)),
                fgz2 * ((((gx * gx) * lx) + ((gz * gz) * lx)) + ((gx * gy) * ly)),
                fgz2 * (((gx * gz) * ly) - ((gy * gz) * lx))]

    def _endpoint_var(self, D, Jl, Pt, cov):
        Jdt = [D[i * 4 + j] for i in range(3) for j in range(3)]
        cur = _se3_apply(D, Pt)
        Jp = self._jacob3D_2D(cur[0], cur[1], cur[2])
        T1 = [(Jp[i * 3 + 0] * Jdt[0 * 3 + j] + Jp[i * 3 + 1] * Jdt[1 * 3 + j]) + Jp[i * 3 + 2] * Jdt[2 * 3 + j]
              for i in range(2) for j in range(3)]
        T2 = [(T1[i * 3 + 0] * cov[0 * 3 + j] + T1[i * 3 + 1] * cov[1 * 3 + j]) + T1[i * 3 + 2] * cov[2 * 3 + j]
              for i in range(2) for j in range(3)]
        T3 = [(T2[i * 3 + 0] * Jdt[j * 3 + 0] + T2[i * 3 + 1] * Jdt[j * 3 + 1]) + T2[i * 3 + 2] * Jdt[j * 3 + 2]
              for i in range(2) for j in range(3)]
        M = [(T3[i * 3 + 0] * Jp[j * 3 + 0] + T3[i * 3 + 1] * Jp[j * 3 + 1]) + T3[i * 3 + 2] * Jp[j * 3 + 2]
             for i in range(2) for j in range(2)]
        r0 = Jl[0] * M[0] + Jl[1] * M[2]
        r1 = Jl[0] * M[1] + Jl[1] * M[3]
        return r0 * Jl[0] + r1 * Jl[1]

    # getPoseInfoOnLine (src/stereoFrameHandler.cpp:1342-1411)
    def pose_info_on_line(self, D, Jl, sP, eP, covS, covE, c0, c1):
        sPt = [(1 - c0) * sP[k] + c0 * eP[k] for k in range(3)]
        ePt = [(1 - c1) * eP[k] + c1 * sP[k] for k in range(3)]
        a0, q0 = (1 - c0) * (1 - c0), c0 * c0
        a1, q1 = (1 - c1) * (1 - c1), c1 * c1
        covSt = [a0 * covS[i] + q0 * covE[i] for i in range(9)]
        covEt = [a1 * covE[i] + q1 * covS[i] for i in range(9)]
        vs = self._endpoint_var(D, Jl, sPt, covSt)
        ve = self._endpoint_var(D, Jl, ePt, covEt)
        det = vs * ve - 0.0 * 0.0
        invdet = _div(1.0, det)
        i00, i10, i01, i11 = ve * invdet, -0.0 * invdet, -0.0 * invdet, vs * invdet
        Js = self._pose_jac(_se3_apply(D, sPt), Jl[0], Jl[1])
        Je = self._pose_jac(_se3_apply(D, ePt), Jl[0], Jl[1])
        T0 = [Js[i] * i00 + Je[i] * i10 for i in range(6)]
        T1 = [Js[i] * i01 + Je[i] * i11 for i in range(6)]
        return [T0[i] * Js[j] + T1[i] * Je[j] for i in range(6) for j in range(6)]

    # getPoseInfoPoint (src/stereoFrameHandler.cpp:1414-1447)
    def pose_info_point(self, D, P, pl_obs):
        cur = _se3_apply(D, P)
        u = self.cx + _div(self.fx * cur[0], cur[2])
        v = self.cy + _div(self.fy * cur[1], cur[2])
        J = self._pose_jac(cur, u - pl_obs[0], v - pl_obs[1])
        return [J[i] * J[j] for i in range(6) for j in range(6)]

    def _projection(self, P):
        return [self.cx + _div(self.fx * P[0], P[2]), self.cy + _div(self.fy * P[1], P[2])]

    def search(self, D, lines: dict, mls: list, tot: list) -> int:
        """The loop over the matched lines (:1659-1762) on invCov_sum = tot (36 entries, the lines' r = 0
        infos L["inv"] included).  Each line dict ends with its cut, info and (where
        updateEndPointByRatio moved them) endpoints; returns the number of search steps."""
        s = self.step
        nb = [(s, 0.0), (-s, 0.0), (0.0, s), (0.0, -s), (s, s), (s, -s), (-s, s), (-s, -s)]
        lo, hi = self.rng
        steps = 0
        for li in mls:
            L = lines[li]
            cut = L["cut"]
            metric_back = self.metric(tot)
            tot = [tot[i] - L["inv"][i] for i in range(36)]
            while cut[0] + cut[1] <= 1.0:
                steps += 1
                hit, cand, cand_info = False, None, None
                metric_init = metric_back
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
                    if m > metric_init:
                        metric_init, cand, cand_info, hit = m, rt, tmp, True
                if not hit:
                    break
                cut[0], cut[1] = cand
                L["inv"] = cand_info
                metric_back = metric_init
            # updateEndPointByRatio (:1451-1470)
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
        return steps

    def line_cut(self, prev: gfpl.FrameHost, curr: gfpl.FrameHost, track: dict) -> int:
        """lineCut() on prev (in place: ls_cut, ls_invcov and the cut endpoints of the matched
        lines); returns the number of search steps (iterations of the while loop)."""
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
        for li in mls:
            L = lines[li]
            L["cut"] = [0.0, 0.0]
            L["inv"] = self.pose_info_on_line(D, L["Jl"], L["sP"], L["eP"], L["covS"], L["covE"], 0.0, 0.0)
            tot = [tot[i] + L["inv"][i] for i in range(36)]
        for pi in mpt:
            tmp = self.pose_info_point(D, a["pt_P"][pi].tolist(), a["pt_pl_obs"][pi].tolist())
            tot = [tot[i] + tmp[i] for i in range(36)]
        steps = self.search(D, lines, mls, tot)
        for li, L in lines.items():
            a["ls_cut"][li] = L["cut"]
            a["ls_invcov"][li] = L["inv"]
            for f, k in (("ls_sP", "sP"), ("ls_eP", "eP"), ("ls_spl", "spl"), ("ls_epl", "epl"),
                         ("ls_sdisp", "sdisp"), ("ls_edisp", "edisp")):
                if k in L:
                    a[f][li] = L[k]
        return steps


def oracle_to_cross(o: "O.OracleHandler", fr: gfpl.Frames, seq: int):
    """The oracle's insertStereoPair up to crossFrameMatchingLines (the line cut not run)."""
    o.begin_frame(fr, seq)
    o.stereoPoints()
    o.stereoLines()
    o.estimateStereoUncertainty()
    o.crossFrameMatchingPoints()
    o.crossFrameMatchingLines()


def substituted_insert(o: "O.OracleHandler", fr: gfpl.Frames, seq: int, ref: CutRef) -> int:
    """The oracle's insertStereoPair with ref's line cut in place of its own: the stages up to
    crossFrameMatchingLines, then ref's cut written into PREV (optimizePose and updateFrame follow as
    usual).  Returns the cut's step count."""
    oracle_to_cross(o, fr, seq)
    prev = o.read_frame(gfpl.PREV)
    steps = ref.line_cut(prev, o.read_frame(gfpl.CURR), o.read_track())
    o.write_frame(gfpl.PREV, prev)
    return steps
