"""gfpl — Python host side of the MI355X-native GF-PL-SLAM tracking path.

Thin ctypes mirror of ``include/gfpl.h``.  The compute path is the HIP library
``gf-pl-slam_amd/lib/libgfpl_hip.so`` (hand-written gfx950 kernels); this module
only marshals structs and (optionally) torch device buffers.  There is no CPU
fallback: the product classes raise if the HIP library is missing.

The class names mirror the reference's operator interface
(``StVO::StereoFrameHandler`` — include/stereoFrameHandler.h:38-174) so the parity
tests read like the reference's own call sequence (app/plslam_mod.cpp:375-477):
``initialize`` -> ``insertStereoPair`` -> ``optimizePose`` -> ``updateFrame``.
"""
from __future__ import annotations

import ctypes as C
import enum
import json
import os
from typing import Optional

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(PKG_DIR, "lib")
REPO_DIR = os.path.dirname(PKG_DIR)

DESC = 32
MAX_LEVELS = 8
MAX_MATCHED_PT = 2048
MAX_MATCHED_LS = 1024
PREV, CURR = 0, 1
HAMMING, HAMMING2 = 1, 2

ERRORS = {0: "ok", -1: "invalid argument", -2: "HIP runtime error", -3: "no HIP device",
          -4: "knn-2 needs at least 2 train descriptors", -5: "capacity exceeded",
          -6: "call order violated", -7: "unsupported config", -8: "device memory allocation failed"}


class StepSlot(enum.IntEnum):
    """Slots of a sequence's step record (``debug_step_records``): the GFPL_STEP_* constants of
    include/gfpl.h, member for member (tests/test_abi.py compares them)."""
    B_STEREO_POINTS = 0
    B_STEREO_LINES = 1
    B_CROSS_POINTS = 2
    B_CROSS_LINES = 3
    B_LINE_CUT = 4
    B_POSE = 5
    B_TOTAL = 6
    B_CUT_SEARCH = 7
    N_O = 8
    N_K = 9
    M_O = 10
    S_P = 11
    S_L = 12
    M_P = 13
    M_L = 14
    N_INLIERS = 15
    CUT_STEPS = 16
    CUT_EXACT = 17
    INLIERS_POSE = 18
    CUT_UNBOUNDED = 19
    PROOF_REDONE = 20
    PROOF_STEPS = 21
    PROOF_VREF = 22
    PROOF_LINES = 23


STEP_REC = len(StepSlot)


class GfplError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        super().__init__(f"{what}: gfpl error {code} ({ERRORS.get(code, '?')})")
        self.code = code


# --------------------------------------------------------------- structs --
class Camera(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("b", C.c_double), ("n_levels", C.c_int),
                ("scale", C.c_float * MAX_LEVELS), ("inv_scale", C.c_float * MAX_LEVELS),
                ("lvl_cols", C.c_int * MAX_LEVELS), ("lvl_rows", C.c_int * MAX_LEVELS),
                ("lvl_offset", C.c_int64 * MAX_LEVELS), ("pyr_bytes", C.c_int64),
                ("sigma2_pt", C.c_double * MAX_LEVELS), ("sigma2_ln", C.c_double * MAX_LEVELS)]


class Config(C.Structure):
    _fields_ = [("best_lr_matches", C.c_int), ("lr_in_parallel", C.c_int),
                ("use_line_conf_cut", C.c_int), ("cut_with_max_vol", C.c_int),
                ("ratio_disp_std", C.c_double), ("ratio_disp_std_hor", C.c_double),
                ("max_line_match_num", C.c_int), ("max_point_match_num", C.c_int),
                ("max_dist_epip", C.c_double), ("min_disp", C.c_double),
                ("max_ratio_12_p", C.c_double), ("point_match_radius", C.c_double),
                ("stereo_overlap_th", C.c_double), ("line_horiz_th", C.c_double),
                ("desc_th_l", C.c_double), ("line_cov_th", C.c_double),
                ("homog_th", C.c_double), ("min_features", C.c_int),
                ("max_iters", C.c_int), ("max_iters_ref", C.c_int),
                ("min_error", C.c_double), ("min_error_change", C.c_double),
                ("inlier_k", C.c_double), ("motion_step_th", C.c_double),
                ("orb_scale_factor", C.c_double), ("orb_n_levels", C.c_int),
                ("lsd_scale", C.c_double), ("cut_step", C.c_double),
                ("cut_rng", C.c_double * 2), ("proj_gate_px", C.c_double),
                ("min_entropy_ratio", C.c_double), ("max_kf_num_frames", C.c_int),
                ("cut_certify", C.c_double), ("cut_proof", C.c_int)]


KEYPOINT_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4")])
# cv::KeyPoint fields ORBextractor::operator() fills (src/ORBextractor.cc:1085-1101)
CV_KEYPOINT_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4")])
KEYLINE_DT = np.dtype([("sx", "<f4"), ("sy", "<f4"), ("ex", "<f4"), ("ey", "<f4"),
                       ("angle", "<f4"), ("octave", "<i4")])

_vp = C.c_void_p


class Frames(C.Structure):
    _fields_ = [("batch", C.c_int), ("kp_cap", C.c_int), ("kl_cap", C.c_int),
                ("n_kp_l", _vp), ("n_kp_r", _vp), ("kp_l", _vp), ("kp_r", _vp),
                ("pdesc_l", _vp), ("pdesc_r", _vp),
                ("n_kl_l", _vp), ("n_kl_r", _vp), ("kl_l", _vp), ("kl_r", _vp),
                ("ldesc_l", _vp), ("ldesc_r", _vp), ("pyr_r", _vp), ("time_stamp", _vp),
                ("ready", _vp), ("consumed", _vp)]


# (name, dtype, per-feature shape) of gfpl_frame_host arrays, in struct order
PT_FIELDS = [("pt_pl", np.float64, (2,)), ("pt_pl_obs", np.float64, (2,)),
             ("pt_disp", np.float64, ()), ("pt_P", np.float64, (3,)),
             ("pt_sigma2", np.float64, ()), ("pt_idx", np.int32, ()),
             ("pt_level", np.int32, ()), ("pt_inlier", np.uint8, ()),
             ("pdesc", np.uint8, (DESC,))]
LS_FIELDS = [("ls_spl", np.float64, (2,)), ("ls_epl", np.float64, (2,)),
             ("ls_spl_obs", np.float64, (2,)), ("ls_epl_obs", np.float64, (2,)),
             ("ls_sdisp", np.float64, ()), ("ls_edisp", np.float64, ()),
             ("ls_sdisp_obs", np.float64, ()), ("ls_edisp_obs", np.float64, ()),
             ("ls_angle", np.float64, ()), ("ls_sigma2", np.float64, ()),
             ("ls_sP", np.float64, (3,)), ("ls_eP", np.float64, (3,)),
             ("ls_le", np.float64, (3,)), ("ls_le_obs", np.float64, (3,)),
             ("ls_covS", np.float64, (9,)), ("ls_covE", np.float64, (9,)),
             ("ls_cut", np.float64, (2,)), ("ls_invcov", np.float64, (36,)),
             ("ls_idx", np.int32, ()), ("ls_level", np.int32, ()),
             ("ls_inlier", np.uint8, ()), ("ldesc", np.uint8, (DESC,))]
POSE_FIELDS = [("Tfw", 16), ("DT", 16), ("DT_cov", 36), ("Tfw_cov", 36), ("DT_cov_eig", 6)]


class FrameHostStruct(C.Structure):
    _fields_ = ([("n_pt", C.c_int), ("n_ls", C.c_int)]
                + [(n, _vp) for n, _, _ in PT_FIELDS]
                + [(n, _vp) for n, _, _ in LS_FIELDS]
                + [(n, C.c_double * k) for n, k in POSE_FIELDS]
                + [("err_norm", C.c_double), ("time_stamp", C.c_double)])


class TrackHost(C.Structure):
    _fields_ = [("n_matched_pt", C.c_int), ("n_matched_ls", C.c_int),
                ("matched_pt", C.c_int32 * MAX_MATCHED_PT),
                ("matched_ls", C.c_int32 * MAX_MATCHED_LS),
                ("n_inliers", C.c_int), ("n_inliers_pt", C.c_int), ("n_inliers_ls", C.c_int),
                ("num_frame_loss", C.c_int)]

    def as_dict(self) -> dict:
        return {"matched_pt": np.array(self.matched_pt[: self.n_matched_pt], dtype=np.int32),
                "matched_ls": np.array(self.matched_ls[: self.n_matched_ls], dtype=np.int32),
                "n_inliers": self.n_inliers, "n_inliers_pt": self.n_inliers_pt,
                "n_inliers_ls": self.n_inliers_ls, "num_frame_loss": self.num_frame_loss}


class KFState(C.Structure):
    """gfpl_kf_state: keyframe-decision state (include/stereoFrameHandler.h:147-153)."""
    _fields_ = [("T_prevKF", C.c_double * 16), ("cov_prevKF_currF", C.c_double * 36),
                ("entropy_first_prevKF", C.c_double), ("entropy_ratio", C.c_double),
                ("prev_f_iskf", C.c_int), ("num_frame_since_kf", C.c_int), ("need_new_kf", C.c_int)]

    def as_dict(self) -> dict:
        return {"T_prevKF": np.array(self.T_prevKF[:]).reshape(4, 4),
                "cov_prevKF_currF": np.array(self.cov_prevKF_currF[:]).reshape(6, 6),
                "entropy_first_prevKF": self.entropy_first_prevKF, "entropy_ratio": self.entropy_ratio,
                "prev_f_iskf": self.prev_f_iskf, "num_frame_since_kf": self.num_frame_since_kf,
                "need_new_kf": self.need_new_kf}


class KFViewStruct(C.Structure):
    """gfpl_kf_view: one keyframe's stereo features (KeyFrame::stereo_frame)."""
    _fields_ = [("n_pt", C.c_int), ("pdesc", _vp), ("P", _vp), ("pl", _vp), ("pt_sigma2", _vp),
                ("n_ls", C.c_int), ("ldesc", _vp), ("sP", _vp), ("eP", _vp), ("le", _vp), ("ls_sigma2", _vp),
                ("T_kf_w", C.c_double * 16)]


KF_PT = [("pdesc", "pdesc"), ("P", "pt_P"), ("pl", "pt_pl"), ("pt_sigma2", "pt_sigma2")]
KF_LS = [("ldesc", "ldesc"), ("sP", "ls_sP"), ("eP", "ls_eP"), ("le", "ls_le"), ("ls_sigma2", "ls_sigma2")]


class KeyFrameView:
    """The arrays of one KeyFrame (src/keyFrame.cpp:26-58) that the keyframe
    consumers read: stereo_pt / stereo_ls rows of a FrameHost and T_kf_w.
    device=None keeps host arrays (oracle); otherwise they are copied to that
    torch device once and stay resident."""

    def __init__(self, fh: "FrameHost", T_kf_w, device=None):
        self.s = KFViewStruct()
        self.s.n_pt, self.s.n_ls = fh.n_pt, fh.n_ls
        self.s.T_kf_w[:] = [float(x) for x in np.asarray(T_kf_w, np.float64).reshape(16)]
        self.keep = {}
        for cf, fn in KF_PT + KF_LS:
            n = fh.n_pt if cf in dict(KF_PT) else fh.n_ls
            a = np.ascontiguousarray(fh.arr[fn][:max(n, 1)])
            if device is not None:
                import torch
                a = torch.from_numpy(a.copy()).to(device)
            self.keep[cf] = a
            setattr(self.s, cf, _ptr(a))


class LoopParams(C.Structure):
    """gfpl_loop_params: Config::lcRes / lcUnc / lcInl / lcTrs / lcRot (src/config.cpp:62-66);
    LoopParams.default() fills the reference's values."""
    _fields_ = [("lc_res", C.c_double), ("lc_unc", C.c_double), ("lc_inl", C.c_double),
                ("lc_trs", C.c_double), ("lc_rot", C.c_double)]

    @classmethod
    def default(cls, **over) -> "LoopParams":
        p = cls()
        hiplib().gfpl_default_loop_params(C.byref(p))
        for k, v in over.items():
            setattr(p, k, v)
        return p


class LoopResult(C.Structure):
    """gfpl_loop_result: MapHandler::isLoopClosure's decision for one candidate pair; gates bit 0 res,
    1 unc, 2 inl, 3 trs, 4 rot; pose_inc is valid when is_lc."""
    _fields_ = [("is_lc", C.c_int32), ("gates", C.c_int32), ("n_pt", C.c_int32), ("n_ls", C.c_int32),
                ("n_pt_inl", C.c_int32), ("n_ls_inl", C.c_int32), ("iters", C.c_int32), ("pad", C.c_int32),
                ("e", C.c_double), ("unc", C.c_double), ("ratio_inliers", C.c_double), ("trs", C.c_double),
                ("rot", C.c_double), ("x_inc", C.c_double * 6), ("pose_inc", C.c_double * 6),
                ("T_inc", C.c_double * 16)]


LBA_MAX_KFS = 16   # GFPL_LBA_MAX_KFS
LBA_STOP_ITERS, LBA_STOP_DERR, LBA_STOP_ERR, LBA_STOP_STEP = 0, 1, 2, 3
LBA_SINGULAR, LBA_HMAX_RANGE = 1, 2


class LbaParams(C.Structure):
    """gfpl_lba_params: Config::lambdaLbaLM / lambdaLbaK / maxItersLba (src/config.cpp:55-57);
    LbaParams.default() fills the reference's values."""
    _fields_ = [("lambda_lm", C.c_double), ("lambda_k", C.c_double), ("max_iters", C.c_int32), ("pad", C.c_int32)]

    @classmethod
    def default(cls, **over) -> "LbaParams":
        p = cls()
        hiplib().gfpl_default_lba_params(C.byref(p))
        for k, v in over.items():
            setattr(p, k, v)
        return p


class LbaCounts(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_fix", C.c_int32), ("n_pt", C.c_int32), ("n_ls", C.c_int32),
                ("n_pt_obs", C.c_int32), ("n_ls_obs", C.c_int32)]


class LbaProblemStruct(C.Structure):
    _fields_ = [("n", LbaCounts)] + [(k, _vp) for k in (
        "x_kf", "T_kf", "T_fix", "pt", "ls", "pt_obs", "pt_sigma", "ls_obs", "ls_sigma", "x_out",
        "pt_obs_lm", "pt_obs_kf", "ls_obs_lm", "ls_obs_kf")]


class LbaResult(C.Structure):
    """gfpl_lba_result: iters is the reference's loop variable at exit; stop LBA_STOP_*; status bits
    LBA_SINGULAR / LBA_HMAX_RANGE; hmax the truncated largest diagonal; lambda, err, err_prev at exit."""
    _fields_ = [("iters", C.c_int32), ("stop", C.c_int32), ("status", C.c_int32), ("hmax", C.c_int32),
                ("lambda_", C.c_double), ("err", C.c_double), ("err_prev", C.c_double)]


LBA_DOUBLES = [("x_kf", 6), ("T_kf", 16), ("T_fix", 16), ("pt", 3), ("ls", 6), ("pt_obs", 2), ("pt_sigma", 1),
               ("ls_obs", 3), ("ls_sigma", 1)]
LBA_INDICES = ["pt_obs_lm", "pt_obs_kf", "ls_obs_lm", "ls_obs_kf"]


class LbaProblem:
    """One local bundle adjustment (gfpl_lba_problem) from numpy arrays: x_kf [n_kf][6] and T_kf
    [n_kf][4][4] (KeyFrame::x_kf_w and T_kf_w of the local keyframes, which the reference reads
    separately), T_fix [n_fix][4][4], pt [n_pt][3], ls [n_ls][6], and per observation its local
    landmark (pt_obs_lm), keyframe slot (pt_obs_kf: >= 0 local keyframe, -1 - f fixed pose f), the
    observation (pt_obs [.][2], ls_obs [.][3]) and sigma.  A landmark's observations are contiguous.
    The arrays are kept as given (float64 / int32 copies); check() runs gfpl_lba_check on them."""

    def __init__(self, x_kf, T_kf, T_fix, pt, ls, pt_obs_lm, pt_obs_kf, pt_obs, pt_sigma, ls_obs_lm, ls_obs_kf,
                 ls_obs, ls_sigma):
        loc = locals()
        self.a = {}
        for k, w in LBA_DOUBLES:
            self.a[k] = np.ascontiguousarray(np.asarray(loc[k], np.float64).reshape(-1, w))
        for k in LBA_INDICES:
            self.a[k] = np.ascontiguousarray(np.asarray(loc[k], np.int32).reshape(-1))
        self.counts = LbaCounts(len(self.a["x_kf"]), len(self.a["T_fix"]), len(self.a["pt"]), len(self.a["ls"]),
                                len(self.a["pt_obs_lm"]), len(self.a["ls_obs_lm"]))

    def struct(self, dev=None) -> LbaProblemStruct:
        """The C record: index arrays on the host; the doubles on the host (dev=None, for check()) or
        the device tensors of `dev` (a dict name -> tensor)."""
        s = LbaProblemStruct()
        s.n = self.counts
        for k in LBA_INDICES:
            setattr(s, k, _ptr(self.a[k]) if len(self.a[k]) else None)
        for k, _ in LBA_DOUBLES:
            src = self.a[k] if dev is None else dev[k]
            setattr(s, k, _ptr(src) if len(self.a[k]) else None)
        if dev is not None:
            s.x_out = _ptr(dev["x_out"])
        return s

    def check(self) -> int:
        return hiplib().gfpl_lba_check(C.byref(self.struct()))

    def workspace(self):
        """(hbm_bytes, lds_bytes) of gfpl_lba_workspace."""
        hbm, lds = C.c_int64(0), C.c_int32(0)
        check(hiplib().gfpl_lba_workspace(C.byref(self.counts), C.byref(hbm), C.byref(lds)), "lba_workspace")
        return hbm.value, lds.value


def lbaWorkspace(n_kf, n_fix, n_pt, n_ls, n_pt_obs, n_ls_obs):
    """gfpl_lba_workspace: (return code, hbm_bytes, lds_bytes) for one problem of these counts."""
    hbm, lds = C.c_int64(0), C.c_int32(0)
    cnt = LbaCounts(n_kf, n_fix, n_pt, n_ls, n_pt_obs, n_ls_obs)
    rc = hiplib().gfpl_lba_workspace(C.byref(cnt), C.byref(hbm), C.byref(lds))
    return rc, hbm.value, lds.value


GBA_MAX_KFS = 256   # GFPL_GBA_MAX_KFS
GBA_STOP_ITERS, GBA_STOP_DERR, GBA_STOP_ERR, GBA_STOP_STEP = 0, 1, 2, 3
GBA_SINGULAR, GBA_HMAX_RANGE, GBA_INDEFINITE = 1, 2, 4


class GbaCounts(C.Structure):
    """gfpl_gba_counts: a problem's counts, its (landmark, keyframe) pairs and the terms of S."""
    _fields_ = [("n", LbaCounts), ("n_pt_pairs", C.c_int32), ("n_ls_pairs", C.c_int32), ("n_terms", C.c_int32),
                ("pad", C.c_int32)]

    @classmethod
    def of(cls, n_kf, n_fix, n_pt, n_ls, n_pt_obs, n_ls_obs, n_pt_pairs, n_ls_pairs, n_terms) -> "GbaCounts":
        return cls(LbaCounts(n_kf, n_fix, n_pt, n_ls, n_pt_obs, n_ls_obs), n_pt_pairs, n_ls_pairs, n_terms, 0)

    def flat(self):
        return [getattr(self.n, f) for f, _ in LbaCounts._fields_] + [self.n_pt_pairs, self.n_ls_pairs, self.n_terms]


GbaParams = LbaParams   # gfpl_gba_params: the GBA reads lambdaLbaLM, lambdaLbaK, maxItersLba too
GbaResult = LbaResult   # gfpl_gba_result; status bits GBA_SINGULAR / GBA_HMAX_RANGE / GBA_INDEFINITE


def gbaCheck(problem: LbaProblem):
    """gfpl_gba_check on an LbaProblem (host only): (return code, GbaCounts the problem takes)."""
    cnt = GbaCounts()
    rc = hiplib().gfpl_gba_check(C.byref(problem.struct()), C.byref(cnt))
    return rc, cnt


def gbaWorkspace(counts):
    """gfpl_gba_workspace: (return code, hbm_bytes, lds_bytes) for one problem of these counts (a
    GbaCounts, or the nine numbers of GbaCounts.of)."""
    cnt = counts if isinstance(counts, GbaCounts) else GbaCounts.of(*[int(v) for v in counts])
    hbm, lds = C.c_int64(0), C.c_int32(0)
    rc = hiplib().gfpl_gba_workspace(C.byref(cnt), C.byref(hbm), C.byref(lds))
    return rc, hbm.value, lds.value


# DBoW2::WeightingType and the keyframe database's modes (include/gfpl.h)
BOW_TF_IDF, BOW_TF, BOW_IDF, BOW_BINARY = 0, 1, 2, 3
BOW_L1_NORM = 0
BOW_MODE_P, BOW_MODE_L, BOW_MODE_PL = 0, 1, 2


class VocabDesc(C.Structure):
    """gfpl_vocab_desc: a DBoW2 vocabulary tree as flat host arrays."""
    _fields_ = [("n_nodes", C.c_int), ("child_off", _vp), ("child", _vp), ("desc", _vp), ("weight", _vp),
                ("word_id", _vp), ("weighting", C.c_int), ("scoring", C.c_int)]


class BowVec(C.Structure):
    """gfpl_bow_vec: a BowVector on the device, count entries in ascending word id."""
    _fields_ = [("ids", _vp), ("values", _vp), ("count", C.c_int)]


class BowStats(C.Structure):
    """gfpl_bow_stats: what insertKFBowVectorPL weighs the two scores with (src/mapHandler.cpp:2940-2972)."""
    _fields_ = [("n_pt", C.c_int32), ("n_ls", C.c_int32), ("std_pt", C.c_double), ("std_ls", C.c_double)]


class LcSearchParams(C.Structure):
    """gfpl_lc_search_params: Config::lcKFDist / lcKFMaxDist / lcNKFClosest / minLMCovGraph / minKFLocalMap;
    LcSearchParams.default() fills the reference's values (100, 20, 4, 30, 3)."""
    _fields_ = [("lc_kf_dist", C.c_int32), ("lc_kf_max_dist", C.c_int32), ("lc_nkf_closest", C.c_int32),
                ("min_lm_cov_graph", C.c_int32), ("min_kf_local_map", C.c_int32)]

    @classmethod
    def default(cls, **over) -> "LcSearchParams":
        p = cls()
        hiplib().gfpl_default_lc_search_params(C.byref(p))
        for k, v in over.items():
            setattr(p, k, v)
        return p


class LcSearchInfo(C.Structure):
    """gfpl_lc_search_info: lookForLoopCandidates' intermediate values (what the reference prints)."""
    _fields_ = [("lc_min_score", C.c_double), ("nkf_closest", C.c_int32), ("idx_max", C.c_int32),
                ("n_list", C.c_int32), ("pad", C.c_int32)]


class MapViewStruct(C.Structure):
    """gfpl_map_view: the local map rows lookForCommonMatches' second stage reads."""
    _fields_ = [("n_pt", C.c_int), ("pdesc", _vp), ("P", _vp), ("n_ls", C.c_int), ("ldesc", _vp), ("L", _vp)]


class MapView:
    """Local map points / lines (med_desc row 0, point3D, line3D) as numpy arrays,
    copied to `device` (torch) when given."""

    def __init__(self, pdesc, P, ldesc, L, device=None):
        self.s = MapViewStruct()
        arrs = {"pdesc": np.ascontiguousarray(pdesc, np.uint8).reshape(-1, 32),
                "P": np.ascontiguousarray(P, np.float64).reshape(-1, 3),
                "ldesc": np.ascontiguousarray(ldesc, np.uint8).reshape(-1, 32),
                "L": np.ascontiguousarray(L, np.float64).reshape(-1, 6)}
        self.s.n_pt, self.s.n_ls = len(arrs["pdesc"]), len(arrs["ldesc"])
        self.keep = {}
        for k, a in arrs.items():
            if device is not None:
                import torch
                a = torch.from_numpy(a.copy()).to(device) if a.size else torch.zeros(1, device=device)
            self.keep[k] = a
            setattr(self.s, k, _ptr(a) if (device is not None or a.size) else 0)


class FuseParams(C.Structure):
    """gfpl_fuse_params: Config::maxPointPointError / maxPointLineError / maxDirLineError
    (src/config.cpp:46-48); FuseParams.default() fills the reference's values."""
    _fields_ = [("max_point_point_error", C.c_double), ("max_point_line_error", C.c_double),
                ("max_dir_line_error", C.c_double)]

    @classmethod
    def default(cls, **over) -> "FuseParams":
        p = cls()
        hiplib().gfpl_default_fuse_params(C.byref(p))
        for k, v in over.items():
            setattr(p, k, v)
        return p


class FuseMapStruct(C.Structure):
    """gfpl_fuse_map"""
    _fields_ = [("map", MapViewStruct), ("pt_kf", _vp), ("ls_kf", _vp), ("n_kf", C.c_int), ("T_kf", _vp)]


class FuseMap:
    """gfpl_fuse_map: the local landmarks fuseLandmarksFromLocalMap searches (med_desc row 0, point3D /
    line3D, kf_obs_list[0]) and the keyframes' T_kf_w [n_kf][16], copied to `device` (torch)."""

    def __init__(self, pdesc, P, pt_kf, ldesc, L, ls_kf, T_kf, device="cuda"):
        import torch
        self.view = MapView(pdesc, P, ldesc, L, device=device)
        self.s = FuseMapStruct()
        self.s.map = self.view.s
        T = np.ascontiguousarray(T_kf, np.float64).reshape(-1, 16)
        self.s.n_kf = len(T)
        self.keep = {}
        for k, a in (("pt_kf", np.ascontiguousarray(pt_kf, np.int32).reshape(-1)),
                     ("ls_kf", np.ascontiguousarray(ls_kf, np.int32).reshape(-1)), ("T_kf", T)):
            a = torch.from_numpy(a.copy()).to(device) if a.size else torch.zeros(1, device=device)
            self.keep[k] = a
            setattr(self.s, k, _ptr(a))
        if len(self.keep["pt_kf"]) < self.s.map.n_pt or len(self.keep["ls_kf"]) < self.s.map.n_ls:
            raise ValueError("FuseMap: one keyframe index per landmark")


class OrbParams(C.Structure):
    """gfpl_orb_params: ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)."""
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int)]


class LsdParams(C.Structure):
    """gfpl_lsd_params: LSDDetectorC::LSDOptions + Config::lsdNFeatures as StereoFrame builds
    them (src/stereoFrame.cpp:1163-1172; defaults src/config.cpp:143-152, min_length =
    Config::minLineLength 0.025 * min(W, H), src/stereoFrame.cpp:151)."""
    _fields_ = [("refine", C.c_int), ("scale", C.c_double), ("quant", C.c_double), ("ang_th", C.c_double),
                ("density_th", C.c_double), ("n_bins", C.c_int), ("min_length", C.c_double),
                ("n_features", C.c_int)]

    @classmethod
    def reference(cls, width: int, height: int, n_features: int = 300, min_line_length: float = 0.025):
        return cls(1, 1.0, 2.0, 22.5, 0.6, 1024, min_line_length * min(width, height), n_features)


class DetectorParams(C.Structure):
    """gfpl_detector_params: the ORB + LSD options StereoFrame's detection runs with
    (src/stereoFrame.cpp:33-36, 1160-1172) and the raw LSD segment capacity."""
    _fields_ = [("orb", OrbParams), ("lsd", LsdParams), ("seg_cap", C.c_int)]

    @classmethod
    def reference(cls, cam: "Camera", cfg: Optional["Config"] = None, nfeatures: Optional[int] = None):
        p = cls()
        check(hiplib().gfpl_detector_params_default(C.byref(cam), C.byref(cfg) if cfg is not None else None,
                                                    C.byref(p)), "detector_params_default")
        if nfeatures is not None:
            p.orb.nfeatures = nfeatures
        return p


class DetectionsHost(C.Structure):
    _fields_ = [("n_kp_l", C.c_int), ("n_kp_r", C.c_int), ("n_kl_l", C.c_int), ("n_kl_r", C.c_int),
                ("kp_l", _vp), ("kp_r", _vp), ("pdesc_l", _vp), ("pdesc_r", _vp),
                ("kl_l", _vp), ("kl_r", _vp), ("ldesc_l", _vp), ("ldesc_r", _vp)]


class RectifySide(C.Structure):
    """gfpl_rectify_side: one camera of the rig as PinholeStereoCamera's distortion constructors take
    it (src/pinholeStereoCamera.cpp:49-94): raw K (fx fy cx cy), distortion D, rectifying R (row-major
    3x3) and the rectified P (fx fy cx cy); model 0 = pinhole radial-tangential, 1 = equidistant."""
    _fields_ = [("model", C.c_int), ("K", C.c_double * 4), ("D", C.c_double * 8), ("n_dist", C.c_int),
                ("R", C.c_double * 9), ("P", C.c_double * 4)]

    @classmethod
    def make(cls, K, D, R, P, equi: bool = False) -> "RectifySide":
        s = cls()
        D = [float(v) for v in np.asarray(D, np.float64).reshape(-1)]
        if len(D) > 8:
            raise GfplError(-7, f"{len(D)} distortion coefficients")
        s.model = 1 if equi else 0
        s.K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(-1)]
        s.D[:len(D)] = D
        s.n_dist = len(D)
        s.R[:] = [float(v) for v in np.asarray(R, np.float64).reshape(-1)]
        s.P[:] = [float(v) for v in np.asarray(P, np.float64).reshape(-1)]
        return s


class SynthParams(C.Structure):
    _fields_ = [("n_kp", C.c_int), ("n_kl", C.c_int), ("n_world_pts", C.c_int),
                ("n_world_lines", C.c_int), ("dt", C.c_double), ("v_fwd", C.c_double),
                ("yaw_rate", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double),
                ("px_noise", C.c_double), ("distractor_frac", C.c_double),
                ("margin", C.c_int), ("seed", C.c_uint64),
                ("traj", _vp), ("n_traj", C.c_int), ("traj_t", _vp), ("respawn", C.c_int),
                ("outlier_frac", C.c_double), ("pyr_from_l0", C.c_int)]


# ------------------------------------------------------------- libraries --
_LIBS: dict = {}


def lib_path(name: str) -> str:
    # GFPL_LIB_DIR: load an alternative in-tree build (kernel experiments in tools/)
    return os.path.join(os.environ.get("GFPL_LIB_DIR", LIB_DIR), name)


def _load(name: str) -> C.CDLL:
    if name not in _LIBS:
        p = lib_path(name)
        if not os.path.exists(p):
            raise GfplError(-3, f"{p} is not built (run __graft_entry__.build())")
        _LIBS[name] = C.CDLL(p)
    return _LIBS[name]


def hiplib() -> C.CDLL:
    """The product library (HIP kernels + C ABI).  Raises if not built.

    torch (when importable) is imported first so the process has ONE HIP
    runtime: torch's libamdhip64 is then what libgfpl_hip.so's NEEDED
    libamdhip64.so.7 resolves to (a second copy loaded under another file name
    would see no devices)."""
    if "libgfpl_hip.so" not in _LIBS:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = _load("libgfpl_hip.so")
    if not getattr(L, "_gfpl_typed", False):
        P = C.c_void_p
        sigs = {
            "gfpl_abi_version": ([], C.c_int),
            "gfpl_config_default": ([P], C.c_int),
            "gfpl_camera_init": ([P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                  C.c_double, C.c_double, P], C.c_int),
            "gfpl_create": ([C.c_int, P, C.POINTER(P)], C.c_int),
            "gfpl_create_async": ([C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_get_stream": ([P], C.c_void_p),
            "gfpl_event_create": ([P, C.POINTER(P)], C.c_int),
            "gfpl_event_destroy": ([P], C.c_int),
            "gfpl_event_record": ([P, P], C.c_int),
            "gfpl_event_wait": ([P, P], C.c_int),
            "gfpl_event_synchronize": ([P], C.c_int),
            "gfpl_event_record_count": ([P, P], C.c_int),
            "gfpl_orb_extract_async": ([P, P, C.c_int, P, P, P, P, P, P, C.c_int64], C.c_int),
            "gfpl_orb_status": ([P], C.c_int),
            "gfpl_lsd_detect_async": ([P, P, C.c_int, P, P, P], C.c_int),
            "gfpl_lsd_status": ([P], C.c_int),
            "gfpl_lbd_compute_async": ([P, P, C.c_int, P, P, P], C.c_int),
            "gfpl_lbd_status": ([P], C.c_int),
            "gfpl_destroy": ([P], C.c_int),
            "gfpl_set_camera": ([P, P], C.c_int),
            "gfpl_set_config": ([P, P], C.c_int),
            "gfpl_get_camera": ([P, P], C.c_int),
            "gfpl_get_config": ([P, P], C.c_int),
            "gfpl_synchronize": ([P], C.c_int),
            "gfpl_copy_to_host": ([P, P, P, C.c_size_t], C.c_int),
            "gfpl_seqbatch_create": ([P, C.c_int, C.c_int, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_seqbatch_destroy": ([P], C.c_int),
            "gfpl_seqbatch_bytes": ([P], C.c_int64),
            "gfpl_initialize": ([P, P], C.c_int),
            "gfpl_insert_stereo_pair": ([P, P], C.c_int),
            "gfpl_optimize_pose": ([P], C.c_int),
            "gfpl_optimize_pose_ini": ([P, P], C.c_int),
            "gfpl_update_frame": ([P], C.c_int),
            "gfpl_frame_step": ([P, P], C.c_int),
            "gfpl_upload_frames": ([P, P, P], C.c_int),
            "gfpl_upload_frames_async": ([P, P, C.c_int, C.c_int, P], C.c_int),
            "gfpl_upload_wait": ([P, C.c_int64], C.c_int),
            "gfpl_upload_frames_l0_async": ([P, P, C.c_int, C.c_int, C.c_int64, P], C.c_int),
            "gfpl_staged_frames": ([P, C.c_int, P], C.c_int),
            "gfpl_stereo_points": ([P, P], C.c_int),
            "gfpl_stereo_lines": ([P, P], C.c_int),
            "gfpl_line_uncertainty": ([P], C.c_int),
            "gfpl_cross_points": ([P], C.c_int),
            "gfpl_cross_lines": ([P], C.c_int),
            "gfpl_line_cut": ([P], C.c_int),
            "gfpl_knn2_hamming": ([P, P, C.c_int, P, C.c_int, C.c_int, P, P], C.c_int),
            "gfpl_kf_common_matches": ([P, P, P, P, P, P, P], C.c_int),
            "gfpl_kf_local_map_matches": ([P, P, P, C.c_double, C.c_double, P, P, P, P], C.c_int),
            "gfpl_default_loop_params": ([P], None),
            "gfpl_default_fuse_params": ([P], None),
            "gfpl_map_fuse_search": ([P, P, P, P, P, P, P, P, P, P, P], C.c_int),
            "gfpl_map_fuse_debug_ms": ([P, C.c_int, P], C.c_int),
            "gfpl_kf_loop_closure": ([P, P, P, C.c_int, P, C.c_int, C.c_int, P, P, P, P, P], C.c_int),
            "gfpl_vocab_create": ([P, P, P], C.c_int),
            "gfpl_vocab_destroy": ([P], C.c_int),
            "gfpl_vocab_check": ([P], C.c_int),
            "gfpl_bow_transform": ([P, P, C.c_int, P, P, C.c_int, P, P, P], C.c_int),
            "gfpl_bow_score": ([P, P, P, C.c_int, P], C.c_int),
            "gfpl_kf_bow_stats": ([P, C.c_int, P, P, C.c_int, P], C.c_int),
            "gfpl_bowdb_create": ([P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P], C.c_int),
            "gfpl_bowdb_destroy": ([P], C.c_int),
            "gfpl_bowdb_insert": ([P, C.c_int, P, P, P], C.c_int),
            "gfpl_bowdb_erase": ([P, C.c_int], C.c_int),
            "gfpl_bowdb_vector": ([P, C.c_int, C.c_int, P, P, P], C.c_int),
            "gfpl_default_lc_search_params": ([P], None),
            "gfpl_kf_loop_candidates": ([P, P, P, C.c_int, P, P, P], C.c_int),
            "gfpl_read_frame": ([P, C.c_int, C.c_int, P], C.c_int),
            "gfpl_write_frame": ([P, C.c_int, C.c_int, P], C.c_int),
            "gfpl_read_track": ([P, C.c_int, P], C.c_int),
            "gfpl_read_last_track": ([P, C.c_int, P], C.c_int),
            "gfpl_need_new_kf": ([P, P], C.c_int),
            "gfpl_curr_frame_is_kf": ([P, P], C.c_int),
            "gfpl_read_kf_state": ([P, C.c_int, P], C.c_int),
            "gfpl_write_track": ([P, C.c_int, P], C.c_int),
            "gfpl_set_timing": ([P, C.c_int], C.c_int),
            "gfpl_get_stage_times": ([P, P], C.c_int),
            "gfpl_get_kernel_times": ([P, P], C.c_int),
            "gfpl_last_step_kernel_bytes": ([P, P], C.c_int),
            "gfpl_last_step_bytes": ([P, P], C.c_int),
            "gfpl_last_step_stage_bytes": ([P, P], C.c_int),
            "gfpl_last_step_counts": ([P, P], C.c_int),
            "gfpl_last_step_track_counts": ([P, P], C.c_int),
            "gfpl_last_step_cut_proof": ([P, P], C.c_int),
            "gfpl_debug_cut_records": ([P, C.c_int, P, C.c_int], C.c_int),
            "gfpl_debug_step_records": ([P, P], C.c_int),
            "gfpl_debug_clocks": ([P, P], C.c_int),
            "gfpl_lsd_create": ([P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_lsd_destroy": ([P], C.c_int),
            "gfpl_lsd_detect": ([P, P, C.c_int, P, P, P], C.c_int),
            "gfpl_lsd_sort_desc": ([P, P, C.c_int], C.c_int),
            "gfpl_strerror": ([C.c_int], C.c_char_p),
            "gfpl_orb_create": ([P, C.c_int, C.c_int, P, C.c_int, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_orb_destroy": ([P], C.c_int),
            "gfpl_orb_pyramid_bytes": ([P, P], C.c_int),
            "gfpl_orb_extract": ([P, P, C.c_int, P, P, P, P, P, P, C.c_int64], C.c_int),
            "gfpl_lbd_create": ([P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_lbd_destroy": ([P], C.c_int),
            "gfpl_lbd_compute": ([P, P, C.c_int, P, P, P], C.c_int),
            "gfpl_lbd_gradients": ([P, P, P], C.c_int),
            "gfpl_detector_params_default": ([P, P, P], C.c_int),
            "gfpl_detector_create": ([P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_detector_destroy": ([P], C.c_int),
            "gfpl_detect_stereo_async": ([P, P, P, C.c_int, P, P], C.c_int),
            "gfpl_detect_stereo_host": ([P, P, P, C.c_int, P, P], C.c_int),
            "gfpl_detect_stereo": ([P, P, P, C.c_int, P, C.c_int, P], C.c_int),
            "gfpl_detector_status": ([P], C.c_int),
            "gfpl_detector_discard": ([P, P], C.c_int),
            "gfpl_read_detections": ([P, P, C.c_int, P], C.c_int),
            "gfpl_rectify_maps_host": ([P, C.c_int, C.c_int, P, P], C.c_int),
            "gfpl_rectifier_create": ([P, P, P, C.c_int, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_rectifier_destroy": ([P], C.c_int),
            "gfpl_rectifier_read_maps": ([P, C.c_int, P, P], C.c_int),
            "gfpl_rectify": ([P, C.c_int, P, C.c_int, P], C.c_int),
            "gfpl_rectify_async": ([P, C.c_int, P, C.c_int, P], C.c_int),
            "gfpl_rectify_stereo_async": ([P, P, P, C.c_int, P, P], C.c_int),
            "gfpl_rectify_host": ([P, C.c_int, P, C.c_int, P], C.c_int),
            "gfpl_detector_set_rectifier": ([P, P], C.c_int),
            "gfpl_default_lba_params": ([P], None),
            "gfpl_lba_check": ([P], C.c_int),
            "gfpl_lba_workspace": ([P, P, P], C.c_int),
            "gfpl_lba_create": ([P, P, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_lba_destroy": ([P], C.c_int),
            "gfpl_lba_solve": ([P, P, C.c_int, P, P], C.c_int),
            "gfpl_lba_debug_system": ([P, C.c_int, C.c_int, P, P, P, P, P, P, P], C.c_int),
            "gfpl_lmstore_create": ([P, C.c_int, C.c_int, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_lmstore_destroy": ([P], C.c_int),
            "gfpl_lmstore_bytes": ([P], C.c_int64),
            "gfpl_lm_ops_check": ([P, C.c_int, P, C.c_int, C.c_int, P, C.c_int], C.c_int),
            "gfpl_lmstore_apply": ([P, P, C.c_int, P, P, C.c_int], C.c_int),
            "gfpl_lm_fuse_check": ([P, C.c_int, P, C.c_int, C.c_int, P, C.c_int, P], C.c_int),
            "gfpl_lmstore_fuse": ([P, P, C.c_int, P, P, C.c_int], C.c_int),
            "gfpl_lmstore_gather": ([P, P, C.c_int, P, P], C.c_int),
            "gfpl_lmstore_read": ([P, C.c_int, P, P, P, P], C.c_int),
            "gfpl_lmstore_debug_ms": ([P, P], C.c_int),
            "gfpl_lmstore_observe_pairs": ([P, P, C.c_int, P, C.c_int, P, P, C.c_int, C.c_int], C.c_int),
            "gfpl_lmstore_observe_local": ([P, P, C.c_int, P, C.c_int, P, C.c_int, P], C.c_int),
            "gfpl_lmstore_free_ids": ([P, P, C.c_int], C.c_int),
            "gfpl_lmstore_gather_ids": ([P, P, C.c_int, P, P], C.c_int),
            "gfpl_lmstore_counts": ([P, P], C.c_int),
            "gfpl_default_kfmap_params": ([P], None),
            "gfpl_kfmap_bytes": ([P], C.c_int64),
            "gfpl_kfmap_create": ([P, P, C.POINTER(P)], C.c_int),
            "gfpl_kfmap_destroy": ([P], C.c_int),
            "gfpl_kfmap_counts": ([P, P, P, P], C.c_int),
            "gfpl_kfmap_add_keyframe": ([P, C.c_int, C.c_int, P], C.c_int),
            "gfpl_kfmap_observe_pairs": ([P, C.c_int, C.c_int, C.c_int, P, C.c_int, P, P, P], C.c_int),
            "gfpl_kfmap_observe_local": ([P, C.c_int, C.c_int, P, C.c_int, P, C.c_int, P, C.c_int, P], C.c_int),
            "gfpl_kfmap_form_local_map": ([P, P], C.c_int),
            "gfpl_kfmap_select": ([P, C.c_int, C.c_int, C.c_int, P, P], C.c_int),
            "gfpl_kfmap_unmatched": ([P, C.c_int, C.c_int, P, P], C.c_int),
            "gfpl_kfmap_local_keyframes": ([P, P, P], C.c_int),
            "gfpl_kfmap_remove_bad": ([P, P, P, P, P, P], C.c_int),
            "gfpl_kfmap_set_inlier": ([P, C.c_int, P, C.c_int, C.c_int], C.c_int),
            "gfpl_kfmap_erase_keyframe": ([P, C.c_int], C.c_int),
            "gfpl_kfmap_read_keyframe": ([P, C.c_int, P, P, P], C.c_int),
            "gfpl_kfmap_write_keyframe_idx": ([P, C.c_int, C.c_int, C.c_int, C.c_int, P], C.c_int),
            "gfpl_kfmap_read_landmarks": ([P, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P], C.c_int),
            "gfpl_kfmap_write_landmarks": ([P, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P], C.c_int),
            "gfpl_kfmap_export_graph": ([P, P, P, P, P, P, P, P, P], C.c_int),
            "gfpl_kfmap_debug_ms": ([P, P], C.c_int),
            "gfpl_mapgeo_bytes": ([P], C.c_int64),
            "gfpl_mapgeo_create": ([P, P, C.POINTER(P)], C.c_int),
            "gfpl_mapgeo_destroy": ([P], C.c_int),
            "gfpl_mapgeo_set_keyframe": ([P, C.c_int, P, P], C.c_int),
            "gfpl_mapgeo_read_keyframe": ([P, C.c_int, P, P], C.c_int),
            "gfpl_mapgeo_arrays": ([P, P, P, P, P], C.c_int),
            "gfpl_mapgeo_observe_pairs": ([P, C.c_int, C.c_int, C.c_int, P, P, P, P, C.c_int, C.c_int], C.c_int),
            "gfpl_mapgeo_observe_local": ([P, C.c_int, C.c_int, P, P, C.c_int, P, C.c_int, P], C.c_int),
            "gfpl_mapgeo_free": ([P, C.c_int, P, C.c_int], C.c_int),
            "gfpl_mapgeo_read_landmarks": ([P, C.c_int, C.c_int, C.c_int, P, P, P, P], C.c_int),
            "gfpl_mapgeo_write_landmarks": ([P, C.c_int, C.c_int, C.c_int, P, P, P, P], C.c_int),
            "gfpl_mapgeo_assemble": ([P, P, C.c_int, P, P], C.c_int),
            "gfpl_mapgeo_assembled_ids": ([P, P, P, P, P], C.c_int),
            "gfpl_mapgeo_read_assembled": ([P, P, P, P, P, P], C.c_int),
            "gfpl_mapgeo_lba": ([P, P, P, P, P, P], C.c_int),
            "gfpl_mapgeo_debug_ms": ([P, P], C.c_int),
            "gfpl_default_gba_params": ([P], None),
            "gfpl_gba_check": ([P, P], C.c_int),
            "gfpl_gba_workspace": ([P, P, P], C.c_int),
            "gfpl_gba_create": ([P, P, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_gba_destroy": ([P], C.c_int),
            "gfpl_gba_solve": ([P, P, C.c_int, P, P], C.c_int),
            "gfpl_gba_debug_system": ([P, C.c_int, C.c_int, P, P, P, P, P, P, P, P], C.c_int),
            "gfpl_default_pgo_params": ([P], None),
            "gfpl_pgo_check": ([P, P, P], C.c_int),
            "gfpl_pgo_workspace": ([P, P, P], C.c_int),
            "gfpl_pgo_create": ([P, P, C.c_int, C.POINTER(P)], C.c_int),
            "gfpl_pgo_destroy": ([P], C.c_int),
            "gfpl_pgo_solve": ([P, P, C.c_int, P, P], C.c_int),
            "gfpl_pgo_debug_system": ([P, C.c_int, P, P, P, P, P, P, P, P, P], C.c_int),
            "gfpl_pgo_debug_ms": ([P, P, P], C.c_int),
        }
        for n, (a, r) in sigs.items():
            try:
                f = getattr(L, n)
            except AttributeError:   # partial builds: the missing entry point fails when called
                continue
            f.argtypes = a
            f.restype = r
        L._gfpl_typed = True
    return L


def synthlib() -> C.CDLL:
    L = _load("libgfpl_synth.so")
    if not getattr(L, "_gfpl_typed", False):
        P = C.c_void_p
        L.gfpl_synth_default.argtypes = [P]
        L.gfpl_synth_default.restype = None
        L.gfpl_synth_batch.argtypes = ([P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
                                       + [P] * 14 + [C.c_int])
        L.gfpl_synth_batch.restype = C.c_int
        L.gfpl_synth_image.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, P]
        L.gfpl_synth_image.restype = C.c_int
        L.gfpl_synth_frame_ex.argtypes = [P, P, C.c_int, C.c_int, C.c_int, C.c_int] + [P] * 16
        L.gfpl_synth_frame_ex.restype = C.c_int
        L._gfpl_typed = True
    return L


def check(code: int, what: str = "") -> None:
    if code != 0:
        raise GfplError(code, what)


# ------------------------------------------------------------ parameters --
def default_config(**over) -> Config:
    cfg = Config()
    check(hiplib().gfpl_config_default(C.byref(cfg)), "config_default")
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


# Cameras of the BASELINE configs (intrinsics from the reference's YAMLs).
CAMERAS = {
    # config/gazebo_params.yaml:2,8-11 — the reference's synthetic VGA rig (cfg 2)
    "vga": dict(width=640, height=480, fx=554.25626, fy=554.25626, cx=320.0, cy=240.0, b=0.1),
    # config/euroc_params.yaml:2,8-11 (raw left K; cfg 1 and 4)
    "euroc": dict(width=752, height=480, fx=458.654, fy=457.296, cx=367.215, cy=248.375, b=0.110077842),
    # config/kitti/kitti00-02.yaml:2-13 (cfg 3)
    "kitti": dict(width=1241, height=376, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, b=0.537165719),
    # gazebo x3 (cfg 5 stress)
    "stress": dict(width=1920, height=1080, fx=1662.76878, fy=1662.76878, cx=960.0, cy=540.0, b=0.1),
}


EUROC_SEQS = ["mh_01", "mh_02", "mh_03", "mh_04", "mh_05", "v1_01", "v1_02", "v1_03"]


EUROC_MAX_POSES = 512


def euroc_traj(seq: str = "mh_01", n: int = 64):
    """First n ground-truth camera poses (3x4 row-major T_w<-c) and timestamps [s] of a
    EuRoC sequence, from the reference's config/asl/gt-ass/<seq> files (data/euroc_gt.npz,
    the first 512 poses of each; tests/golden/make_euroc_fixture.py).  n beyond the stored
    poses raises: the generator never wraps a trajectory around."""
    if n > EUROC_MAX_POSES:
        raise ValueError(f"euroc_traj: {n} poses requested, {EUROC_MAX_POSES} stored for {seq}")
    with np.load(os.path.join(os.path.dirname(LIB_DIR), "data", "euroc_gt.npz")) as d:
        T = np.ascontiguousarray(d[seq + "_T"][:n])
        t = np.ascontiguousarray(d[seq + "_t"][:n])
    return T, t


def make_camera(name: str = "vga", cfg: Optional[Config] = None, **over) -> Camera:
    p = dict(CAMERAS[name])
    p.update(over)
    cfg = cfg or default_config()
    cam = Camera()
    check(hiplib().gfpl_camera_init(C.byref(cam), p["width"], p["height"], p["fx"], p["fy"],
                                    p["cx"], p["cy"], p["b"], C.byref(cfg)), "camera_init")
    return cam


def synth_image(seq: int, frame: int, width: int, height: int, seed: int = 0x6A09E667) -> np.ndarray:
    """A synthetic grey image [height][width] u8 (gfpl_synth_image: shapes on a gradient +
    noise), deterministic in (seed, seq, frame)."""
    out = np.zeros((height, width), np.uint8)
    check(synthlib().gfpl_synth_image(seed, seq, frame, width, height, out.ctypes.data), "synth_image")
    return out


def synth_keylines(n: int, w: int, h: int, seed: int, min_len: float = 2.0, max_len: float = 200.0,
                   border: bool = False) -> np.ndarray:
    """n synthetic octave-0 keylines (KEYLINE_DT) inside a w x h image: fractional endpoints,
    the LSD wrapper's angle = atan2(ey - sy, ex - sx) in float (src/LSDDetector_custom.cpp:285);
    border=True clamps the far endpoint onto the image edge."""
    rng = np.random.default_rng(seed)
    kl = np.zeros(n, KEYLINE_DT)
    for i in range(n):
        while True:
            sx, sy = rng.uniform(0, w - 1), rng.uniform(0, h - 1)
            a = rng.uniform(-np.pi, np.pi)
            ln = rng.uniform(min_len, max_len)
            ex, ey = sx + ln * np.cos(a), sy + ln * np.sin(a)
            if border:
                ex, ey = min(max(ex, 0.0), w - 1.0), min(max(ey, 0.0), h - 1.0)
            if 0 <= ex <= w - 1 and 0 <= ey <= h - 1:
                break
        fs, fe = np.float32(sx), np.float32(sy)
        gx, gy = np.float32(ex), np.float32(ey)
        kl[i] = (fs, fe, gx, gy, np.arctan2(gy - fe, gx - fs).astype(np.float32), 0)
    return kl


def synth_true_counts(cam: Camera, sp: SynthParams, seq: int, frame: int, kp_cap: int = 0, kl_cap: int = 0):
    """(true keypoints, true keylines) per side in frame `frame` of sequence `seq`: the
    detections that observe a landmark / 3-D segment (the rest are distractors)."""
    kp_cap, kl_cap = kp_cap or sp.n_kp, kl_cap or sp.n_kl
    n = np.zeros(6, np.int32)
    kp = np.zeros((2, kp_cap), KEYPOINT_DT)
    kl = np.zeros((2, kl_cap), KEYLINE_DT)
    pd = np.zeros((2, kp_cap, DESC), np.uint8)
    ld = np.zeros((2, kl_cap, DESC), np.uint8)
    pyr = np.zeros(cam.pyr_bytes, np.uint8)
    ts = np.zeros(1, np.float64)
    nt = np.zeros(2, np.int32)
    a = n.ctypes.data
    check(synthlib().gfpl_synth_frame_ex(C.byref(sp), C.byref(cam), seq, frame, kp_cap, kl_cap, a, a + 4,
                                         kp[0].ctypes.data, kp[1].ctypes.data, pd[0].ctypes.data, pd[1].ctypes.data,
                                         a + 8, a + 12, kl[0].ctypes.data, kl[1].ctypes.data, ld[0].ctypes.data,
                                         ld[1].ctypes.data, pyr.ctypes.data, ts.ctypes.data, None, nt.ctypes.data),
          "synth_frame_ex")
    return int(nt[0]), int(nt[1])


def synth_params(**over) -> SynthParams:
    sp = SynthParams()
    synthlib().gfpl_synth_default(C.byref(sp))
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


def _ptr(a) -> int:
    if a is None:
        return 0
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a.data_ptr())   # torch tensor


# ----------------------------------------------------- synthetic batches --
class HostFrames:
    """Synthetic input frames on the host: arrays [F][B][cap] (numpy)."""

    def __init__(self, cam: Camera, sp: SynthParams, n_seq: int, n_frames: int,
                 kp_cap: int, kl_cap: int, seq0: int = 0, frame0: int = 0, threads: int = 0):
        self.cam, self.sp = cam, sp
        self.B, self.F, self.kp_cap, self.kl_cap = n_seq, n_frames, kp_cap, kl_cap
        F, B = n_frames, n_seq
        self.n_kp_l = np.zeros((F, B), np.int32)
        self.n_kp_r = np.zeros((F, B), np.int32)
        self.kp_l = np.zeros((F, B, kp_cap), KEYPOINT_DT)
        self.kp_r = np.zeros((F, B, kp_cap), KEYPOINT_DT)
        self.pdesc_l = np.zeros((F, B, kp_cap, DESC), np.uint8)
        self.pdesc_r = np.zeros((F, B, kp_cap, DESC), np.uint8)
        self.n_kl_l = np.zeros((F, B), np.int32)
        self.n_kl_r = np.zeros((F, B), np.int32)
        self.kl_l = np.zeros((F, B, kl_cap), KEYLINE_DT)
        self.kl_r = np.zeros((F, B, kl_cap), KEYLINE_DT)
        self.ldesc_l = np.zeros((F, B, kl_cap, DESC), np.uint8)
        self.ldesc_r = np.zeros((F, B, kl_cap, DESC), np.uint8)
        self.pyr_r = np.zeros((F, B, cam.pyr_bytes), np.uint8)
        self.time_stamp = np.zeros((F, B), np.float64)
        threads = threads or min(16, os.cpu_count() or 1)
        check(synthlib().gfpl_synth_batch(
            C.byref(sp), C.byref(cam), seq0, B, frame0, F, kp_cap, kl_cap,
            *[_ptr(a) for a in self.arrays()], threads), "synth_batch")

    def arrays(self):
        return [self.n_kp_l, self.n_kp_r, self.kp_l, self.kp_r, self.pdesc_l, self.pdesc_r,
                self.n_kl_l, self.n_kl_r, self.kl_l, self.kl_r, self.ldesc_l, self.ldesc_r,
                self.pyr_r, self.time_stamp]

    def frames(self, f: int) -> Frames:
        """gfpl_frames with HOST pointers for frame f (what the oracle reads)."""
        a = [x[f] for x in self.arrays()]
        return make_frames(self.B, self.kp_cap, self.kl_cap, a)


class HostBatch:
    """One input frame of B sequences in host memory, refilled in place frame by frame
    (the bench's input ring: generate on the host, upload with gfpl_upload_frames).
    pinned=True page-locks the buffers (torch pinned memory) so the upload runs at the
    PCIe DMA rate."""

    def __init__(self, cam: Camera, sp: SynthParams, n_seq: int, kp_cap: int, kl_cap: int,
                 seq0: int = 0, pinned: bool = False):
        self.cam, self.sp, self.B, self.kp_cap, self.kl_cap, self.seq0 = cam, sp, n_seq, kp_cap, kl_cap, seq0
        B = n_seq
        spec = [((B,), np.int32), ((B,), np.int32), ((B, kp_cap), KEYPOINT_DT), ((B, kp_cap), KEYPOINT_DT),
                ((B, kp_cap, DESC), np.uint8), ((B, kp_cap, DESC), np.uint8),
                ((B,), np.int32), ((B,), np.int32), ((B, kl_cap), KEYLINE_DT), ((B, kl_cap), KEYLINE_DT),
                ((B, kl_cap, DESC), np.uint8), ((B, kl_cap, DESC), np.uint8),
                ((B, cam.pyr_bytes), np.uint8), ((B,), np.float64)]
        self._keep, self._arrs = [], []
        for shape, dt in spec:
            dt = np.dtype(dt)
            n = int(np.prod(shape)) * dt.itemsize
            if pinned:
                import torch
                t = torch.empty(n, dtype=torch.uint8, pin_memory=True)
                self._keep.append(t)
                a = t.numpy().view(dt).reshape(shape)
            else:
                a = np.zeros(shape, dt)
            self._arrs.append(a)
        self.frame_idx = -1

    def arrays(self):
        return self._arrs

    def fill(self, frame_idx: int, threads: int = 0, seq0: Optional[int] = None, n: Optional[int] = None):
        """Generate frame `frame_idx` of sequences [seq0, seq0 + n) (gfpl_synth_batch) into
        the first n rows (default: the batch's own seq0 and all B rows)."""
        threads = threads or min(16, os.cpu_count() or 1)
        seq0 = self.seq0 if seq0 is None else seq0
        n = self.B if n is None else n
        if not 0 < n <= self.B:
            raise ValueError(f"fill: {n} sequences into a batch of {self.B}")
        check(synthlib().gfpl_synth_batch(
            C.byref(self.sp), C.byref(self.cam), seq0, n, frame_idx, 1, self.kp_cap, self.kl_cap,
            *[_ptr(a) for a in self._arrs], threads), "synth_batch")
        self.frame_idx, self.n = frame_idx, n

    def frames(self, n: Optional[int] = None) -> Frames:
        """gfpl_frames (HOST pointers) of the first n rows (default all B)."""
        n = self.B if n is None else n
        return make_frames(n, self.kp_cap, self.kl_cap, [a[:n] for a in self._arrs])

    def nbytes(self) -> int:
        return sum(a.nbytes for a in self._arrs)


def make_frames(B: int, kp_cap: int, kl_cap: int, arrs) -> Frames:
    fr = Frames()
    fr.batch, fr.kp_cap, fr.kl_cap = B, kp_cap, kl_cap
    names = ["n_kp_l", "n_kp_r", "kp_l", "kp_r", "pdesc_l", "pdesc_r", "n_kl_l", "n_kl_r",
             "kl_l", "kl_r", "ldesc_l", "ldesc_r", "pyr_r", "time_stamp"]
    for n, a in zip(names, arrs):
        setattr(fr, n, _ptr(a))
    fr._keep = list(arrs)   # keep buffers alive
    return fr


def input_bytes_per_frame(cam: Camera, kp_cap: int, kl_cap: int) -> int:
    """Bytes of one sequence's input frame in the [B][cap] layout."""
    return (2 * 4 + 2 * kp_cap * (KEYPOINT_DT.itemsize + DESC) + 2 * 4 + 2 * kl_cap * (KEYLINE_DT.itemsize + DESC)
            + cam.pyr_bytes + 8)


class DeviceFrames:
    """Input frames resident in HBM (torch uint8 buffers), one gfpl_frames per frame."""

    def __init__(self, host: HostFrames = None, device: str = "cuda"):
        self.bufs = []
        if host is None:
            return
        import torch
        self.B, self.kp_cap, self.kl_cap = host.B, host.kp_cap, host.kl_cap
        for a in host.arrays():
            t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1))
            self.bufs.append(t.to(device))

    @classmethod
    def generate(cls, cam: Camera, sp: SynthParams, n_seq: int, n_frames: int, kp_cap: int, kl_cap: int,
                 seq0: int = 0, device="cuda", threads: int = 0) -> "DeviceFrames":
        """Generate frame by frame on the host and stage each into HBM, so host memory
        holds one frame of the batch at a time (frames are independent given the
        sequence seed, gfpl_synth)."""
        import torch
        d = cls(None)
        d.B, d.kp_cap, d.kl_cap = n_seq, kp_cap, kl_cap
        for f in range(n_frames):
            h = HostFrames(cam, sp, n_seq, 1, kp_cap, kl_cap, seq0=seq0, frame0=f, threads=threads)
            arrs = h.arrays()
            if not d.bufs:
                d.bufs = [torch.empty((n_frames, a[0].nbytes), dtype=torch.uint8, device=device) for a in arrs]
            for buf, a in zip(d.bufs, arrs):
                buf[f].copy_(torch.from_numpy(np.ascontiguousarray(a[0]).view(np.uint8).reshape(-1)))
            del h
        return d

    def frames(self, f: int) -> Frames:
        arrs = [b[f] for b in self.bufs]
        return make_frames(self.B, self.kp_cap, self.kl_cap, arrs)

    def frames_slice(self, f: int, s0: int, n: int) -> Frames:
        """Frame f of sequences [s0, s0 + n) (a view: every field is [B][...] row-major)."""
        if s0 < 0 or n <= 0 or s0 + n > self.B:
            raise ValueError(f"sequence slice [{s0}, {s0 + n}) outside [0, {self.B})")
        arrs = [b[f].view(self.B, -1)[s0:s0 + n] for b in self.bufs]
        return make_frames(n, self.kp_cap, self.kl_cap, arrs)

    def nbytes(self) -> int:
        return sum(b.numel() for b in self.bufs)


# ----------------------------------------------------------- frame state --
class FrameHost:
    """numpy-backed gfpl_frame_host (one sequence's frame state)."""

    def __init__(self, kp_cap: int, kl_cap: int):
        self.kp_cap, self.kl_cap = kp_cap, kl_cap
        self.s = FrameHostStruct()
        self.arr = {}
        for n, dt, sh in PT_FIELDS:
            self.arr[n] = np.zeros((kp_cap,) + sh, dt)
            setattr(self.s, n, self.arr[n].ctypes.data)
        for n, dt, sh in LS_FIELDS:
            self.arr[n] = np.zeros((kl_cap,) + sh, dt)
            setattr(self.s, n, self.arr[n].ctypes.data)

    @property
    def n_pt(self) -> int:
        return self.s.n_pt

    @property
    def n_ls(self) -> int:
        return self.s.n_ls

    def get(self, name: str) -> np.ndarray:
        if name in self.arr:
            n = self.s.n_pt if name.startswith("pt_") or name == "pdesc" else self.s.n_ls
            return self.arr[name][:n]
        if name in ("err_norm", "time_stamp"):
            return np.array(getattr(self.s, name))
        k = dict(POSE_FIELDS)[name]
        v = np.ctypeslib.as_array(getattr(self.s, name))[:k].copy()
        return v.reshape(4, 4) if k == 16 else v.reshape(6, 6) if k == 36 else v

    def pose(self) -> dict:
        return {n: self.get(n) for n, _ in POSE_FIELDS} | {"err_norm": float(self.s.err_norm)}

    def ptr(self):
        return C.byref(self.s)


# ---------------------------------------------------------- GPU handles --
class Context:
    """gfpl_ctx: one HIP device + stream + camera + config.  stream: a hipStream_t handle
    (0 = the default stream); own_stream=True gives the context its own non-blocking stream
    (gfpl_create_async), e.g. for detection beside a tracking context."""

    def __init__(self, cam: Camera, cfg: Config, device: int = 0, stream: int = 0, own_stream: bool = False):
        self.L = hiplib()
        h = C.c_void_p()
        if own_stream:
            check(self.L.gfpl_create_async(device, C.byref(h)), "gfpl_create_async")
        else:
            check(self.L.gfpl_create(device, C.c_void_p(stream), C.byref(h)), "gfpl_create")
        self.h = h
        self.device = device
        check(self.L.gfpl_set_camera(h, C.byref(cam)), "set_camera")
        check(self.L.gfpl_set_config(h, C.byref(cfg)), "set_config")
        self.cam, self.cfg = cam, cfg

    def synchronize(self):
        check(self.L.gfpl_synchronize(self.h), "synchronize")

    @property
    def stream(self) -> int:
        """the hipStream_t handle the context enqueues on (0: the default stream)"""
        return int(self.L.gfpl_get_stream(self.h) or 0)

    def torch_stream(self):
        """the context's stream as a torch stream (torch work ordered with the gfpl calls)"""
        import torch
        dev = torch.device("cuda", self.device)
        return torch.cuda.ExternalStream(self.stream, device=dev) if self.stream else torch.cuda.default_stream(dev)

    def set_config(self, cfg: Config):
        """gfpl_set_config between steps (e.g. the line cut's proof mode); the context keeps a copy."""
        check(self.L.gfpl_set_config(self.h, C.byref(cfg)), "set_config")
        self.cfg = cfg

    def set_timing(self, on: bool):
        check(self.L.gfpl_set_timing(self.h, int(on)), "set_timing")

    def stage_times(self) -> np.ndarray:
        out = np.zeros(7, np.float32)
        check(self.L.gfpl_get_stage_times(self.h, out.ctypes.data), "stage_times")
        return out

    def kernel_times(self) -> np.ndarray:
        """[k_cut_prep, k_cut_search (k_cut_search_eig with cut_with_max_vol = 0), k_cut_finish, k_pose]
        device ms of the last step."""
        out = np.zeros(4, np.float32)
        check(self.L.gfpl_get_kernel_times(self.h, out.ctypes.data), "kernel_times")
        return out

    def knn2(self, q_dev, nq: int, t_dev, nt: int, cell: int, idx_dev, dist_dev) -> int:
        return self.L.gfpl_knn2_hamming(self.h, _ptr(q_dev), nq, _ptr(t_dev), nt, cell,
                                        _ptr(idx_dev), _ptr(dist_dev))

    def lookForCommonMatches(self, kf0: KeyFrameView, kf1: KeyFrameView):
        """MapHandler::lookForCommonMatches keyframe-pair stage (src/mapHandler.cpp:199-470):
        the accepted (kf0 row, kf1 row) point and line pairs, in the order the reference's
        loops visit them; the map bookkeeping stays with the caller."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        pp = torch.zeros(2 * max(kf0.s.n_pt, 1), dtype=torch.int32, device=dev)
        lp = torch.zeros(2 * max(kf0.s.n_ls, 1), dtype=torch.int32, device=dev)
        npt, nls = C.c_int(0), C.c_int(0)
        torch.cuda.synchronize()
        check(self.L.gfpl_kf_common_matches(self.h, C.byref(kf0.s), C.byref(kf1.s), _ptr(pp), C.byref(npt),
                                            _ptr(lp), C.byref(nls)), "kf_common_matches")
        return (pp[: 2 * npt.value].cpu().numpy().reshape(-1, 2),
                lp[: 2 * nls.value].cpu().numpy().reshape(-1, 2))

    def lookForLocalMapMatches(self, local_map: MapView, kf1_unmatched: KeyFrameView,
                               max_kf_epip_p: float = 1.0, max_kf_epip_l: float = 1.0):
        """lookForCommonMatches local-map stage (src/mapHandler.cpp:472-772): (map row,
        kf1 unmatched row) point and line pairs in the reference's loop order."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        pp = torch.zeros(2 * max(local_map.s.n_pt, 1), dtype=torch.int32, device=dev)
        lp = torch.zeros(2 * max(local_map.s.n_ls, 1), dtype=torch.int32, device=dev)
        npt, nls = C.c_int(0), C.c_int(0)
        torch.cuda.synchronize()
        check(self.L.gfpl_kf_local_map_matches(self.h, C.byref(local_map.s), C.byref(kf1_unmatched.s),
                                               max_kf_epip_p, max_kf_epip_l, _ptr(pp), C.byref(npt),
                                               _ptr(lp), C.byref(nls)), "kf_local_map_matches")
        return (pp[: 2 * npt.value].cpu().numpy().reshape(-1, 2),
                lp[: 2 * nls.value].cpu().numpy().reshape(-1, 2))

    def fuseSearch_rc(self, fuse_map: "FuseMap", params: Optional["FuseParams"] = None):
        """gfpl_map_fuse_search: (return code, dict of pt_loc, pt_pairs, ls_loc, ls_pairs as numpy arrays)."""
        import torch
        s = fuse_map.s
        dev = torch.device("cuda", torch.cuda.current_device())
        out = {k: torch.zeros(w * max(n, 1), dtype=torch.int32, device=dev)
               for k, w, n in (("pt_loc", 1, s.map.n_pt), ("pt_pairs", 2, s.map.n_pt), ("ls_loc", 1, s.map.n_ls),
                               ("ls_pairs", 2, s.map.n_ls))}
        cnt = {k: C.c_int(0) for k in out}
        prm = params or FuseParams.default()
        torch.cuda.synchronize()
        rc = self.L.gfpl_map_fuse_search(self.h, C.byref(s), C.byref(prm), _ptr(out["pt_loc"]), C.byref(cnt["pt_loc"]),
                                         _ptr(out["pt_pairs"]), C.byref(cnt["pt_pairs"]), _ptr(out["ls_loc"]),
                                         C.byref(cnt["ls_loc"]), _ptr(out["ls_pairs"]), C.byref(cnt["ls_pairs"]))
        res = {}
        for k, t in out.items():
            w = 2 if k.endswith("pairs") else 1
            a = t[: w * cnt[k].value].cpu().numpy()
            res[k] = a.reshape(-1, 2) if w == 2 else a
        return rc, res

    def fuseSearch(self, fuse_map: "FuseMap", params: Optional["FuseParams"] = None) -> dict:
        """The candidate search of fuseLandmarksFromLocalMap (src/mapHandler.cpp:859-1056): pt_loc / ls_loc
        (map row of every selected row) and pt_pairs / ls_pairs ((i, t) over the selected list, the
        reference's map_local_*_to_fuse) in the reference's order."""
        rc, res = self.fuseSearch_rc(fuse_map, params)
        check(rc, "map_fuse_search")
        return res

    def fuseSearch_device_ms(self, kind: int):
        """gfpl_map_fuse_debug_ms: (select, knn-2, gate) device milliseconds of the last fuseSearch, per kind."""
        ms = (C.c_float * 3)()
        check(self.L.gfpl_map_fuse_debug_ms(self.h, int(kind), ms), "map_fuse_debug_ms")
        return [float(v) for v in ms]

    def isLoopClosure(self, kf0_views, kf1_views, params: Optional[LoopParams] = None):
        """MapHandler::isLoopClosure (src/mapHandler.cpp:3078-3545) for a batch of candidate pairs
        (kf0_views[i], kf1_views[i]) in one call: per pair (LoopResult, pt_pairs [n_pt][2], pt_inlier
        [n_pt] u8, ls_pairs [n_ls][2], ls_inlier [n_ls]); the pairs are (kf0 row, kf1 row) in kf0 row
        order.  A single KeyFrameView pair may be passed instead of two lists."""
        import torch
        if isinstance(kf0_views, KeyFrameView):
            kf0_views, kf1_views = [kf0_views], [kf1_views]
        n = len(kf0_views)
        if len(kf1_views) != n:
            raise GfplError(-1, "isLoopClosure: kf0_views and kf1_views differ in length")
        prm = params if params is not None else LoopParams.default()
        v0 = (KFViewStruct * max(n, 1))(*[k.s for k in kf0_views])
        v1 = (KFViewStruct * max(n, 1))(*[k.s for k in kf1_views])
        pt_cap = max([k.s.n_pt for k in kf0_views] + [1])
        ls_cap = max([k.s.n_ls for k in kf0_views] + [1])
        dev = torch.device("cuda", torch.cuda.current_device())
        pp = torch.zeros((max(n, 1), pt_cap, 2), dtype=torch.int32, device=dev)
        pi = torch.zeros((max(n, 1), pt_cap), dtype=torch.uint8, device=dev)
        lp = torch.zeros((max(n, 1), ls_cap, 2), dtype=torch.int32, device=dev)
        li = torch.zeros((max(n, 1), ls_cap), dtype=torch.uint8, device=dev)
        out = (LoopResult * max(n, 1))()
        torch.cuda.synchronize()
        check(self.L.gfpl_kf_loop_closure(self.h, v0, v1, n, C.byref(prm), pt_cap, ls_cap, _ptr(pp), _ptr(pi),
                                          _ptr(lp), _ptr(li), out), "kf_loop_closure")
        pp, pi, lp, li = pp.cpu().numpy(), pi.cpu().numpy(), lp.cpu().numpy(), li.cpu().numpy()
        res = []
        for i in range(n):
            r = LoopResult.from_buffer_copy(out[i])
            res.append((r, pp[i, :r.n_pt].copy(), pi[i, :r.n_pt].copy(), lp[i, :r.n_ls].copy(), li[i, :r.n_ls].copy()))
        return res

    def bowTransform(self, voc: "Vocabulary", desc_sets, cap: Optional[int] = None):
        """TemplatedVocabulary::transform(features, BowVector&) for a batch of descriptor sets (device u8
        tensors [count][32], e.g. a keyframe's pdesc_l or ldesc_l) in one call: per set (word ids int32,
        values f64), in ascending word id.  cap: the rows of the output arrays (default: the largest
        count)."""
        import torch
        n = len(desc_sets)
        counts = [int(d.shape[0]) for d in desc_sets]
        if cap is None:
            cap = max(counts + [1])
        dev = torch.device("cuda", self.device)
        ptrs = (C.c_void_p * max(n, 1))(*[_ptr(d) if c else None for d, c in zip(desc_sets, counts)])
        cnt = (C.c_int * max(n, 1))(*counts)
        ids = torch.zeros((max(n, 1), max(cap, 1)), dtype=torch.int32, device=dev)
        vals = torch.zeros((max(n, 1), max(cap, 1)), dtype=torch.float64, device=dev)
        nw = (C.c_int * max(n, 1))()
        torch.cuda.synchronize()
        check(self.L.gfpl_bow_transform(self.h, voc.h, n, ptrs, cnt, cap, _ptr(ids), _ptr(vals), nw), "bow_transform")
        ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
        return [(ids[i, :nw[i]].copy(), vals[i, :nw[i]].copy()) for i in range(n)]

    def bowScore(self, a, b) -> np.ndarray:
        """L1Scoring::score(a[i], b[i]) for a batch of pairs in one call; a vector is (word ids, values)
        as numpy arrays or device tensors, or a BowVec (BowDatabase.vector_device).  Returns f64 [n]."""
        import torch
        n = len(a)
        if len(b) != n:
            raise GfplError(-1, "bowScore: a and b differ in length")
        dev = torch.device("cuda", self.device)
        keep = []

        def vec(v):
            if isinstance(v, BowVec):
                return v
            i, x = v
            if isinstance(i, np.ndarray):
                i = torch.from_numpy(np.ascontiguousarray(i, np.int32)).to(dev)
                x = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
            keep.append((i, x))
            return BowVec(_ptr(i) if len(i) else None, _ptr(x) if len(i) else None, len(i))

        va = (BowVec * max(n, 1))(*[vec(v) for v in a])
        vb = (BowVec * max(n, 1))(*[vec(v) for v in b])
        out = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        check(self.L.gfpl_bow_score(self.h, va, vb, n, _ptr(out)), "bow_score")
        return out.cpu().numpy()[:n].copy()

    def _ba_run(self, solver_cls, problems, prm, debug=None):
        """One solve of a solver made for these problems (LbaSolver or GbaSolver) and closed after it."""
        counts = []
        for p in problems:   # the host rules first: nothing is allocated for a refused problem
            rc, c = solver_cls.check_counts(p)
            if rc != 0:
                raise GfplError(rc, solver_cls._name + "_check")
            counts.append(c)
        caps = [max(col) for col in zip(solver_cls._min_caps, *counts)]
        solver = solver_cls(self, caps, max(len(problems), 1))
        try:
            return solver.solve(problems, prm, debug)
        finally:
            solver.close()

    def localBundleAdjustment(self, problems, params: Optional[LbaParams] = None):
        """MapHandler::localBundleAdjustment's solver (levMarquardtOptimizationLBA, src/mapHandler.cpp:
        1217-1713) for a batch of LbaProblem in one call (a single problem may be passed).  Per problem
        a dict: result (LbaResult), T_kf [n_kf][4][4] = expmap_se3(X), pt, ls and x_kf, the pose part of
        X at exit.  The problems' own arrays are not changed."""
        single = isinstance(problems, LbaProblem)
        res = self._ba_run(LbaSolver, [problems] if single else list(problems), params if params is not None else LbaParams.default())
        return res[0] if single else res

    def lbaDebugSystem(self, problem: LbaProblem, iteration: int, params: Optional[LbaParams] = None):
        """Test hook (gfpl_lba_debug_system): the undamped system of `iteration` (0: the pre-pass) —
        the pose blocks U, the landmark blocks V_pt / V_ls, the coupling blocks W_pt / W_ls (landmark
        rows, pose columns), g and err — from a solve of iteration + 1 iterations."""
        prm = LbaParams.default() if params is None else LbaParams.from_buffer_copy(params)
        prm.max_iters = iteration + 1
        return self._ba_run(LbaSolver, [problem], prm, debug=(0, iteration))[1]

    def globalBundleAdjustment(self, problems, params: Optional[LbaParams] = None):
        """MapHandler::globalBundleAdjustment's solver (levMarquardtOptimizationGBA, src/mapHandler.cpp:
        1950-2544) for one LbaProblem or a list of them: the local keyframes are every alive keyframe but
        keyframe 0, which is a fixed pose.  Per problem the dict of Context.localBundleAdjustment.  The
        problems' own arrays are not changed."""
        single = isinstance(problems, LbaProblem)
        res = self._ba_run(GbaSolver, [problems] if single else list(problems), params if params is not None else LbaParams.default())
        return res[0] if single else res

    def gbaDebugSystem(self, problem: LbaProblem, iteration: int, params: Optional[LbaParams] = None):
        """Test hook (gfpl_gba_debug_system): the undamped system of `iteration` (0: the pre-pass) from a
        solve of iteration + 1 iterations: U, g, V_pt, V_ls, err, and the coupling blocks under the
        diagonal per (landmark, keyframe) pair: W_pt [point pairs][3][6], W_ls [line pairs][6][6], pairs."""
        prm = LbaParams.default() if params is None else LbaParams.from_buffer_copy(params)
        prm.max_iters = iteration + 1
        return self._ba_run(GbaSolver, [problem], prm, debug=(0, iteration))[1]

    def _pgo_run(self, problems, prm, debug=None):
        counts = []
        for p in problems:   # the host rules first: nothing is allocated for a refused problem
            rc, c = p.check(prm)
            if rc != 0:
                raise GfplError(rc, "pgo_check")
            counts.append(c)
        solver = PoseGraph(self, counts, max(len(problems), 1))
        try:
            return solver.solve(problems, prm, debug)
        finally:
            solver.close()

    def loopClosureOptimization(self, problems, params: Optional["PoseGraphParams"] = None):
        """MapHandler::loopClosureOptimizationCovGraphG2O / EssGraphG2O (src/mapHandler.cpp:4187-4419,
        :3950-4184; params.variant) for a batch of PoseGraphProblem in one call (a single problem may be
        passed): the pose graph, its Levenberg-Marquardt solve and the correction of every keyframe
        pose and owned landmark, all on the device.  Per problem a dict (see PoseGraph.solve)."""
        single = isinstance(problems, PoseGraphProblem)
        res = self._pgo_run([problems] if single else list(problems), params if params is not None else PoseGraphParams.default())
        return res[0] if single else res

    def pgoDebugSystem(self, problem: "PoseGraphProblem", params: Optional["PoseGraphParams"] = None):
        """Test hook (gfpl_pgo_debug_system): iteration 0's chi2, b, the diagonal and envelope blocks (and
        H, the dense lower triangle they make), the vertex and edge lists, Z and the start poses X0,
        from a solve of one iteration.  Returns (that solve's results, the system)."""
        prm = PoseGraphParams.default() if params is None else PoseGraphParams.from_buffer_copy(params)
        prm.max_iters = 1
        return self._pgo_run([problem], prm, debug=0)

    def close(self):
        """gfpl_destroy.  Refused (GfplError, the handle kept) while a StereoFrameHandler
        created on this context is still open: close those first."""
        if getattr(self, "h", None):
            check(self.L.gfpl_destroy(self.h), "gfpl_destroy (close the StereoFrameHandlers of this context first)")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Event:
    """gfpl_event: record on one context's stream, make another context's stream wait."""

    def __init__(self, ctx: Context):
        self.L = ctx.L
        h = C.c_void_p()
        check(self.L.gfpl_event_create(ctx.h, C.byref(h)), "gfpl_event_create")
        self.h = h

    def record(self, ctx: Context):
        check(self.L.gfpl_event_record(self.h, ctx.h), "gfpl_event_record")

    def wait(self, ctx: Context):
        """ctx's stream waits for the last record"""
        check(self.L.gfpl_event_wait(ctx.h, self.h), "gfpl_event_wait")

    def synchronize(self):
        check(self.L.gfpl_event_synchronize(self.h), "gfpl_event_synchronize")

    @property
    def record_count(self) -> int:
        """records so far (gfpl_event_record, or a tracker call's gfpl_frames.consumed mark)"""
        n = C.c_int64(0)
        check(self.L.gfpl_event_record_count(self.h, C.byref(n)), "gfpl_event_record_count")
        return n.value

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_event_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BaSolver:
    """What LbaSolver and GbaSolver share: the object behind gfpl_<_name>_create / _solve / _debug_system /
    _destroy.  A subclass names the entry points, makes its counts type from caps and says what the
    debug hook returns besides U, g, V_pt and V_ls."""
    _name = ""
    _min_caps = ()      # the counts of a solver made for no problem

    def __init__(self, ctx: "Context", caps, max_problems: int):
        self.ctx, self.L = ctx, ctx.L
        self.caps = self._counts(caps)
        self.h = C.c_void_p()
        check(self._c("create")(ctx.h, C.byref(self.caps), max_problems, C.byref(self.h)), self._name + "_create")

    def _c(self, what):
        return getattr(self.L, "gfpl_%s_%s" % (self._name, what))

    def solve(self, problems, params: Optional[LbaParams] = None, debug=None):
        """Per problem a dict (see Context.localBundleAdjustment).  debug = (i, iteration): also the
        system of the solver's debug hook for problem i, as the second element of a pair."""
        import torch
        prm = params if params is not None else LbaParams.default()
        n = len(problems)
        dev = torch.device("cuda", self.ctx.device)
        devs, structs = [], (LbaProblemStruct * max(n, 1))()
        for i, p in enumerate(problems):
            d = {k: torch.from_numpy(p.a[k].copy()).to(dev) for k, _ in LBA_DOUBLES}
            d["x_out"] = d["x_kf"].clone()   # (a problem whose Hmax leaves the int range writes nothing)
            devs.append(d)
            structs[i] = p.struct(d)
        out = (LbaResult * max(n, 1))()
        torch.cuda.synchronize()
        check(self._c("solve")(self.h, structs, n, C.byref(prm), out), self._name + "_solve")
        res = []
        for i, d in enumerate(devs):
            res.append(dict(result=LbaResult.from_buffer_copy(out[i]), T_kf=d["T_kf"].cpu().numpy().reshape(-1, 4, 4),
                            pt=d["pt"].cpu().numpy(), ls=d["ls"].cpu().numpy(), x_kf=d["x_out"].cpu().numpy()))
        if debug is None:
            return res
        i, it = debug
        c = problems[i].counts
        sysd = dict(U=np.zeros((c.n_kf, 6, 6)), g=np.zeros(6 * c.n_kf + 3 * c.n_pt + 6 * c.n_ls),
                    V_pt=np.zeros((c.n_pt, 3, 3)), V_ls=np.zeros((c.n_ls, 6, 6)), **self._debug_blocks(problems[i]))
        err = C.c_double(0.0)   # (the dict's order is the hook's argument order)
        check(self._c("debug_system")(self.h, i, it, *[_ptr(v) for v in sysd.values()], C.byref(err)),
              self._name + "_debug_system")
        sysd["err"] = np.float64(err.value)
        return res, sysd

    def close(self):
        if getattr(self, "h", None):
            check(self._c("destroy")(self.h), self._name + "_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GbaSolver(_BaSolver):
    """gfpl_gba: the device workspace of up to max_problems global bundle adjustments whose counts
    (GbaCounts, or the nine numbers of GbaCounts.of) stay within caps; solve() may be called any number
    of times (per problem the dict of Context.globalBundleAdjustment).  The context cannot be closed
    while the solver is open."""
    _name, _min_caps = "gba", (1, 0, 0, 0, 0, 0, 0, 0, 0)

    @staticmethod
    def _counts(caps):
        return caps if isinstance(caps, GbaCounts) else GbaCounts.of(*[int(v) for v in caps])

    @staticmethod
    def check_counts(problem: LbaProblem):
        rc, c = gbaCheck(problem)
        return rc, c.flat()

    @staticmethod
    def _debug_blocks(problem: LbaProblem):
        rc, g = gbaCheck(problem)
        check(rc, "gba_check")
        return dict(W_pt=np.zeros((g.n_pt_pairs, 3, 6)), W_ls=np.zeros((g.n_ls_pairs, 6, 6)),
                    pairs=np.zeros((g.n_pt_pairs + g.n_ls_pairs, 2), np.int32))


class LbaSolver(_BaSolver):
    """gfpl_lba: the device workspace of up to max_problems local bundle adjustments whose counts stay
    within caps (n_kf, n_fix, n_pt, n_ls, n_pt_obs, n_ls_obs); solve() may be called any number of
    times.  The context cannot be closed while the solver is open."""
    _name, _min_caps = "lba", (1, 0, 0, 0, 0, 0)

    @staticmethod
    def _counts(caps):
        return caps if isinstance(caps, LbaCounts) else LbaCounts(*[int(v) for v in caps])

    @staticmethod
    def check_counts(problem: LbaProblem):
        return problem.check(), [getattr(problem.counts, f) for f, _ in LbaCounts._fields_]

    @staticmethod
    def _debug_blocks(problem: LbaProblem):
        c = problem.counts
        return dict(W_pt=np.zeros((c.n_pt, c.n_kf, 3, 6)), W_ls=np.zeros((c.n_ls, c.n_kf, 6, 6)))


# ------------------------------------------------- loop-closure pose graph --
PGO_COV, PGO_ESS = 0, 1
PGO_STOP_ITERS, PGO_STOP_STEP, PGO_STOP_DCHI2, PGO_STOP_REJECT, PGO_STOP_NOFREE = 0, 1, 2, 3, 4
PGO_SINGULAR = 1
PGO_VERT_FIXED, PGO_VERT_LC_J, PGO_VERT_LC_I = 1, 2, 4
PGO_BLOCK, PGO_RED, PGO_PANEL = 256, 78, 16   # k_pgo's threads, reduction lanes per free vertex, LDS panel (gfpl_layout.hpp)
PGO_GUARD = 32                                # sentinel doubles on either side of every device array of a solve


class PoseGraphParams(C.Structure):
    """gfpl_pgo_graph_params: Config::minLMEssGraph / minLMCovGraph (src/config.cpp:50-51), the variant
    (PGO_COV / PGO_ESS) and the iteration (optimize(100), setUserLambdaInit(1e-10), 10 retries)."""
    _fields_ = [("min_lm_ess_graph", C.c_int32), ("min_lm_cov_graph", C.c_int32), ("variant", C.c_int32),
                ("max_iters", C.c_int32), ("max_rejects", C.c_int32), ("pad", C.c_int32), ("lambda_init", C.c_double)]

    @classmethod
    def default(cls, **over) -> "PoseGraphParams":
        p = cls()
        hiplib().gfpl_default_pgo_params(C.byref(p))
        for k, v in over.items():
            setattr(p, k, v)
        return p


class PgoCounts(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_kf", "n_lc", "n_vert", "n_free", "n_edge", "env_blocks", "n_pt", "n_ls")]


class PgoProblemStruct(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_kf", "n_lc", "n_pt", "n_ls")] + [(k, _vp) for k in (
        "alive", "full_graph", "lc", "lc_pose", "T_kf", "x_kf", "pt", "ls", "pt_dir", "ls_dir", "pt_kf_start", "pt_kf_idx",
        "ls_kf_start", "ls_kf_idx", "pt_dir_off", "ls_dir_off", "pt_freed", "ls_freed")]


class PgoResult(C.Structure):
    """gfpl_pgo_result: iters accepted iterations; stop PGO_STOP_*; status bit PGO_SINGULAR; rejects the
    rejected trials; the graph's counts; lambda, chi2_0 and chi2 at exit."""
    _fields_ = [("iters", C.c_int32), ("stop", C.c_int32), ("status", C.c_int32), ("rejects", C.c_int32),
                ("n_vert", C.c_int32), ("n_free", C.c_int32), ("n_edge", C.c_int32), ("kf_curr", C.c_int32),
                ("lambda_", C.c_double), ("chi2_0", C.c_double), ("chi2", C.c_double)]


def _csr(lists, n_kf):
    start = np.zeros(n_kf + 1, np.int32)
    for i in range(n_kf):
        start[i + 1] = start[i] + len(lists[i])
    idx = np.array([j for l in lists for j in l], np.int32).reshape(-1)
    return start, idx


class PoseGraphProblem:
    """One loop-closure optimisation (gfpl_pgo_problem) from numpy arrays: alive [n_kf], full_graph
    [n_kf][n_kf], lc [n_lc][3] (kf_prev, kf_curr, flag) with lc_pose [n_lc][6], T_kf [n_kf][4][4]; the
    map: pt [n_pt][3], ls [n_ls][6], pt_own / ls_own (per keyframe the list of landmark ids it owns,
    an id < 0 a freed landmark), optional pt_dirs / ls_dirs (per landmark an [n][3] array: dir_list;
    None: the caller does not keep them on the device) and pt_freed / ls_freed marks."""

    def __init__(self, alive, full_graph, lc, lc_pose, T_kf, pt=None, ls=None, pt_own=None, ls_own=None,
                 pt_dirs=None, ls_dirs=None, pt_freed=None, ls_freed=None):
        a = self.a = {}
        a["alive"] = np.ascontiguousarray(np.asarray(alive).astype(np.uint8).reshape(-1))
        n_kf = self.n_kf = len(a["alive"])
        a["full_graph"] = np.ascontiguousarray(np.asarray(full_graph, np.int32).reshape(n_kf, n_kf))
        a["lc"] = np.array(lc, np.int32).reshape(-1, 3)            # (copies: the caller's lists stay the caller's)
        a["lc_pose"] = np.array(lc_pose, np.float64).reshape(-1, 6)
        a["T_kf"] = np.ascontiguousarray(np.asarray(T_kf, np.float64).reshape(-1, 16))
        a["pt"] = np.ascontiguousarray(np.asarray(pt if pt is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3))
        a["ls"] = np.ascontiguousarray(np.asarray(ls if ls is not None else np.zeros((0, 6)), np.float64).reshape(-1, 6))
        for k, own, dirs, freed, n in (("pt", pt_own, pt_dirs, pt_freed, len(a["pt"])), ("ls", ls_own, ls_dirs, ls_freed, len(a["ls"]))):
            own = own if own is not None else [[] for _ in range(n_kf)]
            a[k + "_kf_start"], a[k + "_kf_idx"] = _csr(own, n_kf)
            if dirs is not None:
                off = np.zeros(n + 1, np.int32)
                for j in range(n):
                    off[j + 1] = off[j] + len(dirs[j])
                a[k + "_dir_off"] = off
                rows = [np.asarray(d, np.float64).reshape(-1, 3) for d in dirs]
                a[k + "_dir"] = np.ascontiguousarray(np.concatenate(rows + [np.zeros((0, 3))]))
            else:
                a[k + "_dir_off"] = a[k + "_dir"] = None
            a[k + "_freed"] = None if freed is None else np.ascontiguousarray(np.asarray(freed).astype(np.uint8).reshape(-1))

    DEVICE = ("T_kf", "x_kf", "pt", "ls", "pt_dir", "ls_dir")

    def struct(self, dev=None) -> PgoProblemStruct:
        """The C record: the index arrays on the host; the map's doubles on the host (dev=None, for
        check()) or the device tensors of `dev` (a dict name -> tensor)."""
        a, s = self.a, PgoProblemStruct()
        s.n_kf, s.n_lc, s.n_pt, s.n_ls = self.n_kf, len(a["lc"]), len(a["pt"]), len(a["ls"])
        for k in ("alive", "full_graph", "lc", "lc_pose", "pt_kf_start", "pt_kf_idx", "ls_kf_start", "ls_kf_idx",
                  "pt_dir_off", "ls_dir_off", "pt_freed", "ls_freed"):
            setattr(s, k, _ptr(a[k]) if a[k] is not None and a[k].size else None)
        if dev is None:
            self._x = np.zeros((self.n_kf, 6))
            dev = dict(a, x_kf=self._x)
        for k in self.DEVICE:
            v = dev.get(k)
            setattr(s, k, _ptr(v) if v is not None and (k.endswith("_dir") or len(v)) else None)
        return s

    def check(self, params: Optional[PoseGraphParams] = None):
        """gfpl_pgo_check (host only): (return code, PgoCounts of the graph)."""
        prm = params if params is not None else PoseGraphParams.default()
        cnt = PgoCounts()
        rc = hiplib().gfpl_pgo_check(C.byref(self.struct()), C.byref(prm), C.byref(cnt))
        return rc, cnt


def pgoWorkspace(counts: PgoCounts):
    """gfpl_pgo_workspace: (return code, hbm_bytes, lds_bytes) for one problem of these counts."""
    hbm, lds = C.c_int64(0), C.c_int32(0)
    rc = hiplib().gfpl_pgo_workspace(C.byref(counts), C.byref(hbm), C.byref(lds))
    return rc, hbm.value, lds.value


class PoseGraph:
    """gfpl_pgo: the device workspace of up to max_problems loop-closure optimisations whose counts
    stay within caps (a PgoCounts, or the largest of a list of them); solve() may be called any number
    of times.  The context cannot be closed while the object is open."""

    def __init__(self, ctx: "Context", caps, max_problems: int):
        self.ctx, self.L = ctx, ctx.L
        if not isinstance(caps, PgoCounts):
            caps = PgoCounts(*[max([getattr(c, f) for c in caps] + [1 if f in ("n_kf", "n_lc", "n_edge") else 0])
                               for f, _ in PgoCounts._fields_])
        self.caps = caps
        self.h = C.c_void_p()
        check(self.L.gfpl_pgo_create(ctx.h, C.byref(self.caps), max_problems, C.byref(self.h)), "pgo_create")

    def solve(self, problems, params: Optional[PoseGraphParams] = None, debug=None):
        """Per problem a dict: result (PgoResult), T_kf [n_kf][4][4], x_kf [n_kf][6] (NaN rows: keyframes
        the call did not move), pt, ls, pt_dirs / ls_dirs (per landmark, or None) and guards_ok (the
        PGO_GUARD sentinels on either side of every device array are untouched).  The problems' own
        arrays are not changed.  debug = i: also gfpl_pgo_debug_system of problem i (params.max_iters
        must be 1), as the second element of a pair."""
        import torch
        prm = params if params is not None else PoseGraphParams.default()
        n = len(problems)
        dev = torch.device("cuda", self.ctx.device)
        G, SENT = PGO_GUARD, -6.02214076e23
        fulls, devs, structs = [], [], (PgoProblemStruct * max(n, 1))()
        for i, p in enumerate(problems):
            src = dict(p.a, x_kf=np.full((p.n_kf, 6), np.nan))
            full, d = {}, {}
            for k in PoseGraphProblem.DEVICE:
                if src[k] is None:
                    d[k] = None
                    continue
                h = np.concatenate([np.full(G, SENT), src[k].reshape(-1), np.full(G, SENT)])
                full[k] = torch.from_numpy(h).to(dev)
                d[k] = full[k][G:G + src[k].size]
            fulls.append(full)
            devs.append(d)
            structs[i] = p.struct(d)
        out = (PgoResult * max(n, 1))()
        torch.cuda.synchronize()
        check(self.L.gfpl_pgo_solve(self.h, structs, n, C.byref(prm), out), "pgo_solve")
        res = []
        for i, p in enumerate(problems):
            host = {k: t.cpu().numpy() for k, t in fulls[i].items()}
            ok = all((h[:G] == SENT).all() and (h[-G:] == SENT).all() for h in host.values())
            get = lambda k, w: host[k][G:-G].reshape(-1, w).copy()
            r = dict(result=PgoResult.from_buffer_copy(out[i]), T_kf=get("T_kf", 16).reshape(-1, 4, 4), x_kf=get("x_kf", 6),
                     pt=get("pt", 3), ls=get("ls", 6), guards_ok=bool(ok))
            for k in ("pt", "ls"):
                if p.a[k + "_dir"] is None:
                    r[k + "_dirs"] = None
                else:
                    rows, off = get(k + "_dir", 3), p.a[k + "_dir_off"]
                    r[k + "_dirs"] = [rows[off[j]:off[j + 1]] for j in range(len(off) - 1)]
            res.append(r)
        if debug is None:
            return res
        rc, c = problems[debug].check(prm)
        check(rc, "pgo_check")
        sysd = dict(b=np.zeros(6 * c.n_free), diag=np.zeros((c.n_free, 6, 6)), env=np.zeros((c.env_blocks, 6, 6)),
                    env_first=np.zeros(c.n_free, np.int32), vert=np.zeros((c.n_vert, 4), np.int32),
                    edge=np.zeros((c.n_edge, 4), np.int32), Z=np.zeros((c.n_edge, 4, 4)), X0=np.zeros((c.n_vert, 4, 4)))
        chi2 = C.c_double(0.0)
        check(self.L.gfpl_pgo_debug_system(self.h, debug, C.byref(chi2), *[_ptr(sysd[k]) if sysd[k].size else None for k in (
            "b", "diag", "env", "env_first", "vert", "edge", "Z", "X0")]), "pgo_debug_system")
        sysd["chi2"] = np.float64(chi2.value)
        # the dense lower triangle of the free system from the envelope rows
        nf = c.n_free
        H = np.zeros((6 * nf, 6 * nf))
        o = 0
        for r_ in range(nf):
            f = int(sysd["env_first"][r_])
            for cc in range(f, r_):
                H[6 * r_:6 * r_ + 6, 6 * cc:6 * cc + 6] = sysd["env"][o + cc - f]
            H[6 * r_:6 * r_ + 6, 6 * r_:6 * r_ + 6] = sysd["diag"][r_]
            o += r_ - f + 1
        sysd["H"] = H
        return res, sysd

    def ms(self):
        """gfpl_pgo_debug_ms: device milliseconds (k_pgo, k_pgo_correct) of the last solve."""
        a, b = C.c_float(0.0), C.c_float(0.0)
        check(self.L.gfpl_pgo_debug_ms(self.h, C.byref(a), C.byref(b)), "pgo_debug_ms")
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            check(self.L.gfpl_pgo_destroy(self.h), "pgo_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LM_MAX_OBS = 64
LM_ADD, LM_ERASE_OBS, LM_FREE = 0, 1, 2
LM_APPEND_LM = 3   # fuse / lm_fuse_check only
LM_BLOCK, LM_PLAN_TILE = 256, 2048   # the device planner: pairs per workgroup of its check, of its compaction


def _lm_ops(ops) -> np.ndarray:
    """Ops as an int32 [n][4] array of gfpl_lm_op rows (lm, kind, arg, src)."""
    a = np.ascontiguousarray(ops, np.int32)
    return a.reshape(-1, 4) if a.size else np.zeros((0, 4), np.int32)


def lm_ops_check(ops, counts, obs_cap: int, src_rows):
    """gfpl_lm_ops_check (host only): (return code, counts after).  counts [lm_cap] before the ops;
    src_rows: the rows of every source.  A refused list returns the counts unchanged."""
    o = _lm_ops(ops)
    cnt = np.array(counts, np.int32)
    rows = np.ascontiguousarray(src_rows, np.int32).reshape(-1)
    rc = hiplib().gfpl_lm_ops_check(_ptr(o), len(o), _ptr(cnt), len(cnt), int(obs_cap),
                                    _ptr(rows) if len(rows) else 0, len(rows))
    return rc, cnt


def lm_fuse_check(ops, counts, obs_cap: int, src_rows):
    """gfpl_lm_fuse_check (host only): (return code, counts after, n_rows) of a fuse list, the ops
    run one after another.  A refused list returns the counts unchanged and n_rows 0."""
    o = _lm_ops(ops)
    cnt = np.array(counts, np.int32)
    rows = np.ascontiguousarray(src_rows, np.int32).reshape(-1)
    n_rows = C.c_int64(-1)
    rc = hiplib().gfpl_lm_fuse_check(_ptr(o), len(o), _ptr(cnt), len(cnt), int(obs_cap),
                                     _ptr(rows) if len(rows) else 0, len(rows), C.byref(n_rows))
    return rc, cnt, int(n_rows.value)


class LandmarkStore:
    """gfpl_lmstore: desc_list and med_desc of lm_cap MapPoints or MapLines on the device
    (src/mapFeatures.cpp:28-92).  apply() takes ops [n][4] (lm, kind, arg, src) and the source
    descriptor arrays (torch device tensors [rows][32] uint8); gather() compacts the median rows of
    an id list into a device tensor; read() copies one landmark to the host.  observe_pairs(),
    observe_local(), free() and gather_ids() are the same from the device arrays a KeyframeMap leaves
    (the op list is planned on the device); counts() returns the device's counts.  The context cannot
    be closed while the store is open."""

    def __init__(self, ctx: "Context", lm_cap: int, obs_cap: int, max_ops: int):
        self.ctx, self.L = ctx, ctx.L
        self.lm_cap, self.obs_cap, self.max_ops = int(lm_cap), int(obs_cap), int(max_ops)
        self.h = C.c_void_p()
        check(self.L.gfpl_lmstore_create(ctx.h, self.lm_cap, self.obs_cap, self.max_ops, C.byref(self.h)), "lmstore_create")

    def apply_rc(self, ops, srcs, src_rows=None, src_ptrs=None) -> int:
        """gfpl_lmstore_apply's return code.  src_ptrs overrides the sources' device addresses (the
        tests pass a misaligned one)."""
        import torch
        o = _lm_ops(ops)
        srcs = list(srcs)
        rows = np.array([int(s.shape[0]) for s in srcs] if src_rows is None else src_rows, np.int32)
        ptrs = (C.c_void_p * max(len(srcs), 1))(*([_ptr(s) for s in srcs] if src_ptrs is None else src_ptrs))
        torch.cuda.synchronize()
        return self.L.gfpl_lmstore_apply(self.h, _ptr(o), len(o), ptrs if len(srcs) else None,
                                         _ptr(rows) if len(srcs) else 0, len(srcs))

    def apply(self, ops, srcs, src_rows=None) -> None:
        check(self.apply_rc(ops, srcs, src_rows), "lmstore_apply")

    def fuse_rc(self, ops, srcs, src_rows=None, src_ptrs=None) -> int:
        """gfpl_lmstore_fuse's return code: ADD, FREE and LM_APPEND_LM ops run one after another over
        the whole list (MapHandler::loopClosureFuseLandmarks' merges, without a row leaving the device)."""
        import torch
        o = _lm_ops(ops)
        srcs = list(srcs)
        rows = np.array([int(s.shape[0]) for s in srcs] if src_rows is None else src_rows, np.int32)
        ptrs = (C.c_void_p * max(len(srcs), 1))(*([_ptr(s) for s in srcs] if src_ptrs is None else src_ptrs))
        torch.cuda.synchronize()
        return self.L.gfpl_lmstore_fuse(self.h, _ptr(o), len(o), ptrs if len(srcs) else None,
                                        _ptr(rows) if len(srcs) else 0, len(srcs))

    def fuse(self, ops, srcs, src_rows=None) -> None:
        check(self.fuse_rc(ops, srcs, src_rows), "lmstore_fuse")

    def gather(self, ids, with_idx: bool = False):
        """Device tensor [n][32] of the ids' median rows (a MapView's pdesc / ldesc); with_idx: also
        their med_idx [n]."""
        import torch
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        dev = torch.device("cuda", self.ctx.device)
        out = torch.zeros((max(len(ids), 1), 32), dtype=torch.uint8, device=dev)
        idx = torch.full((max(len(ids), 1),), -2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        check(self.L.gfpl_lmstore_gather(self.h, _ptr(ids), len(ids), _ptr(out), _ptr(idx)), "lmstore_gather")
        return (out[: len(ids)], idx[: len(ids)]) if with_idx else out[: len(ids)]

    # ---- the device-id calls: the arrays are the ones KeyframeMap / MapGeometry take and return.  A list is a
    # torch int32 device tensor (a host list is uploaded), a descriptor array a torch uint8 device tensor
    # [rows][32]; either may be given as a raw (device address, rows) tuple instead.
    def _list(self, a, cols: int = 0):
        """(address, rows, the tensor that keeps it alive)"""
        import torch
        if isinstance(a, tuple):
            return int(a[0]), int(a[1]), None
        if not isinstance(a, torch.Tensor):
            a = np.ascontiguousarray(a, np.int32)
            a = a.reshape(-1, cols) if cols else a.reshape(-1)
            a = torch.from_numpy(a.copy()).to(torch.device("cuda", self.ctx.device))
        return _ptr(a), int(a.shape[0]), a

    @staticmethod
    def _rows(d):
        return (int(d[0]), int(d[1])) if isinstance(d, tuple) else (_ptr(d), int(d.shape[0]))

    def observe_pairs_rc(self, desc0, desc1, pairs, lm_out, first_new: int) -> int:
        """gfpl_lmstore_observe_pairs' return code."""
        import torch
        (d0, n0), (d1, n1) = self._rows(desc0), self._rows(desc1)
        p, n, _kp = self._list(pairs, 2)
        out, n_out, _ko = self._list(lm_out)
        if n_out != n:
            raise ValueError(f"observe_pairs: {n} pairs, {n_out} lm_out entries")
        torch.cuda.synchronize()
        return self.L.gfpl_lmstore_observe_pairs(self.h, d0, n0, d1, n1, p, out, n, int(first_new))

    def observe_pairs(self, desc0, desc1, pairs, lm_out, first_new: int) -> None:
        """The descriptor half of the keyframe-pair stage: pairs / lm_out / first_new as KeyframeMap.observe_pairs
        took and returned them, desc0 / desc1 the two keyframes' descriptor rows."""
        check(self.observe_pairs_rc(desc0, desc1, pairs, lm_out, first_new), "lmstore_observe_pairs")

    def observe_local_rc(self, desc1, pairs, unm_rows, lm_out) -> int:
        import torch
        d1, n1 = self._rows(desc1)
        p, n, _kp = self._list(pairs, 2)
        unm, n_unm, _ku = self._list(unm_rows)
        out, n_out, _ko = self._list(lm_out)
        if n_out != n:
            raise ValueError(f"observe_local: {n} pairs, {n_out} lm_out entries")
        torch.cuda.synchronize()
        return self.L.gfpl_lmstore_observe_local(self.h, d1, n1, p, n, unm, n_unm, out)

    def observe_local(self, desc1, pairs, unm_rows, lm_out) -> None:
        """The local-map stage: landmark lm_out[i] receives row unm_rows[pairs[i][1]] of desc1."""
        check(self.observe_local_rc(desc1, pairs, unm_rows, lm_out), "lmstore_observe_local")

    def free_rc(self, ids) -> int:
        import torch
        t, n, _k = self._list(ids)
        torch.cuda.synchronize()
        return self.L.gfpl_lmstore_free_ids(self.h, t, n)

    def free(self, ids) -> None:
        """GFPL_LM_FREE of every listed id (KeyframeMap.remove_bad's device list)."""
        check(self.free_rc(ids), "lmstore_free_ids")

    def gather_ids(self, ids, n: Optional[int] = None, with_idx: bool = False):
        """gather() with the id list on the device (KeyframeMap.select's tensor); n: the first n ids only."""
        import torch
        t, rows, _k = self._list(ids)
        n = rows if n is None else int(n)
        if not 0 <= n <= rows:
            raise ValueError(f"gather_ids: n = {n} of {rows} ids")
        dev = torch.device("cuda", self.ctx.device)
        out = torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=dev)
        idx = torch.full((max(n, 1),), -2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        check(self.L.gfpl_lmstore_gather_ids(self.h, t, n, _ptr(out), _ptr(idx)), "lmstore_gather_ids")
        return (out[:n], idx[:n]) if with_idx else out[:n]

    def counts(self) -> np.ndarray:
        """every landmark's count as the device holds it [lm_cap]"""
        cnt = np.zeros(self.lm_cap, np.int32)
        check(self.L.gfpl_lmstore_counts(self.h, _ptr(cnt)), "lmstore_counts")
        return cnt

    def read(self, lm: int) -> dict:
        """count, med_idx, desc_list [obs_cap][32] (rows at and past count are whatever the store
        last held there) and med_desc [32] of one landmark."""
        cnt, mi = C.c_int32(0), C.c_int32(0)
        rows = np.zeros((self.obs_cap, 32), np.uint8)
        med = np.zeros(32, np.uint8)
        check(self.L.gfpl_lmstore_read(self.h, int(lm), C.byref(cnt), C.byref(mi), _ptr(rows), _ptr(med)), "lmstore_read")
        return dict(count=cnt.value, med_idx=mi.value, desc_list=rows, med_desc=med)

    def nbytes(self) -> int:
        return int(self.L.gfpl_lmstore_bytes(self.h))

    def last_device_ms(self) -> float:
        """gfpl_lmstore_debug_ms: device time of the last apply's or gather's kernels."""
        ms = C.c_float(0.0)
        check(self.L.gfpl_lmstore_debug_ms(self.h, C.byref(ms)), "lmstore_debug_ms")
        return float(ms.value)

    def close(self):
        if getattr(self, "h", None):
            check(self.L.gfpl_lmstore_destroy(self.h), "lmstore_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KFMAP_TILE = 2048                                         # GFPL_KFMAP_TILE
KFMAP_LOCAL, KFMAP_LOCAL_UNSEEN, KFMAP_ALIVE = 0, 1, 2    # GFPL_KFMAP_*
KFMAP_POINTS, KFMAP_LINES = 0, 1


class KfMapCaps(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("kf_cap", "pt_rows", "ls_rows", "pt_lm_cap", "ls_lm_cap", "obs_cap")]


class KfMapParams(C.Structure):
    """gfpl_kfmap_params: Config::minLMCovGraph, minKFLocalMap, minLMObs and removeBadMapLandmarks' literal 10."""
    _fields_ = [(k, C.c_int32) for k in ("min_lm_cov_graph", "min_kf_local_map", "min_lm_obs", "cull_age")]

    @classmethod
    def default(cls, **over) -> "KfMapParams":
        p = cls()
        hiplib().gfpl_default_kfmap_params(C.byref(p))
        for k, v in over.items():
            setattr(p, k, v)
        return p


class KfMapKf(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("alive", "local", "n_pt", "n_ls")]


def kfmap_bytes(caps: KfMapCaps) -> int:
    """gfpl_kfmap_bytes (host only): device bytes of an object with these caps, -1 for caps it refuses."""
    return int(hiplib().gfpl_kfmap_bytes(C.byref(caps)))


class KeyframeMap:
    """gfpl_kfmap: the index half of one map on the device (the features' idx of every keyframe,
    kf_obs_list and owner of every landmark, full_graph, the local flags) with MapHandler's operations
    on it.  Device lists go in and come out as torch int32 tensors; the *_rc methods return the C
    code, the others raise GfplError.  The context cannot be closed while the map is open."""

    def __init__(self, ctx: "Context", kf_cap: int, pt_rows: int, ls_rows: int, pt_lm_cap: int, ls_lm_cap: int, obs_cap: int):
        self.ctx, self.L = ctx, ctx.L
        self.caps = KfMapCaps(kf_cap, pt_rows, ls_rows, pt_lm_cap, ls_lm_cap, obs_cap)
        self.h = C.c_void_p()
        check(self.L.gfpl_kfmap_create(ctx.h, C.byref(self.caps), C.byref(self.h)), "kfmap_create")

    def _dev(self):
        import torch
        return torch.device("cuda", self.ctx.device)

    def _out(self, n: int):
        import torch
        t = torch.full((max(int(n), 1),), -7, dtype=torch.int32, device=self._dev())
        torch.cuda.synchronize()
        return t

    def _in(self, a, cols: int = 0):
        """a device int32 tensor of the list (tensors pass through), synchronised before the C call"""
        import torch
        if not isinstance(a, torch.Tensor):
            a = np.ascontiguousarray(a, np.int32)
            a = a.reshape(-1, cols) if cols else a.reshape(-1)
            a = torch.from_numpy(a.copy()).to(self._dev())
        torch.cuda.synchronize()
        return a

    def counts(self):
        """(n_kf, next point id, next line id)"""
        v = [C.c_int32(0) for _ in range(3)]
        check(self.L.gfpl_kfmap_counts(self.h, *[C.byref(x) for x in v]), "kfmap_counts")
        return tuple(x.value for x in v)

    def add_keyframe_rc(self, n_pt: int, n_ls: int):
        kf = C.c_int32(-1)
        rc = self.L.gfpl_kfmap_add_keyframe(self.h, int(n_pt), int(n_ls), C.byref(kf))
        return rc, kf.value

    def add_keyframe(self, n_pt: int, n_ls: int) -> int:
        rc, kf = self.add_keyframe_rc(n_pt, n_ls)
        check(rc, "kfmap_add_keyframe")
        return kf

    def observe_pairs_rc(self, kind: int, kf0: int, kf1: int, pairs):
        """(code, lm_out tensor [n], first_new, n_new)"""
        p = self._in(pairs, 2)
        n = int(p.shape[0])
        out = self._out(n)
        first, new = C.c_int32(-1), C.c_int32(-1)
        rc = self.L.gfpl_kfmap_observe_pairs(self.h, int(kind), int(kf0), int(kf1), _ptr(p), n, _ptr(out),
                                             C.byref(first), C.byref(new))
        return rc, out[:n], first.value, new.value

    def observe_pairs(self, kind: int, kf0: int, kf1: int, pairs):
        rc, out, first, new = self.observe_pairs_rc(kind, kf0, kf1, pairs)
        check(rc, "kfmap_observe_pairs")
        return out, first, new

    def observe_local_rc(self, kind: int, kf1: int, pairs, sel_ids, unm_rows):
        """(code, lm_out tensor [n])"""
        p, sel, unm = self._in(pairs, 2), self._in(sel_ids), self._in(unm_rows)
        n = int(p.shape[0])
        out = self._out(n)
        rc = self.L.gfpl_kfmap_observe_local(self.h, int(kind), int(kf1), _ptr(p), n, _ptr(sel), int(sel.shape[0]),
                                             _ptr(unm), int(unm.shape[0]), _ptr(out))
        return rc, out[:n]

    def observe_local(self, kind: int, kf1: int, pairs, sel_ids, unm_rows):
        rc, out = self.observe_local_rc(kind, kf1, pairs, sel_ids, unm_rows)
        check(rc, "kfmap_observe_local")
        return out

    def form_local_map(self, params: Optional[KfMapParams] = None) -> None:
        prm = params if params is not None else KfMapParams.default()
        check(self.L.gfpl_kfmap_form_local_map(self.h, C.byref(prm)), "kfmap_form_local_map")

    def select(self, kind: int, which: int, kf1: int = 0):
        """device tensor of the selected landmark ids, in map order"""
        out = self._out(self.counts()[1 + int(kind)] if kind in (0, 1) else 0)
        n = C.c_int32(-1)
        check(self.L.gfpl_kfmap_select(self.h, int(kind), int(which), int(kf1), _ptr(out), C.byref(n)), "kfmap_select")
        return out[: n.value]

    def unmatched(self, kind: int, kf: int):
        """device tensor of kf's rows without a landmark, in row order"""
        out = self._out(self.caps.ls_rows if kind else self.caps.pt_rows)
        n = C.c_int32(-1)
        check(self.L.gfpl_kfmap_unmatched(self.h, int(kind), int(kf), _ptr(out), C.byref(n)), "kfmap_unmatched")
        return out[: n.value]

    def local_keyframes(self) -> np.ndarray:
        out = np.zeros(self.caps.kf_cap, np.int32)
        n = C.c_int32(-1)
        check(self.L.gfpl_kfmap_local_keyframes(self.h, _ptr(out), C.byref(n)), "kfmap_local_keyframes")
        return out[: n.value]

    def remove_bad(self, params: Optional[KfMapParams] = None):
        """(removed point ids, removed line ids): device tensors in map order"""
        prm = params if params is not None else KfMapParams.default()
        _, npt, nls = self.counts()
        pt, ls = self._out(npt), self._out(nls)
        a, b = C.c_int32(-1), C.c_int32(-1)
        check(self.L.gfpl_kfmap_remove_bad(self.h, C.byref(prm), _ptr(pt), C.byref(a), _ptr(ls), C.byref(b)), "kfmap_remove_bad")
        return pt[: a.value], ls[: b.value]

    def set_inlier_rc(self, kind: int, ids, value: int) -> int:
        t = self._in(ids)
        return self.L.gfpl_kfmap_set_inlier(self.h, int(kind), _ptr(t), int(t.shape[0]), int(value))

    def set_inlier(self, kind: int, ids, value: int) -> None:
        check(self.set_inlier_rc(kind, ids, value), "kfmap_set_inlier")

    def erase_keyframe_rc(self, kf: int) -> int:
        return self.L.gfpl_kfmap_erase_keyframe(self.h, int(kf))

    def erase_keyframe(self, kf: int) -> None:
        check(self.erase_keyframe_rc(kf), "kfmap_erase_keyframe")

    def read_keyframe(self, kf: int) -> dict:
        """alive, local, and the features' idx of the rows in use"""
        rec = KfMapKf()
        pt, ls = np.zeros(self.caps.pt_rows, np.int32), np.zeros(self.caps.ls_rows, np.int32)
        check(self.L.gfpl_kfmap_read_keyframe(self.h, int(kf), C.byref(rec), _ptr(pt), _ptr(ls)), "kfmap_read_keyframe")
        return dict(alive=rec.alive, local=rec.local, pt_idx=pt[: rec.n_pt], ls_idx=ls[: rec.n_ls])

    def write_keyframe_idx_rc(self, kind: int, kf: int, row0: int, idx) -> int:
        a = np.ascontiguousarray(idx, np.int32).reshape(-1)
        return self.L.gfpl_kfmap_write_keyframe_idx(self.h, int(kind), int(kf), int(row0), len(a), _ptr(a))

    def write_keyframe_idx(self, kind: int, kf: int, row0: int, idx) -> None:
        check(self.write_keyframe_idx_rc(kind, kf, row0, idx), "kfmap_write_keyframe_idx")

    def read_landmarks(self, kind: int, id0: int = 0, n: Optional[int] = None) -> dict:
        """alive, local, inlier, n_obs, owner [n] and kf_obs [n][obs_cap] of ids [id0, id0 + n); n: up to the next id"""
        n = self.counts()[1 + int(kind)] - id0 if n is None else int(n)
        d = dict(alive=np.zeros(n, np.uint8), local=np.zeros(n, np.uint8), inlier=np.zeros(n, np.uint8),
                 n_obs=np.zeros(n, np.int32), owner=np.zeros(n, np.int32), kf_obs=np.zeros((n, self.caps.obs_cap), np.int32))
        check(self.L.gfpl_kfmap_read_landmarks(self.h, int(kind), int(id0), n, *[_ptr(d[k]) for k in
              ("alive", "local", "inlier", "n_obs", "owner", "kf_obs")]), "kfmap_read_landmarks")
        return d

    def write_landmarks_rc(self, kind: int, id0: int, alive, local, inlier, n_obs, owner, kf_obs) -> int:
        a = [np.ascontiguousarray(v, np.uint8).reshape(-1) for v in (alive, local, inlier)]
        b = [np.ascontiguousarray(v, np.int32).reshape(-1) for v in (n_obs, owner)]
        o = np.ascontiguousarray(kf_obs, np.int32).reshape(len(a[0]), self.caps.obs_cap)
        return self.L.gfpl_kfmap_write_landmarks(self.h, int(kind), int(id0), len(a[0]), *[_ptr(v) for v in a + b + [o]])

    def write_landmarks(self, kind: int, id0: int, alive, local, inlier, n_obs, owner, kf_obs) -> None:
        check(self.write_landmarks_rc(kind, id0, alive, local, inlier, n_obs, owner, kf_obs), "kfmap_write_landmarks")

    def export_graph(self) -> dict:
        """alive, full_graph and the two ownership lists as gfpl_pgo_problem takes them (numpy)"""
        nkf, npt, nls = self.counts()
        d = dict(alive=np.zeros(nkf, np.uint8), full_graph=np.zeros((nkf, nkf), np.int32))
        for k, n in (("pt", npt), ("ls", nls)):
            d[k + "_kf_start"], d[k + "_kf_idx"] = np.zeros(nkf + 1, np.int32), np.zeros(max(n, 1), np.int32)
            d[k + "_freed"] = np.zeros(max(n, 1), np.uint8)
        check(self.L.gfpl_kfmap_export_graph(self.h, *[_ptr(d[k]) for k in (
            "alive", "full_graph", "pt_kf_start", "pt_kf_idx", "pt_freed", "ls_kf_start", "ls_kf_idx", "ls_freed")]),
            "kfmap_export_graph")
        for k, n in (("pt", npt), ("ls", nls)):
            d[k + "_kf_idx"] = d[k + "_kf_idx"][: d[k + "_kf_start"][nkf]]
            d[k + "_freed"] = d[k + "_freed"][:n]
        return d

    def nbytes(self) -> int:
        return kfmap_bytes(self.caps)

    def last_device_ms(self) -> float:
        """gfpl_kfmap_debug_ms: device time between the first and the last kernel of the last call"""
        ms = C.c_float(0.0)
        check(self.L.gfpl_kfmap_debug_ms(self.h, C.byref(ms)), "kfmap_debug_ms")
        return float(ms.value)

    def close(self):
        if getattr(self, "h", None):
            check(self.L.gfpl_kfmap_destroy(self.h), "kfmap_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MapGeoLists(C.Structure):
    """gfpl_mapgeo_lists: HOST copies of an assembled problem's four index lists."""
    _fields_ = [(k, _vp) for k in ("pt_obs_lm", "pt_obs_kf", "ls_obs_lm", "ls_obs_kf")] + [
        ("cap_pt_obs", C.c_int32), ("cap_ls_obs", C.c_int32)]


def mapgeo_bytes(caps: KfMapCaps) -> int:
    """gfpl_mapgeo_bytes (host only): device bytes of an object with these caps, -1 for caps it refuses."""
    return int(hiplib().gfpl_mapgeo_bytes(C.byref(caps)))


class MapGeoView:
    """The arrays of a gfpl_kf_view that gfpl_mapgeo reads, on the device: P / pl [n_pt][3] / [n_pt][2]
    and sP / eP / le [n_ls][3] (numpy float64 or None)."""

    def __init__(self, device, P=None, pl=None, sP=None, eP=None, le=None):
        import torch
        self.s = KFViewStruct()
        self.keep = {}
        for k, v, w in (("P", P, 3), ("pl", pl, 2), ("sP", sP, 3), ("eP", eP, 3), ("le", le, 3)):
            if v is None:
                continue
            a = np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1, w))
            self.keep[k] = torch.from_numpy(a.copy()).to(device) if len(a) else None
            setattr(self.s, k, _ptr(self.keep[k]))
            if k == "pl":
                self.s.n_pt = len(a)
            if k == "le":
                self.s.n_ls = len(a)
        torch.cuda.synchronize()


class MapGeometry:
    """gfpl_mapgeo: the geometry half of one map on the device (T_kf_w / x_kf_w of every keyframe,
    point3D / line3D, obs_list and sigma_list of every landmark), beside a KeyframeMap of the same caps
    and indexed by its ids.  Views are MapGeoView or KeyFrameView objects with device arrays; device
    lists are torch int32 tensors; the *_rc methods return the C code, the others raise GfplError."""

    LM_W, OBS_W = (3, 6), (2, 3)

    def __init__(self, ctx: "Context", kf_cap: int, pt_rows: int, ls_rows: int, pt_lm_cap: int, ls_lm_cap: int, obs_cap: int):
        self.ctx, self.L = ctx, ctx.L
        self.caps = KfMapCaps(kf_cap, pt_rows, ls_rows, pt_lm_cap, ls_lm_cap, obs_cap)
        self.h = C.c_void_p()
        check(self.L.gfpl_mapgeo_create(ctx.h, C.byref(self.caps), C.byref(self.h)), "mapgeo_create")

    def _dev(self):
        import torch
        return torch.device("cuda", self.ctx.device)

    def _in(self, a, cols: int = 0):
        import torch
        if not isinstance(a, torch.Tensor):
            a = np.ascontiguousarray(a, np.int32)
            a = a.reshape(-1, cols) if cols else a.reshape(-1)
            a = torch.from_numpy(a.copy()).to(self._dev())
        torch.cuda.synchronize()
        return a

    def view(self, **arrays) -> MapGeoView:
        return MapGeoView(self._dev(), **arrays)

    def set_keyframe_rc(self, kf: int, T_kf_w, x_kf_w) -> int:
        T = np.ascontiguousarray(np.asarray(T_kf_w, np.float64).reshape(16))
        x = np.ascontiguousarray(np.asarray(x_kf_w, np.float64).reshape(6))
        return self.L.gfpl_mapgeo_set_keyframe(self.h, int(kf), _ptr(T), _ptr(x))

    def set_keyframe(self, kf: int, T_kf_w, x_kf_w) -> None:
        check(self.set_keyframe_rc(kf, T_kf_w, x_kf_w), "mapgeo_set_keyframe")

    def read_keyframe(self, kf: int):
        """(T_kf_w [4][4], x_kf_w [6])"""
        T, x = np.zeros(16), np.zeros(6)
        check(self.L.gfpl_mapgeo_read_keyframe(self.h, int(kf), _ptr(T), _ptr(x)), "mapgeo_read_keyframe")
        return T.reshape(4, 4), x

    def arrays(self) -> dict:
        """the device addresses of T_kf, x_kf, point3D, line3D (ints)"""
        v = [C.c_void_p() for _ in range(4)]
        check(self.L.gfpl_mapgeo_arrays(self.h, *[C.byref(x) for x in v]), "mapgeo_arrays")
        return dict(zip(("T_kf", "x_kf", "point3D", "line3D"), [x.value for x in v]))

    def observe_pairs_rc(self, kind: int, kf0: int, kf1: int, v0, v1, pairs, lm_out, first_new: int) -> int:
        p, out = self._in(pairs, 2), self._in(lm_out)
        return self.L.gfpl_mapgeo_observe_pairs(self.h, int(kind), int(kf0), int(kf1), C.byref(v0.s), C.byref(v1.s), _ptr(p),
                                                _ptr(out), int(p.shape[0]), int(first_new))

    def observe_pairs(self, kind: int, kf0: int, kf1: int, v0, v1, pairs, lm_out, first_new: int) -> None:
        check(self.observe_pairs_rc(kind, kf0, kf1, v0, v1, pairs, lm_out, first_new), "mapgeo_observe_pairs")

    def observe_local_rc(self, kind: int, kf1: int, v1, pairs, unm_rows, lm_out) -> int:
        p, unm, out = self._in(pairs, 2), self._in(unm_rows), self._in(lm_out)
        return self.L.gfpl_mapgeo_observe_local(self.h, int(kind), int(kf1), C.byref(v1.s), _ptr(p), int(p.shape[0]), _ptr(unm),
                                                int(unm.shape[0]), _ptr(out))

    def observe_local(self, kind: int, kf1: int, v1, pairs, unm_rows, lm_out) -> None:
        check(self.observe_local_rc(kind, kf1, v1, pairs, unm_rows, lm_out), "mapgeo_observe_local")

    def free_rc(self, kind: int, ids) -> int:
        t = self._in(ids)
        return self.L.gfpl_mapgeo_free(self.h, int(kind), _ptr(t), int(t.shape[0]))

    def free(self, kind: int, ids) -> None:
        check(self.free_rc(kind, ids), "mapgeo_free")

    def read_landmarks(self, kind: int, id0: int, n: int) -> dict:
        """lm3d [n][3 or 6], n_obs [n], obs [n][obs_cap][2 or 3], sigma [n][obs_cap]"""
        oc = self.caps.obs_cap
        d = dict(lm3d=np.zeros((n, self.LM_W[kind])), n_obs=np.zeros(n, np.int32), obs=np.zeros((n, oc, self.OBS_W[kind])),
                 sigma=np.zeros((n, oc)))
        check(self.L.gfpl_mapgeo_read_landmarks(self.h, int(kind), int(id0), int(n), *[_ptr(d[k]) for k in
              ("lm3d", "n_obs", "obs", "sigma")]), "mapgeo_read_landmarks")
        return d

    def write_landmarks_rc(self, kind: int, id0: int, lm3d, n_obs, obs, sigma) -> int:
        c = np.ascontiguousarray(n_obs, np.int32).reshape(-1)
        n, oc = len(c), self.caps.obs_cap
        a = np.ascontiguousarray(np.asarray(lm3d, np.float64).reshape(n, self.LM_W[kind]))
        o = np.ascontiguousarray(np.asarray(obs, np.float64).reshape(n, oc, self.OBS_W[kind]))
        s = np.ascontiguousarray(np.asarray(sigma, np.float64).reshape(n, oc))
        return self.L.gfpl_mapgeo_write_landmarks(self.h, int(kind), int(id0), n, _ptr(a), _ptr(c), _ptr(o), _ptr(s))

    def write_landmarks(self, kind: int, id0: int, lm3d, n_obs, obs, sigma) -> None:
        check(self.write_landmarks_rc(kind, id0, lm3d, n_obs, obs, sigma), "mapgeo_write_landmarks")

    def assemble_rc(self, kfmap: "KeyframeMap", which: int, host_lists: bool = True):
        """(code, LbaProblemStruct, lists): the struct's doubles are the object's device buffers; with
        host_lists the index lists are numpy arrays (kept in `lists`) cut to the counts."""
        p = LbaProblemStruct()
        oc = self.caps.obs_cap
        keep = None
        if host_lists:
            cp, cl = self.caps.pt_lm_cap * oc, self.caps.ls_lm_cap * oc
            keep = dict(pt_obs_lm=np.full(cp, -9, np.int32), pt_obs_kf=np.full(cp, -9, np.int32),
                        ls_obs_lm=np.full(cl, -9, np.int32), ls_obs_kf=np.full(cl, -9, np.int32))
            ls = MapGeoLists(*[_ptr(keep[k]) for k in LBA_INDICES], cp, cl)
        rc = self.L.gfpl_mapgeo_assemble(self.h, kfmap.h, int(which), C.byref(p), C.byref(ls) if host_lists else None)
        if rc == 0 and host_lists:
            keep = {k: v[: (p.n.n_pt_obs if k.startswith("pt") else p.n.n_ls_obs)] for k, v in keep.items()}
        return rc, p, keep

    def assemble(self, kfmap: "KeyframeMap", which: int, host_lists: bool = True):
        rc, p, keep = self.assemble_rc(kfmap, which, host_lists)
        check(rc, "mapgeo_assemble")
        return p, keep

    def read_assembled(self, p: LbaProblemStruct) -> dict:
        """gfpl_mapgeo_read_assembled: the last assembly's doubles (x_kf ... ls_sigma) and id lists
        (kf_list, fix_list, pt_list, ls_list) as numpy arrays of p's counts"""
        n = p.n
        h = LbaProblemStruct()
        out = {}
        for k, w, cnt in (("x_kf", 6, n.n_kf), ("T_kf", 16, n.n_kf), ("T_fix", 16, n.n_fix), ("pt", 3, n.n_pt), ("ls", 6, n.n_ls),
                          ("pt_obs", 2, n.n_pt_obs), ("pt_sigma", 1, n.n_pt_obs), ("ls_obs", 3, n.n_ls_obs), ("ls_sigma", 1, n.n_ls_obs)):
            out[k] = np.zeros((cnt, w))
            setattr(h, k, _ptr(out[k]) if cnt else None)
        ids = {k: np.zeros(max(cnt, 1), np.int32) for k, cnt in
               (("kf_list", n.n_kf), ("fix_list", n.n_fix), ("pt_list", n.n_pt), ("ls_list", n.n_ls))}
        check(self.L.gfpl_mapgeo_read_assembled(self.h, C.byref(h), *[_ptr(v) for v in ids.values()]), "mapgeo_read_assembled")
        for k, cnt in (("kf_list", n.n_kf), ("fix_list", n.n_fix), ("pt_list", n.n_pt), ("ls_list", n.n_ls)):
            out[k] = ids[k][:cnt]
        return out

    def lba_rc(self, kfmap: "KeyframeMap", solver: "LbaSolver", params: Optional[LbaParams] = None):
        """(code, LbaResult, LbaCounts): gfpl_mapgeo_lba on an open LbaSolver of the same context"""
        prm = params if params is not None else LbaParams.default()
        res, cnt = LbaResult(), LbaCounts()
        rc = self.L.gfpl_mapgeo_lba(self.h, kfmap.h, solver.h, C.byref(prm), C.byref(res), C.byref(cnt))
        return rc, res, cnt

    def lba(self, kfmap: "KeyframeMap", solver: "LbaSolver", params: Optional[LbaParams] = None):
        rc, res, cnt = self.lba_rc(kfmap, solver, params)
        check(rc, "mapgeo_lba")
        return res, cnt

    def nbytes(self) -> int:
        return mapgeo_bytes(self.caps)

    def last_device_ms(self) -> float:
        ms = C.c_float(0.0)
        check(self.L.gfpl_mapgeo_debug_ms(self.h, C.byref(ms)), "mapgeo_debug_ms")
        return float(ms.value)

    def close(self):
        if getattr(self, "h", None):
            check(self.L.gfpl_mapgeo_destroy(self.h), "mapgeo_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StereoFrameHandler:
    """B independent StVO::StereoFrameHandler objects resident on one GPU.

    Method names follow include/stereoFrameHandler.h:38-174."""

    def __init__(self, ctx: Context, batch: int, kp_cap: int, kl_cap: int):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        check(self.L.gfpl_seqbatch_create(ctx.h, batch, kp_cap, kl_cap, C.byref(h)), "seqbatch_create")
        self.h = h
        self.B, self.kp_cap, self.kl_cap = batch, kp_cap, kl_cap

    def initialize(self, fr: Frames):
        check(self.L.gfpl_initialize(self.h, C.byref(fr)), "initialize")

    def insertStereoPair(self, fr: Frames):
        check(self.L.gfpl_insert_stereo_pair(self.h, C.byref(fr)), "insert_stereo_pair")

    def optimizePose(self, DT_ini=None):
        """optimizePose(prev_frame->DT) (the app's call, Q2), or optimizePose(Matrix4d DT_ini)
        with DT_ini a 4x4 (all sequences) or [B,4,4] host array."""
        if DT_ini is None:
            check(self.L.gfpl_optimize_pose(self.h), "optimize_pose")
            return
        d = np.asarray(DT_ini, dtype=np.float64)
        d = np.ascontiguousarray(np.broadcast_to(d.reshape(-1, 4, 4), (self.B, 4, 4)))
        check(self.L.gfpl_optimize_pose_ini(self.h, d.ctypes.data), "optimize_pose_ini")

    def updateFrame(self):
        check(self.L.gfpl_update_frame(self.h), "update_frame")

    def frameStep(self, fr: Frames):
        check(self.L.gfpl_frame_step(self.h, C.byref(fr)), "frame_step")

    # stage entry points
    def stereoPoints(self, fr: Frames):
        check(self.L.gfpl_stereo_points(self.h, C.byref(fr)), "stereo_points")

    def stereoLines(self, fr: Frames):
        check(self.L.gfpl_stereo_lines(self.h, C.byref(fr)), "stereo_lines")

    def estimateStereoUncertainty(self):
        check(self.L.gfpl_line_uncertainty(self.h), "line_uncertainty")

    def crossFrameMatchingPoints(self):
        check(self.L.gfpl_cross_points(self.h), "cross_points")

    def crossFrameMatchingLines(self):
        check(self.L.gfpl_cross_lines(self.h), "cross_lines")

    def estimateProjUncertainty_submodular(self):
        check(self.L.gfpl_line_cut(self.h), "line_cut")

    # state transfer
    def upload_frames(self, host: Frames) -> Frames:
        """gfpl_upload_frames: copy one batch of HOST input frames into the seqbatch's
        device staging area (synchronous, PCIe) and return its device view."""
        dev = Frames()
        check(self.L.gfpl_upload_frames(self.h, C.byref(host), C.byref(dev)), "upload_frames")
        dev._keep = [host]
        return dev

    def upload_async(self, host: Frames, s0: int, slot: int, l0_stride: int = 0) -> int:
        """gfpl_upload_frames_async: enqueue the copy of host.batch sequences of HOST frames
        into sequences [s0, s0 + host.batch) of staging buffer `slot` on the seqbatch's copy
        stream; returns the ticket for upload_wait (host memory untouched until then).
        l0_stride > 0 (gfpl_upload_frames_l0_async): only level 0 of each right pyramid is
        copied (rows l0_stride bytes apart) and the device builds levels 1.. from it."""
        t = C.c_int64()
        if l0_stride > 0:
            check(self.L.gfpl_upload_frames_l0_async(self.h, C.byref(host), s0, slot, l0_stride, C.byref(t)),
                  "upload_frames_l0_async")
        else:
            check(self.L.gfpl_upload_frames_async(self.h, C.byref(host), s0, slot, C.byref(t)), "upload_frames_async")
        return t.value

    def upload_wait(self, ticket: int):
        check(self.L.gfpl_upload_wait(self.h, ticket), "upload_wait")

    def staged_frames(self, slot: int) -> Frames:
        """Device view of staging buffer `slot` (every tracker call reading it waits for its copies)."""
        dev = Frames()
        check(self.L.gfpl_staged_frames(self.h, slot, C.byref(dev)), "staged_frames")
        return dev

    def read_frame(self, which: int, seq: int) -> FrameHost:
        fh = FrameHost(self.kp_cap, self.kl_cap)
        check(self.L.gfpl_read_frame(self.h, which, seq, fh.ptr()), "read_frame")
        return fh

    def write_frame(self, which: int, seq: int, fh: FrameHost):
        check(self.L.gfpl_write_frame(self.h, which, seq, fh.ptr()), "write_frame")

    def read_track(self, seq: int) -> dict:
        t = TrackHost()
        check(self.L.gfpl_read_track(self.h, seq, C.byref(t)), "read_track")
        return t.as_dict()

    def read_last_track(self, seq: int) -> dict:
        """The track of the step before the last updateFrame / frameStep: the matched lists
        it cleared and the inlier counters (gfpl_read_last_track)."""
        t = TrackHost()
        check(self.L.gfpl_read_last_track(self.h, seq, C.byref(t)), "read_last_track")
        return t.as_dict()

    # keyframe decision (src/stereoFrameHandler.cpp:2309-2379)
    def needNewKF(self) -> np.ndarray:
        """needNewKF() of every sequence; returns the [B] decisions (bool)."""
        flags = np.zeros(self.B, np.int32)
        check(self.L.gfpl_need_new_kf(self.h, flags.ctypes.data), "need_new_kf")
        return flags.astype(bool)

    def currFrameIsKF(self, mask=None):
        """currFrameIsKF() for the sequences where mask is true (None: the last
        needNewKF decisions)."""
        if mask is None:
            check(self.L.gfpl_curr_frame_is_kf(self.h, None), "curr_frame_is_kf")
            return
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(mask), (self.B,)), dtype=np.int32)
        check(self.L.gfpl_curr_frame_is_kf(self.h, m.ctypes.data), "curr_frame_is_kf")

    def read_kf_state(self, seq: int) -> dict:
        st = KFState()
        check(self.L.gfpl_read_kf_state(self.h, seq, C.byref(st)), "read_kf_state")
        return st.as_dict()

    def write_track(self, seq: int, tr: TrackHost):
        check(self.L.gfpl_write_track(self.h, seq, C.byref(tr)), "write_track")

    def last_step_bytes(self) -> int:
        v = C.c_int64()
        check(self.L.gfpl_last_step_bytes(self.h, C.byref(v)), "last_step_bytes")
        return v.value

    def last_step_stage_bytes(self) -> np.ndarray:
        v = np.zeros(7, np.int64)
        check(self.L.gfpl_last_step_stage_bytes(self.h, v.ctypes.data), "last_step_stage_bytes")
        return v

    STEP_COUNTS = ["N_o", "N_k", "M_o", "S_p", "S_l", "M_p", "M_l", "n_inliers"]

    def last_step_counts(self) -> dict:
        """Per-sequence means of the counts the last step's bytes are priced on
        (gfpl_last_step_counts): keypoints / keylines (both sides), SAD keypoints,
        stereo points / lines of the new frame, matched points / lines, inliers."""
        v = np.zeros(8, np.int64)
        check(self.L.gfpl_last_step_counts(self.h, v.ctypes.data), "last_step_counts")
        return {n: float(x) / self.B for n, x in zip(self.STEP_COUNTS, v)}

    def last_step_track_counts(self) -> dict:
        """The last step, summed over the batch (gfpl_last_step_track_counts): line-cut greedy
        steps, those the certified search evaluated exactly, and the inliers
        left after optimize_pose."""
        v = np.zeros(4, np.int64)
        check(self.L.gfpl_last_step_track_counts(self.h, v.ctypes.data), "last_step_track_counts")
        return {"steps": int(v[0]), "exact_steps": int(v[1]), "inliers_after_pose": int(v[2]),
                "lines_unbounded": int(v[3])}

    def last_step_cut_proof(self) -> dict:
        """Proven line cut (cut_proof 1) of the last step, summed over the batch
        (gfpl_last_step_cut_proof): sequences redone by the eager-proven search because the
        recorded search could not be proven, margined steps proven, reference variances
        evaluated, lines with margined steps."""
        v = np.zeros(4, np.int64)
        check(self.L.gfpl_last_step_cut_proof(self.h, v.ctypes.data), "last_step_cut_proof")
        return {"redone": int(v[0]), "steps_proven": int(v[1]), "vref_evals": int(v[2]), "lines": int(v[3])}

    def debug_cut_records(self, b: int, n_lines: int) -> np.ndarray:
        """gfpl_debug_cut_records: sequence b's line-cut records [n_lines][80] (float64)."""
        out = np.zeros((n_lines, 80), np.float64)
        check(self.L.gfpl_debug_cut_records(self.h, b, out.ctypes.data, n_lines), "debug_cut_records")
        return out

    def debug_step_records(self) -> np.ndarray:
        """gfpl_debug_step_records: every sequence's record of the last step [B][STEP_REC] (int64),
        columns StepSlot."""
        out = np.zeros((self.B, STEP_REC), np.int64)
        check(self.L.gfpl_debug_step_records(self.h, out.ctypes.data), "debug_step_records")
        return out

    def debug_clocks(self) -> np.ndarray:
        """gfpl_debug_clocks: per-sequence debug slots [B][8] (int64): the instrumented builds' clocks;
        in the product build slots 6 / 7 hold the measured-mode line-cut wave's HW_ID / XCC_ID, and with
        cut_with_max_vol = 0 slots 0 / 1 the search's Jacobi sweeps that rotated / metric evaluations."""
        out = np.zeros((self.B, 8), np.int64)
        check(self.L.gfpl_debug_clocks(self.h, out.ctypes.data), "debug_clocks")
        return out

    def last_step_kernel_bytes(self) -> np.ndarray:
        v = np.zeros(4, np.int64)
        check(self.L.gfpl_last_step_kernel_bytes(self.h, v.ctypes.data), "last_step_kernel_bytes")
        return v

    def nbytes(self) -> int:
        return int(self.L.gfpl_seqbatch_bytes(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_seqbatch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def track_from_dict(d: dict) -> TrackHost:
    t = TrackHost()
    t.n_matched_pt = len(d["matched_pt"])
    t.n_matched_ls = len(d["matched_ls"])
    for i, v in enumerate(d["matched_pt"]):
        t.matched_pt[i] = int(v)
    for i, v in enumerate(d["matched_ls"]):
        t.matched_ls[i] = int(v)
    t.n_inliers, t.n_inliers_pt, t.n_inliers_ls = d["n_inliers"], d["n_inliers_pt"], d["n_inliers_ls"]
    t.num_frame_loss = d["num_frame_loss"]
    return t


class ORBextractor:
    """ORB_SLAM2::ORBextractor on the GPU (include/ORBextractor.h:49-106; constructor
    src/ORBextractor.cc:410-470, operator() :1043-1105), as StereoFrame builds it
    (src/stereoFrame.cpp:33-36).  One extractor serves images of one size; __call__
    takes one host image like the reference's operator(), extract() a batch of images
    already on the device (the product path's form).

    ctx: a Context (its device and stream), or None for a bare context on `device`."""

    def __init__(self, nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int, minThFAST: int,
                 width: int, height: int, max_images: int = 1, kp_cap: Optional[int] = None,
                 ctx: Optional[Context] = None, device: int = 0):
        self.L = hiplib()
        self.prm = OrbParams(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
        self.width, self.height, self.max_images = width, height, max_images
        self.kp_cap = kp_cap or nfeatures + 64 * nlevels + 64
        self._own = None
        if ctx is None:
            h = C.c_void_p()
            check(self.L.gfpl_create(device, None, C.byref(h)), "gfpl_create")
            self._own = h
            ch = h
        else:
            ch = ctx.h
        self._ctx = ctx
        o = C.c_void_p()
        check(self.L.gfpl_orb_create(ch, width, height, C.byref(self.prm), max_images, self.kp_cap, C.byref(o)),
              "orb_create")
        self.h = o
        b = C.c_int64()
        check(self.L.gfpl_orb_pyramid_bytes(o, C.byref(b)), "orb_pyramid_bytes")
        self.pyramid_bytes = b.value
        # ORBextractor tables (:414-431)
        sc = [1.0]
        for _ in range(1, nlevels):
            sc.append(float(np.float32(sc[-1]) * np.float32(scaleFactor)))
        self.mvScaleFactor = np.array(sc, np.float32)
        self.mvLevelSigma2 = self.mvScaleFactor * self.mvScaleFactor
        self.mvInvScaleFactor = np.float32(1.0) / self.mvScaleFactor
        self.mvInvLevelSigma2 = np.float32(1.0) / self.mvLevelSigma2
        self.mvImagePyramid = []

    # the reference's accessors (include/ORBextractor.h:65-88)
    def GetLevels(self) -> int: return self.prm.nlevels
    def GetScaleFactor(self) -> float: return float(np.float32(self.prm.scale_factor))
    def GetScaleFactors(self): return self.mvScaleFactor.copy()
    def GetInverseScaleFactors(self): return self.mvInvScaleFactor.copy()
    def GetScaleSigmaSquares(self): return self.mvLevelSigma2.copy()
    def GetInverseScaleSigmaSquares(self): return self.mvInvLevelSigma2.copy()

    def level_sizes(self):
        """(cols, rows) of every level: cvRound(W / scale), cvRound(H / scale) (:1111-1112)."""
        return [(int(np.rint(np.float32(self.width) * self.mvInvScaleFactor[l])),
                 int(np.rint(np.float32(self.height) * self.mvInvScaleFactor[l]))) for l in range(self.prm.nlevels)]

    def extract(self, images_dev, n: int, kps_dev, desc_dev, n_kp_dev, angle_dev=None, response_dev=None,
                pyramid_dev=None, pyr_stride: int = 0) -> None:
        """gfpl_orb_extract on device buffers: images [n][H][W] u8; per image i the rows
        [i*kp_cap, i*kp_cap + n_kp[i]) of kps (KEYPOINT_DT) / desc (32 B) / angle / response."""
        check(self.L.gfpl_orb_extract(self.h, _ptr(images_dev), n, _ptr(kps_dev), _ptr(desc_dev), _ptr(n_kp_dev),
                                      _ptr(angle_dev), _ptr(response_dev), _ptr(pyramid_dev), pyr_stride),
              "orb_extract")

    def extract_async(self, images_dev, n: int, kps_dev, desc_dev, n_kp_dev, angle_dev=None, response_dev=None,
                      pyramid_dev=None, pyr_stride: int = 0) -> None:
        """gfpl_orb_extract_async: enqueued on the context's stream; status() reports capacity errors."""
        check(self.L.gfpl_orb_extract_async(self.h, _ptr(images_dev), n, _ptr(kps_dev), _ptr(desc_dev),
                                            _ptr(n_kp_dev), _ptr(angle_dev), _ptr(response_dev), _ptr(pyramid_dev),
                                            pyr_stride), "orb_extract_async")

    def status(self) -> None:
        check(self.L.gfpl_orb_status(self.h), "orb_status")

    def __call__(self, image: np.ndarray):
        """operator()(image, noArray(), keypoints, descriptors) on one HOST grey image:
        returns (keypoints [CV_KEYPOINT_DT], descriptors [n][32] u8); mvImagePyramid holds
        the level images afterwards."""
        import torch
        image = np.ascontiguousarray(image, np.uint8)
        if image.shape != (self.height, self.width):
            raise ValueError(f"image {image.shape} != ({self.height}, {self.width})")
        dev = torch.device("cuda", torch.cuda.current_device())
        img = torch.from_numpy(image).to(dev)
        kc = self.kp_cap
        kps = torch.zeros(kc * KEYPOINT_DT.itemsize, dtype=torch.uint8, device=dev)
        desc = torch.zeros(kc * DESC, dtype=torch.uint8, device=dev)
        nkp = torch.zeros(1, dtype=torch.int32, device=dev)
        ang = torch.zeros(kc, dtype=torch.float32, device=dev)
        rsp = torch.zeros(kc, dtype=torch.float32, device=dev)
        pyr = torch.zeros(self.pyramid_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.extract(img, 1, kps, desc, nkp, ang, rsp, pyr, self.pyramid_bytes)
        n = int(nkp.item())
        k = kps.cpu().numpy().view(KEYPOINT_DT)[:n]
        out = np.zeros(n, CV_KEYPOINT_DT)
        out["x"], out["y"], out["octave"] = k["x"], k["y"], k["octave"]
        out["size"] = np.float32(31) * self.mvScaleFactor[k["octave"]]   # scaledPatchSize (:1090)
        out["angle"] = ang[:n].cpu().numpy()
        out["response"] = rsp[:n].cpu().numpy()
        p = pyr.cpu().numpy()
        self.mvImagePyramid, off = [], 0
        for (w, h) in self.level_sizes():
            self.mvImagePyramid.append(p[off:off + w * h].reshape(h, w).copy())
            off += w * h
        return out, desc.cpu().numpy().reshape(kc, DESC)[:n].copy()

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_orb_destroy(self.h)
            self.h = None
        if getattr(self, "_own", None):
            self.L.gfpl_destroy(self._own)
            self._own = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LSDDetector:
    """line_descriptor::LSDDetectorC on the GPU, the detect(image, keylines, scale, numOctaves,
    opts) path StereoFrame uses (3rdparty/line_descriptor/src/LSDDetector_custom.cpp:218-316,
    src/stereoFrame.cpp:1160-1186: LSD_REFINE_STD at scale 1, one octave, the min-length
    filter, the response sort + resize to Config::lsdNFeatures) for images of one size.
    detect() takes one host image like the reference; detect_batch() device buffers (the
    product path's form, writing keylines where gfpl_lbd_compute / gfpl_frames read them)."""

    def __init__(self, width: int, height: int, params: Optional["LsdParams"] = None, max_images: int = 1,
                 kl_cap: int = 512, seg_cap: int = 4096, ctx: Optional[Context] = None, device: int = 0):
        self.L = hiplib()
        self.width, self.height, self.max_images, self.kl_cap, self.seg_cap = width, height, max_images, kl_cap, seg_cap
        self.params = params if params is not None else LsdParams.reference(width, height)
        self._own = None
        if ctx is None:
            h = C.c_void_p()
            check(self.L.gfpl_create(device, None, C.byref(h)), "gfpl_create")
            self._own = h
            ch = h
        else:
            ch = ctx.h
        self._ctx = ctx
        o = C.c_void_p()
        check(self.L.gfpl_lsd_create(ch, C.byref(self.params), width, height, max_images, kl_cap, seg_cap,
                                     C.byref(o)), "lsd_create")
        self.h = o

    def detect_batch(self, images_dev, n: int, keylines_dev, n_kl_dev, response_dev=None) -> None:
        check(self.L.gfpl_lsd_detect(self.h, _ptr(images_dev), n, _ptr(keylines_dev), _ptr(n_kl_dev),
                                     _ptr(response_dev) if response_dev is not None else None), "lsd_detect")

    def detect_async(self, images_dev, n: int, keylines_dev, n_kl_dev, response_dev=None) -> None:
        """gfpl_lsd_detect_async: enqueued on the context's stream; status() reports capacity errors."""
        check(self.L.gfpl_lsd_detect_async(self.h, _ptr(images_dev), n, _ptr(keylines_dev), _ptr(n_kl_dev),
                                           _ptr(response_dev) if response_dev is not None else None), "lsd_detect_async")

    def status(self) -> None:
        check(self.L.gfpl_lsd_status(self.h), "lsd_status")

    def sort_desc(self, a_dev, n: int) -> None:
        """ledger S2 test hook: std::sort by descending high 32 bits of a device u64 array."""
        check(self.L.gfpl_lsd_sort_desc(self.h, _ptr(a_dev), n), "lsd_sort_desc")

    def detect(self, image: np.ndarray):
        """detect(image, keylines, ...) on one HOST image: (keylines KEYLINE_DT, response f32)."""
        import torch
        image = np.ascontiguousarray(image, np.uint8)
        if image.shape != (self.height, self.width):
            raise ValueError(f"image {image.shape} != ({self.height}, {self.width})")
        dev = torch.device("cuda", torch.cuda.current_device())
        d_img = torch.from_numpy(image).to(dev)
        d_kl = torch.zeros(self.kl_cap * KEYLINE_DT.itemsize, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        d_r = torch.zeros(self.kl_cap, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        self.detect_batch(d_img, 1, d_kl, d_n, d_r)
        n = int(d_n.cpu()[0])
        kl = d_kl.cpu().numpy().view(KEYLINE_DT)[:n].copy()
        return kl, d_r.cpu().numpy()[:n].copy()

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_lsd_destroy(self.h)
            self.h = None
        if getattr(self, "_own", None):
            self.L.gfpl_destroy(self._own)
            self._own = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BinaryDescriptor:
    """line_descriptor::BinaryDescriptor on the GPU, the compute() path StereoFrame uses
    (3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:539-687; computeLBD
    :1026-1372): 32-byte LBD descriptors of octave-0 keylines (Config::lsdOctaveNum = 1)
    for images of one size.  compute() takes one host image like the reference;
    compute_batch() device buffers (the product path's form)."""

    def __init__(self, width: int, height: int, max_images: int = 1, kl_cap: int = 512,
                 ctx: Optional[Context] = None, device: int = 0):
        self.L = hiplib()
        self.width, self.height, self.max_images, self.kl_cap = width, height, max_images, kl_cap
        self._own = None
        if ctx is None:
            h = C.c_void_p()
            check(self.L.gfpl_create(device, None, C.byref(h)), "gfpl_create")
            self._own = h
            ch = h
        else:
            ch = ctx.h
        self._ctx = ctx
        o = C.c_void_p()
        check(self.L.gfpl_lbd_create(ch, width, height, max_images, kl_cap, C.byref(o)), "lbd_create")
        self.h = o

    def compute_batch(self, images_dev, n: int, keylines_dev, n_kl_dev, desc_dev) -> None:
        check(self.L.gfpl_lbd_compute(self.h, _ptr(images_dev), n, _ptr(keylines_dev), _ptr(n_kl_dev),
                                      _ptr(desc_dev)), "lbd_compute")

    def compute_async(self, images_dev, n: int, keylines_dev, n_kl_dev, desc_dev) -> None:
        """gfpl_lbd_compute_async: enqueued on the context's stream; status() reports errors."""
        check(self.L.gfpl_lbd_compute_async(self.h, _ptr(images_dev), n, _ptr(keylines_dev), _ptr(n_kl_dev),
                                            _ptr(desc_dev)), "lbd_compute_async")

    def status(self) -> None:
        check(self.L.gfpl_lbd_status(self.h), "lbd_status")

    def compute(self, image: np.ndarray, keylines: np.ndarray) -> np.ndarray:
        """compute(image, keylines, descriptors) on one HOST image; keylines: KEYLINE_DT rows.
        Returns [n][32] u8."""
        import torch
        image = np.ascontiguousarray(image, np.uint8)
        if image.shape != (self.height, self.width):
            raise ValueError(f"image {image.shape} != ({self.height}, {self.width})")
        n = len(keylines)
        if n > self.kl_cap:
            raise ValueError(f"{n} keylines > kl_cap {self.kl_cap}")
        dev = torch.device("cuda", torch.cuda.current_device())
        kl = np.zeros(self.kl_cap, KEYLINE_DT)
        kl[:n] = keylines
        d_img = torch.from_numpy(image).to(dev)
        d_kl = torch.from_numpy(kl.view(np.uint8)).to(dev)
        d_n = torch.tensor([n], dtype=torch.int32, device=dev)
        d_desc = torch.zeros(self.kl_cap * DESC, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.compute_batch(d_img, 1, d_kl, d_n, d_desc)
        return d_desc.cpu().numpy().reshape(self.kl_cap, DESC)[:n].copy()

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_lbd_destroy(self.h)
            self.h = None
        if getattr(self, "_own", None):
            self.L.gfpl_destroy(self._own)
            self._own = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rectify_maps(side: RectifySide, width: int, height: int):
    """gfpl_rectify_maps_host: the CV_16SC2 + CV_16UC1 maps of one camera, built on the host
    (no device needed).  Returns (map1 int16 [H][W][2] (x, y), map2 uint16 [H][W])."""
    if width < 1 or height < 1:
        raise GfplError(-1, "rectify_maps_host")
    map1 = np.zeros((height, width, 2), np.int16)
    map2 = np.zeros((height, width), np.uint16)
    check(hiplib().gfpl_rectify_maps_host(C.byref(side), width, height, map1.ctypes.data, map2.ctypes.data),
          "rectify_maps_host")
    return map1, map2


class StereoRectifier:
    """gfpl_rectifier: PinholeStereoCamera::rectifyImage / rectifyImagesLR
    (src/pinholeStereoCamera.cpp:96-119) for batches of 8-bit images on the device: the maps of
    both cameras are built on the host (ledger R1-R5) and uploaded once; rectify() is
    cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) with them (R6), enqueued on the context's stream."""

    def __init__(self, left: RectifySide, right: RectifySide, width: int, height: int, ctx: Context):
        self.L = ctx.L
        self.ctx, self.width, self.height = ctx, width, height
        self.left, self.right = left, right
        h = C.c_void_p()
        check(self.L.gfpl_rectifier_create(ctx.h, C.byref(left), C.byref(right), width, height, C.byref(h)),
              "rectifier_create")
        self.h = h

    def rectify(self, side: int, src, n: int, out, sync: bool = False) -> None:
        """src / out: device u8 [n][H][W] (distinct buffers); side 0 = left, 1 = right"""
        f = self.L.gfpl_rectify if sync else self.L.gfpl_rectify_async
        check(f(self.h, side, _ptr(src), n, _ptr(out)), "rectify")

    def rectify_stereo(self, src_l, src_r, n: int, out_l, out_r) -> None:
        """rectifyImagesLR for n stereo frames: both sides in one launch"""
        check(self.L.gfpl_rectify_stereo_async(self.h, _ptr(src_l), _ptr(src_r), n, _ptr(out_l), _ptr(out_r)),
              "rectify_stereo_async")

    def rectify_host(self, side: int, images: np.ndarray) -> np.ndarray:
        """rectifyImage on HOST images [n][H][W] (or one [H][W]) u8; returns the rectified copy"""
        src = np.ascontiguousarray(images, np.uint8)
        if src.shape[-2:] != (self.height, self.width):
            raise ValueError(f"images {src.shape} != (..., {self.height}, {self.width})")
        out = np.empty_like(src)
        n = 1 if src.ndim == 2 else int(np.prod(src.shape[:-2]))
        check(self.L.gfpl_rectify_host(self.h, side, src.ctypes.data, n, out.ctypes.data), "rectify_host")
        return out

    def maps(self, side: int):
        """the uploaded maps of one side, read back: (map1 int16 [H][W][2], map2 uint16 [H][W])"""
        map1 = np.zeros((self.height, self.width, 2), np.int16)
        map2 = np.zeros((self.height, self.width), np.uint16)
        check(self.L.gfpl_rectifier_read_maps(self.h, side, map1.ctypes.data, map2.ctypes.data), "rectifier_read_maps")
        return map1, map2

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_rectifier_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StereoDetector:
    """gfpl_detector: StereoFrame's detection from a stereo pair of images on the device —
    ORB of both images (the right pyramid kept for the sub-pixel refinement), LSD with the
    lsdNFeatures cut and LBD of both (src/stereoFrame.cpp:148-172, 411-450, 1128-1227), for
    up to `batch` stereo frames per call, on two streams of the detector's own.  detect()
    returns the gfpl_frames view the tracker (StereoFrameHandler.initialize / insertStereoPair
    / frameStep) reads with no copy, ordered by the view's ready / consumed events: at most
    `sets` views may be outstanding (a tracker call reading a view, or discard(), frees it)."""

    def __init__(self, ctx: Context, batch: int, kp_cap: int, kl_cap: int, params: Optional[DetectorParams] = None,
                 sets: int = 2):
        self.L = ctx.L
        self.ctx, self.B, self.kp_cap, self.kl_cap = ctx, batch, kp_cap, kl_cap
        self.params = params if params is not None else DetectorParams.reference(ctx.cam, ctx.cfg)
        h = C.c_void_p()
        check(self.L.gfpl_detector_create(ctx.h, C.byref(self.params), batch, kp_cap, kl_cap, sets, C.byref(h)),
              "detector_create")
        self.h = h

    def detect(self, left, right, time_stamp, n: Optional[int] = None) -> Frames:
        """left / right: device u8 [n][H][W] (torch), time_stamp: device f64 [n]; produced on
        the context's stream.  Asynchronous (status() reports capacity errors)."""
        n = self.B if n is None else n
        fr = Frames()
        check(self.L.gfpl_detect_stereo_async(self.h, _ptr(left), _ptr(right), n, _ptr(time_stamp), C.byref(fr)),
              "detect_stereo_async")
        fr._keep = [left, right, time_stamp]
        return fr

    def detect_host(self, left: np.ndarray, right: np.ndarray, time_stamp) -> Frames:
        """HOST images [n][H][W] u8 (or one [H][W] image) and time stamps [n]."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        ts = np.ascontiguousarray(np.atleast_1d(time_stamp), np.float64)
        n = 1 if left.ndim == 2 else left.shape[0]
        if right.shape != left.shape or len(ts) != n:
            raise ValueError("detect_host: left / right / time stamps disagree")
        fr = Frames()
        check(self.L.gfpl_detect_stereo_host(self.h, left.ctypes.data, right.ctypes.data, n, ts.ctypes.data,
                                             C.byref(fr)), "detect_stereo_host")
        return fr

    def set_rectifier(self, rectifier: Optional["StereoRectifier"]) -> None:
        """gfpl_detector_set_rectifier: detect() / detect_host() then take raw images (None detaches)"""
        check(self.L.gfpl_detector_set_rectifier(self.h, rectifier.h if rectifier is not None else None),
              "detector_set_rectifier")
        self._rectifier = rectifier

    def status(self) -> None:
        check(self.L.gfpl_detector_status(self.h), "detector_status")

    def discard(self, fr: Frames) -> None:
        check(self.L.gfpl_detector_discard(self.h, C.byref(fr)), "detector_discard")

    def read(self, fr: Frames, seq: int) -> dict:
        """one sequence's detections of a view, on the host: kp_l / kp_r (KEYPOINT_DT),
        pdesc_l / pdesc_r, kl_l / kl_r (KEYLINE_DT), ldesc_l / ldesc_r"""
        out = {"kp_l": np.zeros(fr.kp_cap, KEYPOINT_DT), "kp_r": np.zeros(fr.kp_cap, KEYPOINT_DT),
               "pdesc_l": np.zeros((fr.kp_cap, DESC), np.uint8), "pdesc_r": np.zeros((fr.kp_cap, DESC), np.uint8),
               "kl_l": np.zeros(fr.kl_cap, KEYLINE_DT), "kl_r": np.zeros(fr.kl_cap, KEYLINE_DT),
               "ldesc_l": np.zeros((fr.kl_cap, DESC), np.uint8), "ldesc_r": np.zeros((fr.kl_cap, DESC), np.uint8)}
        d = DetectionsHost()
        for k, a in out.items():
            setattr(d, k, a.ctypes.data)
        check(self.L.gfpl_read_detections(self.ctx.h, C.byref(fr), seq, C.byref(d)), "read_detections")
        n = {"kp": (d.n_kp_l, d.n_kp_r), "pdesc": (d.n_kp_l, d.n_kp_r), "kl": (d.n_kl_l, d.n_kl_r),
             "ldesc": (d.n_kl_l, d.n_kl_r)}
        return {k: a[:n[k.split("_")[0]][0 if k.endswith("_l") else 1]].copy() for k, a in out.items()}

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_detector_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------ loop-closure candidate search --
class Vocabulary:
    """gfpl_vocab: a DBoW2 TemplatedVocabulary<FORB> on the device.  Flat arrays: child_off
    [n_nodes + 1] / child (each node's children in Node::children order, node 0 the root), desc
    [n_nodes][32] u8, weight [n_nodes] f64, word_id [n_nodes] (-1 on inner nodes).  ctx may be None
    for the host-side validation alone (it then raises GfplError -1 after the tree passed)."""

    def __init__(self, ctx: Optional[Context], child_off, child, desc, weight, word_id, weighting: int = BOW_TF_IDF,
                 scoring: int = BOW_L1_NORM):
        self.L = ctx.L if ctx is not None else hiplib()
        self.child_off = np.ascontiguousarray(child_off, np.int32)
        self.child = np.ascontiguousarray(child, np.int32)
        self.desc = np.ascontiguousarray(desc, np.uint8)
        self.weight = np.ascontiguousarray(weight, np.float64)
        self.word_id = np.ascontiguousarray(word_id, np.int32)
        self.weighting, self.scoring = int(weighting), int(scoring)
        n = len(self.child_off) - 1
        if self.desc.size != 32 * n or len(self.weight) != n or len(self.word_id) != n:
            raise ValueError("Vocabulary: desc, weight and word_id want one row per node")
        if n < 0 or len(self.child) < int(self.child_off.max()):
            raise ValueError("Vocabulary: child is shorter than child_off says")
        child = self.child if len(self.child) else np.zeros(1, np.int32)
        d = VocabDesc(n, self.child_off.ctypes.data, child.ctypes.data, self.desc.ctypes.data, self.weight.ctypes.data,
                      self.word_id.ctypes.data, self.weighting, self.scoring)
        h = C.c_void_p()
        check(self.L.gfpl_vocab_create(ctx.h if ctx is not None else None, C.byref(d), C.byref(h)), "vocab_create")
        self.h = h

    @staticmethod
    def parse_text(path: str):
        """TemplatedVocabulary::loadFromTextFile's format (TemplatedVocabulary.h:1338-1424): the first
        line `k L scoring weighting`, then one node per line, `parent isLeaf b0 ... b31 weight`; node ids
        count up from 1 in file order (0 is the root), a node's children come in file order, word ids
        count up over the lines with isLeaf > 0.  Blank lines are skipped.  Returns the arrays
        Vocabulary takes, as a dict."""
        with open(path) as f:
            lines = f.read().split("\n")
        k, L, scoring, weighting = [int(x) for x in lines[0].split()[:4]]
        if k < 0 or k > 20 or L < 1 or L > 10 or scoring < 0 or scoring > 5 or weighting < 0 or weighting > 3:
            raise ValueError("Vocabulary.from_text: not a vocabulary text file")
        parent, desc, weight, word_id = [0], [[0] * 32], [0.0], [-1]
        n_words = 0
        for ln in lines[1:]:
            t = ln.split()
            if not t:
                continue
            if len(t) < 35:
                raise ValueError("Vocabulary.from_text: short node line")
            parent.append(int(t[0]))
            desc.append([int(x) for x in t[2:34]])
            weight.append(float(t[34]))
            if int(t[1]) > 0:
                word_id.append(n_words)
                n_words += 1
            else:
                word_id.append(-1)
        n = len(parent)
        kids = [[] for _ in range(n)]
        for i in range(1, n):
            if not 0 <= parent[i] < i:
                raise ValueError("Vocabulary.from_text: a node's parent must come before it")
            kids[parent[i]].append(i)
        child_off = np.zeros(n + 1, np.int32)
        child_off[1:] = np.cumsum([len(c) for c in kids])
        child = np.array([c for cs in kids for c in cs], np.int32)
        return dict(child_off=child_off, child=child, desc=np.array(desc, np.uint8), weight=np.array(weight, np.float64),
                    word_id=np.array(word_id, np.int32), weighting=weighting, scoring=scoring)

    @classmethod
    def from_text(cls, ctx: Optional[Context], path: str) -> "Vocabulary":
        return cls(ctx, **cls.parse_text(path))

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_vocab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bowStats(pl, spl, epl) -> BowStats:
    """gfpl_kf_bow_stats: vector_stdv of a keyframe's point positions pl [n_pt][2] and line midpoints
    (spl + epl) * 0.5 [n_ls][2] (src/mapHandler.cpp:2940-2972), on the host."""
    pl = np.ascontiguousarray(pl, np.float64).reshape(-1, 2)
    spl = np.ascontiguousarray(spl, np.float64).reshape(-1, 2)
    epl = np.ascontiguousarray(epl, np.float64).reshape(-1, 2)
    if len(spl) != len(epl):
        raise ValueError("bowStats: spl and epl differ in length")
    out = BowStats()
    pad = np.zeros((1, 2))
    check(hiplib().gfpl_kf_bow_stats((pl if len(pl) else pad).ctypes.data, len(pl), (spl if len(spl) else pad).ctypes.data,
                                     (epl if len(epl) else pad).ctypes.data, len(spl), C.byref(out)), "kf_bow_stats")
    return out


def lookForLoopCandidates(conf_col, alive, graph_col, kf_curr_idx: int, params: Optional[LcSearchParams] = None):
    """MapHandler::lookForLoopCandidates (src/mapHandler.cpp:3002-3076) on the host: conf_col[i] =
    conf_matrix[i][kf_curr_idx], alive[i] = map_keyframes[i] != NULL, graph_col[i] =
    full_graph[i][kf_curr_idx].  Returns (is_lc_candidate, kf_prev_idx, LcSearchInfo)."""
    n = max(int(kf_curr_idx), 1)
    cc = np.zeros(n, np.float64)
    al = np.zeros(n, np.uint8)
    gr = np.zeros(n, np.int32)
    k = max(int(kf_curr_idx), 0)
    cc[:k] = np.asarray(conf_col, np.float64)[:k]
    al[:k] = np.asarray(alive)[:k] != 0
    gr[:k] = np.asarray(graph_col, np.int32)[:k]
    prm = params if params is not None else LcSearchParams.default()
    prev, info = C.c_int(-1), LcSearchInfo()
    r = hiplib().gfpl_kf_loop_candidates(cc.ctypes.data, al.ctypes.data, gr.ctypes.data, int(kf_curr_idx), C.byref(prm),
                                         C.byref(prev), C.byref(info))
    if r < 0:
        raise GfplError(r, "kf_loop_candidates")
    return bool(r), prev.value, info


class BowDatabase:
    """gfpl_bowdb: the BowVectors of the map's keyframes on the device and a row of the confusion
    matrix per insert (MapHandler::insertKFBowVectorP / L / PL, src/mapHandler.cpp:2865-3000)."""

    def __init__(self, ctx: Context, voc_p: Optional[Vocabulary], voc_l: Optional[Vocabulary], mode: int, kf_cap: int,
                 pt_cap: int, ls_cap: int):
        self.L = ctx.L
        self.ctx, self.mode, self.kf_cap, self.cap = ctx, mode, kf_cap, (pt_cap, ls_cap)
        self.voc = (voc_p, voc_l)   # they must outlive the database
        h = C.c_void_p()
        check(self.L.gfpl_bowdb_create(ctx.h, voc_p.h if voc_p else None, voc_l.h if voc_l else None, mode, kf_cap,
                                       pt_cap, ls_cap, C.byref(h)), "bowdb_create")
        self.h = h

    def insert(self, kf_idx: int, kf=None, stats: Optional[BowStats] = None, row: Optional[np.ndarray] = None,
               pdesc=None, ldesc=None) -> np.ndarray:
        """gfpl_bowdb_insert.  kf: a KeyFrameView (device arrays), or give the device u8 tensors pdesc /
        ldesc [n][32] alone.  row: f64 array of at least kf_idx + 1 entries to write into (entries of
        erased or never-inserted keyframes keep what it held); default zeros.  Returns row[:kf_idx + 1]."""
        import torch
        if kf is not None:
            v = kf.s if isinstance(kf, KeyFrameView) else kf
        else:
            v = KFViewStruct()
            for n_f, p_f, t in (("n_pt", "pdesc", pdesc), ("n_ls", "ldesc", ldesc)):
                if t is not None and int(t.shape[0]):
                    setattr(v, n_f, int(t.shape[0]))
                    setattr(v, p_f, _ptr(t))
        if row is None:
            row = np.zeros(max(kf_idx, 0) + 1, np.float64)
        if row.dtype != np.float64 or not row.flags.c_contiguous or len(row) < kf_idx + 1:
            raise ValueError("BowDatabase.insert: row wants a contiguous f64 array of kf_idx + 1 entries")
        torch.cuda.synchronize()
        check(self.L.gfpl_bowdb_insert(self.h, kf_idx, C.byref(v), C.byref(stats) if stats is not None else None,
                                       row.ctypes.data), "bowdb_insert")
        return row[:kf_idx + 1]

    def _mode_insert(self, mode, kf_idx, kf, stats, row, pdesc, ldesc):
        if self.mode != mode:
            raise GfplError(-1, "BowDatabase: created in another mode")
        return self.insert(kf_idx, kf, stats, row, pdesc, ldesc)

    def insertKFBowVectorP(self, kf_idx: int, kf=None, row=None, pdesc=None):
        return self._mode_insert(BOW_MODE_P, kf_idx, kf, None, row, pdesc, None)

    def insertKFBowVectorL(self, kf_idx: int, kf=None, row=None, ldesc=None):
        return self._mode_insert(BOW_MODE_L, kf_idx, kf, None, row, None, ldesc)

    def insertKFBowVectorPL(self, kf_idx: int, kf=None, stats: Optional[BowStats] = None, row=None, pdesc=None, ldesc=None):
        return self._mode_insert(BOW_MODE_PL, kf_idx, kf, stats, row, pdesc, ldesc)

    def erase(self, kf_idx: int):
        """map_keyframes[kf_idx] = NULL as the database sees it"""
        check(self.L.gfpl_bowdb_erase(self.h, kf_idx), "bowdb_erase")

    def vector_device(self, kind: int, kf_idx: int) -> BowVec:
        """the stored vector (kind 0: descDBoW_P, 1: descDBoW_L) as a device triple"""
        v = BowVec()
        check(self.L.gfpl_bowdb_vector(self.h, kind, kf_idx, C.byref(v), None, None), "bowdb_vector")
        return v

    def vector(self, kind: int, kf_idx: int):
        """the stored vector copied to the host: (word ids int32, values f64)"""
        v = self.vector_device(kind, kf_idx)
        ids, vals = np.zeros(max(v.count, 1), np.int32), np.zeros(max(v.count, 1), np.float64)
        check(self.L.gfpl_bowdb_vector(self.h, kind, kf_idx, C.byref(v), ids.ctypes.data, vals.ctypes.data), "bowdb_vector")
        return ids[:v.count], vals[:v.count]

    def close(self):
        if getattr(self, "h", None):
            self.L.gfpl_bowdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
