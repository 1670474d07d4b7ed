"""Local bundle adjustment problems built from a seed, for tests/test_lba_cpu.py and test_lba_gpu.py.

A problem is a small local map: keyframes near the origin looking along +z (T_kf_w maps keyframe to
world coordinates, so the reference projects with its inverse), points and line segments 4 to 10 m in
front of them, observations by projection through the true poses plus pixel noise, and perturbed
estimates to start from.  Every case is a function of its arguments alone.
"""
from dataclasses import dataclass

import numpy as np

import gfpl
import lba_ref as R
import loop_closure_ref as LR
import oracle as O

MAX_KFS = gfpl.LBA_MAX_KFS


def setup(cam_over=()):
    cfg = gfpl.default_config()
    return gfpl.make_camera("vga", cfg, **dict(cam_over)), cfg


def _pose(rng, rot, trs):
    x = np.concatenate([rng.uniform(-trs, trs, 3), rng.uniform(-rot, rot, 3)])
    return O.expmap_se3(x)


def _proj(cam, T_kf_w, P):
    Pc = O.inverse_se3(T_kf_w)[:3, :] @ np.append(P, 1.0)
    return np.array([cam.cx + cam.fx * Pc[0] / Pc[2], cam.cy + cam.fy * Pc[1] / Pc[2]])


def _observers(rng, j, n_kf, n_fix, obs):
    """keyframe slots of landmark j's observations.  obs: an int (that many distinct random keyframes,
    local or fixed), or a callable (rng, j) -> list of slots"""
    if callable(obs):
        return list(obs(rng, j))
    pool = list(range(n_kf)) + [-1 - f for f in range(n_fix)]
    k = min(obs, len(pool))
    return [pool[i] for i in sorted(rng.choice(len(pool), k, replace=False))]


def make_problem(cam, seed, n_kf, n_fix, n_pt, n_ls, obs=3, noise=0.5, lm_noise=0.05, pose_noise=0.01, stale=0.0,
                 exact=False):
    """exact: observations without noise and estimates at the truth (every residual is then set to an
    exact zero by observing the estimate's own projection as the device computes it)."""
    rng = np.random.default_rng(seed)
    T_true = [_pose(rng, 0.05, 0.5) for _ in range(n_kf)]
    T_fix = [_pose(rng, 0.05, 0.5) for _ in range(n_fix)]
    if exact:
        noise = lm_noise = pose_noise = 0.0
    T_kf = [T @ _pose(rng, pose_noise, pose_noise) if pose_noise else T for T in T_true]
    x_kf = [LR.logmap_se3(T @ _pose(rng, stale, stale)) if stale else LR.logmap_se3(T) for T in T_kf]
    P = np.stack([rng.uniform(-2, 2, n_pt), rng.uniform(-1.5, 1.5, n_pt), rng.uniform(4, 10, n_pt)], 1).reshape(-1, 3)
    A = np.stack([rng.uniform(-2, 2, n_ls), rng.uniform(-1.5, 1.5, n_ls), rng.uniform(4, 10, n_ls)], 1).reshape(-1, 3)
    Lw = np.concatenate([A, A + rng.uniform(-0.8, 0.8, (n_ls, 3))], 1).reshape(-1, 6)
    pose_of = lambda s: T_true[s] if s >= 0 else T_fix[-1 - s]
    pt_lm, pt_kf, pt_obs, ls_lm, ls_kf, ls_obs = [], [], [], [], [], []
    for j in range(n_pt):
        for s in _observers(rng, j, n_kf, n_fix, obs):
            pt_lm.append(j)
            pt_kf.append(s)
            pt_obs.append(_proj(cam, pose_of(s), P[j]) + noise * rng.standard_normal(2))
    for j in range(n_ls):
        for s in _observers(rng, n_pt + j, n_kf, n_fix, obs):
            p, q = _proj(cam, pose_of(s), Lw[j, :3]), _proj(cam, pose_of(s), Lw[j, 3:])
            l = np.cross(np.append(p, 1.0), np.append(q, 1.0))
            l = l / np.sqrt(l[0] * l[0] + l[1] * l[1])
            l[2] += noise * rng.standard_normal()
            ls_lm.append(j)
            ls_kf.append(s)
            ls_obs.append(l)
    pt = P + lm_noise * rng.standard_normal(P.shape)
    ls = Lw + lm_noise * rng.standard_normal(Lw.shape)
    pt_sigma = rng.uniform(0.5, 2.0, len(pt_lm))
    ls_sigma = rng.uniform(0.5, 2.0, len(ls_lm))
    prob = gfpl.LbaProblem(np.array(x_kf).reshape(-1, 6), np.array(T_kf).reshape(-1, 16), np.array(T_fix).reshape(-1, 16),
                           pt, ls, pt_lm, pt_kf, np.array(pt_obs).reshape(-1, 2), pt_sigma, ls_lm, ls_kf,
                           np.array(ls_obs).reshape(-1, 3), ls_sigma)
    if exact:
        _zero_residuals(cam, prob)
    return prob


def _zero_residuals(cam, prob):
    """point observations := the projections the pre-pass itself computes, so p_err is exactly 0.  A
    line's two endpoint errors vanish exactly only when both endpoints project alike, so the lines of an
    exact case are degenerate segments P = Q observed by l = (1, 0, -u): 1 * u + 0 * v - u is exactly 0."""
    a = prob.a
    Ti = {s: O.inverse_se3(T.reshape(4, 4)) for s, T in enumerate(a["T_kf"])}
    Ti.update({-1 - f: O.inverse_se3(T.reshape(4, 4)) for f, T in enumerate(a["T_fix"])})
    if len(a["pt_obs_lm"]):
        T = np.array([Ti[int(s)] for s in a["pt_obs_kf"]])
        a["pt_obs"][:] = R._proj(cam, R._apply(T, a["pt"][a["pt_obs_lm"]]))
    if len(a["ls_obs_lm"]):
        a["ls"][:, 3:] = a["ls"][:, :3]
        T = np.array([Ti[int(s)] for s in a["ls_obs_kf"]])
        pu = R._proj(cam, R._apply(T, a["ls"][a["ls_obs_lm"], :3]))
        l = a["ls_obs"]
        l[:, 0], l[:, 1] = 1.0, 0.0                 # 1 * u + 0 * v exactly, so the offset cancels it exactly
        l[:, 2] = -pu[:, 0]


@dataclass
class Case:
    name: str
    prob: object
    prm: tuple = R.LBA_DEFAULTS
    cam_over: tuple = ()
    homog: float = None   # None: the context's

    @property
    def group(self):
        return (self.prm, self.cam_over)


def _many(n):
    return lambda rng, j: [int(s) for s in rng.integers(0, 2, n)]   # n observations by keyframes 0 and 1


def size_cases(cam):
    out = []
    k = 0
    for n_kf in (1, 2, 5, MAX_KFS):
        for n_pt, n_ls in ((0, 1), (1, 0), (63, 0), (64, 1), (65, 65), (300, 0), (0, 65)):
            if n_kf == MAX_KFS and n_pt == 300:
                continue   # (300 points with 16 keyframes add no path that 300 with 5 and 65 with 16 lack)
            k += 1
            out.append(Case(f"size_kf{n_kf}_pt{n_pt}_ls{n_ls}", make_problem(cam, 100 + k, n_kf, 2, n_pt, n_ls, obs=3)))
    out.append(Case("size_kf5_pt300_ls65", make_problem(cam, 199, 5, 2, 300, 65, obs=4)))
    return out


def structure_cases(cam):
    one = lambda rng, j: [int(rng.integers(0, 3))]
    fixed_only = lambda rng, j: ([-1, -2] if j % 3 == 0 else [0, 1, -1])
    twice = lambda rng, j: ([1, 0, 1] if j % 2 == 0 else [0, 2, 2, -1])
    wave = lambda rng, j: (_many(70)(rng, j) if j in (0, 7) else [0, 1, 2])
    return [
        Case("one_observation", make_problem(cam, 201, 3, 1, 20, 4, obs=one)),
        Case("fixed_only_landmarks", make_problem(cam, 202, 3, 2, 21, 6, obs=fixed_only)),
        Case("twice_by_one_keyframe", make_problem(cam, 203, 3, 1, 20, 5, obs=twice)),
        Case("more_than_a_wave", make_problem(cam, 204, 3, 1, 9, 8, obs=wave)),
    ]


# seeds whose problem takes err > err_prev at least once under the reference (test_lba_cpu.py asserts it)
REJECT_SEEDS = (304, 312, 315, 317)


def family_cases(cam):
    out = [
        Case("points_only", make_problem(cam, 211, 3, 1, 40, 0)),
        Case("lines_only", make_problem(cam, 212, 3, 1, 0, 30)),
        Case("both", make_problem(cam, 213, 4, 2, 40, 20)),
        Case("max_iters_1", make_problem(cam, 214, 3, 1, 30, 10), prm=(0.001, 10.0, 1)),
        Case("zero_residual", make_problem(cam, 215, 2, 1, 12, 3, exact=True)),
        # lambda = 0: every diagonal of H below 1 (sigma large makes w tiny); 4 observations per landmark.
        # Points only: a residual is a scalar, so a line's 6 x 6 block needs damping whatever it is seen by
        Case("lambda_0", _scaled(make_problem(cam, 216, 3, 2, 30, 0, obs=4), 1e9)),
        Case("singular", _scaled(make_problem(cam, 217, 2, 1, 10, 0, obs=lambda rng, j: [int(rng.integers(0, 2))]), 1e9)),
        Case("stale_x_kf", make_problem(cam, 218, 3, 1, 40, 10, stale=0.02)),
        Case("other_camera", make_problem(cam, 219, 3, 1, 40, 10), cam_over=(("fx", 300.0), ("fy", 310.0))),
        Case("other_lambda_k", make_problem(cam, 220, 3, 1, 40, 10), prm=(0.001, 3.0, 20)),
    ]
    for s in REJECT_SEEDS:
        out.append(Case(f"rejects_{s}", make_problem(cam, s, 3, 0, 40, 0, noise=2.0, lm_noise=0.3, pose_noise=0.05)))
    return out


def _scaled(prob, sigma):
    """sigma_list so large that w = 1 / (1 + |err|^2 sigma) leaves every diagonal of H below 1: Hmax = 0"""
    prob.a["pt_sigma"][:] = sigma
    prob.a["ls_sigma"][:] = sigma
    return prob


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        cam, _ = setup()
        cs = size_cases(cam) + structure_cases(cam) + family_cases(cam)
        _CASES = {c.name: c for c in cs}
    return _CASES


_REFS = {}


def reference(case, **kw):
    """lba_ref.lba with solve_pinned on the case, computed once per (case, options)"""
    key = (case.name, tuple(sorted(kw.items())))
    if key not in _REFS:
        cam, cfg = setup(case.cam_over)
        _REFS[key] = R.lba(cam, cfg.homog_th if case.homog is None else case.homog, case.prob.a, case.prm, **kw)
    return _REFS[key]
