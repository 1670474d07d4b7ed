"""Global bundle adjustment problems for tests/test_gba_cpu.py and test_gba_gpu.py, built on
lba_cases.make_problem: a problem is a gfpl.LbaProblem whose local keyframes are every alive keyframe
but keyframe 0 and whose fixed pose 0 is keyframe 0.  Every case is a function of its arguments alone.

Widths of k_gba.hip the keyframe sizes straddle (gfpl_layout.hpp):
  GBA_LDLT_KFS = 6     block rows of the panel one workgroup of k_gba_ldlt factorises   -> 5, 6, 7, 13
  GBA_BLOCK    = 256   threads of the wide phases and rows per pass of the substitutions: 6 n_kf
                       crosses it between 42 and 43 keyframes                           -> 42, 43
  GFPL_LBA_MAX_KFS = 16  the last size gfpl_lba_solve takes                             -> 16, 17
The landmark counts straddle a wave (63, 64, 65) and GBA_BLOCK (300).
"""
import gba_ref as G
from lba_cases import Case, make_problem, setup, _scaled, _many  # noqa: F401

LDLT_KFS, BLOCK = 6, 256


def _sparse(n_kf):
    """landmark j is seen by keyframes j mod n_kf and (j + 1) mod n_kf and by keyframe 0 (fixed): most
    keyframe pairs share no landmark, so S has empty blocks inside its envelope"""
    return lambda rng, j: sorted({j % n_kf, (j + 1) % n_kf}) + [-1]


def size_cases(cam):
    out = []
    k = 0
    for n_kf in (2, 17):
        for n_pt, n_ls in ((0, 1), (1, 0), (63, 0), (64, 1), (65, 65), (300, 0), (0, 65)):
            k += 1
            out.append(Case(f"size_kf{n_kf}_pt{n_pt}_ls{n_ls}", make_problem(cam, 500 + k, n_kf, 2, n_pt, n_ls, obs=3)))
    for n_kf in (1, 5, 6, 7, 13, 16):
        k += 1
        out.append(Case(f"size_kf{n_kf}", make_problem(cam, 500 + k, n_kf, 1, 24, 6, obs=3)))
    for n_kf in (42, 43):
        k += 1
        out.append(Case(f"size_kf{n_kf}", make_problem(cam, 500 + k, n_kf, 1, 60, 8, obs=_sparse(n_kf)), prm=(0.001, 10.0, 2)))
    out.append(Case("size_kf70", make_problem(cam, 540, 70, 1, 90, 12, obs=4), prm=(0.001, 10.0, 3)))
    return out


def structure_cases(cam):
    one = lambda rng, j: [int(rng.integers(0, 3))]
    fixed_only = lambda rng, j: ([-1, -2] if j % 3 == 0 else [0, 1, -1])
    twice = lambda rng, j: ([1, 0, 1] if j % 2 == 0 else [0, 2, 2, -1])
    wave = lambda rng, j: (_many(70)(rng, j) if j in (0, 7) else [0, 1, 2])
    every = lambda rng, j: (list(range(70)) if j in (0, 41) else sorted({j % 70, (j + 3) % 70}) + [-1])
    idle = lambda rng, j: [0, 2, -1]           # keyframe 1 observes nothing
    return [
        Case("one_observation", make_problem(cam, 601, 3, 1, 20, 4, obs=one)),
        Case("single_observation_in_all", make_problem(cam, 607, 1, 1, 1, 0, obs=lambda rng, j: [0])),
        # two local keyframes, both observing: the landmarks with j % 3 == 0 have no pair at all and still go through
        # the solve (an empty pair list in the inversion, the back-substitution and |DX|^2)
        Case("fixed_only_landmarks", make_problem(cam, 602, 2, 2, 21, 6, obs=fixed_only)),
        Case("twice_by_one_keyframe", make_problem(cam, 603, 3, 1, 20, 5, obs=twice)),
        Case("seventy_by_two_keyframes", make_problem(cam, 604, 3, 1, 9, 8, obs=wave)),
        Case("seen_by_all_70", make_problem(cam, 605, 70, 1, 41, 2, obs=every), prm=(0.001, 10.0, 3)),
        Case("idle_keyframe", make_problem(cam, 606, 3, 1, 20, 0, obs=idle)),
        Case("no_common_landmark", make_problem(cam, 608, 17, 1, 34, 17, obs=_sparse(17))),
    ]


def family_cases(cam):
    return [
        Case("points_only", make_problem(cam, 611, 3, 1, 40, 0)),
        Case("lines_only", make_problem(cam, 612, 3, 1, 0, 30)),
        Case("both", make_problem(cam, 613, 4, 2, 40, 20)),
        Case("max_iters_1", make_problem(cam, 614, 3, 1, 30, 10), prm=(0.001, 10.0, 1)),
        Case("zero_residual", make_problem(cam, 615, 2, 1, 12, 3, exact=True)),
        Case("lambda_0", _scaled(make_problem(cam, 616, 3, 2, 30, 0, obs=4), 1e9)),
        # a small lambda_lm leaves the transposed coupling blocks of the pre-pass undamped enough for its
        # reduced system to be indefinite (test_gba_cpu.py asserts a negative pivot); lines seen 8 times
        Case("lines_small_lambda", make_problem(cam, 621, 6, 2, 0, 20, obs=8), prm=(1e-9, 10.0, 4)),
        Case("both_small_lambda", make_problem(cam, 622, 6, 2, 30, 20, obs=8), prm=(1e-9, 10.0, 4)),
        Case("points_small_lambda", make_problem(cam, 623, 6, 2, 40, 0, obs=8), prm=(1e-9, 10.0, 4)),
        Case("stale_x_kf",make_problem(cam, 618, 3, 1, 40, 10, stale=0.02)),
        Case("other_camera", make_problem(cam, 619, 3, 1, 40, 10), cam_over=(("fx", 300.0), ("fy", 310.0))),
        Case("other_lambda_k", make_problem(cam, 620, 3, 1, 40, 10), prm=(0.001, 3.0, 20)),
    ]


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        cam, _ = setup()
        cs = size_cases(cam) + structure_cases(cam) + family_cases(cam)
        _CASES = {c.name: c for c in cs}
    return _CASES


def points_only():
    """the names of the cases without a line"""
    return tuple(n for n, c in all_cases().items() if len(c.prob.a["ls"]) == 0)


_REFS = {}


def reference(case, prm=None, **kw):
    """gba_ref.gba with solve_pinned on the case, computed once per (case, parameters, options) and
    never changed by its users"""
    prm = case.prm if prm is None else tuple(prm)
    key = (case.name, prm, tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _REFS:
        cam, cfg = setup(case.cam_over)
        _REFS[key] = G.gba(cam, cfg.homog_th if case.homog is None else case.homog, case.prob.a, prm, **kw)
    return _REFS[key]
