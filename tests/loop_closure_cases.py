"""Case builders for the loop-closure check (tests/test_loop_closure_cpu.py, _gpu.py).

Every case is two keyframes as FrameHosts: kf0's 3D features, and kf1's observations projected from
them under a known T (so the Gauss-Newton of computeRelativePoseGN, which moves kf0's 3D onto kf1's
observations, is looking for T), with descriptors planted as known_pair of
tests/test_keyframe_matches.py plants them: kf1's row perm[i] carries kf0's descriptor i with a few
bits flipped.  A case also carries the config fields and gate thresholds it runs with, and what it
is built to show (`expect`), which tests/test_loop_closure_cpu.py checks on the Python reference.
"""
from dataclasses import dataclass, field

import numpy as np

import gfpl
import loop_closure_ref as R

SIZES = [(0, 0), (1, 5), (2, 2), (63, 64), (65, 129), (300, 120), (2048, 1024)]
BIG = "size_2048_1024"


def pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rm = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
          @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T


T_DEFAULT = pose(0.01, -0.02, 0.015, [0.1, -0.05, 0.2])


def proj(cam, P):
    return np.array([cam.cx + (cam.fx * P[0]) / P[2], cam.cy + (cam.fy * P[1]) / P[2]])


@dataclass
class Case:
    name: str
    f0: object
    f1: object
    T: np.ndarray
    max_iters: int = 5
    prm: tuple = R.LC_DEFAULTS
    expect: dict = field(default_factory=dict)
    cam_over: tuple = ()   # make_camera overrides, as sorted items

    @property
    def group(self):
        """cases of one group share the context (camera, config) and the thresholds: one batched call"""
        return (self.max_iters, self.prm, self.cam_over)


def make_pair(cam, n_pt, n_ls, T=T_DEFAULT, seed=1, flips=8, noise=0.0, pt_out=0, ls_out=0):
    """kf0 / kf1 FrameHosts; rows [0, pt_out) of kf0's points and [0, ls_out) of its lines get a kf1
    observation 12 px off (points: a random direction; lines: the line moved 12 px along its normal);
    noise: Gaussian pixel noise on kf1's point observations and line offsets."""
    rng = np.random.default_rng(seed)
    kp, kl = max(n_pt, 2), max(n_ls, 2)
    f0, f1 = gfpl.FrameHost(kp, kl), gfpl.FrameHost(kp, kl)
    f0.s.n_pt = f1.s.n_pt = n_pt
    f0.s.n_ls = f1.s.n_ls = n_ls

    def flipped(d):
        d = d.copy()
        for b in rng.choice(256, flips, replace=False):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        return d

    perm = rng.permutation(n_pt)
    for i in range(n_pt):
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        P = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(2, 8)])
        f0.arr["pdesc"][i] = d
        f0.arr["pt_P"][i] = P
        f0.arr["pt_sigma2"][i] = 1.0 / 1.44 ** rng.integers(1, 4)
        j = perm[i]
        f1.arr["pdesc"][j] = flipped(d)
        f1.arr["pt_sigma2"][j] = 1.0
        off = rng.normal(0.0, noise, 2) if noise else np.zeros(2)
        ang = rng.uniform(0, 2 * np.pi)
        if i < pt_out:
            off = off + 12.0 * np.array([np.cos(ang), np.sin(ang)])
        f1.arr["pt_pl"][j] = proj(cam, T[:3, :3] @ P + T[:3, 3]) + off
    perm = rng.permutation(n_ls)
    for i in range(n_ls):
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        sP = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(2, 8)])
        eP = sP + rng.uniform(-0.8, 0.8, 3)
        eP[2] = max(eP[2], 1.5)
        su, eu = proj(cam, T[:3, :3] @ sP + T[:3, 3]), proj(cam, T[:3, :3] @ eP + T[:3, 3])
        le = np.cross([su[0], su[1], 1.0], [eu[0], eu[1], 1.0])
        le = le / np.hypot(le[0], le[1])
        if noise:
            le[2] += rng.normal(0.0, noise)
        if i < ls_out:
            le[2] += 12.0
        f0.arr["ldesc"][i] = d
        f0.arr["ls_sP"][i], f0.arr["ls_eP"][i] = sP, eP
        f0.arr["ls_sigma2"][i] = 1.0 / 1.44 ** rng.integers(1, 4)
        j = perm[i]
        f1.arr["ldesc"][j] = flipped(d)
        f1.arr["ls_le"][j] = le
        f1.arr["ls_sigma2"][j] = 1.0
    return f0, f1


def _size_cases(cam):
    out = []
    for k, (n_pt, n_ls) in enumerate(SIZES):
        f0, f1 = make_pair(cam, n_pt, n_ls, seed=10 + k)
        # every planted correspondence is mutual (U4: a kind with < 2 rows yields none)
        exp = {"n_pt": n_pt if n_pt >= 2 else 0, "n_ls": n_ls if n_ls >= 2 else 0}
        if n_pt >= 63:   # (fewer rows leave the 6-dof pose under-determined by five line residuals / two points)
            exp["all_inliers"] = True
            exp["gates"] = 31
        if (n_pt, n_ls) == (0, 0):
            exp["exit"] = R.EXIT_X      # H = 0, g = 0: x_inc = 0
            exp["e_nan"] = True         # 0 / 0
        out.append(Case(f"size_{n_pt}_{n_ls}", f0, f1, T_DEFAULT, expect=exp))
    return out


def _mutuality_cases(cam):
    out = []
    # duplicate kf1 descriptors: kf1 row t + 1 becomes a copy of row t; the kf0 row whose partner was
    # overwritten loses its match, and of the two equal rows the lower index answers kf0's query
    f0, f1 = make_pair(cam, 64, 64, seed=31)
    f1.arr["pdesc"][21] = f1.arr["pdesc"][20]
    f1.arr["ldesc"][41] = f1.arr["ldesc"][40]
    out.append(Case("dup_kf1_desc", f0, f1, T_DEFAULT, expect={"n_pt": 63, "n_ls": 63}))
    # a knn tie: kf1 row b is rewritten at the same distance (8 flips) from kf0 row q as q's partner a
    f0, f1 = make_pair(cam, 64, 64, seed=32)
    rng = np.random.default_rng(99)
    for key in ("pdesc", "ldesc"):
        q = 5
        d = f0.arr[key][q].copy()
        a = next(j for j in range(64) if bin(int.from_bytes(bytes(f0.arr[key][q] ^ f1.arr[key][j]), "little")).count("1") == 8)
        b = (a + 7) % 64
        for bit in rng.choice(256, 8, replace=False):
            d[bit // 8] ^= np.uint8(1 << (bit % 8))
        f1.arr[key][b] = d
    out.append(Case("knn_tie", f0, f1, T_DEFAULT, expect={"n_pt": 63, "n_ls": 63}))
    return out


def _outlier_cases(cam):
    # N = 20 + 10 = 30 features and lc_inl = 0.8: 25 inliers give 25 / 30 > 0.8; 24 give 24 / 30, which
    # rounds to the double of the literal 0.8 and is not greater
    out = []
    prm = (1.5, 0.01, 0.8, 1.5, 35.0)
    f0, f1 = make_pair(cam, 20, 10, seed=41, pt_out=3, ls_out=2)
    out.append(Case("outliers_share_above", f0, f1, T_DEFAULT, prm=prm,
                    expect={"n_pt_inl": 17, "n_ls_inl": 8, "gates": 31}))
    f0, f1 = make_pair(cam, 20, 10, seed=41, pt_out=4, ls_out=2)
    out.append(Case("outliers_share_at", f0, f1, T_DEFAULT, prm=prm,
                    expect={"n_pt_inl": 16, "n_ls_inl": 8, "gates": 31 ^ 4}))
    return out


def _gate_cases(cam):
    # one noisy pair that passes every gate at the defaults; each case moves ONE threshold across it
    # (true motion: |t| = 0.23 m, rotation 1.5 degrees)
    out = []
    base = dict(zip(("lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot"), R.LC_DEFAULTS))
    f0, f1 = make_pair(cam, 120, 60, seed=51, noise=0.5)
    out.append(Case("gates_all_hold", f0, f1, T_DEFAULT, expect={"gates": 31}))
    for bit, (k, v) in enumerate([("lc_res", 0.0), ("lc_unc", 0.0), ("lc_inl", 1.0), ("lc_trs", 0.05), ("lc_rot", 0.5)]):
        prm = tuple((base | {k: v}).values())
        out.append(Case(f"gate_{k[3:]}_fails", f0, f1, T_DEFAULT, prm=prm, expect={"gates": 31 ^ (1 << bit)}))
    return out


def _path_cases(cam):
    out = []
    f0, f1 = make_pair(cam, 100, 50, seed=61, noise=0.5)
    out.append(Case("max_iters_0", f0, f1, T_DEFAULT, max_iters=0, expect={"iters": 0, "identity": True, "e": 0.0}))
    out.append(Case("max_iters_1", f0, f1, T_DEFAULT, max_iters=1, expect={"iters": 1, "exit": R.EXIT_BUDGET}))
    # T = I without noise: e < eps at the first evaluation, T_inc stays I (logmap's theta <= 1e-6 branch)
    f0, f1 = make_pair(cam, 100, 50, T=np.eye(4), seed=62)
    out.append(Case("identity_exit_e", f0, f1, np.eye(4), expect={"iters": 1, "exit": R.EXIT_E, "identity": True}))
    # a half turn about the optical axis: (x, y, z) -> (-x, -y, z) keeps the features in front
    Tpi = pose(0.0, 0.0, np.pi, [0.0, 0.0, 0.0])
    f0, f1 = make_pair(cam, 100, 50, T=Tpi, seed=63)
    out.append(Case("half_turn", f0, f1, Tpi, expect={}))
    # a point whose gz^2 = 1e-8 is below homog_th = 1e-7 at the first iteration (T_inc = I)
    f0, f1 = make_pair(cam, 100, 50, seed=64)
    f0.arr["pt_P"][3] = [1e-5, -2e-5, 1e-4]
    out.append(Case("below_homog_th", f0, f1, T_DEFAULT, expect={"homog_row": 3}))
    # enough iterations on noisy data for the error to stall: |e - err_prev| < eps
    f0, f1 = make_pair(cam, 100, 50, seed=65, noise=0.5)
    out.append(Case("stall_exit_de", f0, f1, T_DEFAULT, max_iters=100, expect={"exit": R.EXIT_DE}))
    # a residual exactly ON sqrt(7.815): with the principal point at (0, 0), P = (0, 0, 3) projects to
    # (0, 0) under T_inc = I (max_iters = 0), the observation is (chi, 0), so |err| = sqrt(chi * chi) = chi
    # (sqrt(fl(x^2)) = |x| in round-to-nearest binary arithmetic): not an outlier under `>`
    over = (("cx", 0.0), ("cy", 0.0))
    cam0 = gfpl.make_camera("vga", gfpl.default_config(), **dict(over))
    f0, f1 = make_pair(cam0, 2, 0, seed=66)
    rc, i12, _ = R.O.knn2(f0.arr["pdesc"][:2], f1.arr["pdesc"][:2], 1)
    f0.arr["pt_P"][0] = [0.0, 0.0, 3.0]
    f1.arr["pt_pl"][i12[0, 0]] = [np.sqrt(7.815), 0.0]
    out.append(Case("on_chi_threshold", f0, f1, None, max_iters=0, cam_over=over,
                    expect={"n_pt": 2, "inlier_row0": 1}))
    return out


_CASES, _REFS = None, {}


def setup(cam_over=()):
    cfg = gfpl.default_config()
    return gfpl.make_camera("vga", cfg, **dict(cam_over)), cfg


def all_cases():
    global _CASES
    if _CASES is None:
        cam, _ = setup()
        cs = _size_cases(cam) + _mutuality_cases(cam) + _outlier_cases(cam) + _gate_cases(cam) + _path_cases(cam)
        _CASES = {c.name: c for c in cs}
    return _CASES


def reference(name):
    """the Python reference's result of a case, computed once per process"""
    if name not in _REFS:
        c = all_cases()[name]
        cam, _ = setup(c.cam_over)
        _REFS[name] = R.is_loop_closure(cam, gfpl.default_config(max_iters=c.max_iters), c.f0, c.f1, c.prm)
    return _REFS[name]
