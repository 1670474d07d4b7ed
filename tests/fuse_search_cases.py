"""Inputs of gfpl_map_fuse_search's tests: a local map of points or lines seen from a 4-keyframe
trajectory, with planted rows: families of near-duplicate descriptors whose members lie around
the gates' thresholds (so second neighbours are real matches and the gates decide both ways),
one descriptor repeated at several indices, rows on and past the image border, rows at and behind
z = 0, and (lines) zero-length, reversed, parallel and skew segments.  assert_not_blunt() checks
on the reference alone that the gates are reached and decide both ways.
"""
import numpy as np

import lm_fuse_ref as FR
import lm_store_cases as LC

N_KF = 4
SIZES = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049)   # 1024: the kernels' compaction chunk


def cam_dict(cam):
    return dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, width=cam.width, height=cam.height)


def trajectory():
    """T_kf [4][16]: a turn about y and a drift, keyframe 0 the identity."""
    T = np.zeros((N_KF, 4, 4))
    for k in range(N_KF):
        a = 0.06 * k
        T[k] = np.eye(4)
        T[k, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        T[k, :3, 3] = [0.3 * k, -0.02 * k, 0.1 * k]
    return T.reshape(N_KF, 16)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _in_view(rng, cam, margin=60.0):
    """a point in the camera frame whose pixel lies well inside the image"""
    z = rng.uniform(2.0, 8.0)
    u, v = rng.uniform(margin, cam["width"] - margin), rng.uniform(margin, cam["height"] - margin)
    return np.array([(u - cam["cx"]) * z / cam["fx"], (v - cam["cy"]) * z / cam["fy"], z])


def _rot(axis, ang):
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def make_map(cam, n: int, lines: bool, seed: int):
    """(desc [n][32], X [n][3 or 6], kf [n], T_kf [4][16]); the geometry is given in the frame the
    search projects in (Pf = R X + t with T_kf[kf] as written) and mapped back to X."""
    rng = np.random.default_rng([seed, n, int(lines)])
    T = trajectory()
    desc, Xf, kfs = [], [], []

    def push(d, xf, kf):
        desc.append(d), Xf.append(np.asarray(xf, np.float64).reshape(-1)), kfs.append(kf)

    def segment():
        s = _in_view(rng, cam, 120.0)
        return s, s + _unit(rng) * rng.uniform(0.3, 1.2)
    while len(desc) < n:
        kf = int(rng.integers(0, N_KF))
        what = rng.random()
        if what < 0.55:                                   # a family around the thresholds
            m = int(rng.integers(2, 5))
            fam = LC.near_duplicates(rng, m)
            if not lines:
                a = _in_view(rng, cam)
                for j in range(m):
                    push(fam[j], a + (_unit(rng) * rng.uniform(0.03, 0.17) if j else 0), kf)
            else:
                s, e = segment()
                for j in range(m):
                    mode = rng.random()
                    if j == 0:
                        sj, ej = s, e
                    elif mode < 0.5:                      # parallel, shifted: straddles maxPointLineError
                        sj, ej = s + _unit(rng) * rng.uniform(0.02, 0.14), e + _unit(rng) * rng.uniform(0.02, 0.14)
                    elif mode < 0.9:                      # skew about the middle: straddles maxDirLineError
                        R, mid = _rot(_unit(rng), rng.uniform(0.03, 0.2)), 0.5 * (s + e)
                        sj, ej = mid + R @ (s - mid), mid + R @ (e - mid)
                    else:                                 # the same segment the other way round
                        sj, ej = e + _unit(rng) * 0.01, s + _unit(rng) * 0.01
                    push(fam[j], np.r_[sj, ej], kf)
        elif what < 0.62:                                 # one descriptor at several indices
            d = rng.integers(0, 256, 32, dtype=np.uint8)
            a = _in_view(rng, cam)
            for j in range(int(rng.integers(2, 4))):
                off = _unit(rng) * rng.uniform(0.0, 0.2)
                push(d, a + off if not lines else np.r_[a + off, a + off + [0.5, 0.1, 0.0]], kf)
        elif what < 0.70:                                 # the image border and z <= 0
            z = float(rng.choice([-2.0, 0.0, 1e-9, 3.0]))
            u = float(rng.choice([0.0, -1.0, 1e-7, cam["width"], cam["width"] - 1e-7, cam["width"] / 2]))
            v = float(rng.choice([0.0, cam["height"], cam["height"] / 2, cam["height"] + 3]))
            a = np.array([(u - cam["cx"]) * z / cam["fx"], (v - cam["cy"]) * z / cam["fy"], z])
            d = rng.integers(0, 256, 32, dtype=np.uint8)
            push(d, a if not lines else (np.r_[_in_view(rng, cam), a] if rng.random() < 0.5 else np.r_[a, _in_view(rng, cam)]), kf)
        elif what < 0.73 and lines:                       # a zero-length line, its descriptor shared with a proper one
            d = rng.integers(0, 256, 32, dtype=np.uint8)
            s, e = segment()
            push(d, np.r_[s, s], kf)
            push(d, np.r_[s, e], kf)
        else:                                             # a landmark of its own
            d = rng.integers(0, 256, 32, dtype=np.uint8)
            push(d, _in_view(rng, cam) if not lines else np.r_[segment()], kf)
    order = rng.permutation(len(desc))[:n]                # families spread over the indices
    desc = np.array([desc[i] for i in order], np.uint8).reshape(n, 32)
    kfs = np.array([kfs[i] for i in order], np.int32)
    Xf = np.array([Xf[i] for i in order], np.float64).reshape(n, 6 if lines else 3)
    # X = R^T (Xf - t) per endpoint
    X = np.zeros_like(Xf)
    for i in range(n):
        M = T[kfs[i]].reshape(4, 4)
        for c in range(0, Xf.shape[1], 3):
            X[i, c:c + 3] = M[:3, :3].T @ (Xf[i, c:c + 3] - M[:3, 3])
    # (keyframe 0 is the identity: its rows keep their border values exactly)
    return desc, X, kfs, T


_checked = {}


def assert_not_blunt(cam, seed=1):
    """On the reference alone, over the sizes the GPU tests run: of the line pairs that reach the
    gate at least 0.15 take each branch of d1.norm() > d2.norm(); at least 0.2 of the point pairs
    and of the line pairs that reach the gate are accepted and at least 0.2 rejected; an accepted
    pair has its mirror."""
    key = (cam["width"], cam["height"], seed)
    if key not in _checked:
        tot = {False: dict(reached=0, accepted=0, mirror=0), True: dict(reached=0, accepted=0, mirror=0)}
        branch, left_out = [], 0
        for lines in (False, True):
            for n in SIZES:
                if n < 31:
                    continue
                desc, X, kf, T = make_map(cam, n, lines, seed)
                st = {}
                loc, pairs, bad = FR.search(cam, desc, X, kf, T, stats=st)
                assert not bad and len(loc) > 0.8 * n
                left_out += n - len(loc)
                tot[lines]["reached"] += st["reached"]
                tot[lines]["accepted"] += st["accepted"]
                have = {tuple(p) for p in pairs.tolist()}
                tot[lines]["mirror"] += sum((t, i) in have for i, t in have)
                branch += st["branch"]
        assert left_out >= 100          # the select does leave rows out
        _checked[key] = (tot, float(np.mean(branch)))
    tot, first = _checked[key]
    print(f"fuse search generator: d1.norm() > d2.norm() in {first:.3f} of the line pairs; accepted "
          f"{tot[False]['accepted']}/{tot[False]['reached']} point pairs, {tot[True]['accepted']}/{tot[True]['reached']} line pairs")
    assert 0.15 <= first <= 0.85, first
    for lines in (False, True):
        frac = tot[lines]["accepted"] / tot[lines]["reached"]
        assert 0.2 <= frac <= 0.8, (lines, frac)
        assert tot[lines]["mirror"] >= 1
