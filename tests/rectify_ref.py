"""Independent numpy restatement of the rectification ledger R1-R6: the
CV_16SC2 + CV_16UC1 maps of cv::initUndistortRectifyMap / cv::fisheye::initUndistortRectifyMap
and cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit images.  Not a call into the product:
the tests compare gfpl_rectify_maps_host and k_rectify against this, bit for bit.

All arithmetic is IEEE f64, one rounding per operation (numpy does not contract a*b+c), in
the ledger's expression order; R2's ray is accumulated by a loop over the columns (vectorised
over the rows), R4's atan goes through math.atan (the C library's, as the product's)."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDENTITY = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]


# a tilted rig: rotation about (1, 2, 0.5) by 0.03 rad (orthonormal to f64 rounding)
def small_rotation(angle=0.03, axis=(1.0, 2.0, 0.5)):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx).reshape(-1).tolist()


# an equidistant (fisheye) camera with four non-zero coefficients
EQUI = dict(K=[190.97, 190.97, 254.93, 256.89], D=[0.0034823, 0.0007150, -0.0020532, 0.00020293],
            R=small_rotation(0.02, (0.3, -1.0, 0.2)), P=[150.0, 150.0, 255.5, 255.25], equi=True)


def euroc():
    """the EuRoC rig of tests/golden/euroc_rectify.json: (width, height, left, right) with each
    side a dict(K, D, R, P, equi)"""
    c = json.load(open(os.path.join(GOLDEN, "euroc_rectify.json")))
    left = dict(K=c["Kl"], D=c["Dl"], R=c["Rl"], P=c["P"], equi=False)
    right = dict(K=c["Kr"], D=c["Dr"], R=c["Rr"], P=c["P"], equi=False)
    return c["width"], c["height"], left, right


def inverse_PR(P, R):
    """R1: inverse(Pm R) by the first-row cofactor expansion"""
    f64 = np.float64
    pfx, pfy, pcx, pcy = (f64(v) for v in P)
    R = [f64(v) for v in R]
    m00, m01, m02 = pfx * R[0] + pcx * R[6], pfx * R[1] + pcx * R[7], pfx * R[2] + pcx * R[8]
    m10, m11, m12 = pfy * R[3] + pcy * R[6], pfy * R[4] + pcy * R[7], pfy * R[5] + pcy * R[8]
    m20, m21, m22 = R[6], R[7], R[8]
    c00 = m11 * m22 - m12 * m21
    c01 = m12 * m20 - m10 * m22
    c02 = m10 * m21 - m11 * m20
    det = m00 * c00 + m01 * c01 + m02 * c02
    d = f64(1.0) / det
    return [c00 * d, (m02 * m21 - m01 * m22) * d, (m01 * m12 - m02 * m11) * d,
            c01 * d, (m00 * m22 - m02 * m20) * d, (m02 * m10 - m00 * m12) * d,
            c02 * d, (m01 * m20 - m00 * m21) * d, (m00 * m11 - m01 * m10) * d]


def _round_sat(v):
    """R5: round half to even, saturating to int32 (NaN -> INT_MIN)"""
    r = np.rint(v)
    out = np.empty(r.shape, np.int64)
    lo = ~(r > -2147483648.0)
    hi = r >= 2147483647.0
    ok = ~(lo | hi)
    out[lo] = -2147483648
    out[hi] = 2147483647
    out[ok] = r[ok].astype(np.int64)
    return out


def maps(K, D, R, P, width, height, equi=False):
    """R1-R5: (map1 int16 [H][W][2], map2 uint16 [H][W])"""
    f64 = np.float64
    iR = inverse_PR(P, R)
    fx, fy, cx, cy = (f64(v) for v in K)
    Dz = [f64(v) for v in D] + [f64(0)] * (8 - len(D))
    i = np.arange(height, dtype=np.float64)
    # R2: column j holds the row's first ray after j serial additions
    X = np.empty((height, width)); Y = np.empty((height, width)); Wd = np.empty((height, width))
    _x, _y, _w = i * iR[1] + iR[2], i * iR[4] + iR[5], i * iR[7] + iR[8]
    for j in range(width):
        X[:, j], Y[:, j], Wd[:, j] = _x, _y, _w
        _x, _y, _w = _x + iR[0], _y + iR[3], _w + iR[6]
    with np.errstate(all="ignore"):
        if not equi:   # R3
            k1, k2, p1, p2, k3, k4, k5, k6 = Dz
            w = f64(1.0) / Wd
            x, y = X * w, Y * w
            x2, y2 = x * x, y * y
            r2, _2xy = x2 + y2, f64(2) * x * y
            kr = (f64(1) + ((k3 * r2 + k2) * r2 + k1) * r2) / (f64(1) + ((k6 * r2 + k5) * r2 + k4) * r2)
            xd = x * kr + p1 * _2xy + p2 * (r2 + f64(2) * x2)
            yd = y * kr + p1 * (r2 + f64(2) * y2) + p2 * _2xy
            u, v = fx * xd + cx, fy * yd + cy
        else:          # R4
            x, y = X / Wd, Y / Wd
            r = np.sqrt(x * x + y * y)
            th = np.array([math.atan(t) for t in r.reshape(-1)], np.float64).reshape(r.shape)
            th2 = th * th
            th4 = th2 * th2
            th6 = th4 * th2
            th8 = th4 * th4
            thd = th * (f64(1) + Dz[0] * th2 + Dz[1] * th4 + Dz[2] * th6 + Dz[3] * th8)
            scale = np.where(r == 0, f64(1), thd / np.where(r == 0, f64(1), r))
            u, v = fx * x * scale + cx, fy * y * scale + cy
        iu, iv = _round_sat(u * f64(32)), _round_sat(v * f64(32))   # R5
    map1 = np.stack([(iu >> 5) & 0xFFFF, (iv >> 5) & 0xFFFF], axis=-1).astype(np.uint16).view(np.int16)
    map2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map1, map2


def remap(src, map1, map2):
    """R6 on u8 images [..., H, W] (the maps shared by the leading axes)"""
    src = np.asarray(src, np.uint8)
    H, W = src.shape[-2:]
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    a, b = (map2 & 31).astype(np.int64), ((map2 >> 5) & 31).astype(np.int64)

    def tap(dy, dx):
        y, x = sy + dy, sx + dx
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        v = src[..., np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64)
        return np.where(inside, v, 0)

    acc = ((32 - a) * (32 - b) * tap(0, 0) + a * (32 - b) * tap(0, 1) + (32 - a) * b * tap(1, 0)
           + a * b * tap(1, 1) + 512) >> 10
    return acc.astype(np.uint8)


def random_images(n, height, width, seed):
    """u8 noise with runs of 0 and of 255 (so saturated neighbours meet every weight)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, height, width), dtype=np.uint8)
    for k in range(n):
        for val in (0, 255):
            for _ in range(6):
                y, x = int(rng.integers(0, height)), int(rng.integers(0, width))
                h, w = int(rng.integers(1, max(2, height // 4))), int(rng.integers(1, max(2, width // 3)))
                img[k, y:y + h, x:x + w] = val
    return img
