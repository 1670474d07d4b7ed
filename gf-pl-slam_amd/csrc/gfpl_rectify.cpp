// gfpl_rectify.cpp — host-side builder of the stereo rectification maps (ledger R1-R5,
// DESIGN.md §4f): what PinholeStereoCamera's constructor gets from
// cv::initUndistortRectifyMap(K, D, R, P, size, CV_16SC2, map1, map2), or from
// cv::fisheye::initUndistortRectifyMap for the equidistant model
// (src/pinholeStereoCamera.cpp:24-119), once per camera, in plain f64.
//
// The ray of pixel (j, i) is accumulated serially along the row (R2): the order of
// those additions is part of the result, so the maps are built here and uploaded, never
// on the device.  No HIP in this file: it also serves callers without a GPU.
#include "../../include/gfpl.h"

#include <climits>
#include <cmath>

namespace {

// R5: cvRound-style conversion, round-half-even (the default rounding mode), saturating
inline int round_sat(double v) {
    const double r = std::nearbyint(v);
    if (!(r > -2147483648.0)) return INT_MIN;   // also NaN
    if (r >= 2147483647.0) return INT_MAX;
    return (int)r;
}

}  // namespace

extern "C" int gfpl_rectify_maps_host(const gfpl_rectify_side* s, int width, int height, int16_t* map1,
                                      uint16_t* map2) {
    if (!s || !map1 || !map2 || width < 1 || height < 1 || width > 8192 || height > 8192) return GFPL_E_INVALID;
    if (s->model != 0 && s->model != 1) return GFPL_E_INVALID;
    if (s->model == 0 && s->n_dist != 4 && s->n_dist != 5 && s->n_dist != 8) return GFPL_E_UNSUPPORTED;
    if (s->model == 1 && s->n_dist != 4) return GFPL_E_UNSUPPORTED;
    double D[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < s->n_dist; ++i) D[i] = s->D[i];
    const double fx = s->K[0], fy = s->K[1], cx = s->K[2], cy = s->K[3];
    const double* R = s->R;
    // R1: m = Pm R with Pm = [pfx 0 pcx; 0 pfy pcy; 0 0 1], then the closed-form inverse
    const double pfx = s->P[0], pfy = s->P[1], pcx = s->P[2], pcy = s->P[3];
    const double m00 = pfx * R[0] + pcx * R[6], m01 = pfx * R[1] + pcx * R[7], m02 = pfx * R[2] + pcx * R[8];
    const double m10 = pfy * R[3] + pcy * R[6], m11 = pfy * R[4] + pcy * R[7], m12 = pfy * R[5] + pcy * R[8];
    const double m20 = R[6], m21 = R[7], m22 = R[8];
    const double c00 = m11 * m22 - m12 * m21;
    const double c01 = m12 * m20 - m10 * m22;
    const double c02 = m10 * m21 - m11 * m20;
    const double det = m00 * c00 + m01 * c01 + m02 * c02;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return GFPL_E_INVALID;
    const double d = 1.0 / det;
    const double iR[9] = {c00 * d, (m02 * m21 - m01 * m22) * d, (m01 * m12 - m02 * m11) * d,
                          c01 * d, (m00 * m22 - m02 * m20) * d, (m02 * m10 - m00 * m12) * d,
                          c02 * d, (m01 * m20 - m00 * m21) * d, (m00 * m11 - m01 * m10) * d};
    const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4], k4 = D[5], k5 = D[6], k6 = D[7];
    for (int i = 0; i < height; ++i) {
        // R2: the row's first ray, then one serial addition per pixel
        double _x = i * iR[1] + iR[2], _y = i * iR[4] + iR[5], _w = i * iR[7] + iR[8];
        int16_t* m1 = map1 + 2 * (size_t)i * width;
        uint16_t* m2 = map2 + (size_t)i * width;
        for (int j = 0; j < width; ++j, _x += iR[0], _y += iR[3], _w += iR[6]) {
            double u, v;
            if (s->model == 0) {   // R3
                const double w = 1. / _w, x = _x * w, y = _y * w;
                const double x2 = x * x, y2 = y * y;
                const double r2 = x2 + y2, _2xy = 2 * x * y;
                const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
                const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
                const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
                u = fx * xd + cx;
                v = fy * yd + cy;
            } else {               // R4 (fisheye coefficients k1..k4 = D[0..3])
                const double x = _x / _w, y = _y / _w;
                const double r = std::sqrt(x * x + y * y);
                const double th = std::atan(r);
                const double th2 = th * th, th4 = th2 * th2, th6 = th4 * th2, th8 = th4 * th4;
                const double thd = th * (1 + D[0] * th2 + D[1] * th4 + D[2] * th6 + D[3] * th8);
                const double scale = (r == 0) ? 1.0 : thd / r;
                u = fx * x * scale + cx;
                v = fy * y * scale + cy;
            }
            // R5: 5 fractional bits; arithmetic shift and two's-complement mask of negative values
            const int iu = round_sat(u * 32), iv = round_sat(v * 32);
            m1[2 * j] = (int16_t)(uint16_t)((unsigned)(iu >> 5) & 0xFFFFu);
            m1[2 * j + 1] = (int16_t)(uint16_t)((unsigned)(iv >> 5) & 0xFFFFu);
            m2[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
        }
    }
    return GFPL_OK;
}
