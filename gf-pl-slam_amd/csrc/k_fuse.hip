// k_fuse.hip — the candidate search of MapHandler::fuseLandmarksFromLocalMap
// (src/mapHandler.cpp:859-1056; include/gfpl.h gfpl_map_fuse_search, DESIGN.md §4l, ledger FU1-FU11).
//
//  k_fuse_select : the local landmarks whose projection under the pose of their first observing
//                  keyframe lies inside the image with z > 0 (:876-887 points, :968-984 lines, both
//                  endpoints), compacted in map order with their median descriptors.  The keyframe
//                  index is device data the host has not seen: a row whose index is outside
//                  [0, n_kf) is not selected, reads no pose and raises *bad_kf.
//  k_fuse_gate   : one selected row per lane: its second neighbour t of the knn-2 of the selected
//                  descriptors against themselves (k_knn2m, between the two launches), t != i, then
//                  the point gate (:909-919) or the line gate (:1024-1053); the accepted (i, t) are
//                  compacted in ascending i.
// Both are one workgroup of 1024 threads that walks the rows in chunks, as k_kf_map_filter and
// k_kf_gate do: keyframe-rate work, and the compaction must keep the order.  The counts stay on the
// device between the launches (the knn-2 reads them there), so a call synchronises once.
#include "gfpl_kernels.hpp"

namespace gfpl {

namespace {

// FU3: a size-3 sum as Eigen 3.3's unvectorised fixed-size reduction takes it
GFPL_DEV double sum3(double a0, double a1, double a2) { return a0 + (a1 + a2); }
GFPL_DEV double norm3(const double* v) { return sqrt(sum3(v[0] * v[0], v[1] * v[1], v[2] * v[2])); }
GFPL_DEV double dot3(const double* a, const double* b) { return sum3(a[0] * b[0], a[1] * b[1], a[2] * b[2]); }

// FU1 / FU2: T as written (T_kf_w, not inverted), strict comparisons
GFPL_DEV bool fuse_inside(const DevCam& cam, const double* T, const double* X) {
    double Pf[3], pf[2];
    se3_apply(T, X, Pf);
    projection(cam, Pf, pf);
    return pf[0] > 0 && pf[0] < cam.width && pf[1] > 0 && pf[1] < cam.height && Pf[2] > 0.0;
}

// FU6: |(p - x) - ((p - x) . d) d|
GFPL_DEV double fuse_point_line(const double* p, const double* x, const double* d) {
    const double w[3] = {p[0] - x[0], p[1] - x[1], p[2] - x[2]};
    const double s = dot3(w, d);
    const double r[3] = {w[0] - s * d[0], w[1] - s * d[1], w[2] - s * d[2]};
    return norm3(r);
}

}  // namespace

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_fuse_select(FuseSelect a) {
    __shared__ int scan[BLOCK / 64 + 1];
    const int stride = a.lines ? 6 : 3;
    int off = 0, bad = 0;
    for (int c0 = 0; c0 < a.n; c0 += BLOCK) {
        const int i = c0 + (int)threadIdx.x;
        int flag = 0;
        if (i < a.n) {
            const int kf = a.kf[i];
            if (kf < 0 || kf >= a.n_kf) {
                bad = 1;
            } else {
                const double* T = a.T_kf + 16 * (size_t)kf;
                const double* X = a.X + (size_t)stride * i;
                flag = fuse_inside(a.cam, T, X) && (!a.lines || fuse_inside(a.cam, T, X + 3));
            }
        }
        int tot;
        const int pos = off + block_exclusive_scan<BLOCK>(flag, scan, &tot);
        if (flag) {   // pos < n: at most one selected row per map row
            a.loc[pos] = i;
        }
        if (flag && a.desc_in) {   // (null for a map of one row: nothing is matched)
            const uint4* s4 = reinterpret_cast<const uint4*>(a.desc_in + 32 * (size_t)i);
            uint4* d4 = reinterpret_cast<uint4*>(a.desc_out + 32 * (size_t)pos);
            d4[0] = s4[0]; d4[1] = s4[1];
        }
        off += tot;
    }
    if (bad) *a.bad_kf = 1;   // (every writer stores the same value)
    if (threadIdx.x == 0) *a.count = off;
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_fuse_gate(FuseGate g) {
    __shared__ int scan[BLOCK / 64 + 1];
    const int n = min(*g.n_sel, g.cap);   // (uniform)
    const int stride = g.lines ? 6 : 3;
    int off = 0;
    for (int c0 = 0; n > 1 && c0 < n; c0 += BLOCK) {
        const int i = c0 + (int)threadIdx.x;
        int flag = 0, t = -1;
        if (i < n) t = g.idx[2 * i + 1];   // the second neighbour, as the reference takes it (lmatches_12[i][1])
        if (t >= 0 && t < n && t != i) {
            const double* A = g.X + (size_t)stride * g.loc[i];
            const double* B = g.X + (size_t)stride * g.loc[t];
            if (!g.lines) {
                // FU4
                const double d[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
                flag = norm3(d) < g.max_pp;
            } else {
                // FU5: unit directions by a division per component; a zero-length line gives NaN, which
                // fails every comparison below
                const double v1[3] = {A[3] - A[0], A[4] - A[1], A[5] - A[2]};
                const double v2[3] = {B[3] - B[0], B[4] - B[1], B[5] - B[2]};
                const double n1 = norm3(v1), n2 = norm3(v2);
                const double d1[3] = {v1[0] / n1, v1[1] / n1, v1[2] / n1};
                const double d2[3] = {v2[0] / n2, v2[1] / n2, v2[2] / n2};
                const double dd[3] = {d1[0] - d2[0], d1[1] - d2[1], d1[2] - d2[2]};
                const double Ld = norm3(dd);
                double dP, dQ;
                if (norm3(d1) > norm3(d2)) {   // FU7: two numbers within an ulp of 1, as written
                    dP = fuse_point_line(B, A, d1);
                    dQ = fuse_point_line(B + 3, A, d1);
                } else {
                    dP = fuse_point_line(A, B, d2);
                    dQ = fuse_point_line(A + 3, B, d2);
                }
                flag = Ld < g.max_dl && dP < g.max_pl && dQ < g.max_pl;
            }
        }
        int tot;
        const int pos = off + block_exclusive_scan<BLOCK>(flag, scan, &tot);
        if (flag) { g.pairs[2 * pos] = i; g.pairs[2 * pos + 1] = t; }   // pos < n <= cap
        off += tot;
    }
    if (threadIdx.x == 0) *g.count = off;
}

hipError_t launch_fuse_select(const FuseSelect& a, hipStream_t s) {
    hipLaunchKernelGGL(k_fuse_select<1024>, dim3(1), dim3(1024), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fuse_gate(const FuseGate& g, hipStream_t s) {
    hipLaunchKernelGGL(k_fuse_gate<1024>, dim3(1), dim3(1024), 0, s, g);
    return hipGetLastError();
}

}  // namespace gfpl
