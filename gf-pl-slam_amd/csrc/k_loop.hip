// k_loop.hip — loop-closure check of a candidate keyframe pair.
//
//  k_loop_closure : MapHandler::isLoopClosure with computeRelativePoseGN
//              (src/mapHandler.cpp:3078-3545): after the knn-2 launches of both kinds and
//              directions (k_knn2m), one workgroup per candidate pair
//              (a) compacts the mutual-best rows of each kind in kf0 order,
//              (b) runs the Gauss-Newton iterations from T_inc = I: the lanes evaluate a
//                  chunk of entries each into LDS rows (J / max(homog, |err|), |err|, w), and
//                  43 reduction lanes (36 H + 6 g + 1 e) add the rows IN LIST ORDER — the
//                  reference's accumulation order (pin N2), so H, g and e are its bits and
//                  the gates compare the same doubles; lane 0 solves and updates T_inc,
//              (c) flags the outliers under the final T_inc,
//              (d) evaluates the five gates and writes the result record.
// Keyframe-rate work, batched over the candidates a keyframe tick yields.
#include "gfpl_kernels.hpp"

namespace gfpl {

namespace {

constexpr int LOOP_BLOCK = 256;
constexpr int LOOP_ROW = 8;     // doubles per chunk row: J[6], |err|, w
constexpr int LOOP_NRED = 43;   // 36 H + 6 g + 1 e

struct LoopState {
    double T[16], H[36], x[6];
    double e, err_prev;
    int stop, iters;
};

// point entry (src/mapHandler.cpp:3312-3339): row = J_aux / max(homog, |err|), |err|, w
GFPL_DEV void loop_point_row(const DevCam& cam, double homog, const double* T, const double* P, const double* obs,
                             double* row) {
    double Pc[3], uv[2], J[6];
    se3_apply(T, P, Pc);
    projection(cam, Pc, uv);
    const double dx = uv[0] - obs[0], dy = uv[1] - obs[1];
    const double nrm = sqrt(dx * dx + dy * dy);
    poseJac(cam, homog, Pc, dx, dy, J);
    const double d = ref_max(homog, nrm);
#pragma unroll
    for (int i = 0; i < 6; ++i) row[i] = J[i] / d;
    row[6] = nrm;
    row[7] = 1.0 / (1.0 + (nrm * nrm) * 1.0);   // sigma2 = 1.0: the (P, pl_obs) constructor's default
}

GFPL_DEV void loop_line_err(const DevCam& cam, const double* T, const double* sP, const double* eP, const double* l,
                            double* sc, double* ec, double* err) {
    double su[2], eu[2];
    se3_apply(T, sP, sc);
    projection(cam, sc, su);
    se3_apply(T, eP, ec);
    projection(cam, ec, eu);
    err[0] = (l[0] * su[0] + l[1] * su[1]) + l[2];
    err[1] = (l[0] * eu[0] + l[1] * eu[1]) + l[2];
}

// line entry (:3349-3397)
GFPL_DEV void loop_line_row(const DevCam& cam, double homog, const double* T, const double* sP, const double* eP,
                            const double* l, double* row) {
    double sc[3], ec[3], err[2], Js[6], Je[6];
    loop_line_err(cam, T, sP, eP, l, sc, ec, err);
    const double nrm = sqrt(err[0] * err[0] + err[1] * err[1]);
    poseJac(cam, homog, sc, l[0], l[1], Js);
    poseJac(cam, homog, ec, l[0], l[1], Je);
    const double d = ref_max(homog, nrm);
#pragma unroll
    for (int i = 0; i < 6; ++i) row[i] = (Js[i] * err[0] + Je[i] * err[1]) / d;
    row[6] = nrm;
    row[7] = 1.0 / (1.0 + (nrm * nrm) * 1.0);
}

// mutual-best rows of one kind, compacted in kf0 order into pairs; returns their count (every thread)
template <int BLOCK>
GFPL_DEV int loop_compact(int n0, const int32_t* i12, const int32_t* i21, int32_t* pairs, int* scan) {
    int off = 0;
    for (int c0 = 0; c0 < n0; c0 += BLOCK) {
        const int q = c0 + (int)threadIdx.x;
        int flag = 0, t = 0;
        if (q < n0) {
            t = i12[2 * q];
            flag = i21[2 * t] == q;
        }
        int tot;
        const int pos = off + block_exclusive_scan<BLOCK>(flag, scan, &tot);
        if (flag) { pairs[2 * pos] = q; pairs[2 * pos + 1] = t; }
        off += tot;
    }
    return off;
}

}  // namespace

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_loop_closure(LoopArgs a) {
    __shared__ int scan[BLOCK / 64 + 1];
    __shared__ double rows[BLOCK * LOOP_ROW];
    __shared__ double red[2][LOOP_NRED + 1];
    __shared__ LoopState S;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const LoopPair pr = a.pairs[b];
    int32_t* ppairs = a.pt_pairs + 2 * (size_t)a.pt_cap * b;
    int32_t* lpairs = a.ls_pairs + 2 * (size_t)a.ls_cap * b;
    uint8_t* pinl = a.pt_inlier + (size_t)a.pt_cap * b;
    uint8_t* linl = a.ls_inlier + (size_t)a.ls_cap * b;

    // (a) mutual best, both kinds (:3136-3166, :3206-3240); fewer than two rows on a side: none (U4)
    const int np = pr.pi12 ? loop_compact<BLOCK>(pr.n0_pt, pr.pi12, pr.pi21, ppairs, scan) : 0;
    const int nl = pr.li12 ? loop_compact<BLOCK>(pr.n0_ls, pr.li12, pr.li21, lpairs, scan) : 0;
    if (tid < 16) S.T[tid] = (tid % 5 == 0) ? 1.0 : 0.0;
    if (tid < 36) S.H[tid] = 0.0;
    if (tid < 6) S.x[tid] = 0.0;
    if (tid == 0) { S.e = 0.0; S.err_prev = 999999999.9; S.stop = 0; S.iters = 0; }
    __syncthreads();   // the pairs (global) and S are visible to the block

    // what reduction lane tid adds of a row: (J_i J_k) w, (J_i |err|) w or (|err| |err|) w
    const int ra = tid < 36 ? tid / 6 : (tid < 42 ? tid - 36 : 6);
    const int rb = tid < 36 ? tid % 6 : 6;

    // (b) Gauss-Newton (:3301-3419)
    for (int it = 0; it < a.max_iters; ++it) {
        double T[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) T[i] = S.T[i];
        for (int kind = 0; kind < 2; ++kind) {
            const int cnt = kind == 0 ? np : nl;
            double acc = 0.0;
            for (int c0 = 0; c0 < cnt; c0 += BLOCK) {
                const int k = c0 + tid;
                if (k < cnt) {
                    double row[LOOP_ROW];
                    if (kind == 0) {
                        const int q = ppairs[2 * k], t = ppairs[2 * k + 1];
                        loop_point_row(a.cam, a.homog_th, T, pr.P0 + 3 * (size_t)q, pr.pl1 + 2 * (size_t)t, row);
                    } else {
                        const int q = lpairs[2 * k], t = lpairs[2 * k + 1];
                        loop_line_row(a.cam, a.homog_th, T, pr.sP0 + 3 * (size_t)q, pr.eP0 + 3 * (size_t)q,
                                      pr.le1 + 3 * (size_t)t, row);
                    }
#pragma unroll
                    for (int i = 0; i < LOOP_ROW; ++i) rows[tid * LOOP_ROW + i] = row[i];
                }
                __syncthreads();
                if (tid < LOOP_NRED) {
                    const int m = min(BLOCK, cnt - c0);
                    for (int r = 0; r < m; ++r) {
                        const double* rw = rows + r * LOOP_ROW;
                        acc = acc + (rw[ra] * rw[rb]) * rw[7];
                    }
                }
                __syncthreads();
            }
            if (tid < LOOP_NRED) red[kind][tid] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            double H[36], g[6];
#pragma unroll
            for (int i = 0; i < 36; ++i) { H[i] = red[0][i] + red[1][i]; S.H[i] = H[i]; }
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = red[0][36 + i] + red[1][36 + i];
            double e = red[0][42] + red[1][42];
            e = e / (double)(nl + np);
            S.e = e;
            S.iters = it + 1;
            const double eps = 2.220446049250313e-16;
            if (fabs(e - S.err_prev) < eps || e < eps) {
                S.stop = 1;
            } else {
                double x[6], E[16], Ei[16], Tn[16];
                ldlt_solve6_one_lane(H, g, x);
                expmap_se3(x, E);
                inverse_se3(E, Ei);
                mat4_mul(T, Ei, Tn);
#pragma unroll
                for (int i = 0; i < 16; ++i) S.T[i] = Tn[i];
#pragma unroll
                for (int i = 0; i < 6; ++i) S.x[i] = x[i];
                const double n2 = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5];
                if (sqrt(n2) < eps) S.stop = 1;
                S.err_prev = e;
            }
        }
        __syncthreads();
        if (S.stop) break;
    }

    // (c) outlier pass under the final T_inc (:3425-3456): |err| sqrt(1.0) > sqrt(7.815)
    double T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = S.T[i];
    const double chi = sqrt(7.815);
    int ninl[2];
    for (int kind = 0; kind < 2; ++kind) {
        const int cnt = kind == 0 ? np : nl;
        int tot_in = 0;
        for (int c0 = 0; c0 < cnt; c0 += BLOCK) {
            const int k = c0 + tid;
            int in = 0;
            if (k < cnt) {
                double nrm;
                if (kind == 0) {
                    const int q = ppairs[2 * k], t = ppairs[2 * k + 1];
                    double Pc[3], uv[2];
                    se3_apply(T, pr.P0 + 3 * (size_t)q, Pc);
                    projection(a.cam, Pc, uv);
                    const double dx = uv[0] - pr.pl1[2 * (size_t)t], dy = uv[1] - pr.pl1[2 * (size_t)t + 1];
                    nrm = sqrt(dx * dx + dy * dy);
                } else {
                    const int q = lpairs[2 * k], t = lpairs[2 * k + 1];
                    double sc[3], ec[3], err[2];
                    loop_line_err(a.cam, T, pr.sP0 + 3 * (size_t)q, pr.eP0 + 3 * (size_t)q, pr.le1 + 3 * (size_t)t, sc, ec,
                                  err);
                    nrm = sqrt(err[0] * err[0] + err[1] * err[1]);
                }
                in = !(nrm * 1.0 > chi);
                (kind == 0 ? pinl : linl)[k] = (uint8_t)in;
            }
            int tot;
            (void)block_exclusive_scan<BLOCK>(in, scan, &tot);
            tot_in += tot;
        }
        ninl[kind] = tot_in;
    }

    // (d) gates and the result record (:3420, :3461-3540)
    if (tid == 0) {
        gfpl_loop_result r;
        double x_inc[6], Hm[36], cov[36], w[6];
        logmap_se3(T, x_inc);
#pragma unroll
        for (int i = 0; i < 36; ++i) Hm[i] = S.H[i];
        inverse6(Hm, cov);
        eig_sym<6>(cov, w);
        const double e = S.e;
        const int N = np + nl, N_inl = ninl[0] + ninl[1];
        const double ratio = (double)N_inl / (double)N;
        const double trs = sqrt((x_inc[0] * x_inc[0] + x_inc[1] * x_inc[1]) + x_inc[2] * x_inc[2]);
        const double rot = (sqrt((x_inc[3] * x_inc[3] + x_inc[4] * x_inc[4]) + x_inc[5] * x_inc[5]) * 180.0) /
                           3.1415926535897932384626433832795;
        int gates = 0;
        if (e < a.prm.lc_res) gates |= 1;
        if (w[5] < a.prm.lc_unc) gates |= 2;
        if (ratio > a.prm.lc_inl) gates |= 4;
        if (trs < a.prm.lc_trs) gates |= 8;
        if (rot < a.prm.lc_rot) gates |= 16;
        r.is_lc = gates == 31;
        r.gates = gates;
        r.n_pt = np; r.n_ls = nl;
        r.n_pt_inl = ninl[0]; r.n_ls_inl = ninl[1];
        r.iters = S.iters; r.pad = 0;
        r.e = e; r.unc = w[5]; r.ratio_inliers = ratio; r.trs = trs; r.rot = rot;
        double pose[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (gates == 31) {
            double Ti[16];
            inverse_se3(T, Ti);
            logmap_se3(Ti, pose);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) { r.x_inc[i] = x_inc[i]; r.pose_inc[i] = pose[i]; }
#pragma unroll
        for (int i = 0; i < 16; ++i) r.T_inc[i] = T[i];
        a.out[b] = r;
    }
}

hipError_t launch_loop_closure(const LoopArgs& a, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_loop_closure<LOOP_BLOCK>, dim3(n), dim3(LOOP_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace gfpl
