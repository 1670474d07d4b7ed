// k_lba.hip — local bundle adjustment of a keyframe tick's local map.
//
//  k_lba : MapHandler::levMarquardtOptimizationLBA (src/mapHandler.cpp:1217-1713), one workgroup
//          per problem, the whole Levenberg-Marquardt loop on the device.  Per iteration
//          (a) the lanes linearise a chunk of observations each into LDS rows (J_pose, J_landmark,
//              |err|, w) and 42 reduction lanes per local keyframe add the rows of their keyframe IN
//              LIST ORDER (points, then lines) — the reference's += order (pin N2), so the pose blocks,
//              their gradient and err have its bits; one more lane adds err,
//          (b) a lane per landmark adds its contiguous observations in order into its block V, its
//              gradient and its coupling blocks W,
//          (c) lane 0 forms int Hmax and lambda (pre-pass) or the stop tests,
//          (d) a lane per landmark damps and inverts V (inverse3 / inverse6) and forms V^-1 g, V^-1 W,
//          (e) the reduced pose system S = U - sum_j W_j V_j^-1 W_j^T (lower triangle) and its right-hand
//              side are formed in LDS, an entry per lane, landmarks in ascending order,
//          (f) LDL^T of S without pivoting and the two triangular solves, a row per lane,
//          (g) back-substitution and squared step per landmark; lane 0 applies the lambda rule,
//          (h) X is updated (poses through expmap / inverse / logmap, landmarks by addition).
//          Every sum's order is a function of the problem alone: no floating-point atomics.
//          DESIGN.md §4h, ledger BA1-BA14.
#include "gfpl_ba.hpp"

namespace gfpl {

namespace {

constexpr int LBA_NACC = (LBA_MAX_KFS * 42 + 1 + LBA_BLOCK - 1) / LBA_BLOCK;   // reduction entries per lane
enum { SI_SING = BA_SI_DONE + 1, SI_ACCEPT };   // the LBA's words after the BA_SI_* prefix

// the landmark blocks are inverted explicitly here (the GBA factorises them, ledger GB11): not shared
template <int D>
GFPL_DEV void lba_invert(const double* A, double* Ai);
template <>
GFPL_DEV void lba_invert<3>(const double* A, double* Ai) { inverse3(A, Ai); }
template <>
GFPL_DEV void lba_invert<6>(const double* A, double* Ai) { inverse6(A, Ai); }

// (b) landmark j of D rows: V, g, W of its observations in list order, its mask, its largest |diagonal|
template <int D>
GFPL_DEV double lba_landmark_sums(const LbaProb& pr, int j, size_t voff, size_t goff, size_t woff) {
    const int nkf = pr.n.n_kf;
    const int o0 = pr.lm_start[j], o1 = pr.lm_start[j + 1];
    int mask = 0;
    for (int o = o0; o < o1; ++o) {
        const int s = pr.obs_kf[o];
        if (s >= 0) mask |= 1 << s;
    }
    double* W = pr.m.W + woff;
    for (int s = 0; s < nkf; ++s)
        if ((mask >> s) & 1)
            for (int i = 0; i < D * 6; ++i) W[s * (D * 6) + i] = 0.0;
    double V[D * D], g[D];
#pragma unroll
    for (int i = 0; i < D * D; ++i) V[i] = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) g[i] = 0.0;
    for (int o = o0; o < o1; ++o) {
        const double* rw = pr.m.rows + (size_t)o * LBA_ROW;
        double JT[6], JL[D];
#pragma unroll
        for (int i = 0; i < 6; ++i) JT[i] = rw[i];
#pragma unroll
        for (int i = 0; i < D; ++i) JL[i] = rw[6 + i];
        const double nrm = rw[12], w = rw[13];
#pragma unroll
        for (int p = 0; p < D; ++p) {
            g[p] = g[p] + (JL[p] * nrm) * w;
#pragma unroll
            for (int q = 0; q < D; ++q) V[p * D + q] = V[p * D + q] + (JL[p] * JL[q]) * w;
        }
        const int s = pr.obs_kf[o];
        if (s >= 0) {
            double* Ws = W + s * (D * 6);
#pragma unroll
            for (int p = 0; p < D; ++p)
#pragma unroll
                for (int k = 0; k < 6; ++k) Ws[p * 6 + k] = Ws[p * 6 + k] + (JL[p] * JT[k]) * w;
        }
    }
    double dmax = 0.0;
#pragma unroll
    for (int i = 0; i < D * D; ++i) pr.m.V[voff + i] = V[i];
#pragma unroll
    for (int p = 0; p < D; ++p) {
        pr.m.glm[goff + p] = g[p];
        const double a = fabs(V[p * D + p]);
        if (a > dmax) dmax = a;
    }
    pr.m.mask[j] = mask;
    return dmax;
}

// (d) damp, invert, V^-1 g and V^-1 W; false when a pivot is not positive and finite
template <int D>
GFPL_DEV bool lba_landmark_invert(const LbaProb& pr, int j, double lambda, size_t voff, size_t goff, size_t woff) {
    double V[D * D], Vi[D * D];
#pragma unroll
    for (int i = 0; i < D * D; ++i) V[i] = pr.m.V[voff + i];
    bool ok = true;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        V[p * D + p] = V[p * D + p] + lambda * V[p * D + p];
        ok = ok && V[p * D + p] > 0.0 && ref_finite(V[p * D + p]);
    }
    lba_invert<D>(V, Vi);
#pragma unroll
    for (int i = 0; i < D * D; ++i) {
        ok = ok && ref_finite(Vi[i]);
        pr.m.Vi[voff + i] = Vi[i];
    }
#pragma unroll
    for (int p = 0; p < D; ++p) {
        double t = Vi[p * D] * pr.m.glm[goff];
#pragma unroll
        for (int q = 1; q < D; ++q) t = t + Vi[p * D + q] * pr.m.glm[goff + q];
        pr.m.z[goff + p] = t;
    }
    const int mask = pr.m.mask[j];
    for (int s = 0; s < pr.n.n_kf; ++s) {
        if (!((mask >> s) & 1)) continue;
        const double* Ws = pr.m.W + woff + s * (D * 6);
        double* Ys = pr.m.Y + woff + s * (D * 6);
        for (int k = 0; k < 6; ++k) {
            double wk[D];
#pragma unroll
            for (int q = 0; q < D; ++q) wk[q] = Ws[q * 6 + k];
#pragma unroll
            for (int p = 0; p < D; ++p) {
                double t = Vi[p * D] * wk[0];
#pragma unroll
                for (int q = 1; q < D; ++q) t = t + Vi[p * D + q] * wk[q];
                Ys[p * 6 + k] = t;
            }
        }
    }
    return ok;
}

// (g) DX_j = V_j^-1 (g_j - W_j DX_kf), keyframes of the mask ascending; returns |DX_j|^2
template <int D>
GFPL_DEV double lba_landmark_back(const LbaProb& pr, int j, const double* dxk, size_t voff, size_t goff, size_t woff,
                                  size_t xoff) {
    double u[D];
#pragma unroll
    for (int p = 0; p < D; ++p) u[p] = pr.m.glm[goff + p];
    const int mask = pr.m.mask[j];
    for (int s = 0; s < pr.n.n_kf; ++s) {
        if (!((mask >> s) & 1)) continue;
        const double* Ws = pr.m.W + woff + s * (D * 6);
#pragma unroll
        for (int p = 0; p < D; ++p)
#pragma unroll
            for (int k = 0; k < 6; ++k) u[p] = u[p] - Ws[p * 6 + k] * dxk[s * 6 + k];
    }
    double n2 = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        double t = pr.m.Vi[voff + p * D] * u[0];
#pragma unroll
        for (int q = 1; q < D; ++q) t = t + pr.m.Vi[voff + p * D + q] * u[q];
        pr.m.DX[xoff + p] = t;
        n2 = p == 0 ? t * t : n2 + t * t;
    }
    return n2;
}

}  // namespace

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_lba(LbaArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const LbaLds L(smem, a.lds_kfs);
    const int tid = threadIdx.x;
    const LbaProb pr = a.probs[blockIdx.x];
    const int nkf = pr.n.n_kf, npt = pr.n.n_pt, nls = pr.n.n_ls, nlm = npt + nls;
    const int npo = pr.n.n_pt_obs, nobs = npo + pr.n.n_ls_obs;
    const int n6 = 6 * nkf;
    const size_t N = (size_t)n6 + 3 * (size_t)npt + 6 * (size_t)nls;
    const double eps = 2.220446049250313e-16;
    double* X = pr.m.X;

    // X = [x_kf | point3D | line3D] (:1111-1209)
    for (size_t i = tid; i < N; i += BLOCK) {
        double v;
        if (i < (size_t)n6) v = pr.x_kf[i];
        else if (i < (size_t)n6 + 3 * (size_t)npt) v = pr.pt[i - n6];
        else v = pr.ls[i - n6 - 3 * (size_t)npt];
        X[i] = v;
    }
    if (tid == 0) {
        ba_state_init(L.sd, L.si, a.prm.lambda_lm);
        pr.m.state[0] = 0;
    }
    __syncthreads();

    const int nred = nkf * 42 + 1;
    for (int it = 0;; ++it) {
        // the iterations read the poses from X (:1480); the pre-pass and every line term read T_kf_w (:1255, :1558)
        if (it > 0 && tid < nkf) {
            double E[16], Ei[16];
            expmap_se3(X + 6 * tid, E);
            inverse_se3(E, Ei);
#pragma unroll
            for (int i = 0; i < 16; ++i) L.Tinv[16 * tid + i] = Ei[i];
        }
        if (tid == 0) L.si[SI_SING] = 0;
        __syncthreads();

        // (a) rows, pose blocks and err
        double acc[LBA_NACC];
#pragma unroll
        for (int u = 0; u < LBA_NACC; ++u) acc[u] = 0.0;
        for (int c0 = 0; c0 < nobs; c0 += BLOCK) {
            const int o = c0 + tid;
            if (o < nobs) {
                const int s = pr.obs_kf[o], j = pr.obs_lm[o];
                double row[LBA_ROW], Ti[16];
                const bool line = o >= npo;
                if (it > 0 && !line && s >= 0) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) Ti[i] = L.Tinv[16 * s + i];
                } else {
                    const double* T = s >= 0 ? pr.T_kf + 16 * (size_t)s : pr.T_fix + 16 * (size_t)(-1 - s);
                    double Tl[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) Tl[i] = T[i];
                    inverse_se3(Tl, Ti);
                }
                if (!line) {
                    const double* Xw = it > 0 ? X + n6 + 3 * (size_t)j : pr.pt + 3 * (size_t)j;
                    double P[3] = {Xw[0], Xw[1], Xw[2]};
                    double ob[2] = {pr.pt_obs[2 * (size_t)o], pr.pt_obs[2 * (size_t)o + 1]};
                    ba_point_row(a.cam, a.homog_th, Ti, P, ob, pr.pt_sigma[o], row);
                } else {
                    const size_t ol = (size_t)(o - npo);
                    const double* Lw = pr.ls + 6 * (size_t)(j - npt);
                    double PQ[6], l[3] = {pr.ls_obs[3 * ol], pr.ls_obs[3 * ol + 1], pr.ls_obs[3 * ol + 2]};
#pragma unroll
                    for (int i = 0; i < 6; ++i) PQ[i] = Lw[i];
                    ba_line_row(a.cam, it > 0 ? 0.0000001 : a.homog_th, Ti, PQ, l, pr.ls_sigma[ol], row);
                }
                double* gr = pr.m.rows + (size_t)o * LBA_ROW;
#pragma unroll
                for (int i = 0; i < LBA_ROW; ++i) { L.rows[tid * LBA_ROW + i] = row[i]; gr[i] = row[i]; }
                L.slot[tid] = s;
            }
            __syncthreads();
            const int m = min(BLOCK, nobs - c0);
#pragma unroll
            for (int u = 0; u < LBA_NACC; ++u) {
                const int t = tid + u * BLOCK;
                if (t < nred - 1) {
                    const int kf = t / 42, e = t % 42;
                    const int ra = e < 36 ? e / 6 : e - 36, rb = e < 36 ? e % 6 : 12;
                    double v = acc[u];
                    for (int r = 0; r < m; ++r)
                        if (L.slot[r] == kf) {
                            const double* rw = L.rows + r * LBA_ROW;
                            v = v + (rw[ra] * rw[rb]) * rw[13];
                        }
                    acc[u] = v;
                } else if (t == nred - 1) {
                    double v = acc[u];
                    for (int r = 0; r < m; ++r) {
                        const double* rw = L.rows + r * LBA_ROW;
                        v = v + (rw[12] * rw[12]) * rw[13];
                    }
                    acc[u] = v;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < LBA_NACC; ++u) {
            const int t = tid + u * BLOCK;
            if (t < nred - 1) {
                const int kf = t / 42, e = t % 42;
                if (e < 36) pr.m.U[kf * 36 + e] = acc[u];
                else pr.m.gk[kf * 6 + (e - 36)] = acc[u];
            } else if (t == nred - 1) {
                L.sd[BA_SD_ERRSUM] = acc[u];
            }
        }
        __syncthreads();   // the rows (global) are visible to the block

        // (b) landmark blocks
        double dmax = 0.0;
        for (int j = tid; j < npt; j += BLOCK) {
            const double d = lba_landmark_sums<3>(pr, j, 9 * (size_t)j, 3 * (size_t)j, (size_t)j * nkf * 18);
            if (d > dmax) dmax = d;
        }
        for (int j = tid; j < nls; j += BLOCK) {
            const double d = lba_landmark_sums<6>(pr, npt + j, 9 * (size_t)npt + 36 * (size_t)j, 3 * (size_t)npt + 6 * (size_t)j,
                                                  (size_t)npt * nkf * 18 + (size_t)j * nkf * 36);
            if (d > dmax) dmax = d;
        }
        if (it == 0) L.red[tid] = dmax;
        __syncthreads();

        // (c) int Hmax and lambda (:1427-1435) or the stop tests (:1650-1653)
        if (tid == 0) {
            pr.m.state[0] = it;
            if (it == 0) {
                L.sd[BA_SD_ERR] = L.sd[BA_SD_ERRSUM] / 0.0;   // err /= (Npt_obs + Nls_obs), both 0 for good
                double hm = 0.0;
                for (int i = 0; i < BLOCK; ++i)
                    if (L.red[i] > hm) hm = L.red[i];
                for (int i = 0; i < n6; ++i) {
                    const double d = fabs(pr.m.U[(i / 6) * 36 + (i % 6) * 7]);
                    if (d > hm) hm = d;
                }
                if (hm >= 2147483648.0) {
                    L.si[BA_SI_STATUS] |= GFPL_LBA_HMAX_RANGE;
                    L.si[BA_SI_HMAX] = 0x7fffffff;
                    L.si[BA_SI_DONE] = 1;
                } else {
                    const int h = (int)hm;
                    L.si[BA_SI_HMAX] = h;
                    L.sd[BA_SD_LAMBDA] = L.sd[BA_SD_LAMBDA] * (double)h;
                }
            } else {
                const double err = L.sd[BA_SD_ERRSUM] / (double)(npt + nls);
                L.sd[BA_SD_ERR] = err;
                if (fabs(err - L.sd[BA_SD_ERRPREV]) < eps) { L.si[BA_SI_STOP] = GFPL_LBA_STOP_DERR; L.si[BA_SI_DONE] = 1; }
                else if (err < eps) { L.si[BA_SI_STOP] = GFPL_LBA_STOP_ERR; L.si[BA_SI_DONE] = 1; }
                L.si[BA_SI_ITERS] = it;
            }
        }
        __syncthreads();
        if (L.si[BA_SI_DONE]) break;
        const double lambda = L.sd[BA_SD_LAMBDA];

        // (d) damped landmark blocks inverted
        {
            bool ok = true;
            for (int j = tid; j < npt; j += BLOCK)
                ok = lba_landmark_invert<3>(pr, j, lambda, 9 * (size_t)j, 3 * (size_t)j, (size_t)j * nkf * 18) && ok;
            for (int j = tid; j < nls; j += BLOCK)
                ok = lba_landmark_invert<6>(pr, npt + j, lambda, 9 * (size_t)npt + 36 * (size_t)j,
                                            3 * (size_t)npt + 6 * (size_t)j, (size_t)npt * nkf * 18 + (size_t)j * nkf * 36) && ok;
            if (!ok) atomicOr(&L.si[SI_SING], 1);
        }
        __syncthreads();

        // (e) S (lower triangle) and its right-hand side, landmarks ascending, keyframes by the mask; S, its
        // factorisation and the solve stay in LDS (the GBA's take a launch per block column): not shared
        // (an entry belongs to one lane throughout; the masks pass through LDS a chunk at a time)
        if (!L.si[SI_SING]) {
            const int ne = n6 * (n6 + 1);
            for (int e = tid; e < ne; e += BLOCK) {
                const int r = e / (n6 + 1), c = e % (n6 + 1);
                if (c < n6 && c > r) continue;
                const int ka = r / 6, ri = r % 6, kb = c / 6, ci = c % 6;
                if (c == n6) L.gr[r] = pr.m.gk[r];
                else if (ka == kb) {
                    const double u = pr.m.U[ka * 36 + ri * 6 + ci];
                    L.S[r * n6 + c] = r == c ? u + lambda * u : u;
                } else L.S[r * n6 + c] = 0.0;
            }
            for (int j0 = 0; j0 < nlm; j0 += BLOCK) {
                __syncthreads();
                if (j0 + tid < nlm) L.slot[tid] = pr.m.mask[j0 + tid];
                __syncthreads();
                const int mj = min(BLOCK, nlm - j0);
                for (int e = tid; e < ne; e += BLOCK) {
                    const int r = e / (n6 + 1), c = e % (n6 + 1);
                    if (c < n6 && c > r) continue;
                    const bool rhs = c == n6;
                    const int ka = r / 6, ri = r % 6, kb = rhs ? ka : c / 6, ci = rhs ? 0 : c % 6;
                    double val = rhs ? L.gr[r] : L.S[r * n6 + c];
                    const int need = (1 << ka) | (1 << kb);
                    for (int jj = 0; jj < mj; ++jj) {
                        if ((L.slot[jj] & need) != need) continue;
                        const int j = j0 + jj;
                        const bool pt = j < npt;
                        const int D = pt ? 3 : 6;
                        const size_t woff = pt ? (size_t)j * nkf * 18 : (size_t)npt * nkf * 18 + (size_t)(j - npt) * nkf * 36;
                        const size_t goff = pt ? 3 * (size_t)j : 3 * (size_t)npt + 6 * (size_t)(j - npt);
                        const double* Wa = pr.m.W + woff + ka * (D * 6) + ri;
                        const double* Yb = rhs ? pr.m.z + goff : pr.m.Y + woff + kb * (D * 6) + ci;
                        const int ys = rhs ? 1 : 6;
                        double t = Wa[0] * Yb[0];
                        for (int p = 1; p < D; ++p) t = t + Wa[p * 6] * Yb[p * ys];
                        val = val - t;
                    }
                    if (rhs) L.gr[r] = val;
                    else L.S[r * n6 + c] = val;
                }
            }
        }
        __syncthreads();

        // (f) LDL^T without pivoting: column k of L below the diagonal, D[k] the pivot
        if (!L.si[SI_SING]) {
            for (int k = 0; k < n6; ++k) {
                const int i = k + tid;
                if (i < n6) {
                    double v = L.S[i * n6 + k];
                    for (int m = 0; m < k; ++m) v = v - (L.S[i * n6 + m] * L.S[k * n6 + m]) * L.D[m];
                    L.S[i * n6 + k] = v;
                }
                __syncthreads();
                const double dk = L.S[k * n6 + k];
                if (!(dk > 0.0 && ref_finite(dk))) {
                    if (tid == 0) L.si[SI_SING] = 1;
                    break;   // uniform: every lane reads the same pivot
                }
                if (tid == 0) L.D[k] = dk;
                if (i > k && i < n6) L.S[i * n6 + k] = L.S[i * n6 + k] / dk;
                __syncthreads();
            }
        }
        __syncthreads();
        const bool sing = L.si[SI_SING] != 0;
        if (!sing) {
            if (tid < n6) L.dx[tid] = L.gr[tid];
            for (int m = 0; m < n6; ++m) {
                __syncthreads();
                if (tid > m && tid < n6) L.dx[tid] = L.dx[tid] - L.S[tid * n6 + m] * L.dx[m];
            }
            __syncthreads();
            if (tid < n6) L.dx[tid] = L.dx[tid] / L.D[tid];
            for (int m = n6 - 1; m > 0; --m) {
                __syncthreads();
                if (tid < m) L.dx[tid] = L.dx[tid] - L.S[m * n6 + tid] * L.dx[m];
            }
            __syncthreads();
            if (tid < n6) pr.m.DX[tid] = L.dx[tid];

            // (g) landmarks
            for (int j = tid; j < npt; j += BLOCK)
                pr.m.q[j] = lba_landmark_back<3>(pr, j, L.dx, 9 * (size_t)j, 3 * (size_t)j, (size_t)j * nkf * 18,
                                                 (size_t)n6 + 3 * (size_t)j);
            for (int j = tid; j < nls; j += BLOCK)
                pr.m.q[npt + j] = lba_landmark_back<6>(pr, npt + j, L.dx, 9 * (size_t)npt + 36 * (size_t)j,
                                                       3 * (size_t)npt + 6 * (size_t)j,
                                                       (size_t)npt * nkf * 18 + (size_t)j * nkf * 36,
                                                       (size_t)n6 + 3 * (size_t)npt + 6 * (size_t)j);
        }
        __syncthreads();

        // |DX|^2: the pose entries, then the landmarks' squares, both in order (lane 0; a chunk through LDS)
        double n2 = 0.0;
        if (!sing && it > 0) {
            if (tid == 0)
                for (int i = 0; i < n6; ++i) n2 = n2 + L.dx[i] * L.dx[i];
            for (int j0 = 0; j0 < nlm; j0 += BLOCK) {
                __syncthreads();
                if (j0 + tid < nlm) L.red[tid] = pr.m.q[j0 + tid];
                __syncthreads();
                if (tid == 0) {
                    const int mj = min(BLOCK, nlm - j0);
                    for (int jj = 0; jj < mj; ++jj) n2 = n2 + L.red[jj];
                }
            }
        }

        // the lambda rule (:1662-1678); a singular solve is DX = 0 with the update skipped
        if (tid == 0) {
            L.sd[BA_SD_N2] = n2;
            int accept = 1;
            if (it > 0) {
                if (L.sd[BA_SD_ERR] > L.sd[BA_SD_ERRPREV]) { L.sd[BA_SD_LAMBDA] = lambda / a.prm.lambda_k; accept = 0; }
                else L.sd[BA_SD_LAMBDA] = lambda * a.prm.lambda_k;
            }
            if (sing) { accept = 0; L.si[BA_SI_STATUS] |= GFPL_LBA_SINGULAR; }
            L.si[SI_ACCEPT] = accept;
        }
        __syncthreads();

        // (h) the update (:1443-1451, :1669-1677): X_i = logmap(expmap(X_i) inverse(expmap(DX_i)))
        if (L.si[SI_ACCEPT]) {
            if (tid < nkf) ba_pose_update(X + 6 * tid, L.dx + 6 * tid);
            for (size_t i = (size_t)n6 + tid; i < N; i += BLOCK) X[i] = X[i] + pr.m.DX[i];
        }
        if (tid == 0) {
            if (it > 0 && sqrt(L.sd[BA_SD_N2]) < eps) {
                L.si[BA_SI_STOP] = GFPL_LBA_STOP_STEP;
                L.si[BA_SI_ITERS] = it;
                L.si[BA_SI_DONE] = 1;
            } else {
                L.sd[BA_SD_ERRPREV] = L.sd[BA_SD_ERR];
                L.si[BA_SI_ITERS] = it + 1;
                if (it + 1 >= a.prm.max_iters) L.si[BA_SI_DONE] = 1;
            }
        }
        __syncthreads();
        if (L.si[BA_SI_DONE]) break;
    }

    // write back (:1691-1712) unless Hmax left the reference's defined behaviour
    if (!(L.si[BA_SI_STATUS] & GFPL_LBA_HMAX_RANGE)) {
        if (tid < nkf) {
            double T[16];
            expmap_se3(X + 6 * tid, T);
#pragma unroll
            for (int i = 0; i < 16; ++i) pr.T_kf[16 * (size_t)tid + i] = T[i];
            if (pr.x_out)
#pragma unroll
                for (int i = 0; i < 6; ++i) pr.x_out[6 * tid + i] = X[6 * tid + i];
        }
        for (size_t i = tid; i < 3 * (size_t)npt; i += BLOCK) pr.pt[i] = X[n6 + i];
        for (size_t i = tid; i < 6 * (size_t)nls; i += BLOCK) pr.ls[i] = X[(size_t)n6 + 3 * (size_t)npt + i];
    }
    if (tid == 0) a.out[blockIdx.x] = ba_record(L.sd, L.si);
}

hipError_t launch_lba(const LbaArgs& a, int n, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};
    const LbaLds size(nullptr, a.lds_kfs);
    hipError_t e = ensure_dyn_lds((const void*)k_lba<LBA_BLOCK>, DYN_LDS_CEILING, &done);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lba<LBA_BLOCK>, dim3(n), dim3(LBA_BLOCK), size.bytes, s, a);
    return hipGetLastError();
}

}  // namespace gfpl
