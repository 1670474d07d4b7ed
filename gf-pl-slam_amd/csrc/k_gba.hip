// k_gba.hip — global bundle adjustment of a whole map: MapHandler::levMarquardtOptimizationGBA
// (src/mapHandler.cpp:1950-2544), ONE PROBLEM OVER MANY WORKGROUPS.  DESIGN.md §4k, ledger GB1-GB12.
//
// Every phase is its own launch; the seams between phases are the stream's order, never a wait
// between workgroups of one launch.  All launches of all iterations are enqueued at once: every
// kernel reads the problem's loop state first and returns when the problem has ended (or, for the
// phases of the solve, when this iteration's system is singular).  Per iteration `it` (0: the pre-pass):
//   k_gba_poses    (it > 0) inverse poses of X, a lane per keyframe
//   k_gba_rows     a lane per observation: J_pose[6], J_landmark[6], |err|, w (gfpl_ba.hpp's rows)
//   k_gba_kf       a workgroup per keyframe: 42 lanes walk its observations IN LIST ORDER into U and g;
//                  one more workgroup adds err in list order
//   k_gba_lm       a lane per landmark: V, g and its coupling blocks W, ONE PER PAIR (landmark, keyframe)
//   k_gba_control  one workgroup: int Hmax and lambda (pre-pass), err and the stop tests
//   k_gba_inv      a lane per landmark: damping, the block's own LDL^T, z = V^-1 g, Y = V^-1 W by substitution
//   k_gba_s        a workgroup per lower block (a >= b) of S: an entry per lane subtracts the planner's
//                  terms, landmarks ascending; the diagonal blocks' workgroups form g_r too
//   k_gba_ldlt     per block column, left-looking: an entry's sum over the finished columns m ascending,
//                  a lane per entry; every workgroup factorises the 6 x 6 diagonal block itself from the
//                  same inputs (the same bits), then divides its panel rows
//   k_gba_subst    one workgroup: the two substitutions in index order, the poses' squared step
//   k_gba_back     a lane per landmark: DX_j and its squared step
//   k_gba_step     one workgroup: |DX|^2 in order, the lambda rule, the stop by step, the loop state
//   k_gba_update   X: poses through expmap / inverse / logmap, landmarks by addition
// and k_gba_final writes T_kf, pt, ls and the record back.  No floating-point atomics; every sum's
// order is a function of the problem alone, never of the grid (GbaGrid), the batch or timing.
// The rules that differ from the LBA are GbaRules (gfpl_kernels.hpp), read where marked "RULE".  The row
// arithmetic (ledger GB8), the loop state's start, the pose update and the record are gfpl_ba.hpp's, one
// text for both solvers.
#include "gfpl_ba.hpp"

namespace gfpl {

namespace {

#define GBA_ENDED(si) (((si)[BA_SI_DONE] | (si)[GBA_SI_DONE_NEXT]) != 0)
// this iteration's system is singular: a landmark block (k_gba_inv) or a pivot of S (k_gba_ldlt, whose
// block columns alternate between two words so that no launch reads a word one of its workgroups writes)
#define GBA_SINGULAR(si) (((si)[GBA_SI_SING] | (si)[GBA_SI_LDLT_BAD0] | (si)[GBA_SI_LDLT_BAD0 + 1]) != 0)

// (not shared with the LBA, which inverts the block explicitly)
// LDL^T of a landmark's damped D x D block (its lower triangle) without pivoting, the big factorisation's
// per-entry order: Fm holds L under the diagonal and the pivots on it.  False when a pivot is not
// positive and finite.  (Not inverse3 / inverse6 as in k_lba: with every step applied a run reaches
// blocks of condition 1e7 and more, where products with an explicit inverse lose the solve's
// backward-error bound, ledger GB11.)
template <int D>
GFPL_DEV bool gba_block_ldlt(const double* A, double* Fm) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
        for (int i = k; i < D; ++i) {
            double v = A[i * D + k];
#pragma unroll
            for (int m = 0; m < k; ++m) v = v - (Fm[i * D + m] * Fm[k * D + m]) * Fm[m * D + m];
            if (i == k) {
                ok = ok && v > 0.0 && ref_finite(v);
                Fm[k * D + k] = v;
            } else {
                Fm[i * D + k] = v / Fm[k * D + k];
                Fm[k * D + i] = 0.0;
            }
        }
    return ok;
}

// x := V^-1 x from the block's factor: forward, diagonal, backward, each row's terms in index order
template <int D>
GFPL_DEV void gba_block_solve(const double* Fm, double* x) {
#pragma unroll
    for (int i = 1; i < D; ++i)
#pragma unroll
        for (int m = 0; m < i; ++m) x[i] = x[i] - Fm[i * D + m] * x[m];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = x[i] / Fm[i * D + i];
#pragma unroll
    for (int i = D - 2; i >= 0; --i)
#pragma unroll
        for (int m = D - 1; m > i; --m) x[i] = x[i] - Fm[m * D + i] * x[m];
}

// first double of pair p's W / Y block: point pairs first (18 each), then line pairs (36 each)
GFPL_DEV size_t gba_woff(const GbaProb& pr, int p) {
    const int npp = pr.n.n_pt_pairs;
    return p < npp ? 18 * (size_t)p : 18 * (size_t)npp + 36 * (size_t)(p - npp);
}
GFPL_DEV size_t gba_voff(const GbaProb& pr, int j) {
    const int npt = pr.n.n.n_pt;
    return j < npt ? 9 * (size_t)j : 9 * (size_t)npt + 36 * (size_t)(j - npt);
}
GFPL_DEV size_t gba_goff(const GbaProb& pr, int j) {
    const int npt = pr.n.n.n_pt;
    return j < npt ? 3 * (size_t)j : 3 * (size_t)npt + 6 * (size_t)(j - npt);
}

// landmark j of D rows: V, g, the W block of each of its pairs, its largest |diagonal|.
// RULE prepass_transposed (:2188-2198): a line's block under the diagonal takes Hij(i,j) = JL_i JT_j w
// at row j, column i in the pre-pass.
template <int D>
GFPL_DEV void gba_landmark_sums(const GbaProb& pr, int j, bool transposed) {
    const int o0 = pr.lm_start[j], o1 = pr.lm_start[j + 1];
    const int p0 = pr.pair_start[j], p1 = pr.pair_start[j + 1];
    const size_t voff = gba_voff(pr, j), goff = gba_goff(pr, j);
    for (int p = p0; p < p1; ++p) {
        double* W = pr.m.W + gba_woff(pr, p);
        for (int i = 0; i < D * 6; ++i) W[i] = 0.0;
    }
    double V[D * D], g[D];
#pragma unroll
    for (int i = 0; i < D * D; ++i) V[i] = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) g[i] = 0.0;
    for (int o = o0; o < o1; ++o) {
        const double* rw = pr.m.rows + (size_t)o * GBA_ROW;
        double JT[6], JL[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) { JT[i] = rw[i]; JL[i] = rw[6 + i]; }
        const double nrm = rw[12], w = rw[13];
#pragma unroll
        for (int p = 0; p < D; ++p) {
            g[p] = g[p] + (JL[p] * nrm) * w;
#pragma unroll
            for (int q = 0; q < D; ++q) V[p * D + q] = V[p * D + q] + (JL[p] * JL[q]) * w;
        }
        const int pair = pr.obs_pair[o];
        if (pair >= 0) {
            double* Ws = pr.m.W + gba_woff(pr, pair);
#pragma unroll
            for (int p = 0; p < D; ++p)
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double h = (D == 6 && transposed) ? (JL[k] * JT[p]) * w : (JL[p] * JT[k]) * w;
                    Ws[p * 6 + k] = Ws[p * 6 + k] + h;
                }
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
    pr.m.dmax[j] = dmax;
}

// damp, factorise, V^-1 g and V^-1 W of every pair by substitution; false when a damped diagonal or a
// pivot of the block is not positive and finite
template <int D>
GFPL_DEV bool gba_landmark_invert(const GbaProb& pr, int j, double lambda) {
    const size_t voff = gba_voff(pr, j), goff = gba_goff(pr, j);
    double V[D * D], Vi[D * D];
#pragma unroll
    for (int i = 0; i < D * D; ++i) V[i] = pr.m.V[voff + i];
    bool ok = true;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        V[p * D + p] = V[p * D + p] + lambda * V[p * D + p];
        ok = ok && V[p * D + p] > 0.0 && ref_finite(V[p * D + p]);
    }
    ok = gba_block_ldlt<D>(V, Vi) && ok;
#pragma unroll
    for (int i = 0; i < D * D; ++i) pr.m.Vi[voff + i] = Vi[i];
    {
        double zj[D];
#pragma unroll
        for (int p = 0; p < D; ++p) zj[p] = pr.m.glm[goff + p];
        gba_block_solve<D>(Vi, zj);
#pragma unroll
        for (int p = 0; p < D; ++p) pr.m.z[goff + p] = zj[p];
    }
    for (int pp = pr.pair_start[j]; pp < pr.pair_start[j + 1]; ++pp) {
        const double* Ws = pr.m.W + gba_woff(pr, pp);
        double* Ys = pr.m.Y + gba_woff(pr, pp);
        for (int k = 0; k < 6; ++k) {
            double wk[D];
#pragma unroll
            for (int q = 0; q < D; ++q) wk[q] = Ws[q * 6 + k];
            gba_block_solve<D>(Vi, wk);
#pragma unroll
            for (int p = 0; p < D; ++p) Ys[p * 6 + k] = wk[p];
        }
    }
    return ok;
}

// DX_j = V_j^-1 (g_j - W_j DX_kf), the landmark's keyframes ascending; returns |DX_j|^2
template <int D>
GFPL_DEV double gba_landmark_back(const GbaProb& pr, int j, size_t xoff) {
    const size_t voff = gba_voff(pr, j), goff = gba_goff(pr, j);
    double u[D];
#pragma unroll
    for (int p = 0; p < D; ++p) u[p] = pr.m.glm[goff + p];
    for (int pp = pr.pair_start[j]; pp < pr.pair_start[j + 1]; ++pp) {
        const double* Ws = pr.m.W + gba_woff(pr, pp);
        const double* dxk = pr.m.DX + 6 * (size_t)pr.pair_kf[pp];
#pragma unroll
        for (int p = 0; p < D; ++p)
#pragma unroll
            for (int k = 0; k < 6; ++k) u[p] = u[p] - Ws[p * 6 + k] * dxk[k];
    }
    double Fm[D * D];
#pragma unroll
    for (int i = 0; i < D * D; ++i) Fm[i] = pr.m.Vi[voff + i];
    gba_block_solve<D>(Fm, u);
    double n2 = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        pr.m.DX[xoff + p] = u[p];
        n2 = p == 0 ? u[p] * u[p] : n2 + u[p] * u[p];
    }
    return n2;
}

}  // namespace

// X = [x_kf | point3D | line3D] (:1857, :1873, :1911) and the loop state
__global__ void __launch_bounds__(GBA_BLOCK) k_gba_init(GbaArgs a) {
    const GbaProb& pr = a.pr;
    const size_t n6 = 6 * (size_t)pr.n.n.n_kf, np3 = 3 * (size_t)pr.n.n.n_pt;
    const size_t N = n6 + np3 + 6 * (size_t)pr.n.n.n_ls;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) pr.m.X[i] = i < n6 ? pr.x_kf[i] : (i < n6 + np3 ? pr.pt[i - n6] : pr.ls[i - n6 - np3]);
    if (i == 0) {
        double* sd = pr.m.sd;
        int32_t* si = pr.m.si;
        ba_state_init(sd, si, a.prm.lambda_lm);
        sd[BA_SD_ERRSUM] = 0.0; sd[BA_SD_N2] = 0.0; sd[GBA_SD_N2POSE] = 0.0;
        si[GBA_SI_DONE_NEXT] = 0; si[GBA_SI_SING] = 0; si[GBA_SI_UPDATE_IT] = -1; si[GBA_SI_LAST_IT] = 0;
        si[GBA_SI_LDLT_BAD0] = 0; si[GBA_SI_LDLT_BAD0 + 1] = 0;
    }
}

// the iterations read the local poses from X (:2261): their inverses once per iteration
__global__ void __launch_bounds__(GBA_BLOCK) k_gba_poses(GbaArgs a) {
    const GbaProb& pr = a.pr;
    if (GBA_ENDED(pr.m.si)) return;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= pr.n.n.n_kf) return;
    double E[16], Ei[16];
    expmap_se3(pr.m.X + 6 * (size_t)s, E);
    inverse_se3(E, Ei);
#pragma unroll
    for (int i = 0; i < 16; ++i) pr.m.Tinv[16 * (size_t)s + i] = Ei[i];
}

__global__ void __launch_bounds__(GBA_BLOCK) k_gba_rows(GbaArgs a, int it) {
    const GbaProb& pr = a.pr;
    if (GBA_ENDED(pr.m.si)) return;
    const int npo = pr.n.n.n_pt_obs, nobs = npo + pr.n.n.n_ls_obs, npt = pr.n.n.n_pt;
    const size_t n6 = 6 * (size_t)pr.n.n.n_kf;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nobs) return;
    const int s = pr.obs_kf[o], j = pr.obs_lm[o];
    double row[GBA_ROW], Ti[16];
    const bool line = o >= npo;
    // the pre-pass and EVERY line term read T_kf_w (:1986, :2094, :2369); fixed poses always (:2263)
    if (it > 0 && !line && s >= 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) Ti[i] = pr.m.Tinv[16 * (size_t)s + i];
    } else {
        const double* T = s >= 0 ? pr.T_kf + 16 * (size_t)s : pr.T_fix + 16 * (size_t)(-1 - s);
        double Tl[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) Tl[i] = T[i];
        inverse_se3(Tl, Ti);
    }
    if (!line) {
        const double* Xw = it > 0 ? pr.m.X + n6 + 3 * (size_t)j : pr.pt + 3 * (size_t)j;
        double P[3] = {Xw[0], Xw[1], Xw[2]};
        double ob[2] = {pr.pt_obs[2 * (size_t)o], pr.pt_obs[2 * (size_t)o + 1]};
        ba_point_row(a.cam, a.homog_th, Ti, P, ob, pr.pt_sigma[o], row);
    } else {
        const size_t ol = (size_t)(o - npo);
        const double* Lw = pr.ls + 6 * (size_t)(j - npt);   // line3D of the map, never X (:2366)
        double PQ[6], l[3] = {pr.ls_obs[3 * ol], pr.ls_obs[3 * ol + 1], pr.ls_obs[3 * ol + 2]};
#pragma unroll
        for (int i = 0; i < 6; ++i) PQ[i] = Lw[i];
        // RULE line_th_homog (:2386): the GBA's iterations keep Config::homogTh()
        const double th = (it > 0 && !a.rules.line_th_homog) ? 0.0000001 : a.homog_th;
        ba_line_row(a.cam, th, Ti, PQ, l, pr.ls_sigma[ol], row);
    }
    double* gr = pr.m.rows + (size_t)o * GBA_ROW;
#pragma unroll
    for (int i = 0; i < GBA_ROW; ++i) gr[i] = row[i];
}

// workgroup s < n_kf: U_s and g_s, its observations in list order; workgroup n_kf: err, every
// observation in list order (a chunk of terms through LDS, lane 0 adds them one by one)
__global__ void __launch_bounds__(GBA_BLOCK) k_gba_kf(GbaArgs a) {
    __shared__ double term[GBA_BLOCK];
    const GbaProb& pr = a.pr;
    if (GBA_ENDED(pr.m.si)) return;
    const int nkf = pr.n.n.n_kf, tid = threadIdx.x;
    if ((int)blockIdx.x < nkf) {
        if (tid >= 42) return;
        const int s = blockIdx.x;
        const int ra = tid < 36 ? tid / 6 : tid - 36, rb = tid < 36 ? tid % 6 : 12;
        double v = 0.0;
        for (int k = pr.kf_start[s]; k < pr.kf_start[s + 1]; ++k) {
            const double* rw = pr.m.rows + (size_t)pr.kf_obs[k] * GBA_ROW;
            v = v + (rw[ra] * rw[rb]) * rw[13];
        }
        if (tid < 36) pr.m.U[(size_t)s * 36 + tid] = v;
        else pr.m.gk[(size_t)s * 6 + (tid - 36)] = v;
        return;
    }
    const int nobs = pr.n.n.n_pt_obs + pr.n.n.n_ls_obs;
    double sum = 0.0;
    for (int c0 = 0; c0 < nobs; c0 += GBA_BLOCK) {
        const int o = c0 + tid;
        if (o < nobs) {
            const double* rw = pr.m.rows + (size_t)o * GBA_ROW;
            term[tid] = (rw[12] * rw[12]) * rw[13];
        }
        __syncthreads();
        if (tid == 0) {
            const int m = min(GBA_BLOCK, nobs - c0);
            for (int r = 0; r < m; ++r) sum = sum + term[r];
        }
        __syncthreads();
    }
    if (tid == 0) pr.m.sd[BA_SD_ERRSUM] = sum;
}

__global__ void __launch_bounds__(GBA_BLOCK) k_gba_lm(GbaArgs a, int it) {
    const GbaProb& pr = a.pr;
    if (GBA_ENDED(pr.m.si)) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= pr.n.n.n_pt + pr.n.n.n_ls) return;
    if (j < pr.n.n.n_pt) gba_landmark_sums<3>(pr, j, false);
    else gba_landmark_sums<6>(pr, j, it == 0 && a.rules.prepass_transposed != 0);
}

// int Hmax and lambda (:2204-2212) or err and the stop tests (:2479-2482)
__global__ void __launch_bounds__(GBA_BLOCK) k_gba_control(GbaArgs a, int it) {
    __shared__ double red[GBA_BLOCK];
    const GbaProb& pr = a.pr;
    double* sd = pr.m.sd;
    int32_t* si = pr.m.si;
    if (GBA_ENDED(si)) return;
    const int tid = threadIdx.x;
    const int nkf = pr.n.n.n_kf, npt = pr.n.n.n_pt, nls = pr.n.n.n_ls, n6 = 6 * nkf;
    const double eps = 2.220446049250313e-16;
    if (it == 0) {
        // the largest |diagonal|: a maximum does not depend on the order it is taken in
        double hm = 0.0;
        for (int j = tid; j < npt + nls; j += GBA_BLOCK)
            if (pr.m.dmax[j] > hm) hm = pr.m.dmax[j];
        for (int i = tid; i < n6; i += GBA_BLOCK) {
            const double d = fabs(pr.m.U[(size_t)(i / 6) * 36 + (i % 6) * 7]);
            if (d > hm) hm = d;
        }
        red[tid] = hm;
        __syncthreads();
        for (int w = GBA_BLOCK / 2; w > 0; w >>= 1) {
            if (tid < w && red[tid + w] > red[tid]) red[tid] = red[tid + w];
            __syncthreads();
        }
    }
    if (tid != 0) return;
    si[GBA_SI_LAST_IT] = it;
    si[GBA_SI_SING] = 0;
    si[GBA_SI_LDLT_BAD0] = 0;
    si[GBA_SI_LDLT_BAD0 + 1] = 0;
    if (it == 0) {
        // `double err` starts undefined (:1964): pinned to 0.0; err /= (Npt_obs + Nls_obs), both 0 for good (:2204)
        sd[BA_SD_ERR] = sd[BA_SD_ERRSUM] / 0.0;
        const double hm = red[0];
        if (hm >= 2147483648.0) {
            si[BA_SI_STATUS] |= GFPL_GBA_HMAX_RANGE;
            si[BA_SI_HMAX] = 0x7fffffff;
            si[BA_SI_DONE] = 1;
        } else {
            const int h = (int)hm;
            si[BA_SI_HMAX] = h;
            sd[BA_SD_LAMBDA] = sd[BA_SD_LAMBDA] * (double)h;
        }
    } else {
        // RULE divisor_zero (:2479): Npt_obs + Nls_obs again; the LBA divides by Npt + Nls
        const double err = sd[BA_SD_ERRSUM] / (a.rules.divisor_zero ? 0.0 : (double)(npt + nls));
        sd[BA_SD_ERR] = err;
        if (fabs(err - sd[BA_SD_ERRPREV]) < eps) { si[BA_SI_STOP] = GFPL_GBA_STOP_DERR; si[BA_SI_DONE] = 1; }
        else if (err < eps) { si[BA_SI_STOP] = GFPL_GBA_STOP_ERR; si[BA_SI_DONE] = 1; }
        si[BA_SI_ITERS] = it;
    }
}

__global__ void __launch_bounds__(GBA_BLOCK) k_gba_inv(GbaArgs a) {
    const GbaProb& pr = a.pr;
    if (GBA_ENDED(pr.m.si)) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= pr.n.n.n_pt + pr.n.n.n_ls) return;
    const double lambda = pr.m.sd[BA_SD_LAMBDA];
    const bool ok = j < pr.n.n.n_pt ? gba_landmark_invert<3>(pr, j, lambda) : gba_landmark_invert<6>(pr, j, lambda);
    if (!ok) atomicOr(&pr.m.si[GBA_SI_SING], 1);
}

// lower block (a, b) = (blockIdx.y, blockIdx.x) of S = U (1 + lambda on the diagonal) - sum_j W_ja^T Y_jb,
// and g_r of keyframe a in the diagonal blocks' workgroups; blocks without terms keep U or 0
__global__ void __launch_bounds__(64) k_gba_s(GbaArgs a) {
    const GbaProb& pr = a.pr;
    if (GBA_ENDED(pr.m.si) || GBA_SINGULAR(pr.m.si)) return;
    const int ka = blockIdx.y, kb = blockIdx.x, tid = threadIdx.x;
    if (kb > ka || tid >= 42) return;
    const bool rhs = tid >= 36;
    if (rhs && ka != kb) return;
    const int ri = rhs ? tid - 36 : tid / 6, ci = rhs ? 0 : tid % 6;
    if (!rhs && ka == kb && ci > ri) return;   // the solve reads the lower triangle
    const size_t n6 = 6 * (size_t)pr.n.n.n_kf;
    const int npt = pr.n.n.n_pt;
    const size_t blk = (size_t)ka * (ka + 1) / 2 + kb;
    double val;
    if (rhs) val = pr.m.gk[6 * (size_t)ka + ri];
    else if (ka == kb) {
        const double u = pr.m.U[(size_t)ka * 36 + ri * 6 + ci];
        val = ri == ci ? u + pr.m.sd[BA_SD_LAMBDA] * u : u;
    } else val = 0.0;
    for (int t = pr.blk_start[blk]; t < pr.blk_start[blk + 1]; ++t) {
        const int j = pr.terms[3 * (size_t)t], pa = pr.terms[3 * (size_t)t + 1], pb = pr.terms[3 * (size_t)t + 2];
        const int D = j < npt ? 3 : 6;
        const double* Wa = pr.m.W + gba_woff(pr, pa) + ri;
        const double* Yb = rhs ? pr.m.z + gba_goff(pr, j) : pr.m.Y + gba_woff(pr, pb) + ci;
        const int ys = rhs ? 1 : 6;
        double s = Wa[0] * Yb[0];
        for (int p = 1; p < D; ++p) s = s + Wa[p * 6] * Yb[p * ys];
        val = val - s;
    }
    if (rhs) pr.m.gr[6 * (size_t)ka + ri] = val;
    else pr.m.S[(6 * (size_t)ka + ri) * n6 + 6 * (size_t)kb + ci] = val;
}

// (S in HBM and a launch per block column; the LBA's S lives in LDS: not shared)
// block column kb of the LDL^T of S's lower triangle without pivoting: the panel's L in place, the diagonal
// block's L transposed above the diagonal (the block itself stays readable for the whole launch), the pivots in D.  v(i,k) = S(i,k) - sum_{m<k} (L_im L_km) D_m, one term at a time with m ascending:
// a lane per entry takes the terms of the finished columns m < 6 kb, then one lane per row takes the
// at most five terms inside the block column.  Local rows 0 .. 5 are the diagonal block (every
// workgroup computes it from the same inputs: the same bits), rows 6 .. are this workgroup's panel.
// RULE any_sign_pivot: a pivot is accepted when finite and non-zero; a negative one is reported.
__global__ void __launch_bounds__(36 * (1 + GBA_MAX_LDLT_ROWS)) k_gba_ldlt(GbaArgs a, int kb, int rows_kf) {
    extern __shared__ __align__(16) unsigned char smem[];
    const GbaProb& pr = a.pr;
    int32_t* si = pr.m.si;
    // the word of the column before this one (written by that launch, read-only in this one); a bad pivot
    // there is handed on in this column's word, so the last column's word tells the phases after
    const int mine = GBA_SI_LDLT_BAD0 + (kb & 1), before = GBA_SI_LDLT_BAD0 + ((kb & 1) ^ 1);
    if (GBA_ENDED(si) || si[GBA_SI_SING]) return;
    if (kb > 0 && si[before]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) si[mine] = 1;
        return;
    }
    const GbaLdltLds L(smem, 6 + 6 * rows_kf);
    const int tid = threadIdx.x, lr = tid / 6, c = tid % 6;
    const int n6 = 6 * pr.n.n.n_kf, k0 = 6 * kb;
    const int row = lr < 6 ? k0 + lr : 6 * (kb + 1 + (int)blockIdx.x * rows_kf) + (lr - 6);
    const bool valid = row < n6 && (lr >= 6 || c <= lr);
    double* S = pr.m.S;
    const double* Dg = pr.m.D;
    if (valid) {
        const double* Li = S + (size_t)row * n6;
        const double* Lk = S + (size_t)(k0 + c) * n6;
        double v = Li[k0 + c];
        // the terms stay one at a time with m ascending; eight terms' operands are loaded ahead of the
        // chain of subtractions, which would otherwise wait for the memory at every term
        int m = 0;
        for (; m + 8 <= k0; m += 8) {
            double li[8], lk[8], dm[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { li[u] = Li[m + u]; lk[u] = Lk[m + u]; dm[u] = Dg[m + u]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) v = v - (li[u] * lk[u]) * dm[u];
        }
        for (; m < k0; ++m) v = v - (Li[m] * Lk[m]) * Dg[m];
        L.part[lr * 6 + c] = v;
    }
    if (tid == 0) { L.flag[0] = 0; L.flag[1] = 0; }
    __syncthreads();
    if (tid == 0) {
        bool bad = false;
        for (int cc = 0; cc < 6 && !bad; ++cc)
            for (int r = cc; r < 6; ++r) {
                double v = L.part[r * 6 + cc];
                for (int m = 0; m < cc; ++m) v = v - (L.Ld[r * 6 + m] * L.Ld[cc * 6 + m]) * L.Dd[m];
                if (r == cc) {
                    const bool good = ref_finite(v) && (a.rules.any_sign_pivot ? v != 0.0 : v > 0.0);
                    if (!good) { bad = true; break; }
                    if (v < 0.0) L.flag[1] = 1;
                    L.Dd[cc] = v;
                    L.Ld[cc * 6 + cc] = 1.0;
                } else {
                    L.Ld[r * 6 + cc] = v / L.Dd[cc];
                }
            }
        if (bad) L.flag[0] = 1;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) {
        if (L.flag[1]) si[BA_SI_STATUS] |= GFPL_GBA_INDEFINITE;
        si[mine] = L.flag[0];
    }
    if (L.flag[0]) return;
    if (lr >= 6 && c == 0 && row < n6) {
        double Lr[6];
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) {
            double v = L.part[lr * 6 + cc];
#pragma unroll
            for (int m = 0; m < cc; ++m) v = v - (Lr[m] * L.Ld[cc * 6 + m]) * L.Dd[m];
            Lr[cc] = v / L.Dd[cc];
        }
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) S[(size_t)row * n6 + k0 + cc] = Lr[cc];
    }
    if (blockIdx.x == 0 && lr < 6) {
        // the diagonal block's L goes ABOVE the diagonal, transposed: the entries under it are what every
        // workgroup of this launch reads as S, in whatever order the workgroups run
        if (c < lr) S[(size_t)(k0 + c) * n6 + k0 + lr] = L.Ld[lr * 6 + c];
        if (c == lr) pr.m.D[k0 + c] = L.Dd[c];
    }
}

// L(i, m), i > m, where k_gba_ldlt left it: a panel entry in place, an entry of a diagonal block transposed above
// the diagonal
GFPL_DEV double gba_l(const double* S, int n6, int i, int m) {
    return i / 6 == m / 6 ? S[(size_t)m * n6 + i] : S[(size_t)i * n6 + m];
}

// L y = g_r, y /= D, L^T dx = y, each row's terms in index order; then the poses' part of |DX|^2
__global__ void __launch_bounds__(GBA_BLOCK) k_gba_subst(GbaArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const GbaProb& pr = a.pr;
    if (GBA_ENDED(pr.m.si) || GBA_SINGULAR(pr.m.si)) return;
    const int n6 = 6 * pr.n.n.n_kf, tid = threadIdx.x;
    const GbaSubstLds L(smem, n6);
    const double* S = pr.m.S;
    for (int i = tid; i < n6; i += GBA_BLOCK) L.y[i] = pr.m.gr[i];
    for (int m = 0; m < n6; ++m) {
        __syncthreads();
        const double ym = L.y[m];
        for (int i = m + 1 + tid; i < n6; i += GBA_BLOCK) L.y[i] = L.y[i] - gba_l(S, n6, i, m) * ym;
    }
    __syncthreads();
    for (int i = tid; i < n6; i += GBA_BLOCK) L.y[i] = L.y[i] / pr.m.D[i];
    for (int m = n6 - 1; m > 0; --m) {
        __syncthreads();
        const double ym = L.y[m];
        for (int i = tid; i < m; i += GBA_BLOCK) L.y[i] = L.y[i] - gba_l(S, n6, m, i) * ym;
    }
    __syncthreads();
    for (int i = tid; i < n6; i += GBA_BLOCK) pr.m.DX[i] = L.y[i];
    if (tid == 0) {
        double n2 = 0.0;
        for (int i = 0; i < n6; ++i) n2 = n2 + L.y[i] * L.y[i];
        pr.m.sd[GBA_SD_N2POSE] = n2;
    }
}

__global__ void __launch_bounds__(GBA_BLOCK) k_gba_back(GbaArgs a) {
    const GbaProb& pr = a.pr;
    if (GBA_ENDED(pr.m.si) || GBA_SINGULAR(pr.m.si)) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int npt = pr.n.n.n_pt;
    if (j >= npt + pr.n.n.n_ls) return;
    const size_t n6 = 6 * (size_t)pr.n.n.n_kf;
    pr.m.q[j] = j < npt ? gba_landmark_back<3>(pr, j, n6 + 3 * (size_t)j)
                        : gba_landmark_back<6>(pr, j, n6 + 3 * (size_t)npt + 6 * (size_t)(j - npt));
}

// |DX|^2 (the poses' entries, then the landmarks' squares in order), the lambda rule (:2493-2509),
// the stop by step (:2511) and the loop variable
__global__ void __launch_bounds__(GBA_BLOCK) k_gba_step(GbaArgs a, int it) {
    __shared__ double term[GBA_BLOCK];
    const GbaProb& pr = a.pr;
    double* sd = pr.m.sd;
    int32_t* si = pr.m.si;
    if (GBA_ENDED(si)) return;
    const int tid = threadIdx.x, nlm = pr.n.n.n_pt + pr.n.n.n_ls;
    const bool sing = GBA_SINGULAR(si);
    const double eps = 2.220446049250313e-16;
    double n2 = 0.0;
    if (!sing && it > 0) {
        if (tid == 0) n2 = sd[GBA_SD_N2POSE];
        for (int j0 = 0; j0 < nlm; j0 += GBA_BLOCK) {
            if (j0 + tid < nlm) term[tid] = pr.m.q[j0 + tid];
            __syncthreads();
            if (tid == 0) {
                const int mj = min(GBA_BLOCK, nlm - j0);
                for (int jj = 0; jj < mj; ++jj) n2 = n2 + term[jj];
            }
            __syncthreads();
        }
    }
    if (tid != 0) return;
    const double lambda = sd[BA_SD_LAMBDA];
    int accept = 1;
    if (it > 0) {
        // err > err_prev is never true under divisor_zero (err is +inf or NaN): every step is applied
        if (sd[BA_SD_ERR] > sd[BA_SD_ERRPREV]) { sd[BA_SD_LAMBDA] = lambda / a.prm.lambda_k; accept = 0; }
        else sd[BA_SD_LAMBDA] = lambda * a.prm.lambda_k;
    }
    if (sing) { accept = 0; si[BA_SI_STATUS] |= GFPL_GBA_SINGULAR; }
    if (accept) si[GBA_SI_UPDATE_IT] = it;
    sd[BA_SD_N2] = n2;
    if (it > 0 && sqrt(n2) < eps) {
        si[BA_SI_STOP] = GFPL_GBA_STOP_STEP;
        si[BA_SI_ITERS] = it;
        si[GBA_SI_DONE_NEXT] = 1;
    } else {
        sd[BA_SD_ERRPREV] = sd[BA_SD_ERR];
        si[BA_SI_ITERS] = it + 1;
        if (it + 1 >= a.prm.max_iters) si[GBA_SI_DONE_NEXT] = 1;
    }
}

// (:2222-2231, :2499-2508): X_i = logmap(expmap(X_i) inverse(expmap(DX_i))), landmarks by addition;
// runs when k_gba_step accepted THIS iteration's step (it may have ended the loop in the same breath)
__global__ void __launch_bounds__(GBA_BLOCK) k_gba_update(GbaArgs a, int it) {
    const GbaProb& pr = a.pr;
    if (pr.m.si[GBA_SI_UPDATE_IT] != it) return;
    const int nkf = pr.n.n.n_kf;
    const size_t n6 = 6 * (size_t)nkf, N = n6 + 3 * (size_t)pr.n.n.n_pt + 6 * (size_t)pr.n.n.n_ls;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double* X = pr.m.X;
    if (i < (size_t)nkf) ba_pose_update(X + 6 * i, pr.m.DX + 6 * i);
    if (n6 + i < N) X[n6 + i] = X[n6 + i] + pr.m.DX[n6 + i];
}

// write back (:2521-2542) unless Hmax left the reference's defined behaviour, and the record
__global__ void __launch_bounds__(GBA_BLOCK) k_gba_final(GbaArgs a) {
    const GbaProb& pr = a.pr;
    const int32_t* si = pr.m.si;
    const int nkf = pr.n.n.n_kf;
    const size_t n6 = 6 * (size_t)nkf, np3 = 3 * (size_t)pr.n.n.n_pt, N = n6 + np3 + 6 * (size_t)pr.n.n.n_ls;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double* X = pr.m.X;
    if (!(si[BA_SI_STATUS] & GFPL_GBA_HMAX_RANGE)) {
        if (i < (size_t)nkf) {
            double T[16];
            expmap_se3(X + 6 * i, T);
#pragma unroll
            for (int k = 0; k < 16; ++k) pr.T_kf[16 * i + k] = T[k];
            if (pr.x_out)
#pragma unroll
                for (int k = 0; k < 6; ++k) pr.x_out[6 * i + k] = X[6 * i + k];
        }
        if (i >= n6 && i < n6 + np3) pr.pt[i - n6] = X[i];
        else if (i >= n6 + np3 && i < N) pr.ls[i - n6 - np3] = X[i];
    }
    if (i == 0) *a.out = ba_record(pr.m.sd, si);
}

int gba_max_lds_bytes(int n_kf) {
    const int l = GbaLdltLds(nullptr, 6 + 6 * GBA_MAX_LDLT_ROWS).bytes, s = GbaSubstLds(nullptr, 6 * n_kf).bytes;
    return l > s ? l : s;
}

hipError_t enqueue_gba(const GbaArgs& a, const GbaGrid& grid, hipStream_t s) {
    const gfpl_lba_counts& n = a.pr.n.n;
    const int nkf = n.n_kf, nlm = n.n_pt + n.n_ls, nobs = n.n_pt_obs + n.n_ls_obs;
    const size_t N = 6 * (size_t)nkf + 3 * (size_t)n.n_pt + 6 * (size_t)n.n_ls;
    const int B = grid.block, R = grid.ldlt_kfs;
    auto blocks = [](size_t cnt, int b) { return dim3((unsigned)((cnt + b - 1) / b)); };
    const int ldlt_lds = GbaLdltLds(nullptr, 6 + 6 * R).bytes, subst_lds = GbaSubstLds(nullptr, 6 * nkf).bytes;
    hipLaunchKernelGGL(k_gba_init, blocks(N, GBA_BLOCK), dim3(GBA_BLOCK), 0, s, a);
    const int iters = a.prm.max_iters > 1 ? a.prm.max_iters : 1;
    for (int it = 0; it < iters; ++it) {
        if (it > 0) hipLaunchKernelGGL(k_gba_poses, blocks((size_t)nkf, B), dim3(B), 0, s, a);
        hipLaunchKernelGGL(k_gba_rows, blocks((size_t)nobs, B), dim3(B), 0, s, a, it);
        hipLaunchKernelGGL(k_gba_kf, dim3(nkf + 1), dim3(GBA_BLOCK), 0, s, a);
        hipLaunchKernelGGL(k_gba_lm, blocks((size_t)nlm, B), dim3(B), 0, s, a, it);
        hipLaunchKernelGGL(k_gba_control, dim3(1), dim3(GBA_BLOCK), 0, s, a, it);
        hipLaunchKernelGGL(k_gba_inv, blocks((size_t)nlm, B), dim3(B), 0, s, a);
        hipLaunchKernelGGL(k_gba_s, dim3(nkf, nkf), dim3(64), 0, s, a);
        for (int kb = 0; kb < nkf; ++kb) {
            const int below = nkf - kb - 1;
            hipLaunchKernelGGL(k_gba_ldlt, dim3(below > 0 ? (below + R - 1) / R : 1), dim3(36 * (1 + R)), ldlt_lds, s, a, kb, R);
        }
        hipLaunchKernelGGL(k_gba_subst, dim3(1), dim3(GBA_BLOCK), subst_lds, s, a);
        hipLaunchKernelGGL(k_gba_back, blocks((size_t)nlm, B), dim3(B), 0, s, a);
        hipLaunchKernelGGL(k_gba_step, dim3(1), dim3(GBA_BLOCK), 0, s, a, it);
        const size_t nup = N - 6 * (size_t)nkf > (size_t)nkf ? N - 6 * (size_t)nkf : (size_t)nkf;
        hipLaunchKernelGGL(k_gba_update, blocks(nup, GBA_BLOCK), dim3(GBA_BLOCK), 0, s, a, it);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_gba_final, blocks(N, GBA_BLOCK), dim3(GBA_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace gfpl
