// k_pgo.hip — the loop-closure pose graph.
//
//  k_pgo         : the solve of MapHandler::loopClosureOptimizationCovGraphG2O / EssGraphG2O
//                  (src/mapHandler.cpp:4187-4419, :3950-4184), one workgroup per problem, the whole
//                  Levenberg-Marquardt loop on the device.  The objective and the iteration are
//                  DESIGN.md §4j's (ledger PG1-PG8).  Per iteration
//                  (a) a lane per edge computes e, J_i, J_j into HBM rows,
//                  (b) PGO_RED reduction lanes per free vertex add its J^T J diagonal block, its J^T e
//                      and the off-diagonal blocks of its envelope row IN THE INCIDENT-EDGE ORDER OF
//                      THE BUILDER; lane 0 adds chi2 in edge order (a chunk through LDS at a time),
//                  (c) LDL^T of H + lambda I over the block envelope without pivoting, a scalar column
//                      at a time; the pivot row is staged in LDS PGO_PANEL block columns at a time,
//                  (d) the two triangular solves, the trial poses, the trial chi2 and the gain ratio.
//                  Every sum's order is a function of the problem alone: no floating-point atomics.
//                  The write-back (:4314-4326, :4368-4372) leaves T_kf_w, x_kf_w and every moved
//                  keyframe's Tkfw_corr.
//  k_pgo_correct : the map correction (:4327-4364, :4374-4411): a lane per owned landmark.
#include "gfpl_kernels.hpp"

namespace gfpl {

namespace {

enum { PD_LAMBDA = 0, PD_NU, PD_CHI2, PD_CHI2T, PD_DMAX, PD_SCALE, PD_CHI2_0, PD_CHI2_PREV };
enum { PI_ITERS = 0, PI_STOP, PI_STATUS, PI_REJECTS, PI_DONE, PI_SING, PI_ACCEPT, PI_REJ_IT };

// the unit quaternion (x, y, z, w), w >= 0, of the rotation of D by the four-branch rule
GFPL_DEV void pgo_quat(const double* D, double* q) {
    const double r00 = D[0], r01 = D[1], r02 = D[2], r10 = D[4], r11 = D[5], r12 = D[6], r20 = D[8], r21 = D[9], r22 = D[10];
    const double tr = (r00 + r11) + r22;
    double x, y, z, w;
    if (tr > 0.0) {
        const double s = sqrt(tr + 1.0) * 2.0;
        w = 0.25 * s; x = (r21 - r12) / s; y = (r02 - r20) / s; z = (r10 - r01) / s;
    } else if (r00 > r11 && r00 > r22) {
        const double s = sqrt(((1.0 + r00) - r11) - r22) * 2.0;
        w = (r21 - r12) / s; x = 0.25 * s; y = (r01 + r10) / s; z = (r02 + r20) / s;
    } else if (r11 > r22) {
        const double s = sqrt(((1.0 + r11) - r00) - r22) * 2.0;
        w = (r02 - r20) / s; x = (r01 + r10) / s; y = 0.25 * s; z = (r12 + r21) / s;
    } else {
        const double s = sqrt(((1.0 + r22) - r00) - r11) * 2.0;
        w = (r10 - r01) / s; x = (r02 + r20) / s; y = (r12 + r21) / s; z = 0.25 * s;
    }
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    x = x / n; y = y / n; z = z / n; w = w / n;
    if (w < 0.0) { x = -x; y = -y; z = -z; w = -w; }
    q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}

// e of one edge and, with JAC, J_i and J_j ([6][6] each, row k: the derivative of e[k])
template <bool JAC>
GFPL_DEV void pgo_edge(const double* Xi, const double* Xj, const double* Z, double* e, double* Ji, double* Jj) {
    double Zi[16], Xii[16], M[16], D[16], q[4];
    inverse_se3(Z, Zi);
    inverse_se3(Xi, Xii);
    mat4_mul(Xii, Xj, M);
    mat4_mul(Zi, M, D);
    pgo_quat(D, q);
    e[0] = D[3]; e[1] = D[7]; e[2] = D[11];
    e[3] = q[0]; e[4] = q[1]; e[5] = q[2];
    if (!JAC) return;
    const double Q[9] = {q[3], -q[2], q[1], q[2], q[3], -q[0], -q[1], q[0], q[3]};   // w I + [q_v]x
    const double S[9] = {0.0, -M[11], M[7], M[11], 0.0, -M[3], -M[7], M[3], 0.0};   // [t_M]x
#pragma unroll
    for (int i = 0; i < 36; ++i) { Ji[i] = 0.0; Jj[i] = 0.0; }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            Jj[a * 6 + b] = D[a * 4 + b];
            Jj[(3 + a) * 6 + 3 + b] = Q[a * 3 + b];
            Ji[a * 6 + b] = -Zi[a * 4 + b];
            Ji[a * 6 + 3 + b] = 2.0 * ((Zi[a * 4 + 0] * S[0 * 3 + b] + Zi[a * 4 + 1] * S[1 * 3 + b]) + Zi[a * 4 + 2] * S[2 * 3 + b]);
            Ji[(3 + a) * 6 + 3 + b] = -((Q[a * 3 + 0] * M[b * 4 + 0] + Q[a * 3 + 1] * M[b * 4 + 1]) + Q[a * 3 + 2] * M[b * 4 + 2]);
        }
}

// X * Delta(d): translation d[0:3], rotation of the quaternion (d[3:6], w = sqrt(1 - |d[3:6]|^2))
GFPL_DEV void pgo_update(const double* X, const double* d, double* Xn) {
    double x = d[3], y = d[4], z = d[5], w;
    const double n2 = (x * x + y * y) + z * z;
    if (n2 > 1.0) {
        const double n = sqrt(n2);
        x = x / n; y = y / n; z = z / n; w = 0.0;
    } else {
        w = sqrt(1.0 - n2);
    }
    double E[16];
    E[0] = 1.0 - 2.0 * (y * y + z * z); E[1] = 2.0 * (x * y - z * w); E[2] = 2.0 * (x * z + y * w); E[3] = d[0];
    E[4] = 2.0 * (x * y + z * w); E[5] = 1.0 - 2.0 * (x * x + z * z); E[6] = 2.0 * (y * z - x * w); E[7] = d[1];
    E[8] = 2.0 * (x * z - y * w); E[9] = 2.0 * (y * z + x * w); E[10] = 1.0 - 2.0 * (x * x + y * y); E[11] = d[2];
    E[12] = 0.0; E[13] = 0.0; E[14] = 0.0; E[15] = 1.0;
    mat4_mul(X, E, Xn);
}

// entry (i, j) of the envelope array A, j's block column inside row i's envelope
GFPL_DEV double* pgo_at(const PgoProb& pr, double* A, int i, int j) {
    const int ri = i / 6;
    return A + ((size_t)pr.env_off[ri] + (size_t)(j / 6 - pr.env_first[ri])) * 36 + (i % 6) * 6 + j % 6;
}

// the edges' e (and rows when jac) at the poses P; esq[e] = e . e
template <bool JAC>
GFPL_DEV void pgo_eval(const PgoProb& pr, const double* P, int tid) {
    for (int ed = tid; ed < pr.n.n_edge; ed += PGO_BLOCK) {
        const int vi = pr.edge[4 * (size_t)ed], vj = pr.edge[4 * (size_t)ed + 1];
        double Xi[16], Xj[16], Z[16], e[6], Ji[36], Jj[36];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            Xi[i] = P[16 * (size_t)vi + i];
            Xj[i] = P[16 * (size_t)vj + i];
            Z[i] = pr.m.Z[16 * (size_t)ed + i];
        }
        pgo_edge<JAC>(Xi, Xj, Z, e, Ji, Jj);
        if (JAC) {
            double* rw = pr.m.rows + (size_t)ed * PGO_ROW;
#pragma unroll
            for (int i = 0; i < 6; ++i) rw[i] = e[i];
#pragma unroll
            for (int i = 0; i < 36; ++i) { rw[6 + i] = Ji[i]; rw[42 + i] = Jj[i]; }
        }
        pr.m.esq[ed] = ((((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]) + e[4] * e[4]) + e[5] * e[5];
    }
}

// 0.0 + v[0] + v[1] + ... on lane 0, a chunk of PGO_BLOCK through LDS at a time (MAX: the largest |v|)
template <bool MAX, class F>
GFPL_DEV double pgo_seq(const PgoLds& L, int n, int tid, F f) {
    double s = 0.0;
    for (int c0 = 0; c0 < n; c0 += PGO_BLOCK) {
        __syncthreads();
        if (c0 + tid < n) L.red[tid] = f(c0 + tid);
        __syncthreads();
        if (tid == 0) {
            const int m = min(PGO_BLOCK, n - c0);
            for (int j = 0; j < m; ++j) {
                if (MAX) { const double a = fabs(L.red[j]); if (!(a <= s)) s = a; }
                else s = s + L.red[j];
            }
        }
    }
    return s;
}

}  // namespace

__global__ void __launch_bounds__(PGO_BLOCK) k_pgo(PgoArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const PgoLds L(smem);
    const int tid = threadIdx.x;
    const PgoProb pr = a.probs[blockIdx.x];
    const int nv = pr.n.n_vert, nf = pr.n.n_free, ne = pr.n.n_edge, nkf = pr.n.n_kf;
    const int N = 6 * nf;
    const double eps = 2.220446049250313e-16;
    double *X = pr.m.X, *Xt = pr.m.Xt;

    // start poses (PG1) and measurements (PG2)
    for (int v = tid; v < nv; v += PGO_BLOCK) {
        const int kf = pr.vert[4 * v], flags = pr.vert[4 * v + 1], id = pr.vert[4 * v + 2];
        double T[16];
        if (flags & PGO_VERT_LC_J) {
            double E[16], Tp[16];
            expmap_se3(pr.lc_pose + 6 * (size_t)id, E);
            const double* src = pr.T_kf + 16 * (size_t)pr.lc[3 * id];
#pragma unroll
            for (int i = 0; i < 16; ++i) Tp[i] = src[i];
            mat4_mul(E, Tp, T);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) T[i] = pr.T_kf[16 * (size_t)kf + i];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) { X[16 * (size_t)v + i] = T[i]; Xt[16 * (size_t)v + i] = T[i]; pr.m.X0[16 * (size_t)v + i] = T[i]; }
    }
    for (int ed = tid; ed < ne; ed += PGO_BLOCK) {
        const int l = pr.edge[4 * (size_t)ed + 2];
        double Z[16];
        if (l >= 0) {
            expmap_se3(pr.lc_pose + 6 * (size_t)l, Z);
        } else {
            double Ti[16], Tj[16], Tii[16];
            const double* si = pr.T_kf + 16 * (size_t)pr.vert[4 * pr.edge[4 * (size_t)ed]];
            const double* sj = pr.T_kf + 16 * (size_t)pr.vert[4 * pr.edge[4 * (size_t)ed + 1]];
#pragma unroll
            for (int i = 0; i < 16; ++i) { Ti[i] = si[i]; Tj[i] = sj[i]; }
            inverse_se3(Ti, Tii);
            mat4_mul(Tii, Tj, Z);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) pr.m.Z[16 * (size_t)ed + i] = Z[i];
    }
    for (int i = tid; i < nkf; i += PGO_BLOCK) pr.m.moved[i] = 0;
    if (tid == 0) {
        L.sd[PD_LAMBDA] = a.prm.lambda_init; L.sd[PD_NU] = 2.0;
        L.si[PI_ITERS] = 0; L.si[PI_STOP] = GFPL_PGO_STOP_ITERS; L.si[PI_STATUS] = 0; L.si[PI_REJECTS] = 0; L.si[PI_DONE] = 0;
        pr.m.state[0] = 0;
    }
    __syncthreads();

    // chi2 at the start
    pgo_eval<false>(pr, X, tid);
    {
        const double* esq = pr.m.esq;
        const double c = pgo_seq<false>(L, ne, tid, [esq](int i) { return esq[i]; });
        if (tid == 0) {
            L.sd[PD_CHI2] = c; L.sd[PD_CHI2_0] = c; L.sd[PD_CHI2_PREV] = c;
            if (nf == 0) { L.si[PI_STOP] = GFPL_PGO_STOP_NOFREE; L.si[PI_DONE] = 1; }
            else if (a.prm.max_iters < 1) L.si[PI_DONE] = 1;
        }
    }
    __syncthreads();

    for (int it = 0; !L.si[PI_DONE]; ++it) {
        // (a) rows
        pgo_eval<true>(pr, X, tid);
        __syncthreads();

        // (b) diagonal blocks, gradient and the envelope rows, each entry one lane's, incident edges in order
        for (int t = tid; t < nf * PGO_RED; t += PGO_BLOCK) {
            const int r = t / PGO_RED, k = t % PGO_RED;
            const int v = pr.free_vert[r];
            const int o0 = pr.inc_start[r], o1 = pr.inc_start[r + 1];
            if (k < 42) {
                const int ca = k < 36 ? k / 6 : k - 36, cb = k % 6;
                double acc = 0.0;
                for (int o = o0; o < o1; ++o) {
                    const int ed = pr.inc[o];
                    const double* rw = pr.m.rows + (size_t)ed * PGO_ROW;
                    const double* J = rw + (pr.edge[4 * (size_t)ed] == v ? 6 : 42);
                    double s;
                    if (k < 36) {
                        s = J[ca] * J[cb];
                        for (int q = 1; q < 6; ++q) s = s + J[q * 6 + ca] * J[q * 6 + cb];
                    } else {
                        s = J[ca] * rw[0];
                        for (int q = 1; q < 6; ++q) s = s + J[q * 6 + ca] * rw[q];
                    }
                    acc = acc + s;
                }
                if (k < 36) pr.m.diag[(size_t)r * 36 + k] = acc;
                else pr.m.b[(size_t)r * 6 + ca] = acc;
            } else {
                const int en = k - 42, ca = en / 6, cb = en % 6;
                const int f = pr.env_first[r];
                double* row = pr.m.H + (size_t)pr.env_off[r] * 36 + en;
                for (int c = f; c <= r; ++c) row[(size_t)(c - f) * 36] = 0.0;
                for (int o = o0; o < o1; ++o) {
                    const int ed = pr.inc[o];
                    if (pr.edge[4 * (size_t)ed + 1] != v) continue;
                    const int c = pr.vert[4 * pr.edge[4 * (size_t)ed] + 3];
                    if (c < 0) continue;
                    const double* rw = pr.m.rows + (size_t)ed * PGO_ROW;
                    const double *Ji = rw + 6, *Jj = rw + 42;
                    double s = Jj[ca] * Ji[cb];
                    for (int q = 1; q < 6; ++q) s = s + Jj[q * 6 + ca] * Ji[q * 6 + cb];
                    row[(size_t)(c - f) * 36] = row[(size_t)(c - f) * 36] + s;
                }
            }
        }
        if (tid == 0) { pr.m.state[0] = it + 1; L.si[PI_REJ_IT] = 0; }
        __syncthreads();

        // the damped trials of this linearisation
        for (;;) {
            const double lambda = L.sd[PD_LAMBDA];
            // (c) L = H + lambda I, then LDL^T in place
            for (size_t i = tid; i < (size_t)pr.n.env_blocks * 36; i += PGO_BLOCK) pr.m.L[i] = pr.m.H[i];
            if (tid == 0) L.si[PI_SING] = 0;
            __syncthreads();
            for (int t = tid; t < nf * 36; t += PGO_BLOCK) {
                const int r = t / 36, k = t % 36;
                double val = pr.m.diag[(size_t)r * 36 + k];
                if (k / 6 == k % 6) val = val + lambda;
                pr.m.L[((size_t)pr.env_off[r + 1] - 1) * 36 + k] = val;
            }
            __syncthreads();
            bool sing = false;
            for (int k = 0; k < N; ++k) {
                const int kb = k / 6;
                const int lo_k = 6 * pr.env_first[kb], imax = 6 * (pr.reach[kb] + 1);
                for (int m0 = lo_k; m0 < k; m0 += 6 * PGO_PANEL) {
                    const int mend = min(m0 + 6 * PGO_PANEL, k);
                    __syncthreads();
                    if (tid < mend - m0) {
                        L.pk[tid] = *pgo_at(pr, pr.m.L, k, m0 + tid);
                        L.pd[tid] = pr.m.D[m0 + tid];
                    }
                    __syncthreads();
                    for (int i = k + tid; i < imax; i += PGO_BLOCK) {
                        const int fi = pr.env_first[i / 6];
                        if (fi > kb) continue;
                        const int ms = max(m0, 6 * fi);
                        if (ms >= mend) continue;
                        double* dst = pgo_at(pr, pr.m.L, i, k);
                        const double* li = pgo_at(pr, pr.m.L, i, ms);   // (i, ms ..) walks block by block
                        double v = *dst;
                        int m = ms;
                        while (m < mend) {
                            const int stop = min(mend, (m / 6 + 1) * 6);
                            for (; m < stop; ++m, ++li) v = v - (*li * L.pk[m - m0]) * L.pd[m - m0];
                            li += 30;
                        }
                        *dst = v;
                    }
                }
                __syncthreads();
                const double dk = *pgo_at(pr, pr.m.L, k, k);
                if (!(dk > 0.0 && ref_finite(dk))) { sing = true; break; }   // uniform: every lane reads the same pivot
                if (tid == 0) pr.m.D[k] = dk;
                for (int i = k + 1 + tid; i < imax; i += PGO_BLOCK) {
                    if (pr.env_first[i / 6] > kb) continue;
                    double* dst = pgo_at(pr, pr.m.L, i, k);
                    *dst = *dst / dk;
                }
                __syncthreads();
            }
            __syncthreads();

            // (d) (H + lambda I) delta = -b
            if (!sing) {
                for (int i = tid; i < N; i += PGO_BLOCK) pr.m.y[i] = -pr.m.b[i];
                for (int m = 0; m < N; ++m) {
                    __syncthreads();
                    const double ym = pr.m.y[m];
                    const int mb = m / 6, imax = 6 * (pr.reach[mb] + 1);
                    for (int i = m + 1 + tid; i < imax; i += PGO_BLOCK) {
                        if (pr.env_first[i / 6] > mb) continue;
                        pr.m.y[i] = pr.m.y[i] - *pgo_at(pr, pr.m.L, i, m) * ym;
                    }
                }
                __syncthreads();
                for (int i = tid; i < N; i += PGO_BLOCK) pr.m.y[i] = pr.m.y[i] / pr.m.D[i];
                for (int m = N - 1; m > 0; --m) {
                    __syncthreads();
                    const double ym = pr.m.y[m];
                    for (int i = 6 * pr.env_first[m / 6] + tid; i < m; i += PGO_BLOCK)
                        pr.m.y[i] = pr.m.y[i] - *pgo_at(pr, pr.m.L, m, i) * ym;
                }
                __syncthreads();
            }
            const double* y = pr.m.y;
            const double* bb = pr.m.b;
            double dmax = 0.0, scale = 0.0;
            if (!sing) {
                dmax = pgo_seq<true>(L, N, tid, [y](int i) { return y[i]; });
                scale = pgo_seq<false>(L, N, tid, [y, bb, lambda](int i) { return y[i] * (lambda * y[i] - bb[i]); });
            }
            if (tid == 0) {
                L.sd[PD_DMAX] = dmax;
                L.sd[PD_SCALE] = scale;
                if (!sing && dmax <= 64.0 * eps) { L.si[PI_STOP] = GFPL_PGO_STOP_STEP; L.si[PI_DONE] = 1; }
            }
            __syncthreads();
            if (L.si[PI_DONE]) break;

            // the trial poses and their chi2; a vertex whose step is all zero keeps its pose
            if (!sing) {
                for (int r = tid; r < nf; r += PGO_BLOCK) {
                    const int v = pr.free_vert[r];
                    double d[6], Xv[16], Xn[16];
                    bool zero = true;
#pragma unroll
                    for (int i = 0; i < 6; ++i) { d[i] = y[6 * r + i]; zero = zero && d[i] == 0.0; }
#pragma unroll
                    for (int i = 0; i < 16; ++i) Xv[i] = X[16 * (size_t)v + i];
                    if (zero) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) Xn[i] = Xv[i];
                    } else {
                        pgo_update(Xv, d, Xn);
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) Xt[16 * (size_t)v + i] = Xn[i];
                }
                __syncthreads();
                pgo_eval<false>(pr, Xt, tid);
                const double* esq = pr.m.esq;
                const double c = pgo_seq<false>(L, ne, tid, [esq](int i) { return esq[i]; });
                if (tid == 0) L.sd[PD_CHI2T] = c;
            }
            if (tid == 0) {
                // Nielsen's rule on the gain ratio
                const double chi2 = L.sd[PD_CHI2], chi2t = L.sd[PD_CHI2T], sc = L.sd[PD_SCALE];
                bool accept = false;
                double rho = 0.0;
                if (!sing && ref_finite(chi2t) && sc > 0.0 && ref_finite(sc)) {
                    rho = (chi2 - chi2t) / sc;
                    // a trial the sum cannot tell from the current poses is taken too; the chi2 rule then stops
                    accept = rho > 0.0 || chi2t - chi2 <= (64.0 * eps) * chi2;
                }
                if (accept) {
                    const double t = 2.0 * rho - 1.0;
                    double f = 1.0 - (t * t) * t;
                    if (f < 1.0 / 3.0) f = 1.0 / 3.0;
                    L.sd[PD_LAMBDA] = lambda * f;
                    L.sd[PD_NU] = 2.0;
                    L.sd[PD_CHI2_PREV] = chi2;
                    L.sd[PD_CHI2] = chi2t;
                } else {
                    L.sd[PD_LAMBDA] = lambda * L.sd[PD_NU];
                    L.sd[PD_NU] = L.sd[PD_NU] * 2.0;
                    L.si[PI_REJECTS] = L.si[PI_REJECTS] + 1;
                    L.si[PI_REJ_IT] = L.si[PI_REJ_IT] + 1;
                    if (sing) L.si[PI_STATUS] |= GFPL_PGO_SINGULAR;
                    if (L.si[PI_REJ_IT] >= a.prm.max_rejects) { L.si[PI_STOP] = GFPL_PGO_STOP_REJECT; L.si[PI_DONE] = 1; }
                }
                L.si[PI_ACCEPT] = accept ? 1 : 0;
            }
            __syncthreads();
            if (L.si[PI_ACCEPT]) {
                for (int r = tid; r < nf; r += PGO_BLOCK) {
                    const int v = pr.free_vert[r];
#pragma unroll
                    for (int i = 0; i < 16; ++i) X[16 * (size_t)v + i] = Xt[16 * (size_t)v + i];
                }
                break;
            }
            if (L.si[PI_DONE]) break;
        }
        __syncthreads();
        if (tid == 0 && !L.si[PI_DONE]) {
            L.si[PI_ITERS] = it + 1;
            const double prev = L.sd[PD_CHI2_PREV], now = L.sd[PD_CHI2];
            if (prev - now <= (64.0 * eps) * prev) { L.si[PI_STOP] = GFPL_PGO_STOP_DCHI2; L.si[PI_DONE] = 1; }
            else if (it + 1 >= a.prm.max_iters) L.si[PI_DONE] = 1;
        }
        __syncthreads();
    }

    // write back (:4314-4326, PG4): every vertex, fixed ones too
    for (int v = tid; v < nv; v += PGO_BLOCK) {
        const int kf = pr.vert[4 * v];
        double Xv[16], x[6], T[16], Tp[16], Tpi[16], C[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) { Xv[i] = X[16 * (size_t)v + i]; Tp[i] = pr.T_kf[16 * (size_t)kf + i]; }
        logmap_se3(Xv, x);
        expmap_se3(x, T);
        logmap_se3(T, x);
        inverse_se3(Tp, Tpi);
        mat4_mul(T, Tpi, C);
#pragma unroll
        for (int i = 0; i < 16; ++i) { pr.T_kf[16 * (size_t)kf + i] = T[i]; pr.m.corr[16 * (size_t)kf + i] = C[i]; }
#pragma unroll
        for (int i = 0; i < 6; ++i) pr.x_kf[6 * (size_t)kf + i] = x[i];
        pr.m.moved[kf] = 1;
    }
    __syncthreads();
    // the keyframes after kf_curr take the LAST optimised keyframe's correction (:4368-4372)
    if (nv > 0) {
        const int last = pr.vert[4 * (nv - 1)];
        for (int kf = pr.kf_curr + 1 + tid; kf < nkf; kf += PGO_BLOCK) {
            if (!pr.alive[kf]) continue;
            double C[16], T[16], Tn[16], x[6];
#pragma unroll
            for (int i = 0; i < 16; ++i) { C[i] = pr.m.corr[16 * (size_t)last + i]; T[i] = pr.T_kf[16 * (size_t)kf + i]; }
            mat4_mul(C, T, Tn);
            logmap_se3(Tn, x);
#pragma unroll
            for (int i = 0; i < 16; ++i) { pr.T_kf[16 * (size_t)kf + i] = Tn[i]; pr.m.corr[16 * (size_t)kf + i] = C[i]; }
#pragma unroll
            for (int i = 0; i < 6; ++i) pr.x_kf[6 * (size_t)kf + i] = x[i];
            pr.m.moved[kf] = 1;
        }
    }
    if (tid == 0) {
        gfpl_pgo_result r;
        r.iters = L.si[PI_ITERS]; r.stop = L.si[PI_STOP]; r.status = L.si[PI_STATUS]; r.rejects = L.si[PI_REJECTS];
        r.n_vert = nv; r.n_free = nf; r.n_edge = ne; r.kf_curr = pr.kf_curr;
        r.lambda = L.sd[PD_LAMBDA]; r.chi2_0 = L.sd[PD_CHI2_0]; r.chi2 = L.sd[PD_CHI2];
        a.out[blockIdx.x] = r;
    }
}

// R p + t as Eigen's block product writes it
GFPL_DEV void pgo_move(const double* C, double* p) {
    const double x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = ((C[i * 4 + 0] * x + C[i * 4 + 1] * y) + C[i * 4 + 2] * z) + C[i * 4 + 3];
}

__global__ void __launch_bounds__(PGO_BLOCK) k_pgo_correct(const PgoProb* probs) {
    const PgoProb& pr = probs[blockIdx.y];
    const int j = blockIdx.x * PGO_BLOCK + threadIdx.x;
    if (j >= pr.n.n_pt + pr.n.n_ls) return;
    const int32_t* job = pr.jobs + 4 * (size_t)j;
    const int lm = job[0], kf = job[1];
    if (!pr.m.moved[kf]) return;
    double C[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) C[i] = pr.m.corr[16 * (size_t)kf + i];
    const bool line = j >= pr.n.n_pt;
    if (!line) {
        pgo_move(C, pr.pt + 3 * (size_t)lm);
    } else {
        pgo_move(C, pr.ls + 6 * (size_t)lm);
        pgo_move(C, pr.ls + 6 * (size_t)lm + 3);
    }
    double* dir = line ? pr.ls_dir : pr.pt_dir;
    if (dir)
        for (int d = 0; d < job[3]; ++d) pgo_move(C, dir + 3 * ((size_t)job[2] + d));   // directions are translated too, as written
}

hipError_t launch_pgo(const PgoArgs& a, int n, hipStream_t s) {
    const PgoLds size(nullptr);
    hipLaunchKernelGGL(k_pgo, dim3(n), dim3(PGO_BLOCK), size.bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_pgo_correct(const PgoProb* probs, int n, int max_jobs, hipStream_t s) {
    hipLaunchKernelGGL(k_pgo_correct, dim3((max_jobs + PGO_BLOCK - 1) / PGO_BLOCK, n), dim3(PGO_BLOCK), 0, s, probs);
    return hipGetLastError();
}

}  // namespace gfpl
