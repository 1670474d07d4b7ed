// gfpl_ba.hpp — the bundle-adjustment arithmetic that k_lba.hip (one workgroup per problem) and
// k_gba.hip (one problem over many launches) share: an observation's row (the association order
// of every product is pinned, ledger BA*, GB8), the start of the Levenberg-Marquardt loop's state
// words BA_SD_* / BA_SI_* (gfpl_layout.hpp), the pose update and the result record.
// Each solver keeps on purpose: the landmark blocks' inversion and back-substitution (explicit
// inverse in the LBA, block LDL^T in the GBA, ledger GB11) and the reduced system with its
// factorisation (LDS-resident against multi-launch).  The choice of an observation's pose and
// landmark, the landmark sums and the loop's control are the same text in both as well, but as
// functions called from both they changed the kernels' instruction text
// (profiles/ba_shared/asm_notes.md), so they stay stated in each.
#pragma once
#include "gfpl_kernels.hpp"

namespace gfpl {

// the six pose terms of :1277-1282 (the landmark's three are its first three) for the error (ex, ey)
GFPL_DEV void ba_jac(const DevCam& cam, double th, const double* g, double ex, double ey, double* J) {
    const double gx = g[0], gy = g[1], gz = g[2];
    const double gz2 = 1.0 / ref_max(th, gz * gz);
    const double a = cam.fx * ex, b = cam.fy * ey;
    J[0] = (gz2 * a) * gz;
    J[1] = (gz2 * b) * gz;
    J[2] = (-gz2) * (a * gx + b * gy);
    J[3] = (-gz2) * (((a * gx) * gy + (b * gy) * gy) + (b * gz) * gz);
    J[4] = gz2 * (((a * gx) * gx + (a * gz) * gz) + (b * gx) * gy);
    J[5] = gz2 * ((b * gx) * gz - (a * gy) * gz);
}

// J^T R, column j (Jij.transpose() * Tiw.block(0,0,3,3))
GFPL_DEV double ba_jtr(const double* J, const double* Ti, int j) {
    return (J[0] * Ti[0 * 4 + j] + J[1] * Ti[1 * 4 + j]) + J[2] * Ti[2 * 4 + j];
}

// point observation (:1252-1293): Ti is the inverse pose
GFPL_DEV void ba_point_row(const DevCam& cam, double th, const double* Ti, const double* Xw, const double* obs, double s2,
                           double* row) {
    double Xc[3], uv[2], J[6];
    se3_apply(Ti, Xw, Xc);
    projection(cam, Xc, uv);
    const double dx = obs[0] - uv[0], dy = obs[1] - uv[1];
    const double nrm = sqrt(dx * dx + dy * dy);
    ba_jac(cam, th, Xc, dx, dy, J);
    const double d = ref_max(th, nrm);
#pragma unroll
    for (int i = 0; i < 6; ++i) row[i] = J[i] / d;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        row[6 + j] = ba_jtr(J, Ti, j) / d;
        row[9 + j] = 0.0;
    }
    row[12] = nrm;
    row[13] = 1.0 / (1.0 + (nrm * nrm) * s2);
}

// line observation (:1331-1402)
GFPL_DEV void ba_line_row(const DevCam& cam, double th, const double* Ti, const double* PQ, const double* l, double s2,
                          double* row) {
    double Pc[3], Qc[3], pu[2], qu[2], JP[6], JQ[6];
    se3_apply(Ti, PQ, Pc);
    se3_apply(Ti, PQ + 3, Qc);
    projection(cam, Pc, pu);
    projection(cam, Qc, qu);
    const double e0 = (l[0] * pu[0] + l[1] * pu[1]) + l[2];
    const double e1 = (l[0] * qu[0] + l[1] * qu[1]) + l[2];
    const double nrm = sqrt(e0 * e0 + e1 * e1);
    ba_jac(cam, th, Pc, e0, e1, JP);
    ba_jac(cam, th, Qc, e0, e1, JQ);
    const double d = ref_max(th, nrm);
#pragma unroll
    for (int i = 0; i < 6; ++i) row[i] = (JP[i] * e0 + JQ[i] * e1) / d;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        row[6 + j] = (ba_jtr(JP, Ti, j) * e0) / d;
        row[9 + j] = (ba_jtr(JQ, Ti, j) * e1) / d;
    }
    row[12] = nrm;
    row[13] = 1.0 / (1.0 + (nrm * nrm) * s2);
}

// ---- the loop's state words sd (BA_SD_*) and si (BA_SI_*), by one lane

// before the pre-pass (:1225-1232, :1964-1966)
GFPL_DEV void ba_state_init(double* sd, int32_t* si, double lambda_lm) {
    sd[BA_SD_LAMBDA] = lambda_lm;
    sd[BA_SD_ERR] = 0.0;   // `double err` starts undefined (:1964): pinned to 0.0
    sd[BA_SD_ERRPREV] = 999999999.9;
    si[BA_SI_ITERS] = 1; si[BA_SI_STOP] = 0; si[BA_SI_STATUS] = 0; si[BA_SI_HMAX] = 0; si[BA_SI_DONE] = 0;
}

// the record of a finished loop
GFPL_DEV gfpl_lba_result ba_record(const double* sd, const int32_t* si) {
    gfpl_lba_result r;
    r.iters = si[BA_SI_ITERS]; r.stop = si[BA_SI_STOP]; r.status = si[BA_SI_STATUS]; r.hmax = si[BA_SI_HMAX];
    r.lambda = sd[BA_SD_LAMBDA]; r.err = sd[BA_SD_ERR]; r.err_prev = sd[BA_SD_ERRPREV];
    return r;
}

// the pose update (:1443-1451, :1669-1677): x = logmap(expmap(x) inverse(expmap(dx)))
GFPL_DEV void ba_pose_update(double* x, const double* dx) {
    double Tp[16], E[16], Ei[16], Tc[16], xn[6];
    expmap_se3(x, Tp);
    expmap_se3(dx, E);
    inverse_se3(E, Ei);
    mat4_mul(Tp, Ei, Tc);
    logmap_se3(Tc, xn);
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = xn[i];
}

}  // namespace gfpl
