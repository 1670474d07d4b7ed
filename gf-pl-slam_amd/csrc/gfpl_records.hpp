// gfpl_records.hpp — the small per-sequence and per-line records the step's kernels, the ABI, the
// tests and tools/ exchange, each stated once: the step record, the debug slots, the line-cut
// records.  (Buffers' sizes and LDS layouts: gfpl_layout.hpp.)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gfpl.h"

namespace gfpl {

// ------------------------------------------------------------- step record --
// DevScratch::bytes: STEP_REC int64 per sequence.  The slots are public (gfpl_debug_step_records
// hands the raw layout out): GFPL_STEP_* in include/gfpl.h, mirrored by gfpl.StepSlot.  Writers:
//   k_step_bytes         every slot but the ones below (zeroes those when their kernel does not run)
//   k_cut_search* (all)  GFPL_STEP_CUT_STEPS, _CUT_EXACT, _CUT_UNBOUNDED
//   k_pose_finish        GFPL_STEP_INLIERS_POSE
//   k_cut_verify         GFPL_STEP_PROOF_REDONE .. _PROOF_LINES (k_cut_verify_detail ORs into _REDONE)
constexpr int STEP_REC = GFPL_STEP_REC;
// a -DGFPL_CUT_CLOCK build of k_cut_search stores the wave's duration (wall clock ticks) where the
// product build counts the lines without a usable bound (tools/cut_balance.py)
constexpr int STEP_CUT_CLOCK_DURATION = GFPL_STEP_CUT_UNBOUNDED;

constexpr int64_t* step_rec(int64_t* bytes, int b) { return bytes + (size_t)STEP_REC * b; }

// ------------------------------------------------------------- debug slots --
// DevScratch::dbg: DBG_REC int64 per sequence (gfpl_debug_clocks).  Several kernels share the eight
// slots; a later kernel of the step overwrites an earlier one's.  Product builds:
//   k_cut_search<false>, cut_proof 0   DBG_CUT_HW_ID, DBG_CUT_XCC_ID   (test_cut_progress_partner_slots)
//   k_cut_verify                       DbgVerify, all eight            (tools/verify_diag.py)
//   k_cut_verify_detail                adds to DBG_VFY_XCHK
//   k_cut_search_eig                   DBG_EIG_SWEEPS, DBG_EIG_EVALS   (tools/cut_metric_times.py)
// Diagnostic builds (PhaseClock / DIAG_STAMP, gfpl_device.hpp), per compile flag:
//   GFPL_CUT_CLOCK     k_cut_search     DbgCutClock: the wave's wall clock at its start / end, HW_ID, XCC_ID;
//                                       its duration in the step record (STEP_CUT_CLOCK_DURATION)
//   GFPL_CUT_PCLOCK    k_cut_search     DbgCutPhase: cycles of step evaluation + decision, exact rounds,
//                                       bookkeeping, transitions | of a transition's three parts (the
//                                       finished line's info + next record and S, open_line + prefetch,
//                                       progress exchange) | iterations << 32 | transitions (tools/cut_phases.py)
//   GFPL_CUTW_CLOCK    k_cut_search_w   DbgCutW: cycles of grid evaluation, decisions, walk, exact rounds,
//                                       transitions | rounds, transitions, steps
//   GFPL_CUTW_TCLOCK   k_cut_search_w   slots 0-6: cycles of a transition's parts (0 the finished line's
//                                       info, 1 the next line's data, 2-6 open_line's)
//   GFPL_VERIFY_CLOCK  k_cut_verify     slots 0-4: cycles of its five per-line phases (over DbgVerify's 0-4)
//   GFPL_SP_CLOCK      k_stereo_points  slots 0-5: wall clock at start, setup done, band scan done, jobs
//                                       sorted (SEG), sub-pixel SAD done, end (tools/sp_phases.py);
//                                       with GFPL_SP_PROBE_NOSAD slot 7 accumulates the scan's keys
//   GFPL_SL_CLOCK      k_stereo_lines   slots 0-4: wall clock at start, train rows staged, knn pass,
//                                       medians, end (tools/sp_phases.py --lines)
//   GFPL_POSE_CLOCK    k_pose           slots 0-7: wave 0's cycles per phase (0 gather, 1 a GN iteration's
//                                       chunk loop, 2 H + solve, 3 pose update, 4 removeOutliers, 5 with
//                                       helper waves a round's evaluation, 7 between the GN runs)
//   GFPL_PFIN_CLOCK    k_pose_finish    DbgPoseFinish: cycles of H^-1, the eigenvalues (wave 1), the rest (wave 0)
constexpr int DBG_REC = 8;
constexpr int64_t* dbg_row(int64_t* dbg, int b) { return dbg + DBG_REC * (size_t)b; }

enum DbgCutSearch { DBG_CUT_HW_ID = 6, DBG_CUT_XCC_ID = 7 };
enum DbgVerify {   // (the four terms and the worst ratio are doubles' bit patterns)
    DBG_VFY_TS = 0, DBG_VFY_TK = 1, DBG_VFY_TA = 2, DBG_VFY_TV = 3,   // the worst line's bound terms / R0
    DBG_VFY_MASK = 4,    // OR of the lanes' reason masks
    DBG_VFY_WORST = 5,   // the worst covered line's E / R0
    DBG_VFY_XCHK = 6,    // steps re-decided with the reference's arithmetic
    DBG_VFY_DLINES = 7   // lines left to k_cut_verify_detail
};
enum DbgCutEig { DBG_EIG_SWEEPS = 0, DBG_EIG_EVALS = 1 };
enum DbgCutClock { DBG_CCK_BEGIN = 0, DBG_CCK_END = 1, DBG_CCK_HW_ID = 2, DBG_CCK_XCC_ID = 3 };
enum DbgCutPhase { DBG_CPK_PHASES = 0 /* 4 */, DBG_CPK_TRANS = 4 /* 3 */, DBG_CPK_COUNTS = 7 };
enum DbgCutW { DBG_CWK_PHASES = 0 /* 5 */, DBG_CWK_ROUNDS = 5, DBG_CWK_TRANS = 6, DBG_CWK_STEPS = 7 };
enum DbgStereo { DBG_SP_PROBE_KEYS = 7 };
enum DbgPoseFinish { DBG_PFIN_INVERSE = 0, DBG_PFIN_EIG = 1, DBG_PFIN_REST = 2 };

// -------------------------------------------------------- line-cut records --
#define CUT_PATH 64   // proven mode: recorded search steps per line (k_cut_search -> k_cut_verify)
#define CUT_P_STAY 8  //   step byte: no neighbour beat the centre (the line ends), else the move j (0-7)
#define CUT_P_EXACT 16 //  step byte flag: the step was decided by the reference's arithmetic (exact round)
#define CUT_KS 22     // proven line cut: ratio keys per side (KParams::cut_keys)

// DevScratch::cut_rec, CUT_REC doubles per matched line: comparison data (k_cut_prep, PD_*) | r = 0
// info (CUT_INFO, lower triangle) | the line's agreement bound as k_cut_search formed it | pad
#define CUT_FAST 56   // doubles of per-line comparison data: polynomials, flags, error bounds
#define CUT_REC 80    // doubles of a per-line cut record (640 B)
constexpr int CUT_INFO = 21;                  // lower triangle of a 6 x 6 info matrix
constexpr int CUT_NX = CUT_FAST + CUT_INFO;   // used part of a line record: comparison data | r = 0 info
constexpr int CUT_NX_EB = 3;                  // record slots CUT_NX .. CUT_NX + 2: CutCmp::eb's 6 floats
                                              // (diagnostics: gfpl_debug_cut_records, tools/cut_diag.py)
#define PD_PS 0      // start side (sP -> eP, t = r0): P coefficients of t^0, t^1, t^2 [3 x 6]
#define PD_PE 18     // end side (eP -> sP, t = r1) [3 x 6]
#define PD_VS 36     // v'_s(t) coefficients of t^0 .. t^4 [5]
#define PD_VE 41     // v'_e(t) [5]
#define PD_OK 46     // 1.0: gz^2 > 2 homog_th at both ends, one sign (fgz2 = fx / gz^2 on the segment)
#define PD_NEXT 47   // list index of the line after this one (k_cut_search's prefetch)
#define PD_ERR 48    // k_cut_bounds: 14 floats (rounded up) packed in 7 doubles, per side (start, end):
                     // eP[6] (|P(t) - P*(t)|, ours + the reference's endpoint Jacobian in P units) | ev
                     // (|v'(t) - v'*(t)|), valid for every t of the range; +inf: no margined steps
static_assert(PD_ERR + 7 <= CUT_FAST && CUT_FAST == 56, "per-line comparison data layout");
static_assert(CUT_REC * 8 == 640 && CUT_NX + CUT_NX_EB <= CUT_REC, "a record is 5 x 128 B: five 16-B loads per lane");

// DevScratch::cut_sum, per sequence: invCov_sum (CUT_INFO doubles, lower triangle) after the r = 0 pass
constexpr int CUT_SUM_REC = 24;

// DevScratch::cut_vmax, per line (proven mode, k_cut_vref -> k_cut_verify): over the ratios its margined
// steps compared, max 1 / v' and max r_v / v' per side [0..3], margined steps + 1024 x variances
// evaluated [4], ratios whose v' comparison failed [5] | k_cut_ebound's operand bounds, 14 floats
constexpr int CUT_VMAX_EB = 6;      // first double of the operand bounds
constexpr int CUT_VMAX = CUT_VMAX_EB + 8;

// DevScratch::cut_dtl, per detail-list entry (k_cut_verify -> k_cut_verify_detail): S_full at the
// line's start | the line's bound terms
#define CUT_DTL 4     // detail-list entries per sequence (a sequence past them is redone eagerly)
constexpr int CUT_DTL_REC = 32;
enum CutDtl {
    DTL_S = 0,   // CUT_INFO doubles
    DTL_K0 = CUT_INFO, DTL_A1, DTL_B1, DTL_CS, DTL_CE, DTL_R0, DTL_RTS, DTL_RTE, DTL_OK, DTL_END
};
static_assert(DTL_END <= CUT_DTL_REC, "cut_dtl record");

}  // namespace gfpl
