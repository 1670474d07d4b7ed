// gfpl_kernels.hpp — launchers implemented in the k_*.hip translation units.
#pragma once
#include "gfpl_layout.hpp"
#include "gfpl_state.hpp"

#include <atomic>
#include <cstdlib>

namespace gfpl {

// An integer from the environment (decimal, or hex with 0x), `dflt` when the variable is unset: the
// launchers' batch-size thresholds and debug switches.  Read at every call, so a process may change
// a variable between launches (the tests do).
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    if (!e) return dflt;
    return (int)strtol(e, nullptr, (e[0] == '0' && (e[1] == 'x' || e[1] == 'X')) ? 16 : 10);
}

// A kernel's dynamic-LDS ceiling above the 64 KB default, set once per device (the attribute
// belongs to the device's kernel object; contexts on several devices may share the process).
// *done: one bit per device id < 64 (idempotent: two threads setting it race harmlessly)
inline hipError_t ensure_dyn_lds(const void* fn, int bytes, std::atomic<unsigned long long>* done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = dev < 64 ? 1ull << dev : 0ull;
    if (bit && (done->load(std::memory_order_acquire) & bit)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && bit) done->fetch_or(bit, std::memory_order_acq_rel);
    return e;
}

// the ceiling every kernel whose layout can exceed 64 KB asks for: a CU's 160 KB less room for static LDS
constexpr int DYN_LDS_CEILING = 160 * 1024 - 1024;

// the batch size up to which the stereo and cross stages run 16 waves per sequence (k_stereo.hip)
int sp_wide_max_b();
hipError_t launch_stereo_points(const KParams& p, hipStream_t s);
hipError_t launch_stereo_lines(const KParams& p, hipStream_t s);
hipError_t launch_line_uncertainty(const KParams& p, hipStream_t s);
hipError_t launch_init(const KParams& p, hipStream_t s);
// k_match.hip: knn-2 of one descriptor set against another (idx / dist [nq][2]), and of B sequences'
// sets at q / t + b * cap * 32 with counts min(nq[b], cap) / min(nt[b], cap) (device), packed
// (idx0, d0, d1) at packed + b * cap * 6 (a frame's two directions share the sequence's block)
hipError_t launch_knn2(const uint8_t* q, int nq, const uint8_t* t, int nt, int cell, int32_t* idx, float* dist,
                       hipStream_t s);
hipError_t launch_knn2_batched(const uint8_t* q, const int* nq, const uint8_t* t, const int* nt, int cap, int B,
                               int cell, int32_t* packed, hipStream_t s);
// launch_knn2 with the two counts on the device (min(*nq, cap) / min(*nt, cap) rows): idx / dist [cap][2]
hipError_t launch_knn2_counts(const uint8_t* q, const int* nq, const uint8_t* t, const int* nt, int cap, int cell,
                              int32_t* idx, float* dist, hipStream_t s);
// radiusMatch rows (count pass, then the rows at row_off) and knn-2 list statistics
hipError_t launch_radius_count(const uint8_t* q, int nq, const uint8_t* t, int nt, int cell, float radius,
                               int32_t* cnt, hipStream_t s);
hipError_t launch_radius_rows(const uint8_t* q, int nq, const uint8_t* t, int nt, int cell, float radius,
                              const int32_t* row_off, int32_t* idx, float* dist, hipStream_t s);
hipError_t launch_match_stats(int kind, const float* d0, const float* d1, int n, int max_num, double* out,
                              hipStream_t s);
hipError_t launch_cross_points(const KParams& p, hipStream_t s);
hipError_t launch_cross_lines(const KParams& p, hipStream_t s);
hipError_t launch_line_cut(const KParams& p, hipStream_t s, const hipEvent_t* marks /* [2] or null */);
hipError_t launch_pose(const KParams& p, hipStream_t s, hipEvent_t mark /* or null */);
hipError_t launch_step_bytes(const KParams& p, hipStream_t s);
hipError_t launch_need_kf(const KParams& p, hipStream_t s);
hipError_t launch_curr_frame_is_kf(const KParams& p, const int32_t* mask /* device [B] */, hipStream_t s);

// lookForCommonMatches keyframe-pair gate (k_kf.hip); all pointers device
struct KfGate {
    DevCam cam;
    double T0[16], T1[16];
    double max_ratio_12_p, desc_th_l;
    int lines, n0;
    int map;                // 0: keyframe pair (DT = inv(T1) T0), 1: local map (Twf = inv(T1))
    const int32_t* loc;     // map mode: query row -> caller's map row
    int p_stride;           // doubles between rows of P0 / eP0 (3, or 6 for line3D)
    double epip_p, epip_l;  // map mode: maxKFEpipP / maxKFEpipL
    const double* le1;      // map mode: kf1 le [n1][3] (lines)
    const int32_t* i12;     // knn-2 kf0 -> kf1 [2 n0]
    const float* d12;
    const int32_t* i21;     // knn-2 kf1 -> kf0 [2 n1]
    const double* P0;       // kf0 P (points) / sP (lines) [n0][3]
    const double* eP0;      // kf0 eP [n0][3] (lines)
    const double* le0;      // kf0 le [n0][3] (lines)
    const double* sigma2_0; // kf0 sigma2 [n0]
    const double* pl1;      // kf1 pl [n1][2] (points)
    int32_t* pairs;         // [2 n0]
    int* count;
};
hipError_t launch_kf_gate(const KfGate& g, hipStream_t s);
// local-map rows in view in front of kf1 (map order): loc / n (device)
hipError_t launch_kf_map_filter(const DevCam& cam, const double* T1, const double* P, int n, int lines,
                                int32_t* loc, uint8_t* desc_out, const uint8_t* desc_in, int* count, hipStream_t s);

// fuseLandmarksFromLocalMap's candidate search (k_fuse.hip); all pointers device
struct FuseSelect {
    DevCam cam;
    int lines, n, n_kf;
    const double* X;          // [n][3] point3D or [n][6] line3D
    const int32_t* kf;        // [n] kf_obs_list[0]
    const double* T_kf;       // [n_kf][16]
    const uint8_t* desc_in;   // [n][32], 16-B aligned; null: no descriptor is copied
    int32_t* loc;             // [n] map row of selected row j
    uint8_t* desc_out;        // [n][32] the selected rows' descriptors
    int* count;               // selected rows
    int* bad_kf;              // set to 1 by a row whose kf is outside [0, n_kf)
};
struct FuseGate {
    int lines, cap;           // cap: the map's rows (what loc / idx / pairs hold)
    const int* n_sel;         // k_fuse_select's count
    const int32_t* loc;
    const int32_t* idx;       // knn-2 of the selected rows against themselves [cap][2]
    const double* X;
    double max_pp, max_pl, max_dl;   // maxPointPointError, maxPointLineError, maxDirLineError
    int32_t* pairs;           // [cap][2] (i, t) over the selected list
    int* count;
};
hipError_t launch_fuse_select(const FuseSelect& a, hipStream_t s);
hipError_t launch_fuse_gate(const FuseGate& g, hipStream_t s);

// isLoopClosure (k_loop.hip): one candidate pair's knn-2 lists and feature arrays; all pointers device.
// pi12 / li12 are null for a kind with fewer than two rows on either keyframe (ledger U4).
struct LoopPair {
    int n0_pt, n0_ls;
    const int32_t *pi12, *pi21;   // point knn-2 kf0 -> kf1 [2 n0_pt], kf1 -> kf0 [2 n1_pt]
    const int32_t *li12, *li21;   // the same for lines
    const double* P0;             // kf0 P [n0_pt][3]
    const double* pl1;            // kf1 pl [n1_pt][2]
    const double *sP0, *eP0;      // kf0 sP / eP [n0_ls][3]
    const double* le1;            // kf1 le [n1_ls][3]
};
struct LoopArgs {
    DevCam cam;
    double homog_th;
    int max_iters;
    gfpl_loop_params prm;
    const LoopPair* pairs;        // [n]
    int pt_cap, ls_cap;
    int32_t* pt_pairs;            // [n][pt_cap][2]
    uint8_t* pt_inlier;           // [n][pt_cap]
    int32_t* ls_pairs;
    uint8_t* ls_inlier;
    gfpl_loop_result* out;        // [n]
};
hipError_t launch_loop_closure(const LoopArgs& a, int n, hipStream_t s);

// DBoW2 transform and score (k_bow.hip); all pointers device.  The vocabulary's arrays are BowVocabMem's.
struct BowVocabDev {
    const uint8_t* desc;
    const BowNode* node;
    const int32_t* rank_word;
    const double* rank_weight;
    int weighting;                // GFPL_BOW_TF_IDF ... GFPL_BOW_BINARY
};
struct BowSet {                   // one descriptor set of a transform call
    const uint8_t* desc;          // [count][32]
    int count, pad;
};
struct BowPair {                  // one pair of a score call: L1Scoring::score(a, b)
    const int32_t* ia; const double* va;
    const int32_t* ib; const double* vb;
    int na, nb;
};
// keys [n][cap]: scratch; word_ids / values [n][cap], n_words [n]: outputs; max_count: the largest count
hipError_t launch_bow_transform(const BowVocabDev& v, const BowSet* sets, int n, int max_count, int cap, int32_t* keys,
                                int32_t* word_ids, double* values, int32_t* n_words, hipStream_t s);
hipError_t launch_bow_score(const BowPair* pairs, int n, double* scores, hipStream_t s);

// levMarquardtOptimizationLBA (k_lba.hip): one problem; all pointers device.  lm_start / obs_lm /
// obs_kf are LbaMem's uploaded index arrays over the unified landmark and observation numbering.
struct LbaProb {
    gfpl_lba_counts n;
    const double* x_kf;
    double* T_kf;
    const double* T_fix;
    double *pt, *ls;
    const double *pt_obs, *pt_sigma, *ls_obs, *ls_sigma;
    double* x_out;
    const int32_t *lm_start, *obs_lm, *obs_kf;
    LbaPtrs m;
};
struct LbaArgs {
    DevCam cam;                   // fx, fy, cx, cy are read
    double homog_th;
    gfpl_lba_params prm;
    const LbaProb* probs;         // [n]
    gfpl_lba_result* out;         // [n]
    int lds_kfs;                  // the largest n_kf of the launch (LbaLds)
};
hipError_t launch_lba(const LbaArgs& a, int n, hipStream_t s);

// levMarquardtOptimizationGBA (k_gba.hip): one problem over many workgroups; all pointers device.
// The index arrays are GbaIdx's uploaded copies of the planner's lists, m the workspace (GbaMem).
// THE RULES THAT DIFFER FROM THE LBA live in GbaRules, read by the kernels at the four places they
// bind (ledger GB3, GB5, GB7, GB9); gfpl_gba_solve passes GBA_RULES_REFERENCE.
struct GbaRules {
    int divisor_zero;         // the iterations divide err by Npt_obs + Nls_obs = 0 (else by Npt + Nls, the LBA's)
    int line_th_homog;        // the iterations' line terms keep homogTh (else 1e-7, the LBA's)
    int prepass_transposed;   // the pre-pass writes a line's coupling block under the diagonal transposed
    int any_sign_pivot;       // a finite non-zero pivot of S of either sign is accepted (else positive only, BA13)
};
constexpr GbaRules GBA_RULES_REFERENCE{1, 1, 1, 1};
struct GbaProb {
    gfpl_gba_counts n;
    const double* x_kf;
    double* T_kf;
    const double* T_fix;
    double *pt, *ls;
    const double *pt_obs, *pt_sigma, *ls_obs, *ls_sigma;
    double* x_out;
    const int32_t *lm_start, *obs_lm, *obs_kf, *obs_pair, *pair_start, *pair_kf, *kf_start, *kf_obs, *blk_start, *terms;
    GbaPtrs m;
};
struct GbaArgs {
    DevCam cam;                   // fx, fy, cx, cy are read
    double homog_th;
    gfpl_lba_params prm;
    GbaRules rules;
    GbaProb pr;
    gfpl_lba_result* out;         // the problem's record
};
// how the wide phases are cut into workgroups; no result depends on it (tests/test_gba_gpu.py)
struct GbaGrid {
    int block = GBA_BLOCK;        // threads per workgroup of the per-observation / per-landmark phases: 64 .. 256
    int ldlt_kfs = GBA_LDLT_KFS;  // block rows per workgroup of k_gba_ldlt: 1 .. GBA_MAX_LDLT_ROWS
};
// every launch of one problem's solve, all iterations, in stream order; nothing is synchronised
hipError_t enqueue_gba(const GbaArgs& a, const GbaGrid& grid, hipStream_t s);
int gba_max_lds_bytes(int n_kf);

// the landmark descriptor store (k_lm.hip); all pointers device.  The store's arrays are LmStoreMem's,
// work / ops LmWorkMem's.
struct LmStoreDev {
    uint8_t* rows;
    int32_t* count;
    int32_t* med_idx;
    uint8_t* med;
    int obs_cap;
};
// work items [work0, work0 + n_work) through lane groups of lm_bucket_lanes(bucket)
hipError_t launch_lm_apply(const LmStoreDev& st, const LmWork* work, const LmOpDev* ops, int work0, int n_work,
                           int bucket, hipStream_t s);
hipError_t launch_lm_gather(const LmStoreDev& st, const int32_t* ids, int n, uint8_t* desc_out, int32_t* med_idx_out,
                            hipStream_t s);
// the same two for a device-planned call: the bucket's range is read from hdr (LM_H_BUCKET) and nothing runs
// when hdr's error word is set.  n_max: the most work items the bucket can hold (the grid is sized from it)
hipError_t launch_lm_apply_dev(const LmStoreDev& st, const LmWork* work, const LmOpDev* ops, const int32_t* hdr, int n_max,
                               int bucket, hipStream_t s);
hipError_t launch_lm_gather_dev(const LmStoreDev& st, const int32_t* hdr, const int32_t* ids, int n, uint8_t* desc_out,
                                int32_t* med_idx_out, hipStream_t s);
// the device planner (k_lm_plan.hip); all pointers device.  The scratch is LmPlanMem's.
struct LmPlanDev {
    int32_t *hdr, *pend, *op0, *place, *tile_w, *tile_o;
    int lm_cap, max_ops, min_g;
};
// one observe call.  first_new: ids from here on are created (lm_cap: none, the local-map stage); unm_rows
// null: column 1 of pairs is a row of desc1, otherwise a row of unm_rows and column 0 is not read
struct LmObserve {
    const uint8_t *desc0, *desc1;
    const int32_t *pairs, *unm_rows, *lm_out;
    int n, n0, n1, n_unm, first_new;
};
// every launch of one call in stream order: check, plan (reduce, scan, scatter, ops), the six buckets
hipError_t enqueue_lm_observe(const LmStoreDev& st, const LmPlanDev& p, const LmObserve& a, LmWork* work, LmOpDev* ops,
                              hipStream_t s);
hipError_t enqueue_lm_free_ids(const LmStoreDev& st, const LmPlanDev& p, const int32_t* ids, int n, hipStream_t s);
hipError_t enqueue_lm_gather_ids(const LmStoreDev& st, const LmPlanDev& p, const int32_t* ids, int n, uint8_t* desc_out,
                                 int32_t* med_idx_out, hipStream_t s);

// the loop-closure pose graph (k_pgo.hip): one problem; all pointers device.  The index arrays are
// PgoIdx's uploaded copies of the planner's lists, m the problem's workspace (PgoMem).
struct PgoProb {
    gfpl_pgo_counts n;            // n_pt / n_ls: point / line jobs
    int32_t kf_curr, pad;
    double *T_kf, *x_kf, *pt, *ls, *pt_dir, *ls_dir;
    const int32_t *vert, *free_vert, *edge, *inc_start, *inc, *env_first, *env_off, *reach, *lc, *alive, *jobs;
    const double* lc_pose;
    PgoPtrs m;
};
struct PgoArgs {
    gfpl_pgo_graph_params prm;
    const PgoProb* probs;         // [n]
    gfpl_pgo_result* out;         // [n]
};
hipError_t launch_pgo(const PgoArgs& a, int n, hipStream_t s);
// the map correction of n problems whose largest job count is max_jobs (> 0)
hipError_t launch_pgo_correct(const PgoProb* probs, int n, int max_jobs, hipStream_t s);

// the map's index half (k_kfmap.hip); all pointers device.  The arrays are KfMapMem's: KfMapLm one
// kind's (points or lines), KfMapCore what the kinds share and the workspace.
struct KfMapLm {
    uint8_t *alive, *local, *inlier;
    int32_t *nobs, *owner, *obs;  // obs [cap][obs_cap]
    int32_t* idx;                 // [kf_cap][rows] the features' idx
    int32_t* kf_n;                // [kf_cap] rows in use
    int rows, cap;
    int next;                     // the kind's next id when the call starts
};
struct KfMapCore {
    int32_t* hdr;                 // KFMAP_H_*
    uint8_t *kf_alive, *kf_local;
    int32_t* graph;               // [kf_cap][kf_cap]
    int32_t *tile, *seen0, *seen1, *pend, *first_row, *pair_n0, *pair_slot;
    int kf_cap, obs_cap;
    int n_kf;                     // keyframes when the call starts
};
// one observe call: kf0 >= 0 the keyframe-pair stage (pairs = kf0 row, kf1 row), kf0 < 0 the local-map
// stage (pairs = row of sel_ids, row of unm_rows).  epoch: the object's call number (> 0)
struct KfMapObserve {
    int kind, kf0, kf1, n, n_sel, n_unm, epoch;
    const int32_t *pairs, *sel_ids, *unm_rows;
    int32_t* lm_out;
};
// one ordered compaction over n items into out, its count into hdr[slot]
enum { KFMAP_SEL_LOCAL = 0, KFMAP_SEL_LOCAL_UNSEEN, KFMAP_SEL_ALIVE, KFMAP_SEL_UNMATCHED, KFMAP_SEL_BAD };
struct KfMapSelect {
    int mode, kf, n, slot;        // kf: kf1 of LOCAL_UNSEEN, the keyframe of UNMATCHED
    int min_lm_obs, cull_age;     // BAD
    int32_t* out;
};
hipError_t enqueue_kfmap_add_keyframe(const KfMapCore& c, const KfMapLm& pt, const KfMapLm& ls, int n_pt, int n_ls, hipStream_t s);
hipError_t enqueue_kfmap_observe(const KfMapCore& c, const KfMapLm& L, const KfMapObserve& a, hipStream_t s);
hipError_t enqueue_kfmap_form_local_map(const KfMapCore& c, const KfMapLm& pt, const KfMapLm& ls, int min_lm_cov_graph,
                                        int min_kf_local_map, hipStream_t s);
hipError_t enqueue_kfmap_select(const KfMapCore& c, const KfMapLm& L, const KfMapSelect& a, hipStream_t s);
// the compaction of the landmarks to remove (a.mode = KFMAP_SEL_BAD), then their removal
hipError_t enqueue_kfmap_remove_bad(const KfMapCore& c, const KfMapLm& L, const KfMapSelect& a, hipStream_t s);
hipError_t enqueue_kfmap_set_inlier(const KfMapCore& c, const KfMapLm& L, const int32_t* ids, int n, int value, hipStream_t s);
hipError_t enqueue_kfmap_erase_keyframe(const KfMapCore& c, int kf, hipStream_t s);

// the map's geometry half (k_mapgeo.hip); all pointers device.  The arrays are MapGeoMem's: MapGeoLm one
// kind's state, MapGeoCore the keyframes, the header and the observe calls' workspace.
struct MapGeoLm {
    double *lm3d, *obs, *sigma;   // [cap][lw], [cap][obs_cap][ow], [cap][obs_cap]
    int32_t* nobs;
    int lw, ow, cap;
};
struct MapGeoCore {
    int32_t* hdr;                 // MAPGEO_H_*
    double *T_kf, *x_kf;
    int32_t *pend, *pair_n0;
    int kf_cap, obs_cap;
};
// one observe call: kf0 >= 0 the keyframe-pair stage, kf0 < 0 the local-map stage (pairs' column 1 is a
// row of unm_rows).  g0 / g1: the 3D geometry of kf0's rows (P, or sP and eP) and the observation of
// either keyframe's rows (pl or le); n0 / n1 the views' rows.
struct MapGeoObserve {
    int kf0, n, n_unm, first_new, n0, n1;
    const int32_t *pairs, *unm_rows, *lm_out;
    const double *P0, *Q0, *o0, *o1;
};
// one assembly.  The kfmap's arrays are read only.  which: GFPL_KFMAP_LOCAL or GFPL_KFMAP_ALIVE
struct MapGeoAsm {
    int which, n_kf, next[2];
    const uint8_t *kf_alive, *kf_local;
    const uint8_t *lm_alive[2], *lm_local[2];
    const int32_t *k_nobs[2], *k_obs[2];   // the kfmap's n_obs and kf_obs [cap][obs_cap]
    int32_t *kf_slot, *kf_mark, *kf_list, *fix_list;
    int32_t *lm_cnt[2], *tile_lm[2], *tile_obs[2], *lm_list[2], *lm_off[2];
    double *a_x_kf, *a_T_kf, *a_T_fix, *a_lm3d[2], *a_obs[2], *a_sigma[2];
    int32_t *a_obs_lm[2], *a_obs_kf[2];
};
hipError_t enqueue_mapgeo_observe(const MapGeoCore& c, const MapGeoLm& L, const MapGeoObserve& a, hipStream_t s);
hipError_t enqueue_mapgeo_free(const MapGeoCore& c, const MapGeoLm& L, const int32_t* ids, int n, hipStream_t s);
hipError_t enqueue_mapgeo_assemble(const MapGeoCore& c, const MapGeoLm& pt, const MapGeoLm& ls, const MapGeoAsm& a, hipStream_t s);
// an assembled problem's index arrays over the LBA's unified numbering (LbaMem: lm_start, obs_lm, obs_kf)
hipError_t enqueue_mapgeo_lba_index(const MapGeoAsm& a, const gfpl_lba_counts& n, int32_t* lm_start, int32_t* obs_lm, int32_t* obs_kf,
                                    hipStream_t s);
// :1688-1712: the solved poses and landmarks of an assembled problem back into the store
hipError_t enqueue_mapgeo_write_back(const MapGeoCore& c, const MapGeoLm& pt, const MapGeoLm& ls, const MapGeoAsm& a,
                                     const gfpl_lba_counts& n, hipStream_t s);

}  // namespace gfpl

namespace gfpl {
// levels 1.. of packed pyramids (the camera's geometry) from their level 0, as ComputePyramid
// resizes them (k_orb.hip: the ORB extractor's O1 tables and k_orb_resize)
struct PyrBuild;
int pyrbuild_create(const gfpl_camera* cam, PyrBuild** out);
hipError_t pyrbuild_run(PyrBuild* pb, uint8_t* pyr, long long stride, int n, hipStream_t s);
void pyrbuild_destroy(PyrBuild* pb);
}  // namespace gfpl

// context accessors for the other extern "C" objects built on a context (gfpl_abi.hip)
int gfpl_ctx_device(const gfpl_ctx* c);
void* gfpl_ctx_stream(const gfpl_ctx* c);
const gfpl_camera* gfpl_ctx_camera(const gfpl_ctx* c);   // NULL before gfpl_set_camera
const gfpl_config* gfpl_ctx_config(const gfpl_ctx* c);
// a detector created on the context counts itself in until it is destroyed (gfpl_destroy refuses meanwhile)
void gfpl_ctx_attach(gfpl_ctx* c);
void gfpl_ctx_detach(gfpl_ctx* c);
// how often the event was recorded (gfpl_event_record, or as a tracker call's gfpl_frames.consumed)
int64_t gfpl_event_records(const gfpl_event* e);
// the rectifier (k_rectify.hip) for the detector: its image size, and one launch on the given
// stream: both sides when src_r / dst_r are given, else `side` alone
int gfpl_rectifier_width(const gfpl_rectifier* r);
int gfpl_rectifier_height(const gfpl_rectifier* r);
int gfpl_rectifier_enqueue(gfpl_rectifier* r, void* stream, int side, const uint8_t* src_l, const uint8_t* src_r,
                           int n, uint8_t* dst_l, uint8_t* dst_r);

namespace gfpl {
// Deferred error status of the stream-ordered detector calls (gfpl_*_async): the kernels
// OR error bits into a device word; each call ends with a copy of it into pinned host
// memory and an event, so the call returns without synchronising; *_status waits for
// the event, reports the bits of every call since the previous status and clears them.
struct AsyncStatus {
    int* dev = nullptr;
    int* host = nullptr;
    hipEvent_t ev = nullptr;
    bool pending = false;
    hipError_t init(int* dev_word, hipStream_t s) {
        dev = dev_word;
        hipError_t e = hipHostMalloc((void**)&host, sizeof(int), hipHostMallocDefault);
        if (e == hipSuccess) { *host = 0; e = hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
        if (e == hipSuccess) e = hipMemsetAsync(dev, 0, sizeof(int), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e;
    }
    hipError_t enqueue(hipStream_t s) {
        hipError_t e = hipMemcpyAsync(host, dev, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(ev, s);
        if (e == hipSuccess) pending = true;
        return e;
    }
    // bits of the calls since the last wait (0 when none is pending)
    hipError_t wait(hipStream_t s, int* bits) {
        *bits = 0;
        if (!pending) return hipSuccess;
        hipError_t e = hipEventSynchronize(ev);
        if (e != hipSuccess) return e;
        *bits = *host;
        pending = false;
        if (*bits) {
            *host = 0;
            e = hipMemsetAsync(dev, 0, sizeof(int), s);   // ordered before the next call's kernels
        }
        return e;
    }
    void destroy() {
        if (host) (void)hipHostFree(host);
        if (ev) (void)hipEventDestroy(ev);
        host = nullptr;
        ev = nullptr;
    }
};
}  // namespace gfpl
