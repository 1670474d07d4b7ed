/*
 * gfpl.h — C ABI of the MI355X-native GF-PL-SLAM tracking hot path.
 *
 * The reference has no FFI: its hot path is the C++ member functions of
 * StVO::StereoFrame / StVO::StereoFrameHandler (include/stereoFrame.h:89-260,
 * include/stereoFrameHandler.h:38-174 of SimonsRoad/gf-pl-slam).  Each entry
 * point below names the reference method it replaces; INTEGRATION.md shows the
 * one-line call a maintainer puts into that method body.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++ / torch types.
 *  - Every function returns int: 0 = GFPL_OK, negative = GFPL_E_*.
 *  - A gfpl_ctx is bound to one HIP device and is not re-entrant; one context
 *    per host thread.  Work is enqueued on the stream passed to gfpl_create
 *    (hipStream_t as void*, NULL = default stream) and is asynchronous unless
 *    the function says it synchronises.
 *  - A gfpl_seqbatch holds B independent stereo sequences (one StereoFrameHandler
 *    each) resident in HBM: prev/curr frame state, matched lists and pose.
 *  - Input frames (gfpl_frames) are DEVICE pointers laid out [B][cap] per
 *    sequence (counts per sequence in n_*).  The right image pyramid is packed
 *    per sequence as consecutive levels of gfpl_camera.lvl_rows x lvl_cols bytes.
 *  - Matrices are row-major double.
 */
#ifndef GFPL_H
#define GFPL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFPL_ABI_VERSION 6   /* 6: STEP_REC 24 (gfpl_debug_step_records writes B x 24 int64), cut_proof 0-3 */

#define GFPL_DESC_BYTES 32          /* ORB rBRIEF / binarised LBD: 256 bit        */
#define GFPL_MAX_LEVELS 8           /* ORB pyramid levels supported              */
#define GFPL_MAX_IMAGE_DIM 2047     /* pyramid level width / height limit        */
#define GFPL_MAX_MATCHED_PT 2048    /* capacity of matched_pt (cap from config)   */
#define GFPL_MAX_MATCHED_LS 1024    /* capacity of matched_ls (cap from config)   */
#define GFPL_PYR_TAIL 64            /* slack after each packed pyramid (bytes)    */

/* error codes */
#define GFPL_OK                   0
#define GFPL_E_INVALID          (-1)   /* bad argument / NULL pointer            */
#define GFPL_E_HIP              (-2)   /* HIP runtime error                     */
#define GFPL_E_NO_DEVICE        (-3)   /* no HIP device / extension not built   */
#define GFPL_E_TOO_FEW_TRAIN    (-4)   /* knn-2 with < 2 train rows (ref UB, U4) */
#define GFPL_E_CAPACITY         (-5)   /* counts exceed the seqbatch capacity    */
#define GFPL_E_STATE            (-6)   /* call order violated (e.g. insert before initialize) */
#define GFPL_E_UNSUPPORTED      (-7)   /* config flag combination not on the path */
#define GFPL_E_NOMEM            (-8)   /* device memory allocation failed        */

/* which frame of a sequence */
#define GFPL_PREV 0
#define GFPL_CURR 1

/* Hamming cell size: 1 = cv::NORM_HAMMING, 2 = cv::NORM_HAMMING2 */
#define GFPL_HAMMING  1
#define GFPL_HAMMING2 2

/* ------------------------------------------------------------------------ */
/* Camera: PinholeStereoCamera (include/pinholeStereoCamera.h:37-103) plus the
 * ORB scale tables of ORBextractor (src/ORBextractor.cc:410-431) and the
 * right-pyramid geometry of ORBextractor::ComputePyramid (:1107-1132).     */
typedef struct gfpl_camera {
    int    width, height;
    double fx, fy, cx, cy, b;
    int    n_levels;                          /* Config::orbNLevels            */
    float  scale[GFPL_MAX_LEVELS];            /* mvScaleFactors                */
    float  inv_scale[GFPL_MAX_LEVELS];        /* mvInvScaleFactors             */
    int    lvl_cols[GFPL_MAX_LEVELS];         /* cvRound(W * inv_scale)        */
    int    lvl_rows[GFPL_MAX_LEVELS];         /* cvRound(H * inv_scale)        */
    int64_t lvl_offset[GFPL_MAX_LEVELS];      /* byte offset of level in packed pyramid */
    int64_t pyr_bytes;                        /* bytes of one packed pyramid: sum of the
                                                 levels + >= GFPL_PYR_TAIL, a multiple of 4
                                                 (gfpl_camera_init: of 256)               */
    double sigma2_pt[GFPL_MAX_LEVELS];        /* PointFeature::sigma2 per level (src/stereoFeatures.cpp:41-47) */
    double sigma2_ln[GFPL_MAX_LEVELS];        /* LineFeature::sigma2 per level  (src/stereoFeatures.cpp:96-101) */
} gfpl_camera;

/* Config values used by the path (src/config.cpp:77-153).  Mutable like the
 * reference's Config::xxx() accessors: fill with gfpl_config_default() and
 * override fields before gfpl_set_config.                                  */
typedef struct gfpl_config {
    int    best_lr_matches;      /* :81  true  (only true is implemented)      */
    int    lr_in_parallel;       /* :79  true  (radius branch of cross points) */
    int    use_line_conf_cut;    /* :83  true                                   */
    int    cut_with_max_vol;     /* :86  true: the line cut's metric is logdet(invCov_sum);
                                    0: getMinEigenValue(invCov_sum) (k_cut_search_eig, DESIGN.md §3
                                    N5): every step exact, cut_certify / cut_proof are ignored   */
    double ratio_disp_std;       /* :84  0.15                                   */
    double ratio_disp_std_hor;   /* :85  0.9                                    */
    int    max_line_match_num;   /* :94  300                                    */
    int    max_point_match_num;  /* :95  500                                    */
    double max_dist_epip;        /* :101 2.0                                    */
    double min_disp;             /* :102 1.0                                    */
    double max_ratio_12_p;       /* :103 0.9                                    */
    double point_match_radius;   /* :104 50.0                                   */
    double stereo_overlap_th;    /* :106 0.5                                    */
    double line_horiz_th;        /* :108 0.1                                    */
    double desc_th_l;            /* :109 0.1                                    */
    double line_cov_th;          /* :110 10.0                                   */
    double homog_th;             /* :121 1e-7                                   */
    int    min_features;         /* :122 10                                     */
    int    max_iters;            /* :124 5                                      */
    int    max_iters_ref;        /* :125 10                                     */
    double min_error;            /* :126 1e-7                                   */
    double min_error_change;     /* :127 1e-7                                   */
    double inlier_k;             /* :128 2.0                                    */
    double motion_step_th;       /* :129 10                                     */
    double orb_scale_factor;     /* :135 1.2                                    */
    int    orb_n_levels;         /* :136 4                                      */
    double lsd_scale;            /* :145 1                                      */
    double cut_step;             /* stepCutRatio 0.05 (src/stereoFrameHandler.cpp:135) */
    double cut_rng[2];           /* rngCutRatio {0,1} (src/stereoFrameHandler.cpp:134)  */
    double proj_gate_px;         /* rng_included 10.0 (src/stereoFrameHandler.cpp:534)  */
    double min_entropy_ratio;    /* :34  0.90  (needNewKF)                      */
    int    max_kf_num_frames;    /* :35  50    (needNewKF)                      */
    double cut_certify;          /* (new) 1e-9: relative margin of the certified line-cut
                                    search; 0 = every neighbour evaluated with
                                    the reference's LLT; nonzero values below 1e-10 are rejected */
    int    cut_proof;            /* (new) what ties a margined line-cut decision to the
                                    reference's own logdet:
                                    0 measured: the comparison operands' measured agreement
                                      with the reference's (not a proof);
                                    1 proven after the fact: the measured search records its
                                      decisions, k_cut_verify proves them with the per-step
                                      agreement bound; a sequence not proven is redone by the
                                      eager-proven search;
                                    2 eager-proven: every step of the search carries the bound;
                                    3 (test hook) as 1, but every sequence is redone eagerly.
                                    A step no bound covers takes the reference's evaluation. */
} gfpl_config;

/* cv::KeyPoint subset used by the path */
typedef struct gfpl_keypoint { float x, y; int octave; } gfpl_keypoint;
/* ORB_SLAM2::ORBextractor parameters (src/ORBextractor.cc:410-470), as the path builds it
 * (src/stereoFrame.cpp:33-36): Config::orbNFeatures, orbScaleFactor, orbNLevels, 20, 7 */
typedef struct gfpl_orb_params {
    int   nfeatures;      /* Config::orbNFeatures (src/config.cpp:134; 2000 in BASELINE cfg 2) */
    float scale_factor;   /* Config::orbScaleFactor 1.2 */
    int   nlevels;        /* Config::orbNLevels 4 */
    int   ini_th_fast;    /* iniThFAST 20 */
    int   min_th_fast;    /* minThFAST 7 */
} gfpl_orb_params;
/* line_descriptor::KeyLine subset (3rdparty/line_descriptor/include/line_descriptor/descriptor_custom.hpp:105-170) */
typedef struct gfpl_keyline { float sx, sy, ex, ey, angle; int octave; } gfpl_keyline;

typedef struct gfpl_event gfpl_event;   /* stream-ordering event (gfpl_event_*) */

/* One batch of input stereo frames (detections already done — detection is out
 * of scope).  All pointers are DEVICE pointers.     */
typedef struct gfpl_frames {
    int batch;                         /* B                                   */
    int kp_cap, kl_cap;                /* row capacity per sequence           */
    const int*           n_kp_l;       /* [B]  points_l.size()                */
    const int*           n_kp_r;       /* [B]  points_r.size()                */
    const gfpl_keypoint* kp_l;         /* [B*kp_cap]                          */
    const gfpl_keypoint* kp_r;         /* [B*kp_cap]                          */
    const uint8_t*       pdesc_l;      /* [B*kp_cap*32]                       */
    const uint8_t*       pdesc_r;      /* [B*kp_cap*32]                       */
    const int*           n_kl_l;       /* [B]  lines_l.size()                 */
    const int*           n_kl_r;       /* [B]                                 */
    const gfpl_keyline*  kl_l;         /* [B*kl_cap]                          */
    const gfpl_keyline*  kl_r;         /* [B*kl_cap]                          */
    const uint8_t*       ldesc_l;      /* [B*kl_cap*32]                       */
    const uint8_t*       ldesc_r;      /* [B*kl_cap*32]                       */
    const uint8_t*       pyr_r;        /* [B*cam.pyr_bytes] right ORB pyramid (4-byte aligned) */
    const double*        time_stamp;   /* [B]                                 */
    /* optional stream ordering with a producer on another context (e.g. the detectors):
     * a tracker call that reads these frames makes its stream wait for `ready` first and
     * records `consumed` once its reads are enqueued.  NULL (zero-initialised): none.   */
    gfpl_event*          ready;
    gfpl_event*          consumed;
} gfpl_frames;

/* Host view of one frame's state (StereoFrame public members the path
 * produces, include/stereoFrame.h:205-259; feature records
 * include/stereoFeatures.h:36-124).  Arrays are caller-allocated with the
 * capacity given to the seqbatch (points: kp_cap, lines: kl_cap).  The CPU
 * oracle fills the same struct, so parity tests compare field by field.   */
typedef struct gfpl_frame_host {
    int n_pt, n_ls;
    /* stereo_pt */
    double*  pt_pl;        /* [cap*2]  pl                    */
    double*  pt_pl_obs;    /* [cap*2]  pl_obs                */
    double*  pt_disp;      /* [cap]                          */
    double*  pt_P;         /* [cap*3]                        */
    double*  pt_sigma2;    /* [cap]                          */
    int32_t* pt_idx;       /* [cap]                          */
    int32_t* pt_level;     /* [cap]                          */
    uint8_t* pt_inlier;    /* [cap]                          */
    uint8_t* pdesc;        /* [cap*32]  pdesc_l (reordered)  */
    /* stereo_ls */
    double*  ls_spl;       /* [cap*2] */
    double*  ls_epl;       /* [cap*2] */
    double*  ls_spl_obs;   /* [cap*2] */
    double*  ls_epl_obs;   /* [cap*2] */
    double*  ls_sdisp;     /* [cap]   */
    double*  ls_edisp;     /* [cap]   */
    double*  ls_sdisp_obs; /* [cap]   */
    double*  ls_edisp_obs; /* [cap]   */
    double*  ls_angle;     /* [cap]   */
    double*  ls_sigma2;    /* [cap]   */
    double*  ls_sP;        /* [cap*3] */
    double*  ls_eP;        /* [cap*3] */
    double*  ls_le;        /* [cap*3] */
    double*  ls_le_obs;    /* [cap*3] */
    double*  ls_covS;      /* [cap*9] covSpt3D */
    double*  ls_covE;      /* [cap*9] covEpt3D */
    double*  ls_cut;       /* [cap*2] cutRatio */
    double*  ls_invcov;    /* [cap*36] invCovPose */
    int32_t* ls_idx;       /* [cap] */
    int32_t* ls_level;     /* [cap] */
    uint8_t* ls_inlier;    /* [cap] */
    uint8_t* ldesc;        /* [cap*32] ldesc_l (reordered) */
    /* pose */
    double Tfw[16], DT[16], DT_cov[36], Tfw_cov[36], DT_cov_eig[6];
    double err_norm, time_stamp;
} gfpl_frame_host;

/* StereoFrameHandler tracking results of the last step
 * (include/stereoFrameHandler.h:120-161). matched_* hold indices into
 * prev_frame->stereo_pt / stereo_ls in list order (duplicates allowed for
 * points).                                                */
typedef struct gfpl_track_host {
    int n_matched_pt;
    int n_matched_ls;
    int32_t matched_pt[GFPL_MAX_MATCHED_PT];
    int32_t matched_ls[GFPL_MAX_MATCHED_LS];
    int n_inliers, n_inliers_pt, n_inliers_ls;
    int num_frame_loss;
} gfpl_track_host;

/* Keyframe-decision state of one StereoFrameHandler (include/stereoFrameHandler.h:147-153). */
typedef struct gfpl_kf_state {
    double T_prevKF[16];          /* row-major                                   */
    double cov_prevKF_currF[36];
    double entropy_first_prevKF;
    double entropy_ratio;         /* of the last gfpl_need_new_kf               */
    int    prev_f_iskf;
    int    num_frame_since_kf;    /* numFrameSinceKeyframe                       */
    int    need_new_kf;           /* decision of the last gfpl_need_new_kf       */
} gfpl_kf_state;

typedef struct gfpl_ctx gfpl_ctx;
typedef struct gfpl_seqbatch gfpl_seqbatch;

/* ---------------------------------------------------------------- setup -- */
int  gfpl_abi_version(void);
/* Config::Config() defaults (src/config.cpp:26-154). */
int  gfpl_config_default(gfpl_config* cfg);
/* Fill the derived tables of a camera (scale tables, pyramid geometry,
 * sigma2 tables) from the intrinsics, image size and ORB pyramid params.   */
int  gfpl_camera_init(gfpl_camera* cam, int width, int height, double fx, double fy,
                      double cx, double cy, double b, const gfpl_config* cfg);

/* context: device + stream + camera + config (replaces the Config singleton
 * src/config.cpp:158-162 and the PinholeStereoCamera* each frame holds).   */
int  gfpl_create(int device, void* hip_stream, gfpl_ctx** out);
/* A context on its own non-blocking stream (created here, destroyed with the context):
 * for a caller without a HIP runtime that wants, e.g., detection and tracking on two
 * contexts ordered by gfpl_event_* instead of one serial stream.                      */
int  gfpl_create_async(int device, gfpl_ctx** out);
/* the hipStream_t (as void*) the context enqueues on */
void* gfpl_get_stream(const gfpl_ctx* ctx);

/* Stream-ordering events between contexts (all asynchronous but synchronize):
 * record on a context's stream, make another context's stream wait for it.           */
int  gfpl_event_create(gfpl_ctx* ctx, gfpl_event** out);
int  gfpl_event_destroy(gfpl_event* ev);
int  gfpl_event_record(gfpl_event* ev, gfpl_ctx* ctx);
int  gfpl_event_wait(gfpl_ctx* ctx, gfpl_event* ev);
int  gfpl_event_synchronize(gfpl_event* ev);
/* how often the event was recorded so far (gfpl_event_record, or by a tracker call as a
 * gfpl_frames.consumed event): a producer reusing buffers checks its views were read.  */
int  gfpl_event_record_count(const gfpl_event* ev, int64_t* count);
/* GFPL_E_STATE while seqbatches or ORB / LBD / LSD objects created on the context
 * are still alive (they use its stream; ORB also reads its camera).           */
int  gfpl_destroy(gfpl_ctx* ctx);
/* GFPL_E_STATE while seqbatches or detector objects of the context live (their pyramid
 * builders and ORB / LSD geometry are laid out for the camera they were created on).
 * GFPL_E_INVALID for bad level tables.                                                 */
int  gfpl_set_camera(gfpl_ctx* ctx, const gfpl_camera* cam);
/* max_point_match_num / max_line_match_num size the matched lists and the cut /
 * pose scratch of a seqbatch when it is created; while any seqbatch of the
 * context lives, a config with a larger budget than its capacity is refused with
 * GFPL_E_CAPACITY (lower budgets are accepted).  Other fields (e.g. cut_proof) may
 * change between steps: each step reads the config current at its launch.     */
int  gfpl_set_config(gfpl_ctx* ctx, const gfpl_config* cfg);
int  gfpl_get_camera(const gfpl_ctx* ctx, gfpl_camera* cam);
int  gfpl_get_config(const gfpl_ctx* ctx, gfpl_config* cfg);
int  gfpl_synchronize(gfpl_ctx* ctx);
/* Copy `bytes` of DEVICE memory (e.g. a field of a gfpl_frames view) to HOST memory after the
 * context's stream drained, for FFI callers without a HIP runtime of their own.  Synchronises. */
int  gfpl_copy_to_host(gfpl_ctx* ctx, void* host_dst, const void* device_src, size_t bytes);

/* B independent sequences (B StereoFrameHandler objects) resident in HBM.
 * kp_cap <= 8192 keypoints and kl_cap <= 2048 keylines per side (config 5:
 * 8000 ORB + 2000 LBD); larger values return GFPL_E_INVALID.               */
int  gfpl_seqbatch_create(gfpl_ctx* ctx, int batch, int kp_cap, int kl_cap, gfpl_seqbatch** out);
int  gfpl_seqbatch_destroy(gfpl_seqbatch* sb);
/* bytes of device memory held by the seqbatch (state + workspace) */
int64_t gfpl_seqbatch_bytes(const gfpl_seqbatch* sb);

/* -------------------------------------------------- tracker entry points -- */
/* StereoFrameHandler::initialize (src/stereoFrameHandler.cpp:45-81) with the
 * detections injected: StereoFrame::extractInitialStereoFeatures matching part
 * (src/stereoFrame.cpp:173-336); Tfw = Tfw_cov = DT = I.                      */
int  gfpl_initialize(gfpl_seqbatch* sb, const gfpl_frames* in);
/* StereoFrameHandler::insertStereoPair (src/stereoFrameHandler.cpp:83-151):
 * stereo matching of the new frame, predictFramePose, prev-frame line
 * uncertainty, crossFrameMatching_Hybrid, estimateProjUncertainty_submodular. */
int  gfpl_insert_stereo_pair(gfpl_seqbatch* sb, const gfpl_frames* in);
/* StereoFrameHandler::optimizePose(prev_frame->DT) (src/stereoFrameHandler.cpp:1939-2030,
 * called as at app/plslam_mod.cpp:408).                                       */
int  gfpl_optimize_pose(gfpl_seqbatch* sb);
/* StereoFrameHandler::optimizePose(Matrix4d DT_ini) with an explicit initial guess per
 * sequence: dt_ini = HOST array [B*16] row-major (NULL = prev_frame->DT).  Synchronises. */
int  gfpl_optimize_pose_ini(gfpl_seqbatch* sb, const double* dt_ini);
/* Copy one batch of HOST input frames (host->* are host pointers, same layout)
 * into staging buffer 0 of the seqbatch and return its device view in *dev
 * (valid until the next upload into that buffer).  Synchronous; for FFI callers
 * without a HIP runtime of their own.  The rate through this path includes PCIe. */
int  gfpl_upload_frames(gfpl_seqbatch* sb, const gfpl_frames* host, gfpl_frames* dev);
/* Stream-ordered upload, no host synchronisation: copy the host->batch sequences of
 * a HOST input batch (pinned memory for an asynchronous DMA) into sequences
 * [s0, s0 + host->batch) of staging buffer `slot` (0 or 1; each holds one input
 * frame of all B sequences, allocated on first use) on the seqbatch's own copy
 * stream.  The copy waits for the last tracker call that read the slot, and every
 * tracker call that reads the slot (gfpl_staged_frames view) waits for the copies
 * enqueued before it — so uploading frame k+1 into one slot overlaps the step on
 * frame k in the other.  *ticket (nullable) names the copy for gfpl_upload_wait;
 * the host memory must stay unchanged until then.                              */
int  gfpl_upload_frames_async(gfpl_seqbatch* sb, const gfpl_frames* host, int s0, int slot, int64_t* ticket);
/* The same with only level 0 of each right pyramid on the host: host->pyr_r holds the
 * level-0 images (lvl_cols[0] x lvl_rows[0] bytes) of the host->batch sequences, l0_stride
 * bytes apart; after the copy the device builds levels 1.. of the staged pyramids as
 * ORBextractor::ComputePyramid does (cv::resize INTER_LINEAR of the level above,
 * src/ORBextractor.cc:1107-1132; the ORB extractor's k_orb_resize), on the copy stream —
 * about half the bytes over PCIe at VGA.                                                   */
int  gfpl_upload_frames_l0_async(gfpl_seqbatch* sb, const gfpl_frames* host, int s0, int slot,
                                 int64_t l0_stride, int64_t* ticket);
/* Block the host until the copy `ticket` (and every copy enqueued before it) is done. */
int  gfpl_upload_wait(gfpl_seqbatch* sb, int64_t ticket);
/* Device view (all B sequences) of staging buffer `slot` (GFPL_E_INVALID before its first upload). */
int  gfpl_staged_frames(gfpl_seqbatch* sb, int slot, gfpl_frames* dev);
/* StereoFrameHandler::updateFrame_ECCV18 state swap (src/stereoFrameHandler.cpp:864-922):
 * prev <- curr, matched lists cleared.  (FAST-threshold adaptation is out of scope;
 * the T_base trajectory log lives in the host mirror, gf-pl-slam_amd/host/stvo.h.) */
int  gfpl_update_frame(gfpl_seqbatch* sb);
/* StereoFrameHandler::needNewKF (src/stereoFrameHandler.cpp:2309-2349) for every
 * sequence on its curr frame (after optimize_pose, as app/plslam_mod.cpp:436):
 * entropy of the covariance accumulated since the last keyframe vs the first one.
 * flags: HOST [B] (synchronises) or NULL; 1 = new keyframe needed.  The decision
 * and the ratio are kept in the sequence's gfpl_kf_state either way.          */
int  gfpl_need_new_kf(gfpl_seqbatch* sb, int32_t* flags);
/* StereoFrameHandler::currFrameIsKF (src/stereoFrameHandler.cpp:2351-2379) for the
 * sequences whose mask entry is nonzero (HOST [B], synchronises; NULL = the last
 * gfpl_need_new_kf decisions, asynchronous): numFrameSinceKeyframe = 0, curr idx
 * renumbered, curr Tfw = Tfw_cov = I, T_prevKF = I, cov_prevKF_currF = 0.     */
int  gfpl_curr_frame_is_kf(gfpl_seqbatch* sb, const int32_t* mask);
int  gfpl_read_kf_state(gfpl_seqbatch* sb, int seq, gfpl_kf_state* out);
/* insert_stereo_pair + optimize_pose + update_frame, one batched step.       */
int  gfpl_frame_step(gfpl_seqbatch* sb, const gfpl_frames* in);

/* ------------------------------------------------------- stage entry points */
/* StereoFrame::extractStereoFeatures_ORBSLAM point branch (src/stereoFrame.cpp:453-630)
 * incl. subPixelStereoRefine_ORBSLAM (:340-404) -> curr stereo_pt, pdesc_l.   */
int  gfpl_stereo_points(gfpl_seqbatch* sb, const gfpl_frames* in);
/* ... line branch (src/stereoFrame.cpp:633-767) -> curr stereo_ls, ldesc_l,
 * plus the covariances estimateStereoUncertainty (:1448-1484) will need.      */
int  gfpl_stereo_lines(gfpl_seqbatch* sb, const gfpl_frames* in);
/* StereoFrame::estimateStereoUncertainty on the PREV frame (src/stereoFrame.cpp:1448-1484). */
int  gfpl_line_uncertainty(gfpl_seqbatch* sb);
/* predictFramePose + crossFrameMatching_Hybrid points (src/stereoFrameHandler.cpp:153-157,451-603) */
int  gfpl_cross_points(gfpl_seqbatch* sb);
/* crossFrameMatching_Hybrid lines (src/stereoFrameHandler.cpp:605-695)       */
int  gfpl_cross_lines(gfpl_seqbatch* sb);
/* estimateProjUncertainty_submodular(0.05,{0,1}) (src/stereoFrameHandler.cpp:1618-1764) */
int  gfpl_line_cut(gfpl_seqbatch* sb);

/* cv::BFMatcher::knnMatch(k=2) with NORM_HAMMING / NORM_HAMMING2 on device
 * buffers (call sites src/stereoFrame.cpp:183-197,256-272,636-656;
 * src/stereoFrameHandler.cpp:617-633).  q: nq x 32 B, t: nt x 32 B (device).
 * out_idx[2*nq], out_dist[2*nq] (device; distance as float like cv::DMatch).
 * Returns GFPL_E_TOO_FEW_TRAIN when nt < 2 (reference UB).        */
int  gfpl_knn2_hamming(gfpl_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                       int cell, int32_t* out_idx, float* out_dist);
/* The same on HOST buffers (copied in and out; synchronous): StereoFrame::matchPointFeatures /
 * matchLineFeatures (src/stereoFrame.cpp:1229-1241), which MapHandler calls from two std::async
 * tasks (src/mapHandler.cpp:223-226,355-356,558-559,686-687).  Thread-safe per context.      */
int  gfpl_knn2_hamming_host(gfpl_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                            int cell, int32_t* out_idx, float* out_dist);
/* cv::BFMatcher::radiusMatch with NORM_HAMMING (cell 1) / NORM_HAMMING2 (cell 2):
 * StereoFrame::matchPointFeatures_radius / matchLineFeatures_radius (src/stereoFrame.cpp:
 * 1243-1257).  Row i holds every train row j with distance <= max_dist (ledger T1), sorted by
 * distance, equal distances in train order (T2); rows are ragged: row i is
 * [row_off[i], row_off[i+1]) of out_idx / out_dist (row_off has nq + 1 entries, always
 * filled).  When row_off[nq] > cap nothing else is written and GFPL_E_CAPACITY is returned
 * (call again with cap >= row_off[nq]).  _host: HOST buffers, synchronous; the device form
 * takes DEVICE q / t / row_off / out_* and returns after the rows are written.              */
int  gfpl_radius_hamming(gfpl_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int cell,
                         float max_dist, int32_t* row_off, int cap, int32_t* out_idx, float* out_dist);
int  gfpl_radius_hamming_host(gfpl_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int cell,
                              float max_dist, int32_t* row_off, int cap, int32_t* out_idx, float* out_dist);
/* Statistics of a knn-2 match list, HOST d0[n] / d1[n] = the best / second distances of each
 * row (vector<vector<DMatch>> rows [0] / [1]): kind 0 pointDescriptorMAD + pointDescriptor-
 * BudgetThres, kind 1 lineDescriptorMAD + lineDescriptorBudgetThres (src/stereoFrame.cpp:
 * 1259-1341).  out[0] nn_mad, out[1] nn12_mad, out[2] thres_budget for max_num (the
 * Config::max*MatchNum the reference reads).  nn_dist_median is the reference's
 * uninitialised value pinned to 0.0 (ledger U1); NaN ratios order above +inf (U12).
 * GFPL_E_INVALID for n < 1 or max_num < 1 (the reference indexes element -1).  Synchronous.   */
int  gfpl_match_stats_host(gfpl_ctx* ctx, int kind, const float* d0, const float* d1, int n, int max_num,
                           double* out);

/* --------------------------------------------- ORB extraction (§8(f)1) ---- */
/* ORB_SLAM2::ORBextractor (src/ORBextractor.cc:410-470 constructor, :1043-1105
 * operator()) as StereoFrame builds it (src/stereoFrame.cpp:33-36), over a batch of
 * grey images on the device.  The extractor owns its workspace for images of
 * width x height (64..2047 px) and up to max_images per call; kp_cap bounds the
 * keypoints returned per image.  Arithmetic of the OpenCV calls pinned as the CPU
 * oracle's ledger O1-O7.                                          */
typedef struct gfpl_orb gfpl_orb;
int  gfpl_orb_create(gfpl_ctx* ctx, int width, int height, const gfpl_orb_params* prm,
                     int max_images, int kp_cap, gfpl_orb** out);
int  gfpl_orb_destroy(gfpl_orb* orb);
/* bytes of one image's packed level images (the gfpl_frames.pyr_r layout) */
int  gfpl_orb_pyramid_bytes(const gfpl_orb* orb, int64_t* bytes);
/* operator()(image, noArray(), keypoints, descriptors) for n images, all pointers
 * DEVICE: images [n][height][width] u8; per image i, rows [i*kp_cap, +n_kp[i]) of
 * kps / desc (32 B) / angle (degrees) / response (FAST score) hold the keypoints
 * in the reference's order (level by level, DistributeOctTree node order),
 * coordinates scaled to level 0.  angle, response, pyramid may be NULL; pyramid
 * receives each image's level images at pyr_stride bytes apart.  When the context has
 * a camera of this image size and pyr_stride is its pyr_bytes (the tracker's
 * gfpl_frames.pyr_r), the extractor's level geometry must be the camera's
 * (GFPL_E_INVALID otherwise).  Synchronises; GFPL_E_CAPACITY when an internal or
 * kp_cap capacity was exceeded.                                                */
int  gfpl_orb_extract(gfpl_orb* orb, const uint8_t* images, int n, gfpl_keypoint* kps,
                      uint8_t* desc, int* n_kp, float* angle, float* response,
                      uint8_t* pyramid, int64_t pyr_stride);
/* The same, stream-ordered: returns after enqueueing on the context's stream (argument
 * errors are still returned at once); the capacity status of every async call since the
 * last status is returned by gfpl_orb_status (which waits for the last of them).      */
int  gfpl_orb_extract_async(gfpl_orb* orb, const uint8_t* images, int n, gfpl_keypoint* kps,
                            uint8_t* desc, int* n_kp, float* angle, float* response,
                            uint8_t* pyramid, int64_t pyr_stride);
int  gfpl_orb_status(gfpl_orb* orb);

/* ---------------------------------------- LBD descriptors (§8(f)2 part) ---- */
/* line_descriptor::BinaryDescriptor::compute(image, keylines, descriptors)
 * (3rdparty/line_descriptor/src/binary_descriptor_custom.cpp:539-687, computeLBD :1026-1372)
 * as StereoFrame::detectLineFeatures calls it (src/stereoFrame.cpp:1194,1220): keylines of
 * octave 0 (Config::lsdOctaveNum = 1; another octave returns GFPL_E_UNSUPPORTED), images of
 * width x height (8..8192 px), up to max_images per call, kl_cap keylines per image.
 * Arithmetic pinned as the CPU oracle's ledger L1-L5.                        */
typedef struct gfpl_lbd gfpl_lbd;
int  gfpl_lbd_create(gfpl_ctx* ctx, int width, int height, int max_images, int kl_cap, gfpl_lbd** out);
int  gfpl_lbd_destroy(gfpl_lbd* lbd);
/* all pointers DEVICE: images [n][height][width] u8, keylines [n][kl_cap] (sx sy ex ey angle
 * octave, LSDDetectorC's fields), n_kl [n]; desc [n][kl_cap][32] receives row i of image j's
 * 32-byte LBD for keyline i < n_kl[j].  Synchronises; GFPL_E_CAPACITY when some n_kl[j] >
 * kl_cap (the first kl_cap are described), GFPL_E_UNSUPPORTED for a keyline of octave != 0. */
int  gfpl_lbd_compute(gfpl_lbd* lbd, const uint8_t* images, int n, const gfpl_keyline* keylines,
                      const int* n_kl, uint8_t* desc);
/* stream-ordered form; gfpl_lbd_status reports (and waits for) the async calls since the last */
int  gfpl_lbd_compute_async(gfpl_lbd* lbd, const uint8_t* images, int n, const gfpl_keyline* keylines,
                            const int* n_kl, uint8_t* desc);
int  gfpl_lbd_status(gfpl_lbd* lbd);
/* test hook of ledger L1-L2: the Gaussian-blurred image's Sobel derivatives of one DEVICE image,
 * grad [height][width] (DEVICE) = dx (low 16 bits) | dy (high 16 bits).  Synchronises.      */
int  gfpl_lbd_gradients(gfpl_lbd* lbd, const uint8_t* image, uint32_t* grad);

/* ---------------------------------------- LSD line detection (§8(f)2) ---- */
/* line_descriptor::LSDDetectorC::detect(image, keylines, scale, numOctaves, opts)
 * (3rdparty/line_descriptor/src/LSDDetector_custom.cpp:218-316) as
 * StereoFrame::detectLineFeatures calls it (src/stereoFrame.cpp:1160-1186): one octave,
 * cv::createLineSegmentDetector(opts...) ->detect (OpenCV 3.4.1 lsd.cpp, LSD_REFINE_STD,
 * scale 1), the keylines' extremes clamped, segments not longer than min_length dropped,
 * then, when more than n_features remain and n_features != 0, std::sort by response
 * (include/auxiliar.h:149-154) and the first n_features kept (:1177-1185).  Arithmetic
 * pinned as the CPU oracle's ledger S1-S7 (oracle/gfpl_lsd_oracle.cpp).   */
typedef struct gfpl_lsd_params {
    int    refine;        /* Config::lsdRefine 1 (= LSD_REFINE_STD; only value supported)  */
    double scale;         /* Config::lsdScale 1 (only value supported)                     */
    double quant;         /* Config::lsdQuant 2.0                                          */
    double ang_th;        /* Config::lsdAngTh 22.5                                         */
    double density_th;    /* Config::lsdDensityTh 0.6                                      */
    int    n_bins;        /* Config::lsdNBins 1024                                         */
    double min_length;    /* Config::minLineLength * min(W, H) (src/stereoFrame.cpp:151)   */
    int    n_features;    /* Config::lsdNFeatures 300 (0 = keep all)                       */
} gfpl_lsd_params;
typedef struct gfpl_lsd gfpl_lsd;
/* images up to 2048 x 2048 (and >= 8 x 8), up to max_images per call; kl_cap keylines out
 * per image; seg_cap raw segments per image (GFPL_E_CAPACITY beyond).                       */
int  gfpl_lsd_create(gfpl_ctx* ctx, const gfpl_lsd_params* prm, int width, int height, int max_images,
                     int kl_cap, int seg_cap, gfpl_lsd** out);
int  gfpl_lsd_destroy(gfpl_lsd* lsd);
/* all pointers DEVICE: images [n][height][width] u8; keylines [n][kl_cap] receives image j's
 * keylines (sx sy ex ey angle octave) in the reference's output order, n_kl [n] their count,
 * response [n][kl_cap] (nullable) KeyLine::response.  Keylines beyond kl_cap are an error
 * (GFPL_E_CAPACITY).  Synchronises.                                                        */
int  gfpl_lsd_detect(gfpl_lsd* lsd, const uint8_t* images, int n, gfpl_keyline* keylines, int* n_kl,
                     float* response);
/* stream-ordered form; gfpl_lsd_status reports (and waits for) the async calls since the last */
int  gfpl_lsd_detect_async(gfpl_lsd* lsd, const uint8_t* images, int n, gfpl_keyline* keylines, int* n_kl,
                           float* response);
int  gfpl_lsd_status(gfpl_lsd* lsd);
/* test hook of ledger S2: std::sort(a, a + n, key(x) > key(y)) with key = the high 32 bits of
 * each element, on DEVICE memory (n <= (width-1)(height-1)); the permutation the seed order
 * and the response sort use.  Synchronises.                                                 */
int  gfpl_lsd_sort_desc(gfpl_lsd* lsd, uint64_t* a, int n);

/* ------------------------------- stereo detection from images (§8(f)1-2) ---- */
/* The detection half of StereoFrame(img_l, img_r, idx, cam, ts) as
 * StereoFrameHandler::initialize / insertStereoPair(const Mat& img_l, const Mat& img_r,
 * int idx, double ts) run it (include/stereoFrameHandler.h:48-53, src/stereoFrame.cpp:
 * 148-172, 411-450, 1128-1227; called at app/plslam_mod.cpp:377,387): ORB of both images
 * (the right one's pyramid kept for the sub-pixel refinement), LSD of both with the
 * lsdNFeatures response cut, LBD of both — for B stereo frames, into device buffers a
 * gfpl_frames view points at, so gfpl_initialize / gfpl_insert_stereo_pair / gfpl_frame_step
 * read them without a copy.  The detector runs on two streams of its own; the view's
 * `ready` event orders the tracker call after the detection and its `consumed` event
 * (recorded by that tracker call) orders the next detection into the same buffer set
 * (`sets` of them, used in turn) after the read.                                        */
typedef struct gfpl_detector_params {
    gfpl_orb_params orb;   /* Config::orbNFeatures / orbScaleFactor / orbNLevels, 20, 7     */
    gfpl_lsd_params lsd;   /* the LSDOptions + lsdNFeatures + min line length              */
    int seg_cap;           /* raw LSD segments per image (GFPL_E_CAPACITY beyond), 4096     */
} gfpl_detector_params;
typedef struct gfpl_detector gfpl_detector;
/* the reference's Config defaults (src/config.cpp:107,134-152) for this camera; cfg NULL =
 * gfpl_config_default.  (BASELINE cfg 2 runs orb.nfeatures = 2000.)                      */
int  gfpl_detector_params_default(const gfpl_camera* cam, const gfpl_config* cfg, gfpl_detector_params* prm);
/* On a context with a camera (GFPL_E_STATE otherwise); images are the camera's size, up
 * to max_batch stereo frames per call; kp_cap / kl_cap rows per image (as the seqbatch's);
 * sets 1..4 buffer sets.  The context cannot be destroyed while the detector lives.      */
int  gfpl_detector_create(gfpl_ctx* ctx, const gfpl_detector_params* prm, int max_batch, int kp_cap,
                          int kl_cap, int sets, gfpl_detector** out);
int  gfpl_detector_destroy(gfpl_detector* det);
/* Stream-ordered detection of n stereo frames: img_l / img_r DEVICE [n][H][W] u8 and
 * time_stamp DEVICE [n], produced on the context's stream (the detection waits for it).
 * *out is the view of the next buffer set (valid until that set is detected into again).
 * GFPL_E_STATE when the set's previous view was never read by a tracker call (nor
 * released with gfpl_detector_discard): at most `sets` views may be outstanding.
 * The inputs are copied on the detector's stream and the context's stream is made to wait
 * for that copy, so the caller may overwrite img_l / img_r / time_stamp with work it
 * enqueues on the context's stream after this call returns.                            */
int  gfpl_detect_stereo_async(gfpl_detector* det, const uint8_t* img_l, const uint8_t* img_r, int n,
                              const double* time_stamp, gfpl_frames* out);
/* The same from HOST images / time stamps (copied before it returns; the detection
 * itself stays asynchronous).                                                            */
int  gfpl_detect_stereo_host(gfpl_detector* det, const uint8_t* img_l, const uint8_t* img_r, int n,
                             const double* time_stamp, gfpl_frames* out);
/* capacity / octave errors of the detections since the last status (waits for them) */
int  gfpl_detector_status(gfpl_detector* det);
/* detect (host_pointers: the _host form) + status: returns after the detection finished */
int  gfpl_detect_stereo(gfpl_detector* det, const uint8_t* img_l, const uint8_t* img_r, int n,
                        const double* time_stamp, int host_pointers, gfpl_frames* out);
/* release a view no tracker call will read (its set may then be detected into again) */
int  gfpl_detector_discard(gfpl_detector* det, const gfpl_frames* view);

/* Host copy of one sequence's detections of a DEVICE gfpl_frames view (the
 * points_l / points_r / pdesc_* / lines_* / ldesc_* members of the reference's StereoFrame
 * after detection).  Arrays are caller-allocated at the view's kp_cap / kl_cap (a NULL
 * array is skipped); waits for the view's `ready` event.                               */
typedef struct gfpl_detections_host {
    int n_kp_l, n_kp_r, n_kl_l, n_kl_r;
    gfpl_keypoint* kp_l;  gfpl_keypoint* kp_r;
    uint8_t* pdesc_l;     uint8_t* pdesc_r;   /* [cap][32] */
    gfpl_keyline* kl_l;   gfpl_keyline* kl_r;
    uint8_t* ldesc_l;     uint8_t* ldesc_r;   /* [cap][32] */
} gfpl_detections_host;
int  gfpl_read_detections(gfpl_ctx* ctx, const gfpl_frames* view, int seq, gfpl_detections_host* out);

/* ------------------------------------------- stereo rectification (§4f) ---- */
/* PinholeStereoCamera's distortion path (src/pinholeStereoCamera.cpp:24-119): the
 * constructor's initUndistortRectifyMap(K, D, R, P, size, CV_16SC2, map1, map2) (or the
 * cv::fisheye one for the equidistant model) per camera, and rectifyImage's
 * cv::remap(src, dst, map1, map2, INTER_LINEAR) per frame, as app/plslam_mod.cpp:348-351
 * runs it on every stereo pair before the tracker sees it.  8-bit single-channel images,
 * BORDER_CONSTANT 0.  R and P are the caller's (cv::stereoRectify is not part of this).
 * Arithmetic pinned as ledger R1-R6.                                    */
typedef struct gfpl_rectify_side {   /* one camera of the rig */
    int    model;        /* 0 = pinhole radial-tangential, 1 = equidistant (fisheye) */
    double K[4];         /* fx fy cx cy of the raw camera                            */
    double D[8]; int n_dist;  /* pinhole: k1 k2 p1 p2 [k3 [k4 k5 k6]] (4, 5 or 8); fisheye: k1..k4 (4) */
    double R[9];         /* rectifying rotation, row-major                            */
    double P[4];         /* fx fy cx cy of the rectified camera (left 3x3 of P)      */
} gfpl_rectify_side;
/* The maps of one camera on the HOST (no device needed): map1 [H][W][2] (x, y) the integer
 * source position, map2 [H][W] the 5 + 5 fractional bits (CV_16SC2 + CV_16UC1).  1..8192 px.
 * GFPL_E_UNSUPPORTED for another coefficient count (thin-prism / tilt terms), GFPL_E_INVALID
 * for another model, a NULL pointer or a singular P R.                                     */
int  gfpl_rectify_maps_host(const gfpl_rectify_side* s, int width, int height,
                            int16_t* map1 /*[H][W][2] x,y*/, uint16_t* map2 /*[H][W]*/);
typedef struct gfpl_rectifier gfpl_rectifier;
/* builds both cameras' maps and uploads them; images of width x height (8..8192 px).  The
 * context cannot be destroyed while the rectifier lives.  GFPL_E_NOMEM when the device
 * allocation fails.                                                                        */
int  gfpl_rectifier_create(gfpl_ctx* ctx, const gfpl_rectify_side* left, const gfpl_rectify_side* right,
                           int width, int height, gfpl_rectifier** out);
int  gfpl_rectifier_destroy(gfpl_rectifier* r);
/* the uploaded maps of side 0 (left) / 1 (right), read back into HOST arrays; synchronises */
int  gfpl_rectifier_read_maps(gfpl_rectifier* r, int side, int16_t* map1, uint16_t* map2);
/* rectifyImage for n images of one side: src / dst DEVICE u8 [n][H][W], side 0 / 1; the two
 * ranges must not overlap (GFPL_E_INVALID).  gfpl_rectify synchronises; the _async forms are
 * enqueued on the context's stream.  gfpl_rectify_stereo_async is rectifyImagesLR: both sides
 * of n stereo frames in one launch.                                                        */
int  gfpl_rectify(gfpl_rectifier* r, int side, const uint8_t* src, int n, uint8_t* dst);
int  gfpl_rectify_async(gfpl_rectifier* r, int side, const uint8_t* src, int n, uint8_t* dst);
int  gfpl_rectify_stereo_async(gfpl_rectifier* r, const uint8_t* src_l, const uint8_t* src_r, int n,
                               uint8_t* dst_l, uint8_t* dst_r);
/* the same from / to HOST images (staged in device memory the rectifier keeps); synchronises */
int  gfpl_rectify_host(gfpl_rectifier* r, int side, const uint8_t* src, int n, uint8_t* dst);
/* Raw images in: with a rectifier attached, gfpl_detect_stereo_async / _host rectify their
 * inputs into the detector's own buffer set instead of copying them (the caller may still
 * overwrite its inputs after the call returns).  The rectifier's image size must be the
 * detector's camera's (GFPL_E_INVALID) and it must outlive the attachment; NULL detaches. */
int  gfpl_detector_set_rectifier(gfpl_detector* det, gfpl_rectifier* r);

/* ------------------------------------------------- keyframe consumers ---- */
/* One keyframe's stereo features as KeyFrame::stereo_frame exposes them
 * (src/keyFrame.cpp:26-58, include/stereoFrame.h public members): row i of
 * every point array is stereo_pt[i] and row i of pdesc its left descriptor
 * (pdesc_l); likewise stereo_ls[i] / ldesc_l.  gfpl_kf_common_matches reads
 * the arrays from DEVICE memory (e.g. a gfpl_frame_host uploaded by the
 * caller, or a frame slot it copied out); T_kf_w is a host 4x4 row-major pose.
 * pdesc and ldesc must be 16-byte aligned (the kernels read a descriptor row as
 * 16-byte vectors): gfpl_kf_common_matches and gfpl_kf_local_map_matches return
 * GFPL_E_INVALID for a misaligned descriptor pointer of a kind they would read. */
typedef struct gfpl_kf_view {
    int            n_pt;
    const uint8_t* pdesc;       /* [n_pt][32]                                  */
    const double*  P;           /* [n_pt][3]  stereo_pt[i]->P                  */
    const double*  pl;          /* [n_pt][2]  stereo_pt[i]->pl                 */
    const double*  pt_sigma2;   /* [n_pt]     stereo_pt[i]->sigma2             */
    int            n_ls;
    const uint8_t* ldesc;       /* [n_ls][32]                                  */
    const double*  sP;          /* [n_ls][3]                                   */
    const double*  eP;          /* [n_ls][3]                                   */
    const double*  le;          /* [n_ls][3]                                   */
    const double*  ls_sigma2;   /* [n_ls]                                      */
    double         T_kf_w[16];  /* KeyFrame::T_kf_w (host)                     */
} gfpl_kf_view;

/* MapHandler::lookForCommonMatches, keyframe-pair stage (src/mapHandler.cpp:
 * 199-470, has_refinement = false as in the reference): DT = inverse_se3(kf1
 * T_kf_w) * kf0 T_kf_w; points: knn-2 NORM_HAMMING kf0->kf1 and kf1->kf0,
 * mutual best, d0/d1 <= max_ratio_12_p, |proj(DT P0) - pl1| * sqrt(sigma2_0) <
 * sqrt(7.815); lines: knn-2 NORM_HAMMING both ways, mutual, d1 - d0 >
 * lineDescriptorMAD(matches_12).nn12 * desc_th_l, |(le0 . proj(DT sP0),
 * le0 . proj(DT eP0))| * sqrt(sigma2_0) < sqrt(7.815).  The accepted (kf0 row,
 * kf1 row) pairs are written in kf0 row order to pt_pairs [2 * kf0->n_pt] and
 * ls_pairs [2 * kf0->n_ls] (device) and their counts to *n_pt_pairs /
 * *n_ls_pairs (host; the call synchronises).  The landmark bookkeeping that
 * follows each accepted pair (MapPoint / MapLine creation, observations,
 * full_graph) stays with the caller, which walks the pairs in the returned
 * order exactly as the reference's loop does.  A kind with fewer than two rows
 * on either keyframe yields no pairs (the reference reads a missing second
 * neighbour: ledger U4).                                                      */
int  gfpl_kf_common_matches(gfpl_ctx* ctx, const gfpl_kf_view* kf0, const gfpl_kf_view* kf1,
                            int32_t* pt_pairs, int* n_pt_pairs, int32_t* ls_pairs, int* n_ls_pairs);

/* The local map as lookForCommonMatches' second stage reads it (src/mapHandler.cpp:
 * 472-772): the map points / lines the caller keeps as local and not yet observed
 * by kf1 (`local && kf_obs_list.back() != kf1_idx`), in map order, with their
 * median descriptor (med_desc.row(0)) and 3D geometry (point3D; line3D = sP, eP).
 * Device pointers; pdesc and ldesc 16-byte aligned (GFPL_E_INVALID otherwise,
 * as for gfpl_kf_view).                                                         */
typedef struct gfpl_map_view {
    int            n_pt;
    const uint8_t* pdesc;       /* [n_pt][32]                                  */
    const double*  P;           /* [n_pt][3]  point3D (world)                  */
    int            n_ls;
    const uint8_t* ldesc;       /* [n_ls][32]                                  */
    const double*  L;           /* [n_ls][6]  line3D (world sP, eP)            */
} gfpl_map_view;

/* lookForCommonMatches, local-map stage (src/mapHandler.cpp:472-772): with
 * Twf = inverse_se3(kf1 T_kf_w), the map rows whose projection lies inside the
 * image in front of the camera (:479-490 points, :615-632 lines, both endpoints)
 * are matched against kf1's UNMATCHED features (the caller passes kf1 compacted
 * to its idx == -1 rows, :495-505 / :637-647): knn-2 NORM_HAMMING both ways,
 * mutual best; points: d0/d1 <= max_ratio_12_p, Pf.z > 0 and |proj(Pf) - pl| <
 * max_kf_epip_p; lines: d1 - d0 > lineDescriptorMAD.nn12 * desc_th_l, both
 * endpoints in front and the SIGNED line residuals le . proj(endpoint) both <
 * max_kf_epip_l (the reference compares them without abs).  Pairs (map row in
 * the caller's map_view, kf1 row) in the reference's loop order; counts on the
 * host (synchronises).  Config::maxKFEpipP / maxKFEpipL default to 1.0
 * (src/config.cpp:42-43).  Fewer than two rows on a side: no pairs (U4).      */
int  gfpl_kf_local_map_matches(gfpl_ctx* ctx, const gfpl_map_view* map, const gfpl_kf_view* kf1,
                               double max_kf_epip_p, double max_kf_epip_l,
                               int32_t* pt_pairs, int* n_pt_pairs, int32_t* ls_pairs, int* n_ls_pairs);

/* MapHandler::isLoopClosure with its solver computeRelativePoseGN (src/mapHandler.cpp:
 * 3078-3545), batched over n candidate keyframe pairs (one workgroup each).  Per pair and
 * feature kind: knn-2 NORM_HAMMING both ways, row i of kf0 kept when it is the best match of
 * its best match (no ratio and no MAD test), pairs in kf0 row order; the features take the
 * class-default sigma2 = 1.0 and inlier = true; Config::maxIters Gauss-Newton iterations from
 * T_inc = I over the point and line residuals of kf0's 3D under T_inc against kf1's
 * observations; the chi-square outlier pass (sqrt(7.815)); the five gates below.  The candidates
 * come from gfpl_bowdb_insert + gfpl_kf_loop_candidates (below); the pose graph stays with the
 * caller.  T_kf_w, pt_sigma2 and ls_sigma2
 * of the views are not read.  A kind with fewer than two rows on either keyframe yields no
 * pairs (ledger U4).                                                                       */
typedef struct gfpl_loop_params { double lc_res, lc_unc, lc_inl, lc_trs, lc_rot; } gfpl_loop_params;
/* Config::lcRes / lcUnc / lcInl / lcTrs / lcRot: 1.5, 0.01, 0.3, 1.5, 35.0 (src/config.cpp:62-66) */
void gfpl_default_loop_params(gfpl_loop_params* prm);
typedef struct gfpl_loop_result {
    int32_t is_lc, gates;            /* gates: bit 0 res, 1 unc, 2 inl, 3 trs, 4 rot (31 = all hold) */
    int32_t n_pt, n_ls;              /* mutual-best pairs (common_pt / common_ls)                    */
    int32_t n_pt_inl, n_ls_inl;      /* of them inliers after the outlier pass                       */
    int32_t iters, pad;              /* GN iterations whose sums were evaluated                      */
    double  e, unc, ratio_inliers, trs, rot;   /* the five gated values (rot in degrees)             */
    double  x_inc[6];                /* logmap_se3(T_inc)                                            */
    double  pose_inc[6];             /* logmap_se3(inverse_se3(T_inc)) when is_lc, else 0            */
    double  T_inc[16];
} gfpl_loop_result;
/* kf0 / kf1: HOST arrays of n views whose pointers are DEVICE memory.  pt_pairs [n][pt_cap][2],
 * pt_inlier [n][pt_cap], ls_pairs [n][ls_cap][2], ls_inlier [n][ls_cap] (device): pair i's first
 * out[i].n_pt / n_ls rows are its (kf0 row, kf1 row) pairs and their inlier flags.  out: host [n].
 * max_iters, homog_th and the camera are the context's.  GFPL_E_INVALID for a NULL pointer, n < 0,
 * a context without a camera, or a view with >= 2 rows of a kind whose arrays of that kind are
 * NULL; GFPL_E_CAPACITY (nothing launched) when some kf0[i].n_pt > pt_cap or n_ls > ls_cap;
 * n = 0 is GFPL_OK.  Synchronises.                                                          */
int  gfpl_kf_loop_closure(gfpl_ctx* ctx, const gfpl_kf_view* kf0, const gfpl_kf_view* kf1, int n,
                          const gfpl_loop_params* prm, int pt_cap, int ls_cap,
                          int32_t* pt_pairs, uint8_t* pt_inlier, int32_t* ls_pairs, uint8_t* ls_inlier,
                          gfpl_loop_result* out);

/* ------------------------------------------- landmark descriptor store ---- */
/* MapPoint / MapLine::desc_list and med_desc on the device (src/mapFeatures.cpp:28-92, 96-162;
 * k_lm.hip, DESIGN.md §4i, ledger LM1-LM7).  A store holds, for lm_cap landmarks, up to obs_cap
 * 32-byte NORM_HAMMING descriptors each, and for every landmark the observation that
 * updateAverageDescDir picks: all pairwise Hamming distances, the element 1 + (n - 1) / 2 of every
 * sorted row (the row includes the landmark's own 0), the first row of least such median.  One
 * store serves points or lines; a caller keeps two.  obs_list, kf_obs_list, dir_list, sigma_list,
 * the 3D geometry and med_obs_dir stay with the caller.                                          */
#define GFPL_LM_MAX_OBS 64          /* observations per landmark the store can hold */
#define GFPL_LM_ADD       0         /* desc_list.push_back(row arg of srcs[src]); a landmark with no observation is created */
#define GFPL_LM_ERASE_OBS 1         /* desc_list.erase(begin() + arg): later observations move down by one */
#define GFPL_LM_FREE      2         /* map_points[lm] = NULL: the landmark holds nothing afterwards */
typedef struct gfpl_lm_op { int32_t lm, kind, arg, src; } gfpl_lm_op;   /* src is read for GFPL_LM_ADD only */
typedef struct gfpl_lmstore gfpl_lmstore;

/* lm_cap >= 1 landmarks (lm_cap * obs_cap * 32 bytes of rows), at most max_ops >= 1 ops per apply.
 * Every landmark starts empty.  The context cannot be destroyed while the store lives.          */
int  gfpl_lmstore_create(gfpl_ctx* ctx, int lm_cap, int obs_cap /*1..GFPL_LM_MAX_OBS*/, int max_ops, gfpl_lmstore** out);
int  gfpl_lmstore_destroy(gfpl_lmstore* st);
int64_t gfpl_lmstore_bytes(const gfpl_lmstore* st);   /* device bytes: the store and the uploaded lists */
/* Host only, no device: simulates the counts of an op list.  counts [lm_cap]: in, every landmark's
 * count before; out, after (unchanged when the list is refused).  The ops are checked in array
 * order and the first that fails decides: GFPL_E_INVALID for a NULL pointer, n < 0, lm_cap < 1,
 * obs_cap outside 1..GFPL_LM_MAX_OBS, a count outside [0, obs_cap], lm outside [0, lm_cap), an
 * unknown kind, an ADD whose src is outside [0, n_srcs) or whose row is outside [0, src_rows[src]),
 * an ERASE_OBS position outside the list as it stands at that op; GFPL_E_CAPACITY for an ADD to a
 * list of obs_cap.  FREE of an empty landmark is allowed.  n = 0 is GFPL_OK.                   */
int  gfpl_lm_ops_check(const gfpl_lm_op* ops, int n, int32_t* counts /*[lm_cap] in: before, out: after*/,
                       int lm_cap, int obs_cap, const int32_t* src_rows, int n_srcs);
/* Applies the ops: those of one landmark in array order, landmarks independently of each other.
 * Afterwards every landmark an op named has the med_idx / med_desc of updateAverageDescDir over its
 * final list (the reference recomputes after every append; nothing reads the value in between); an
 * empty list has count 0, med_idx -1 and a zeroed median row.  Runs gfpl_lm_ops_check against the
 * store's counts before any device work, with the same codes; GFPL_E_CAPACITY also for n > max_ops,
 * GFPL_E_INVALID also for an ADD from a NULL or misaligned srcs[src].  A refused call changes
 * nothing.  ADD rows are read during the call.  Synchronises once.  GFPL_E_HIP from a copy, launch
 * or synchronisation of the call leaves the store's contents unknown: apply, gather and read return
 * GFPL_E_STATE from then on and the store can only be destroyed.                                */
int  gfpl_lmstore_apply(gfpl_lmstore* st, const gfpl_lm_op* ops /*HOST*/, int n,
                        const uint8_t* const* srcs /*HOST array of DEVICE [rows][32], 16-B aligned*/,
                        const int32_t* src_rows, int n_srcs);
/* The median rows of lm_ids, compacted in the order given (ids may repeat): row i of desc_out is
 * med_desc of lm_ids[i], med_idx_out[i] its index in desc_list.  The selection `local &&
 * kf_obs_list.back() != kf1_idx` stays the caller's; desc_out is a gfpl_map_view's pdesc / ldesc.
 * GFPL_E_INVALID, and nothing written, for an id outside [0, lm_cap) or of a landmark without an
 * observation, or a misaligned desc_out.  Synchronises once.                                    */
int  gfpl_lmstore_gather(gfpl_lmstore* st, const int32_t* lm_ids /*HOST [n]*/, int n,
                         uint8_t* desc_out /*DEVICE [n][32], 16-B aligned*/, int32_t* med_idx_out /*DEVICE [n] or NULL*/);
/* One landmark to the host (any output may be NULL).  desc_list receives all obs_cap rows as the
 * store holds them: rows [0, count) are the list, the others whatever was last written there.
 * Synchronises once.                                                                            */
int  gfpl_lmstore_read(gfpl_lmstore* st, int lm, int32_t* count, int32_t* med_idx,
                       uint8_t* desc_list /*HOST [obs_cap][32] or NULL*/, uint8_t* med_desc /*HOST [32] or NULL*/);
/* Instrumentation (tools/bench_lm_store.py): device milliseconds between the first and the last
 * kernel of the store's last apply or gather that launched any; GFPL_E_STATE when there is none.
 * The device-id calls below are covered: from their first kernel to their last.                  */
int  gfpl_lmstore_debug_ms(gfpl_lmstore* st, float* ms);

/* The device-id calls: the store's half of a keyframe tick from the arrays gfpl_kfmap left on the
 * device, beside gfpl_mapgeo's calls of the same names (k_lm_plan.hip, DESIGN.md §4i "the device
 * planner", ledger LM8-LM10).  The op list is built, checked, grouped and
 * bucketed on the device; nothing but the call's error word comes back.
 *
 * Refusals are decided on the device: a check kernel raises bits in an error word, every later
 * kernel of the call reads the word first and neither indexes with the call's data nor changes the
 * store when it is set.  A refused call changes nothing and leaves the scratch cleared.  When
 * refusals of both kinds occur in one call the code is GFPL_E_INVALID (gfpl_mapgeo's rule: the
 * word keeps both bits, INVALID is read first); which pair raised it is not reported.
 * GFPL_E_INVALID: a NULL pointer, n < 0 or a negative row count; a descriptor array (desc0, desc1,
 * desc_out) that is not 16-B aligned (host checks); a pair row outside [0, n0) / [0, n1) /
 * [0, n_unm); an unm_rows value outside [0, n1); an lm_out value outside [-1, lm_cap) or an id
 * outside [0, lm_cap); first_new outside [0, lm_cap]; a created id (>= first_new) whose list is not
 * empty or that two pairs name; a carried id whose list is empty; a gathered id whose list is empty.
 * GFPL_E_CAPACITY: a list that would pass obs_cap; n > max_ops (host check: the scratch holds one
 * word per pair); a call whose ops, two per created pair and one per carried pair, exceed max_ops
 * (decided on the device from the call's own op count: max_ops >= 2 n always suffices for
 * observe_pairs and max_ops >= n for observe_local; free_ids and gather_ids use no ops and take
 * any n).  GFPL_E_STATE as for apply; GFPL_E_HIP from an observe or free call leaves the contents
 * unknown as for apply, GFPL_E_NOMEM when the scratch cannot be allocated (at the first of these
 * calls: a store that never uses them keeps its gfpl_lmstore_bytes).  Each call synchronises
 * once; n = 0 returns GFPL_OK without a launch.  The arrays are read during the call.
 *
 * The device's counts are the authority: these calls change them without the host seeing it, so
 * the next apply, fuse or host-id gather first refreshes the store's host mirror with one copy of
 * count[lm_cap] (calls that never mix the two routes pay nothing).                               */
/* The descriptor half of lookForCommonMatches' keyframe-pair body (src/mapHandler.cpp:280, :287,
 * :315): pairs, lm_out and first_new are what gfpl_kfmap_observe_pairs took and returned, desc0 /
 * desc1 kf0's / kf1's pdesc (ldesc) rows.  Pair i in pair order: lm_out[i] == -1 nothing (:308);
 * lm_out[i] >= first_new (created) ADD row pairs[i][0] of desc0, then ADD row pairs[i][1] of
 * desc1; otherwise (carried) ADD row pairs[i][1] of desc1.  Several pairs may carry one landmark:
 * their rows are appended in pair order (gfpl_mapgeo_observe_pairs' "place").  Afterwards every
 * landmark named has the count / med_idx / med_desc of updateAverageDescDir over its final list. */
int  gfpl_lmstore_observe_pairs(gfpl_lmstore* st, const uint8_t* desc0 /*DEVICE [n0][32]*/, int n0,
                                const uint8_t* desc1 /*DEVICE [n1][32]*/, int n1,
                                const int32_t* pairs /*DEVICE [n][2]*/, const int32_t* lm_out /*DEVICE [n]*/, int n,
                                int first_new);
/* The local-map stage (:615, :757): landmark lm_out[i] receives row unm_rows[pairs[i][1]] of desc1;
 * column 0 of pairs is not read and every named landmark is a carried one.                      */
int  gfpl_lmstore_observe_local(gfpl_lmstore* st, const uint8_t* desc1 /*DEVICE [n1][32]*/, int n1,
                                const int32_t* pairs /*DEVICE [n][2]*/, int n,
                                const int32_t* unm_rows /*DEVICE [n_unm]*/, int n_unm, const int32_t* lm_out /*DEVICE [n]*/);
/* GFPL_LM_FREE of every listed id (the list gfpl_kfmap_remove_bad wrote): count 0, med_idx -1, a
 * zeroed median row, the rows as they are.  An empty landmark or a repeated id is allowed.      */
int  gfpl_lmstore_free_ids(gfpl_lmstore* st, const int32_t* ids /*DEVICE [n]*/, int n);
/* gfpl_lmstore_gather with the id list on the device (gfpl_kfmap_select's output).  A refused
 * call writes neither desc_out nor med_idx_out.                                                 */
int  gfpl_lmstore_gather_ids(gfpl_lmstore* st, const int32_t* ids /*DEVICE [n]*/, int n,
                             uint8_t* desc_out /*DEVICE [n][32], 16-B aligned*/, int32_t* med_idx_out /*DEVICE [n] or NULL*/);
/* Every landmark's count as the device holds it (one copy, one synchronisation; the host mirror is
 * refreshed with it): what a caller of the device-id calls hands gfpl_lm_ops_check.             */
int  gfpl_lmstore_counts(gfpl_lmstore* st, int32_t* counts /*HOST [lm_cap]*/);

/* Ops that cross landmarks: what MapHandler::loopClosureFuseLandmarks (src/mapHandler.cpp:4425 ff.)
 * does to desc_list, without a descriptor leaving the device (DESIGN.md §4i "fuse").             */
#define GFPL_LM_APPEND_LM 3   /* gfpl_lmstore_fuse / gfpl_lm_fuse_check only: desc_list of `lm` += desc_list of landmark
                                 `arg` as it stands at this op; `src` is not read.  apply / ops_check keep refusing it. */
/* Host only, no device: gfpl_lm_ops_check for a fuse list.  The ops run one after another over the
 * whole list, and the first that fails decides.  GFPL_E_INVALID: everything gfpl_lm_ops_check
 * refuses for ADD / FREE, an append whose arg is outside [0, lm_cap) or equals lm or has a count
 * outside [0, obs_cap], an append from or to a landmark whose list is empty at that op, any op that
 * names (as lm or arg) a landmark that an earlier FREE of the list emptied.  GFPL_E_UNSUPPORTED:
 * GFPL_LM_ERASE_OBS.  GFPL_E_CAPACITY: a list beyond obs_cap.  n_rows (may be NULL) receives 1 per
 * ADD or FREE plus the source's length per append, 0 for a refused list.                        */
int  gfpl_lm_fuse_check(const gfpl_lm_op* ops, int n, int32_t* counts /*[lm_cap] in: before, out: after*/, int lm_cap,
                        int obs_cap, const int32_t* src_rows, int n_srcs, int64_t* n_rows /*may be NULL*/);
/* Runs the ops one after another in array order over the whole list (apply orders them per landmark
 * only).  Afterwards every landmark named as an op's lm has the count / med_idx / med_desc of
 * updateAverageDescDir over its final list; a landmark named only as arg is unchanged.  The order of
 * a list is kept: an append adds the source's observations in their order.  Runs gfpl_lm_fuse_check
 * against the store's counts before any device work, with the same codes; GFPL_E_CAPACITY also for
 * n_rows > max_ops, GFPL_E_INVALID also for an ADD from a NULL or misaligned srcs[src]; GFPL_E_STATE
 * and GFPL_E_HIP as for apply.  A refused call changes nothing.  Synchronises once.              */
int  gfpl_lmstore_fuse(gfpl_lmstore* st, const gfpl_lm_op* ops /*HOST*/, int n,
                       const uint8_t* const* srcs /*HOST array of DEVICE [rows][32], 16-B aligned*/,
                       const int32_t* src_rows, int n_srcs);

/* The candidate search of MapHandler::fuseLandmarksFromLocalMap (src/mapHandler.cpp:859-1056; k_fuse.hip,
 * DESIGN.md §4l, ledger FU1-FU11); the list walk that follows it stays the caller's.
 * Per kind: (1) the rows whose projection under T = T_kf[kf] (taken as written: the reference names it
 * Twf and does not invert it) lies strictly inside the image with Pf.z > 0, lines with both endpoints,
 * are compacted in map order: loc[j] is the map row of selected row j; (2) with more than one selected
 * row, knn-2 NORM_HAMMING of the selected median rows against themselves (the tie rule of
 * gfpl_knn2_hamming) and for row i its SECOND neighbour t (lmatches_12[i][1]), skipped when t == i;
 * (3) points: |P_t - P_i| < max_point_point_error; lines: |d1 - d2| < max_dir_line_error and both
 * endpoints of one line within max_point_line_error of the other, which line deciding d1.norm() >
 * d2.norm() as written; all comparisons strict, NaN fails; (4) pairs (i, t) over the selected list in
 * ascending i (map_local_*_to_fuse); both (i, t) and (t, i) may appear.  A kind with n == 0 or fewer than
 * two selected rows yields no pairs.  Counts to the host; synchronises once.  GFPL_E_INVALID: a NULL
 * pointer, a negative count, a misaligned descriptor pointer of a kind with two or more rows, a context
 * without a camera, and (after the device work, outputs then unspecified) a pt_kf / ls_kf entry outside
 * [0, n_kf): such a row is never used as an index.  GFPL_E_NOMEM when the context's workspace cannot grow. */
typedef struct gfpl_fuse_params { double max_point_point_error, max_point_line_error, max_dir_line_error; } gfpl_fuse_params;
void gfpl_default_fuse_params(gfpl_fuse_params* prm);   /* 0.1, 0.1, 0.1 (src/config.cpp:46-48) */
typedef struct gfpl_fuse_map {
    gfpl_map_view  map;      /* the caller's `!= NULL && local` landmarks in map order (:869-874, :961-966); pdesc / ldesc =
                                med rows (gfpl_lmstore_gather), P = point3D, L = line3D                                   */
    const int32_t* pt_kf;    /* DEVICE [n_pt]  kf_obs_list[0]                                                           */
    const int32_t* ls_kf;    /* DEVICE [n_ls]                                                                           */
    int            n_kf;
    const double*  T_kf;     /* DEVICE [n_kf][16]  T_kf_w (the layout of gfpl_pgo_problem.T_kf)                          */
} gfpl_fuse_map;
int  gfpl_map_fuse_search(gfpl_ctx* ctx, const gfpl_fuse_map* m, const gfpl_fuse_params* prm,
                          int32_t* pt_loc /*DEVICE [n_pt]*/, int* n_pt_loc, int32_t* pt_pairs /*DEVICE [n_pt][2]*/, int* n_pt_pairs,
                          int32_t* ls_loc /*DEVICE [n_ls]*/, int* n_ls_loc, int32_t* ls_pairs /*DEVICE [n_ls][2]*/, int* n_ls_pairs);
/* Instrumentation (tools/bench_lm_fuse.py): device milliseconds of the last search's select, knn-2 and
 * gate launches of kind 0 (points) or 1 (lines); GFPL_E_STATE when that kind launched fewer than all three. */
int  gfpl_map_fuse_debug_ms(gfpl_ctx* ctx, int kind, float* ms /*HOST [3]*/);

/* ------------------------------------- the map's index half ------------- */
/* The integer bookkeeping of MapHandler (src/mapHandler.cpp) as one device object per map (k_kfmap.hip,
 * gfpl_kfmap.cpp, DESIGN.md §4m, ledger KM1-KM9): stereo_pt[i]->idx / stereo_ls[i]->idx of every
 * keyframe, kf_obs_list of every landmark, full_graph, map_points_kf_idx / map_lines_kf_idx and the
 * `local` flags, with the reference's operations on them.  kind 0 is points, 1 lines; the two id
 * spaces are independent (max_pt_idx, max_ls_idx).  obs_list, dir_list, sigma_list, pts_list, the 3D
 * geometry, med_obs_dir and the lc_status machine stay with the caller; the descriptors are
 * gfpl_lmstore's.  map_*_kf_idx is kept as one `owner` per landmark: keyframe k's list is the
 * landmarks it owns in ascending id (KM3).
 * Every call synchronises once.  A refused call changes nothing.  GFPL_E_INVALID wins over
 * GFPL_E_CAPACITY when a call's device data earns both.  After GFPL_E_HIP from a launch, copy or
 * synchronisation the state is unknown: every call returns GFPL_E_STATE until the object is destroyed. */
#define GFPL_KFMAP_TILE 2048          /* landmarks (or rows) per workgroup of the ordered compactions */
#define GFPL_KFMAP_LOCAL        0     /* alive && local (localBundleAdjustment :1133-1166, gfpl_fuse_map) */
#define GFPL_KFMAP_LOCAL_UNSEEN 1     /* alive && local && kf_obs_list.back() != kf1 (:520, :642) */
#define GFPL_KFMAP_ALIVE        2     /* map_points[j] != NULL (globalBundleAdjustment) */
typedef struct gfpl_kfmap gfpl_kfmap;
typedef struct gfpl_kfmap_caps {
    int32_t kf_cap;                   /* keyframes */
    int32_t pt_rows, ls_rows;         /* features of one keyframe */
    int32_t pt_lm_cap, ls_lm_cap;     /* landmark ids ever given out (freed ids are not reused) */
    int32_t obs_cap;                  /* entries of one kf_obs_list, 2..GFPL_LM_MAX_OBS */
} gfpl_kfmap_caps;
typedef struct gfpl_kfmap_params { int32_t min_lm_cov_graph, min_kf_local_map, min_lm_obs, cull_age; } gfpl_kfmap_params;
void gfpl_default_kfmap_params(gfpl_kfmap_params* prm);   /* 30, 3, 2, 10 (src/config.cpp:40, 51, 53; the literal of :2558) */
typedef struct gfpl_kfmap_kf { int32_t alive, local, n_pt, n_ls; } gfpl_kfmap_kf;
/* Host only: the device bytes of an object with these caps (state and workspace), -1 for caps it refuses. */
int64_t gfpl_kfmap_bytes(const gfpl_kfmap_caps* caps);
/* MapHandler::initialize's resets (:42-58): no keyframe, no landmark, both next ids 0, a zero graph.
 * GFPL_E_INVALID for a NULL pointer, a cap < 1, kf_cap > 65535, obs_cap outside 2..GFPL_LM_MAX_OBS.  The context cannot be
 * destroyed while the object lives.                                                             */
int  gfpl_kfmap_create(gfpl_ctx* ctx, const gfpl_kfmap_caps* caps, gfpl_kfmap** out);
int  gfpl_kfmap_destroy(gfpl_kfmap* m);
/* n_kf (map_keyframes.size()) and the next ids (max_pt_idx, max_ls_idx); any may be NULL. */
int  gfpl_kfmap_counts(const gfpl_kfmap* m, int32_t* n_kf, int32_t* next_pt, int32_t* next_ls);
/* The first call is initialize's keyframe (:63-67, :88-92), a later one expandGraphs, max_kf_idx++,
 * local = true, the index reset and the list insertion of addKeyFrame (:116-134, :147-150).  The new
 * keyframe has n_pt / n_ls rows, all -1, and owns nothing.  GFPL_E_CAPACITY beyond kf_cap / pt_rows /
 * ls_rows, GFPL_E_INVALID for a negative count.                                                 */
int  gfpl_kfmap_add_keyframe(gfpl_kfmap* m, int n_pt, int n_ls, int32_t* kf_idx);
/* The loop body of lookForCommonMatches' keyframe-pair stage (:266-336, :404-485, has_refinement ==
 * false) over pairs (kf0 row, kf1 row) as gfpl_kf_common_matches returns them.  A kf0 row with idx
 * -1 creates a landmark: id = *first_new + its rank among the creating pairs in pair order, both rows'
 * idx set, kf_obs = [kf0, kf1], owner kf0, inlier, not local (KM9), full_graph[kf0][kf1] and its
 * mirror + 1.  A row carrying an alive landmark sets kf1's row, appends kf1 and adds 1 to
 * full_graph[kf1][o] and its mirror for every entry o != kf1 the list held before the call (two kf0
 * rows may carry one landmark: it receives kf1 twice).  A row carrying a freed landmark does nothing
 * and lm_out is -1 (:308, KM6).  lm_out[i] is pair i's landmark, created iff >= *first_new.
 * GFPL_E_INVALID: a NULL pointer, n < 0, kind outside 0..1, kf0 == kf1, a keyframe out of range or
 * erased, n above either keyframe's rows, a pair row outside its keyframe's rows, a column of pairs
 * that holds a value twice (KM8), a carried id < -1 or >= the next id.  GFPL_E_CAPACITY: a list
 * beyond obs_cap, an id beyond the landmark cap.  Bad device data is never used as an index.    */
int  gfpl_kfmap_observe_pairs(gfpl_kfmap* m, int kind, int kf0, int kf1, const int32_t* pairs /*DEVICE [n][2]*/, int n,
                              int32_t* lm_out /*DEVICE [n]*/, int32_t* first_new, int32_t* n_new);
/* The local-map stage's body (:609-624, :745-764) over pairs (row of the caller's map view, row among
 * kf1's unmatched) as gfpl_kf_local_map_matches returns them: the landmark is sel_ids[p0], the kf1 row
 * unm_rows[p1]; then the append and graph update of an existing landmark above.  lm_out[i] is the
 * landmark.  GFPL_E_INVALID also for p0 outside [0, n_sel), p1 outside [0, n_unm), a sel_ids entry that
 * is not an alive landmark, an unm_rows entry outside kf1's rows; a repeated value in a column of
 * pairs as above, and n > min(n_sel, n_unm) therefore; n_sel above the kind's next id, n_unm above
 * kf1's rows, an unm_rows value that two pairs name.                                             */
int  gfpl_kfmap_observe_local(gfpl_kfmap* m, int kind, int kf1, const int32_t* pairs /*DEVICE [n][2]*/, int n,
                              const int32_t* sel_ids /*DEVICE [n_sel]*/, int n_sel,
                              const int32_t* unm_rows /*DEVICE [n_unm]*/, int n_unm, int32_t* lm_out /*DEVICE [n]*/);
/* formLocalMap (:789-857): every local flag reset; the newest keyframe (back()) local; keyframe i below
 * it local when full_graph[newest][i] >= min_lm_cov_graph or newest - i <= min_kf_local_map; the alive
 * landmarks on a local keyframe's rows local.  An erased keyframe i is skipped (KM1).  GFPL_E_STATE
 * without a keyframe or with the newest erased.                                                 */
int  gfpl_kfmap_form_local_map(gfpl_kfmap* m, const gfpl_kfmap_params* prm);
/* The landmarks of `which` in map order (ascending id); ids holds up to the kind's next id.  kf1 is
 * read for GFPL_KFMAP_LOCAL_UNSEEN only.                                                        */
int  gfpl_kfmap_select(gfpl_kfmap* m, int kind, int which, int kf1, int32_t* ids /*DEVICE*/, int32_t* n);
/* kf's rows with idx == -1, in row order (:539-546, :666-673); rows holds up to the keyframe's rows. */
int  gfpl_kfmap_unmatched(gfpl_kfmap* m, int kind, int kf, int32_t* rows /*DEVICE*/, int32_t* n);
/* alive && local && kf_idx != 0, ascending (:1115-1127); kf_list holds up to kf_cap. */
int  gfpl_kfmap_local_keyframes(gfpl_kfmap* m, int32_t* kf_list /*HOST*/, int32_t* n);
/* removeBadMapLandmarks (:2550-2630): an alive landmark that is not local, with max_kf_idx -
 * kf_obs[0] > cull_age (KM7) and (!inlier or n_obs < min_lm_obs (KM4)) is removed: the first (lowest)
 * row of keyframe kf_obs[0] that carries its id becomes -1, owner becomes -1 when it is kf_obs[0],
 * the landmark is freed.  Rows of other keyframes keep the id (KM5).  A landmark whose kf_obs[0] is
 * an erased keyframe is skipped (KM2).  The removed ids in map order, ready for GFPL_LM_FREE ops;
 * each list holds up to the kind's next id.                                                     */
int  gfpl_kfmap_remove_bad(gfpl_kfmap* m, const gfpl_kfmap_params* prm, int32_t* pt_removed /*DEVICE*/, int32_t* n_pt,
                           int32_t* ls_removed /*DEVICE*/, int32_t* n_ls);
/* inlier = value of the listed landmarks (freed ones are passed over); GFPL_E_INVALID for an id
 * outside [0, next id) or a value outside 0..1.                                                  */
int  gfpl_kfmap_set_inlier(gfpl_kfmap* m, int kind, const int32_t* ids /*DEVICE [n]*/, int n, int value);
/* map_keyframes[kf] = NULL and the zeroed graph row and column (:2777-2784); nothing else of
 * removeRedundantKFs, which the reference disables.                                             */
int  gfpl_kfmap_erase_keyframe(gfpl_kfmap* m, int kf);
/* Read and patch, HOST arrays.  Reads take any keyframe below n_kf (erased ones too) and ids below the
 * cap; outputs may be NULL.  Writes are checked on the host (GFPL_E_INVALID): an alive keyframe, rows
 * within its rows, idx values in [-1, next id); flags 0 / 1, n_obs in [1, obs_cap] for an alive
 * landmark and [0, obs_cap] for a freed one, the first n_obs entries of kf_obs below n_kf, owner in
 * [-1, n_kf), ids below the cap.  write_landmarks takes every array and raises the kind's next id
 * to id0 + n when that is larger (the ids between are freed landmarks).                         */
int  gfpl_kfmap_read_keyframe(gfpl_kfmap* m, int kf, gfpl_kfmap_kf* rec, int32_t* pt_idx /*[pt_rows]*/, int32_t* ls_idx /*[ls_rows]*/);
int  gfpl_kfmap_write_keyframe_idx(gfpl_kfmap* m, int kind, int kf, int row0, int n, const int32_t* idx);
int  gfpl_kfmap_read_landmarks(gfpl_kfmap* m, int kind, int id0, int n, uint8_t* alive, uint8_t* local, uint8_t* inlier,
                               int32_t* n_obs, int32_t* owner, int32_t* kf_obs /*[n][obs_cap]*/);
int  gfpl_kfmap_write_landmarks(gfpl_kfmap* m, int kind, int id0, int n, const uint8_t* alive, const uint8_t* local,
                                const uint8_t* inlier, const int32_t* n_obs, const int32_t* owner, const int32_t* kf_obs);
/* The graph in the shape gfpl_pgo_problem takes, HOST arrays (any kind's three may be NULL together):
 * alive [n_kf], full_graph [n_kf][n_kf], *_kf_start [n_kf + 1], *_kf_idx [up to the next id]: every
 * landmark with an owner under its owner in ascending id, *_freed [next id].                    */
int  gfpl_kfmap_export_graph(gfpl_kfmap* m, uint8_t* alive, int32_t* full_graph, int32_t* pt_kf_start, int32_t* pt_kf_idx,
                             uint8_t* pt_freed, int32_t* ls_kf_start, int32_t* ls_kf_idx, uint8_t* ls_freed);
/* Instrumentation (tools/bench_kfmap.py): device milliseconds between the first and the last kernel of
 * the object's last call that launched any; GFPL_E_STATE when there is none.                     */
int  gfpl_kfmap_debug_ms(gfpl_kfmap* m, float* ms);

/* ------------------------------------- loop-closure candidate search ----- */
/* DBoW2 as MapHandler uses it (insertKFBowVectorP / L / PL, src/mapHandler.cpp:2865-3000, and
 * lookForLoopCandidates, :3002-3076): TemplatedVocabulary<FORB>::transform and L1Scoring::score
 * on the device (k_bow.hip), the keyframe database around them, and the decision over a row of
 * the confusion matrix on the host.  Every double has the reference's bits (DESIGN.md ledger
 * BW1-BW8).                                                                                   */
typedef struct gfpl_vocab gfpl_vocab;
typedef struct gfpl_bowdb gfpl_bowdb;
/* DBoW2::WeightingType / ScoringType */
#define GFPL_BOW_TF_IDF 0
#define GFPL_BOW_TF     1
#define GFPL_BOW_IDF    2
#define GFPL_BOW_BINARY 3
#define GFPL_BOW_L1_NORM 0
/* A vocabulary tree as flat HOST arrays (both of DBoW2's file formats fit: the .yml names node
 * and word ids, the text format implies them).  Node 0 is the root.  child[child_off[i] ..
 * child_off[i + 1]) are node i's children in Node::children order (the descent walks them in
 * that order, the first minimum wins); a node without children is a leaf and ends the descent
 * (the tree may be ragged).  word_id is read on leaves only (-1 on inner nodes).             */
typedef struct gfpl_vocab_desc {
    int            n_nodes;
    const int32_t* child_off;   /* [n_nodes + 1], ascending from 0                            */
    const int32_t* child;       /* [child_off[n_nodes]] node indices                          */
    const uint8_t* desc;        /* [n_nodes][32] (the root's row is never read)               */
    const double*  weight;      /* [n_nodes]                                                  */
    const int32_t* word_id;     /* [n_nodes]                                                  */
    int            weighting;   /* GFPL_BOW_TF_IDF ... GFPL_BOW_BINARY                        */
    int            scoring;     /* GFPL_BOW_L1_NORM                                           */
} gfpl_vocab_desc;
/* Validates on the host, before the context is looked at, then uploads the device copy.
 * GFPL_E_INVALID: NULL array, n_nodes < 2, a root without children (the reference indexes
 * children[0] of it), child_off not ascending from 0, a child index outside [1, n_nodes), a node
 * reachable twice or a cycle, a leaf with word_id < 0, a word id on two leaves, a weighting
 * outside 0..3, a NULL context.  GFPL_E_UNSUPPORTED: a node with more than 32 children, a scoring
 * other than L1_NORM.  GFPL_E_NOMEM: the device copy could not be allocated.  Nodes the root does
 * not reach are ignored.  The context cannot be destroyed while the vocabulary lives.        */
int  gfpl_vocab_create(gfpl_ctx* ctx, const gfpl_vocab_desc* desc, gfpl_vocab** out);
/* the host-side rules alone (no context, no device): GFPL_OK or the code gfpl_vocab_create returns */
int  gfpl_vocab_check(const gfpl_vocab_desc* desc);
int  gfpl_vocab_destroy(gfpl_vocab* voc);

#define GFPL_BOW_MAX_CAP 8192   /* descriptors per set (the set's keys are sorted in 32 KB of LDS) */
/* TemplatedVocabulary::transform(features, BowVector&) (TemplatedVocabulary.h:1065-1122) for n
 * descriptor sets in one call.  desc_ptrs / counts: HOST arrays of n DEVICE pointers ([counts[i]][32]
 * bytes, 16-byte aligned) and row counts.  Outputs (device): word_ids [n][cap] int32 and values
 * [n][cap] double, set i's first n_words[i] entries in ascending word id (std::map's order); n_words:
 * host [n].  GFPL_E_CAPACITY, nothing launched, when a count exceeds cap; GFPL_E_UNSUPPORTED for
 * cap > GFPL_BOW_MAX_CAP; n = 0 is GFPL_OK.  Synchronises.                                     */
int  gfpl_bow_transform(gfpl_ctx* ctx, const gfpl_vocab* voc, int n, const uint8_t* const* desc_ptrs,
                        const int* counts, int cap, int32_t* word_ids, double* values, int* n_words);

/* a BowVector on the device: count entries in ascending word id */
typedef struct gfpl_bow_vec { const int32_t* ids; const double* values; int count; } gfpl_bow_vec;
/* L1Scoring::score(a[i], b[i]) (ScoringObject.cpp:23-68) for n_pairs pairs; a, b: HOST arrays of
 * device triples; scores: DEVICE [n_pairs].  Two vectors without a common word score -0.0.
 * Synchronises.                                                                                */
int  gfpl_bow_score(gfpl_ctx* ctx, const gfpl_bow_vec* a, const gfpl_bow_vec* b, int n_pairs, double* scores);

/* vector_stdv (src/auxiliar.cpp:547-556) of a keyframe's features as insertKFBowVectorPL takes
 * it (:2940-2947, :2961-2972): std_pt over the x and the y of pl, std_ls over the midpoints
 * (spl + epl) * 0.5.  Host arrays [n][2]; zero rows give 0/0 as in the reference (NaN).      */
typedef struct gfpl_bow_stats { int32_t n_pt, n_ls; double std_pt, std_ls; } gfpl_bow_stats;
int  gfpl_kf_bow_stats(const double* pl, int n_pt, const double* spl, const double* epl, int n_ls,
                       gfpl_bow_stats* out);

#define GFPL_BOW_MODE_P  0   /* insertKFBowVectorP  */
#define GFPL_BOW_MODE_L  1   /* insertKFBowVectorL  */
#define GFPL_BOW_MODE_PL 2   /* insertKFBowVectorPL */
/* The BowVectors of up to kf_cap keyframes, resident on the device (KeyFrame::descDBoW_P / _L).
 * voc_l may be NULL in mode P and voc_p in mode L; pt_cap / ls_cap: descriptor rows per keyframe
 * (<= GFPL_BOW_MAX_CAP).  The vocabularies must outlive the database.                        */
int  gfpl_bowdb_create(gfpl_ctx* ctx, const gfpl_vocab* voc_p, const gfpl_vocab* voc_l, int mode, int kf_cap,
                       int pt_cap, int ls_cap, gfpl_bowdb** out);
int  gfpl_bowdb_destroy(gfpl_bowdb* db);
/* insertKFBowVectorP / L / PL for keyframe kf_idx: transforms kf's pdesc / ldesc (only n_pt / pdesc
 * and n_ls / ldesc of the view are read), stores the vectors, scores them against every stored
 * keyframe i < kf_idx in one launch and writes row[i] (HOST, kf_idx + 1 doubles: conf_matrix[kf_idx][i])
 * for those i and for i = kf_idx (the vector against itself); entries of erased or never-inserted
 * keyframes are left as they are.  Mode PL combines the two scores as :2986-2988 do with stats
 * (required in mode PL, of the NEW keyframe; ignored otherwise).  kf_idx = 0 stores the vectors and
 * writes row[0] = 1.0 (MapHandler::initialize).  GFPL_E_INVALID for an index that is negative or was
 * inserted before, GFPL_E_CAPACITY for kf_idx >= kf_cap or more rows than pt_cap / ls_cap.
 * Synchronises.                                                                                */
int  gfpl_bowdb_insert(gfpl_bowdb* db, int kf_idx, const gfpl_kf_view* kf, const gfpl_bow_stats* stats, double* row);
/* map_keyframes[kf_idx] = NULL as the database sees it: later inserts skip it                  */
int  gfpl_bowdb_erase(gfpl_bowdb* db, int kf_idx);
/* the stored vector of a live keyframe; kind 0 = points (descDBoW_P), 1 = lines (descDBoW_L): the
 * device triple in *out and, where ids_host / values_host are not NULL, a host copy of its
 * out->count entries (the copy synchronises)                                                    */
int  gfpl_bowdb_vector(const gfpl_bowdb* db, int kind, int kf_idx, gfpl_bow_vec* out, int32_t* ids_host,
                       double* values_host);

/* Config::lcKFDist, lcKFMaxDist, lcNKFClosest, minLMCovGraph, minKFLocalMap                    */
typedef struct gfpl_lc_search_params {
    int32_t lc_kf_dist, lc_kf_max_dist, lc_nkf_closest, min_lm_cov_graph, min_kf_local_map;
} gfpl_lc_search_params;
/* 100, 20, 4, 30, 3 (src/config.cpp:68-70, 51, 53) */
void gfpl_default_lc_search_params(gfpl_lc_search_params* prm);
typedef struct gfpl_lc_search_info {
    double  lc_min_score;
    int32_t nkf_closest, idx_max;   /* idx_max = -1 when the size gate fails                     */
    int32_t n_list, pad;            /* entries of max_confmat                                    */
} gfpl_lc_search_info;
/* MapHandler::lookForLoopCandidates (:3002-3076), host only: conf_col[i] = conf_matrix[i][kf_curr_idx],
 * alive[i] != 0 where map_keyframes[i] != NULL, graph_col[i] = full_graph[i][kf_curr_idx], each of
 * kf_curr_idx entries.  std::sort orders the list, so equal scores fall as they do in the reference.
 * Returns 1 (candidate, *kf_prev_idx set) or 0 (*kf_prev_idx = -1); GFPL_E_INVALID for a NULL
 * pointer, kf_curr_idx < 0 or a negative parameter.  info may be NULL.                          */
int  gfpl_kf_loop_candidates(const double* conf_col, const uint8_t* alive, const int32_t* graph_col,
                             int kf_curr_idx, const gfpl_lc_search_params* prm, int* kf_prev_idx,
                             gfpl_lc_search_info* info);

/* ------------------------------------------- local bundle adjustment ----- */
/* MapHandler::localBundleAdjustment's solver levMarquardtOptimizationLBA (src/mapHandler.cpp:
 * 1217-1713) for n problems in one call, one workgroup each (k_lba.hip).  The linearisation, the
 * accumulation of H, g and err, Hmax, the damping, the stop tests and the lambda rule are the
 * reference's, quirks included (DESIGN.md ledger BA1-BA14): H, g and err of every iteration
 * have its bits.  The solve is pinned to our own elimination (landmark blocks first, then a dense
 * LDL^T of the reduced pose system without pivoting), not to Eigen's SimplicialLDLT.          */
#define GFPL_LBA_MAX_KFS 16   /* local keyframes per problem: the reduced system (96 x 96 doubles) and a
                                 chunk of observation rows share one workgroup's LDS (LbaLds)  */
typedef struct gfpl_lba gfpl_lba;
/* Config::lambdaLbaLM, lambdaLbaK, maxItersLba: 0.001, 10.0, 20 (src/config.cpp:55-57) */
typedef struct gfpl_lba_params { double lambda_lm, lambda_k; int32_t max_iters, pad; } gfpl_lba_params;
void gfpl_default_lba_params(gfpl_lba_params* prm);
typedef struct gfpl_lba_counts { int32_t n_kf, n_fix, n_pt, n_ls, n_pt_obs, n_ls_obs; } gfpl_lba_counts;
/* One problem.  The doubles are DEVICE arrays, the four index arrays HOST arrays (they are the
 * caller's graph bookkeeping; the call checks them before any device work and uploads them).
 * X = [x_kf | pt | ls] as the reference lays it out.  x_kf is where X starts and T_kf where the
 * first linearisation is taken: KeyFrame::x_kf_w and KeyFrame::T_kf_w, which the reference reads
 * separately and which may differ.  An observation's keyframe slot s >= 0 names local keyframe s,
 * s < 0 the fixed pose -1 - s (a keyframe outside the list, keyframe 0 included).  A landmark's
 * observations are contiguous: *_obs_lm starts at 0 and rises in steps of 0 or 1 to n - 1.      */
typedef struct gfpl_lba_problem {
    gfpl_lba_counts n;
    const double*  x_kf;        /* [n_kf][6]  in                                               */
    double*        T_kf;        /* [n_kf][16] in: T_kf_w; out: expmap_se3(X)                   */
    const double*  T_fix;       /* [n_fix][16]                                                 */
    double*        pt;          /* [n_pt][3]  in / out: point3D                                */
    double*        ls;          /* [n_ls][6]  in / out: line3D                                 */
    const double*  pt_obs;      /* [n_pt_obs][2]                                               */
    const double*  pt_sigma;    /* [n_pt_obs] sigma_list                                       */
    const double*  ls_obs;      /* [n_ls_obs][3]                                               */
    const double*  ls_sigma;    /* [n_ls_obs]                                                  */
    double*        x_out;       /* [n_kf][6]  out: the pose part of X at exit, or NULL         */
    const int32_t* pt_obs_lm;   /* HOST [n_pt_obs] local landmark                              */
    const int32_t* pt_obs_kf;   /* HOST [n_pt_obs] keyframe slot                               */
    const int32_t* ls_obs_lm;   /* HOST [n_ls_obs]                                             */
    const int32_t* ls_obs_kf;   /* HOST [n_ls_obs]                                             */
} gfpl_lba_problem;
#define GFPL_LBA_STOP_ITERS 0   /* the loop ran out of iterations                              */
#define GFPL_LBA_STOP_DERR  1   /* |err - err_prev| < DBL_EPSILON                              */
#define GFPL_LBA_STOP_ERR   2   /* err < DBL_EPSILON                                           */
#define GFPL_LBA_STOP_STEP  3   /* |DX| < DBL_EPSILON                                          */
#define GFPL_LBA_SINGULAR   1   /* status: a pivot that is not positive and finite; that step is dropped */
#define GFPL_LBA_HMAX_RANGE 2   /* status: a diagonal of H >= 2^31 (int Hmax overflows in the reference);
                                   nothing is written but the result record                    */
typedef struct gfpl_lba_result {
    int32_t iters, stop, status, hmax;   /* iters: the reference's loop variable at exit       */
    double  lambda, err, err_prev;
} gfpl_lba_result;
/* Host only, no device: GFPL_E_INVALID for a NULL problem, n_kf < 1, a negative count, no
 * observation at all, a missing index array, landmark ids that do not start at 0, do not rise in
 * steps of 0 or 1 or do not end at n - 1 (every landmark needs an observation), or a keyframe slot
 * outside [-n_fix, n_kf); GFPL_E_CAPACITY for n_kf > GFPL_LBA_MAX_KFS.                         */
int  gfpl_lba_check(const gfpl_lba_problem* p);
/* Host only: the device workspace one problem of these counts takes and the kernel's dynamic LDS. */
int  gfpl_lba_workspace(const gfpl_lba_counts* n, int64_t* hbm_bytes, int32_t* lds_bytes);
/* caps: the largest counts of one problem; room for max_problems of them.  The context needs a
 * camera (GFPL_E_STATE) and cannot be destroyed while the object lives.                        */
int  gfpl_lba_create(gfpl_ctx* ctx, const gfpl_lba_counts* caps, int max_problems, gfpl_lba** out);
int  gfpl_lba_destroy(gfpl_lba* lba);
/* problems, results: HOST arrays of n.  Every problem is checked (gfpl_lba_check) before any device
 * work; GFPL_E_CAPACITY when n or a count exceeds what the object was created for.  homog_th and the
 * camera are the context's.  Synchronises once, for the results.                               */
int  gfpl_lba_solve(gfpl_lba* lba, const gfpl_lba_problem* problems, int n, const gfpl_lba_params* prm,
                    gfpl_lba_result* results);
/* Test hook: the undamped system of the LAST iteration problem i of the last gfpl_lba_solve
 * evaluated (iteration 0 is the pre-pass; a call with max_iters = k + 1 leaves iteration k unless
 * it stopped earlier).  GFPL_E_STATE when that is not `iteration`.  HOST outputs, any may be NULL:
 * U [n_kf][6][6], g [6 n_kf + 3 n_pt + 6 n_ls], V_pt [n_pt][3][3], V_ls [n_ls][6][6], W_pt
 * [n_pt][n_kf][3][6] and W_ls [n_ls][n_kf][6][6] (landmark rows, pose columns: H.block(jdx, idx)),
 * err (after the division).                                                                    */
int  gfpl_lba_debug_system(gfpl_lba* lba, int i, int iteration, double* U, double* g, double* V_pt, double* V_ls,
                           double* W_pt, double* W_ls, double* err);

/* ------------------------------------------ global bundle adjustment ----- */
/* MapHandler::globalBundleAdjustment's solver levMarquardtOptimizationGBA (src/mapHandler.cpp:
 * 1950-2544) over a whole map: one problem spreads over the device, phase by phase, as separate
 * launches in stream order (k_gba.hip).  A problem is a gfpl_lba_problem: the local
 * keyframes are every alive keyframe but keyframe 0 (:1851-1863), keyframe 0 is a fixed pose, and
 * an observation whose keyframe is dead is left out by the caller (:1981).  H, g and err of every
 * iteration have the reference's bits, its quirks included (ledger GB1-GB12): err is divided by
 * counters that stay 0, so it is +inf or NaN, no error stop fires and every step is applied; the
 * pre-pass writes a line's coupling block transposed, so its system can be indefinite.  The solve
 * is the project's own elimination (landmark blocks first, each through its own LDL^T, then a dense
 * LDL^T of the reduced pose system without pivoting), reading the lower triangle of H as
 * SimplicialLDLT does.                                                                          */
#define GFPL_GBA_MAX_KFS 256  /* local keyframes per problem.  Bounded by the dense reduced system S in
                                 HBM ((6 n_kf)^2 doubles: 18.9 MB at 256, four times that at 512) and by
                                 the time of its factorisation (n_kf launches of O(n_kf^2) work each per
                                 iteration: cubic in n_kf, about 20 iterations per solve)          */
typedef struct gfpl_gba gfpl_gba;
typedef gfpl_lba_params gfpl_gba_params;    /* the GBA reads lambdaLbaLM, lambdaLbaK, maxItersLba (:1965-1966) */
typedef gfpl_lba_result gfpl_gba_result;
void gfpl_default_gba_params(gfpl_gba_params* prm);
/* n: a problem's counts; n_pt_pairs / n_ls_pairs: (landmark, distinct local keyframe) pairs of the
 * points / lines, one W and one Y block each; n_terms: contributing terms of S, one per landmark
 * and lower block (a >= b) whose two keyframes both observe it.                                 */
typedef struct gfpl_gba_counts { gfpl_lba_counts n; int32_t n_pt_pairs, n_ls_pairs, n_terms, pad; } gfpl_gba_counts;
#define GFPL_GBA_STOP_ITERS 0
#define GFPL_GBA_STOP_DERR  1   /* cannot fire: err is +inf or NaN (ledger GB3)                 */
#define GFPL_GBA_STOP_ERR   2   /* cannot fire                                                  */
#define GFPL_GBA_STOP_STEP  3   /* |DX| < DBL_EPSILON                                           */
#define GFPL_GBA_SINGULAR   1   /* status: a zero or non-finite pivot of S, or a damped landmark diagonal or a
                                   pivot of a landmark block that is not positive and finite; that step is dropped */
#define GFPL_GBA_HMAX_RANGE 2   /* status: as GFPL_LBA_HMAX_RANGE                               */
#define GFPL_GBA_INDEFINITE 4   /* status, informational: a negative pivot of S was accepted    */
/* Host only, no device: everything gfpl_lba_check refuses, with GFPL_E_CAPACITY for n_kf >
 * GFPL_GBA_MAX_KFS or a pair / term count beyond 32 bits; counts (may be NULL) is what the problem
 * takes of a gfpl_gba object.                                                                   */
int  gfpl_gba_check(const gfpl_lba_problem* p, gfpl_gba_counts* counts);
/* Host only: the device workspace one problem of these counts takes and the largest dynamic LDS of
 * any kernel.                                                                                   */
int  gfpl_gba_workspace(const gfpl_gba_counts* n, int64_t* hbm_bytes, int32_t* lds_bytes);
/* caps: the largest counts of one problem; room for max_problems of them.  The context needs a
 * camera (GFPL_E_STATE) and cannot be destroyed while the object lives.                        */
int  gfpl_gba_create(gfpl_ctx* ctx, const gfpl_gba_counts* caps, int max_problems, gfpl_gba** out);
int  gfpl_gba_destroy(gfpl_gba* gba);
/* problems, results: HOST arrays of n.  Every problem is checked and planned before any device
 * work; GFPL_E_CAPACITY when n or a count exceeds the caps; a refused call changes nothing.  The
 * problems run one after another in stream order; the call synchronises once.  After GFPL_E_HIP the
 * map's contents are unknown and the object returns GFPL_E_STATE until it is destroyed.         */
int  gfpl_gba_solve(gfpl_gba* gba, const gfpl_lba_problem* problems, int n, const gfpl_gba_params* prm,
                    gfpl_gba_result* results);
/* Test hook, as gfpl_lba_debug_system, of the LAST iteration problem i evaluated.  W_pt [point
 * pairs][3][6] and W_ls [line pairs][6][6] are the coupling blocks under the diagonal (landmark rows,
 * pose columns), one per pair in the planner's order; pairs [n_pt_pairs + n_ls_pairs][2] = (landmark in the unified
 * numbering, points first; local keyframe).  Iteration 0 shows the transposed line blocks.       */
int  gfpl_gba_debug_system(gfpl_gba* gba, int i, int iteration, double* U, double* g, double* V_pt, double* V_ls,
                           double* W_pt, double* W_ls, int32_t* pairs, double* err);

/* ------------------------------------- the map's geometry half ---------- */
/* What MapPoint / MapLine / KeyFrame hold beside the indices and the descriptors, as a third device
 * object per map (k_mapgeo.hip, gfpl_mapgeo.cpp, DESIGN.md §4n, ledger MG1-MG7), created with the
 * gfpl_kfmap's caps and indexed by its ids: per keyframe T_kf_w [kf_cap][16] and x_kf_w [kf_cap][6]
 * (gfpl_pgo_problem's T_kf / x_kf layout), per landmark point3D [pt_lm_cap][3] / line3D
 * [ls_lm_cap][6] (gfpl_pgo_problem's pt / ls layout), n_obs, obs_list at a stride of obs_cap (2
 * doubles per point observation: pl; 3 per line observation: le) and sigma_list at the same stride.
 * Entry i of a landmark's obs / sigma belongs to entry i of the gfpl_kfmap's kf_obs: after a pair of
 * matching calls on the two objects their n_obs agree.  dir_list, pts_list and med_obs_dir are not
 * kept (nothing on this path reads them); desc_list is gfpl_lmstore's.
 * The contract is gfpl_kfmap's: host checks first; one synchronisation per call unless stated; a
 * refused call changes nothing; bad device data is never used as an index; GFPL_E_INVALID wins over
 * GFPL_E_CAPACITY; GFPL_E_STATE from every call after a GFPL_E_HIP.                              */
typedef struct gfpl_mapgeo gfpl_mapgeo;
/* Host only: the device bytes of an object with these caps, -1 for caps gfpl_kfmap_create refuses. */
int64_t gfpl_mapgeo_bytes(const gfpl_kfmap_caps* caps);
/* Every n_obs 0, every double 0.  The context cannot be destroyed while the object lives.          */
int  gfpl_mapgeo_create(gfpl_ctx* ctx, const gfpl_kfmap_caps* caps, gfpl_mapgeo** out);
int  gfpl_mapgeo_destroy(gfpl_mapgeo* g);
/* addKeyFrame storing the tracker's pose: T_kf_w [16] and x_kf_w [6], HOST doubles; kf in [0, kf_cap). */
int  gfpl_mapgeo_set_keyframe(gfpl_mapgeo* g, int kf, const double* T_kf_w, const double* x_kf_w);
int  gfpl_mapgeo_read_keyframe(gfpl_mapgeo* g, int kf, double* T_kf_w, double* x_kf_w);   /* HOST; either may be NULL */
/* The DEVICE arrays of the store, fixed for its lifetime (any may be NULL): gfpl_pgo_solve and
 * gfpl_map_fuse_search work on them in place.  No synchronisation.                                 */
int  gfpl_mapgeo_arrays(gfpl_mapgeo* g, double** T_kf, double** x_kf, double** point3D, double** line3D);
/* The geometry half of lookForCommonMatches' keyframe-pair loop body (src/mapHandler.cpp:270-335,
 * :407-480).  pairs, lm_out and first_new are what gfpl_kfmap_observe_pairs took and returned; v0 / v1
 * are kf0's / kf1's views with DEVICE arrays, of which kind 0 reads P and pl, kind 1 sP, eP and le
 * (v0's 3D arrays, both views' observations).  A created landmark (lm_out[i] >= first_new) gets
 * point3D = T_kf_w(kf0) P0 (line3D = [T sP0, T eP0]) with the STORE's pose of kf0, obs = [pl0, pl1]
 * ([le0, le1]), sigma = [1, 1] (the constructor's and addMap*Observation's default), n_obs = 2.  A
 * carried landmark appends pl1 / le1 and 1.0 at place n_obs before the call + the number of pairs
 * j < i with lm_out[j] == lm_out[i]: the reference's order when two kf0 rows carry one landmark.
 * lm_out[i] == -1 does nothing (:308).
 * GFPL_E_INVALID: a NULL pointer, kind outside 0..1, n < 0, a keyframe outside [0, kf_cap), kf0 == kf1,
 * kf0 without a pose (gfpl_mapgeo_set_keyframe), first_new outside [0, lm cap], a NULL or not 8-byte
 * aligned array of the kind that is read, n above either view's rows or the caps' rows, a pair row
 * outside its view, an lm_out value outside [-1, lm cap), a created id whose n_obs is not 0 or that two
 * pairs name, a carried id whose n_obs is 0.  GFPL_E_CAPACITY: a list beyond obs_cap.              */
int  gfpl_mapgeo_observe_pairs(gfpl_mapgeo* g, int kind, int kf0, int kf1, const gfpl_kf_view* v0, const gfpl_kf_view* v1,
                               const int32_t* pairs /*DEVICE [n][2]*/, const int32_t* lm_out /*DEVICE [n]*/, int n, int first_new);
/* The local-map stage (:609-615, :745-764): landmark lm_out[i] receives pl / le of kf1's row
 * unm_rows[pairs[i][1]] and 1.0; place rule and refusals as above (pairs[i][1] outside [0, n_unm) or a
 * row outside v1 is GFPL_E_INVALID; column 0 of pairs is not read).                                */
int  gfpl_mapgeo_observe_local(gfpl_mapgeo* g, int kind, int kf1, const gfpl_kf_view* v1, const int32_t* pairs /*DEVICE [n][2]*/,
                               int n, const int32_t* unm_rows /*DEVICE [n_unm]*/, int n_unm, const int32_t* lm_out /*DEVICE [n]*/);
/* n_obs = 0 of the landmarks gfpl_kfmap_remove_bad listed (ledger MG3: no single observation is ever
 * erased).  GFPL_E_INVALID for an id outside [0, lm cap) or n outside [0, lm cap].                  */
int  gfpl_mapgeo_free(gfpl_mapgeo* g, int kind, const int32_t* ids /*DEVICE [n]*/, int n);
/* Read and patch, HOST arrays, ids [id0, id0 + n) below the cap: lm3d [n][3 or 6], n_obs [n], obs
 * [n][obs_cap][2 or 3], sigma [n][obs_cap].  Reads: any output may be NULL.  Writes take every array;
 * GFPL_E_INVALID for an n_obs outside [0, obs_cap].                                                */
int  gfpl_mapgeo_read_landmarks(gfpl_mapgeo* g, int kind, int id0, int n, double* lm3d, int32_t* n_obs, double* obs, double* sigma);
int  gfpl_mapgeo_write_landmarks(gfpl_mapgeo* g, int kind, int id0, int n, const double* lm3d, const int32_t* n_obs,
                                 const double* obs, const double* sigma);
/* HOST copies of an assembled problem's four index lists, each with room for cap_* entries.        */
typedef struct gfpl_mapgeo_lists {
    int32_t *pt_obs_lm, *pt_obs_kf;   /* [cap_pt_obs] */
    int32_t *ls_obs_lm, *ls_obs_kf;   /* [cap_ls_obs] */
    int32_t cap_pt_obs, cap_ls_obs;
} gfpl_mapgeo_lists;
/* The three gathering loops of localBundleAdjustment (:1113-1209, which = GFPL_KFMAP_LOCAL) or
 * globalBundleAdjustment (:1851-1939, GFPL_KFMAP_ALIVE) on the device, into the object's own buffers;
 * *problem's double arrays point at them (valid until the next assemble / lba call).  The keyframe
 * list is alive && local && kf_idx != 0 ascending (ALIVE: every alive keyframe but 0); landmarks in map
 * order, their observations in list order.  An observation's slot is its keyframe's position in the
 * list, else -1 - (its position among the fixed keyframes): the alive keyframes outside the list that a
 * selected landmark's kf_obs names, in ascending index (MG4).  An observation of an erased keyframe is
 * dropped and a landmark left with none is left out (:1981; for the LBA ledger MG5).  kfmap must have
 * the object's caps and context.  GFPL_E_INVALID also when a selected landmark's n_obs differs between
 * the two objects.  With lists, the four index lists are copied to the host in a second
 * synchronisation and *problem names them, so gfpl_lba_solve / gfpl_gba_check / gfpl_gba_solve take
 * *problem as it is; GFPL_E_CAPACITY when a list does not fit (problem->n is still set).  Without
 * lists the problem's index pointers are NULL.  Only workspace is written.                         */
int  gfpl_mapgeo_assemble(gfpl_mapgeo* g, const gfpl_kfmap* kfmap, int which, gfpl_lba_problem* problem,
                          const gfpl_mapgeo_lists* lists);
/* The DEVICE lists of the last assembly's selected ids, for a scatter of a solver's results: kf_list
 * [n_kf], fix_list [n_fix], pt_list [n_pt], ls_list [n_ls] (any may be NULL).  No synchronisation.  */
int  gfpl_mapgeo_assembled_ids(gfpl_mapgeo* g, const int32_t** kf_list, const int32_t** fix_list, const int32_t** pt_list,
                               const int32_t** ls_list);
/* Read hook: the last assembly's arrays to the HOST.  host's nine double pointers (x_kf ... ls_sigma) name
 * HOST arrays of the last assembly's counts to fill; its other fields are not read.  host and every
 * list may be NULL.  After gfpl_mapgeo_lba the doubles are the solver's outputs.                   */
int  gfpl_mapgeo_read_assembled(gfpl_mapgeo* g, const gfpl_lba_problem* host, int32_t* kf_list, int32_t* fix_list,
                                int32_t* pt_list, int32_t* ls_list);
/* The whole of localBundleAdjustment: assemble GFPL_KFMAP_LOCAL, solve on lba (the assembled index
 * lists reach the solver's workspace on the device), write T_kf_w of the listed keyframes and point3D /
 * line3D of the listed landmarks back (:1688-1712; x_kf_w is not refreshed, BA1).  Two
 * synchronisations (counts, result).  No observation: nothing is solved, GFPL_OK, *result zero
 * (:1212).  GFPL_E_CAPACITY for more than GFPL_LBA_MAX_KFS local keyframes or counts above lba's caps,
 * GFPL_E_INVALID for observations without a local keyframe (MG6), lba of another context; nothing is
 * written then.  counts (may be NULL) receives the assembled counts whenever the assembly ran.     */
int  gfpl_mapgeo_lba(gfpl_mapgeo* g, const gfpl_kfmap* kfmap, gfpl_lba* lba, const gfpl_lba_params* prm,
                     gfpl_lba_result* result, gfpl_lba_counts* counts);
/* Instrumentation (tools/bench_mapgeo.py): device milliseconds between the first and the last kernel
 * of the object's last observe / free / assemble call (for gfpl_mapgeo_lba: its assembly);
 * GFPL_E_STATE when there is none.                                                                */
int  gfpl_mapgeo_debug_ms(gfpl_mapgeo* g, float* ms);

/* ------------------------------------------- loop-closure pose graph ----- */
/* MapHandler::loopClosureOptimizationCovGraphG2O / EssGraphG2O (src/mapHandler.cpp:4187-4419,
 * :3950-4184) for n problems in one call: the pose graph over the keyframes, its
 * Levenberg-Marquardt solve (k_pgo, one workgroup per problem) and the rigid correction of every
 * keyframe pose and every landmark that hangs on it (k_pgo_correct).  The graph (vertices, flags,
 * edge order), the measurements, the start poses and the map correction are the reference's.  The
 * objective and the iteration are pinned by DESIGN.md §4j (ledger PG1-PG8), not by g2o, which the
 * reference tree does not contain.  loopClosureFuseLandmarks, which follows the solve, has its
 * descriptor half in gfpl_lmstore_fuse (the list walk stays the caller's).
 * Not here: per-edge information matrices (the reference passes identity); globalBundleAdjustment
 * is gfpl_gba_solve.                                                                            */
#define GFPL_PGO_COV 0          /* loopClosureOptimizationCovGraphG2O */
#define GFPL_PGO_ESS 1          /* loopClosureOptimizationEssGraphG2O */
typedef struct gfpl_pgo gfpl_pgo;
/* Config::minLMEssGraph, minLMCovGraph (100, 30: src/config.cpp:50-51), the variant, and the
 * iteration: optimize(100), setUserLambdaInit(1e-10), at most max_rejects damped retries of a step */
typedef struct gfpl_pgo_graph_params {
    int32_t min_lm_ess_graph, min_lm_cov_graph, variant, max_iters, max_rejects, pad;
    double  lambda_init;
} gfpl_pgo_graph_params;
void gfpl_default_pgo_params(gfpl_pgo_graph_params* prm);   /* 100, 30, COV, 100, 10, 1e-10 */
/* What a problem takes: keyframes, loop entries, vertices, free vertices, edges, 6 x 6 blocks of the
 * envelope (row r of the free system is stored from its first column f(r) to r), and the landmarks
 * of the point / line ownership lists that are not freed.  As caps of gfpl_pgo_create only n_kf,
 * n_lc, n_edge, env_blocks, n_pt and n_ls are read (n_vert, n_free <= n_kf).                    */
typedef struct gfpl_pgo_counts { int32_t n_kf, n_lc, n_vert, n_free, n_edge, env_blocks, n_pt, n_ls; } gfpl_pgo_counts;
/* One problem.  The doubles of the map are DEVICE arrays, in and out; the index arrays, the loop
 * list and lc_pose are HOST arrays (the caller's graph bookkeeping; checked before any device work
 * and uploaded).  A landmark belongs to one keyframe: *_kf_idx[*_kf_start[i] .. *_kf_start[i + 1])
 * are map_points_kf_idx[i] / map_lines_kf_idx[i]; an entry < 0, or one whose *_freed byte is set, is a
 * freed landmark (map_points[.] == NULL) and is skipped.  *_dir: every landmark's dir_list rows in
 * one array, landmark j's at rows [*_dir_off[j], *_dir_off[j + 1]); NULL (both) when the caller
 * does not keep them on the device.  med_obs_dir is not provided (ledger LM6).                  */
typedef struct gfpl_pgo_problem {
    int32_t        n_kf, n_lc;      /* map_keyframes.size(), lc_idx_list.size()                    */
    int32_t        n_pt, n_ls;      /* rows of pt / ls (the landmark ids of the lists are < these) */
    const uint8_t* alive;           /* HOST [n_kf]: map_keyframes[i] != NULL                       */
    const int32_t* full_graph;      /* HOST [n_kf][n_kf]                                           */
    const int32_t* lc;              /* HOST [n_lc][3]: kf_prev, kf_curr, flag                      */
    const double*  lc_pose;         /* HOST [n_lc][6]: lc_pose_list                                */
    double*        T_kf;            /* [n_kf][16] in / out: T_kf_w                                 */
    double*        x_kf;            /* [n_kf][6]  out: x_kf_w of every keyframe the call moved     */
    double*        pt;              /* [n_pt][3]  in / out: point3D (may be NULL when n_pt = 0)    */
    double*        ls;              /* [n_ls][6]  in / out: line3D                                 */
    double*        pt_dir;          /* [.][3]     in / out, or NULL                                */
    double*        ls_dir;          /* [.][3]     in / out, or NULL                                */
    const int32_t* pt_kf_start;     /* HOST [n_kf + 1], or NULL when n_pt = 0                      */
    const int32_t* pt_kf_idx;       /* HOST [pt_kf_start[n_kf]]                                    */
    const int32_t* ls_kf_start;     /* HOST [n_kf + 1], or NULL when n_ls = 0                      */
    const int32_t* ls_kf_idx;       /* HOST [ls_kf_start[n_kf]]                                    */
    const int32_t* pt_dir_off;      /* HOST [n_pt + 1], read when pt_dir is given                  */
    const int32_t* ls_dir_off;      /* HOST [n_ls + 1], read when ls_dir is given                  */
    const uint8_t* pt_freed;        /* HOST [n_pt] or NULL                                         */
    const uint8_t* ls_freed;        /* HOST [n_ls] or NULL                                         */
} gfpl_pgo_problem;
#define GFPL_PGO_STOP_ITERS  0  /* max_iters iterations ran                                        */
#define GFPL_PGO_STOP_STEP   1  /* |delta|_inf <= 64 DBL_EPSILON: the step is not applied          */
#define GFPL_PGO_STOP_DCHI2  2  /* an accepted step lowered chi2 by <= 64 DBL_EPSILON chi2         */
#define GFPL_PGO_STOP_REJECT 3  /* max_rejects trials of one iteration were rejected               */
#define GFPL_PGO_STOP_NOFREE 4  /* no free vertex: nothing to solve (iters = 0)                    */
#define GFPL_PGO_SINGULAR    1  /* status: a pivot that was not positive and finite (a rejected trial) */
typedef struct gfpl_pgo_result {
    int32_t iters, stop, status, rejects;   /* rejects: rejected trials over the whole solve       */
    int32_t n_vert, n_free, n_edge, kf_curr;
    double  lambda, chi2_0, chi2;
} gfpl_pgo_result;
/* Host only, no device.  Builds the graph and returns its counts (may be NULL).  GFPL_E_INVALID: a
 * NULL pointer, n_kf < 1, an empty loop list, a loop entry outside [0, n_kf) or with kf_prev >=
 * kf_curr, a dead keyframe named by a loop entry, keyframe 0 dead in COV, a negative threshold, a
 * variant other than COV / ESS, an ownership list that does not ascend from 0, names a landmark
 * >= n_pt / n_ls or names one twice, dir offsets that do not ascend from 0.                     */
int  gfpl_pgo_check(const gfpl_pgo_problem* p, const gfpl_pgo_graph_params* prm, gfpl_pgo_counts* counts);
/* Host only: the device workspace one problem of these counts takes and the kernel's dynamic LDS. */
int  gfpl_pgo_workspace(const gfpl_pgo_counts* n, int64_t* hbm_bytes, int32_t* lds_bytes);
/* caps: the largest counts of one problem; room for max_problems of them.  The context cannot be
 * destroyed while the object lives.                                                             */
int  gfpl_pgo_create(gfpl_ctx* ctx, const gfpl_pgo_counts* caps, int max_problems, gfpl_pgo** out);
int  gfpl_pgo_destroy(gfpl_pgo* pgo);
/* problems, results: HOST arrays of n.  Every problem is checked (gfpl_pgo_check) before any device
 * work; GFPL_E_CAPACITY when n or a count exceeds what the object was created for; a refused call
 * changes nothing and leaves the object usable.  Synchronises once.  GFPL_E_HIP from a copy, launch
 * or synchronisation leaves the map's contents unknown: solve and the debug calls return
 * GFPL_E_STATE from then on and the object can only be destroyed.                               */
int  gfpl_pgo_solve(gfpl_pgo* pgo, const gfpl_pgo_problem* problems, int n, const gfpl_pgo_graph_params* prm,
                    gfpl_pgo_result* results);
/* Test hook: problem i of the last gfpl_pgo_solve, which must have run with max_iters = 1 so that
 * the system it leaves is iteration 0's (GFPL_E_STATE otherwise, or when that solve had fewer
 * problems).  HOST outputs, any may be NULL: chi2 and b [6 n_free], diag [n_free][6][6], env
 * [env_blocks][6][6] (the undamped envelope rows; row r's last block is the zeroed place of its
 * diagonal block), env_first [n_free], vert [n_vert][4] (keyframe, flags: bit 0 fixed, 1 is_lc_j,
 * 2 is_lc_i, lc_id or -1, free index or -1), edge [n_edge][4] (vertex i, vertex j, loop entry or
 * -1, 0), Z [n_edge][16], X0 [n_vert][16] (the start poses).  With no free vertex nothing of the
 * system but chi2 is written.                                                                   */
int  gfpl_pgo_debug_system(gfpl_pgo* pgo, int i, double* chi2, double* b, double* diag, double* env,
                           int32_t* env_first, int32_t* vert, int32_t* edge, double* Z, double* X0);
/* Instrumentation (tools/bench_pgo.py): device milliseconds of k_pgo and of k_pgo_correct in the
 * last solve; GFPL_E_STATE when there is none.                                                  */
int  gfpl_pgo_debug_ms(gfpl_pgo* pgo, float* ms_solve, float* ms_correct);

/* ----------------------------------------------------- state transfer ----- */
/* Copy one sequence's frame state device -> host (synchronises).            */
int  gfpl_read_frame(gfpl_seqbatch* sb, int which, int seq, gfpl_frame_host* out);
/* Copy a host frame state into one sequence (synchronises).  Used to start a
 * stage from a given state (e.g. the oracle's), like the reference's
 * simulators build frames through the public members (src/simulate_line_cut.cpp:62-212). */
int  gfpl_write_frame(gfpl_seqbatch* sb, int which, int seq, const gfpl_frame_host* in);
int  gfpl_read_track(gfpl_seqbatch* sb, int seq, gfpl_track_host* out);
/* GFPL_E_CAPACITY for a list longer than the seqbatch's match budget, GFPL_E_INVALID for a matched
 * index outside [0, kp_cap) / [0, kl_cap) (the pose solver and the line cut gather prev-frame
 * records by these indices); checked on the host before anything is copied.                  */
int  gfpl_write_track(gfpl_seqbatch* sb, int seq, const gfpl_track_host* in);
/* The track of the step before the last gfpl_update_frame / gfpl_frame_step: the
 * matched lists it cleared (matched_pt.clear(), src/stereoFrameHandler.cpp:889-890)
 * as they stood, and the inlier counters.  Valid until the next insert; lets a
 * caller that drives gfpl_frame_step inspect each step without splitting it.  */
int  gfpl_read_last_track(gfpl_seqbatch* sb, int seq, gfpl_track_host* out);

/* ----------------------------------------------------- instrumentation ---- */
/* Per-stage device time of the last gfpl_frame_step (HIP events on the
 * context stream), ms: [stereo_points, stereo_lines, cross_points,
 * cross_lines, line_cut, pose, total].  Enable with gfpl_set_timing(ctx,1). */
int  gfpl_set_timing(gfpl_ctx* ctx, int enable);
int  gfpl_get_stage_times(gfpl_ctx* ctx, float* ms7);
/* Algorithmic bytes of the last step (SURVEY.md §8(d) formula, from runtime
 * counts, summed over the batch).  Synchronises.                           */
int  gfpl_last_step_bytes(gfpl_seqbatch* sb, int64_t* bytes);
/* ... per stage: [stereo_points, stereo_lines, cross_points, cross_lines,
 * line_cut, pose, total] (DESIGN.md §Roofline gives each stage's formula). */
int  gfpl_last_step_stage_bytes(gfpl_seqbatch* sb, int64_t* bytes7);
/* The counts those bytes are priced on, summed over the batch: [N_o (keypoints, both
 * sides), N_k (keylines, both sides), M_o (left keypoints reaching the sub-pixel SAD),
 * S_p (stereo points of the new frame), S_l (its stereo lines), M_p (matched_pt), M_l
 * (matched_ls), n_inliers] of the last insert.  Synchronises.                   */
int  gfpl_last_step_counts(gfpl_seqbatch* sb, int64_t* counts8);
/* More of the last step, summed over the batch: [line-cut greedy steps, steps the
 * certified search evaluated with the reference's own arithmetic (the exact fallback,
 * DESIGN.md §3), n_inliers after optimize_pose (removeOutliers; until it runs, the
 * insert's list sizes), searched lines whose agreement bound was unusable —
 * every step of such a line is exact].  Synchronises.                                */
int  gfpl_last_step_track_counts(gfpl_seqbatch* sb, int64_t* counts4);
/* Proven line cut (cut_proof 1) of the last step, summed over the batch: [sequences whose
 * recorded search k_cut_verify could not prove (their line cut was redone by the eager-proven
 * search), margined steps proven after the fact, the reference's endpoint variances evaluated
 * for them, lines with margined steps].  Zeros in the other modes.  Synchronises.        */
int  gfpl_last_step_cut_proof(gfpl_seqbatch* sb, int64_t* counts4);
/* Diagnostics: the line-cut records of sequence b's first n_lines matched lines of the last
 * insert (80 doubles each: comparison data, bounds, r = 0 info, the agreement bound as
 * k_cut_search formed it — DESIGN.md §3; layout in k_cut.hip).  Synchronises.      */
int  gfpl_debug_cut_records(gfpl_seqbatch* sb, int b, double* out, int n_lines);
/* Every sequence's record of the last step: B x GFPL_STEP_REC int64, the slots below (the
 * gfpl_last_step_* calls are their sums over the batch).  Synchronises.                     */
enum {
    /* algorithmic bytes per stage (gfpl_last_step_stage_bytes) and of k_cut_search alone */
    GFPL_STEP_B_STEREO_POINTS = 0,
    GFPL_STEP_B_STEREO_LINES = 1,
    GFPL_STEP_B_CROSS_POINTS = 2,
    GFPL_STEP_B_CROSS_LINES = 3,
    GFPL_STEP_B_LINE_CUT = 4,
    GFPL_STEP_B_POSE = 5,
    GFPL_STEP_B_TOTAL = 6,
    GFPL_STEP_B_CUT_SEARCH = 7,
    /* the counts they are priced on (gfpl_last_step_counts) */
    GFPL_STEP_N_O = 8,
    GFPL_STEP_N_K = 9,
    GFPL_STEP_M_O = 10,
    GFPL_STEP_S_P = 11,
    GFPL_STEP_S_L = 12,
    GFPL_STEP_M_P = 13,
    GFPL_STEP_M_L = 14,
    GFPL_STEP_N_INLIERS = 15,
    /* gfpl_last_step_track_counts */
    GFPL_STEP_CUT_STEPS = 16,      /* line-cut greedy steps */
    GFPL_STEP_CUT_EXACT = 17,      /* ... of them evaluated with the reference's arithmetic */
    GFPL_STEP_INLIERS_POSE = 18,   /* n_inliers after optimize_pose (until it runs: the insert's) */
    GFPL_STEP_CUT_UNBOUNDED = 19,  /* searched lines without a usable agreement bound */
    /* proven line cut, cut_proof 1 / 3 (gfpl_last_step_cut_proof); zero in a step without it */
    GFPL_STEP_PROOF_REDONE = 20,   /* 1: the recorded search was not proven and was redone eagerly */
    GFPL_STEP_PROOF_STEPS = 21,    /* margined steps proven after the fact */
    GFPL_STEP_PROOF_VREF = 22,     /* the reference's endpoint variances evaluated for them */
    GFPL_STEP_PROOF_LINES = 23,    /* lines with margined steps */
    GFPL_STEP_REC = 24
};
int  gfpl_debug_step_records(gfpl_seqbatch* sb, int64_t* out);
/* B x 8 int64 of diagnostic slots: the clocks instrumented builds of the library write (e.g.
 * -DGFPL_SP_CLOCK: k_stereo_points' phase boundaries); in every build, after a measured-mode step
 * with the 8-sequence-per-wave line-cut search, slots 6 / 7 hold that search wave's HW_ID / XCC_ID
 * (its SIMD and wave slot: the progress exchange's partner check).  Every writer of every build is
 * listed in csrc/gfpl_records.hpp.  Synchronises.                                                 */
int  gfpl_debug_clocks(gfpl_seqbatch* sb, int64_t* out);
/* Per-kernel view of the dominant stages (timing enabled, line cut on):
 * ms4 = device ms of [k_cut_prep, k_cut_search, k_cut_finish, k_pose] of the last
 * step (HIP events on the context stream); bytes4 = algorithmic bytes of the same
 * kernels, summed over the batch (each kernel's own inputs read once and
 * outputs written once; 0 for the cut kernels when the step ran no line cut).  */
int  gfpl_get_kernel_times(gfpl_ctx* ctx, float* ms4);
int  gfpl_last_step_kernel_bytes(gfpl_seqbatch* sb, int64_t* bytes4);

const char* gfpl_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* GFPL_H */
