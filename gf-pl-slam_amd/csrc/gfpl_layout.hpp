// gfpl_layout.hpp — every hand-laid-out buffer of the library, stated once.
//
// A layout is one function (or one struct's constructor), run to size and run to place: over a
// null base it yields only the total, over the real base the same takes yield the fields, so the
// size and the pointers cannot disagree.  Carver cuts one device allocation (HBM) into 256-B
// aligned fields; LdsCarver cuts a kernel's dynamic LDS, in the kernel over `smem` and in its
// launcher over null (`.bytes` is the launch's dynamic-LDS size).  Neither forms a pointer from a
// null base.  No HIP API and no device-only type here: a plain host program can include this file
// (tests/layout_check.cpp prints every layout).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define GFPL_HD __host__ __device__
#else
#define GFPL_HD
#endif

namespace gfpl {

// bump allocator over one device allocation (256-B aligned fields); base == nullptr: sizing pass
struct Carver {
    size_t off = 0;
    char* base = nullptr;
    template <typename T>
    T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

// the same over a kernel's dynamic LDS.  Fields are packed: only a take that names an alignment
// rounds the offset (rounding every take left address arithmetic in the kernels that the plain
// sums do not have), so a layout's order must keep every field naturally aligned; layout_check
// verifies that for every shape it prints.
struct LdsCarver {
    unsigned char* base;
    int off = 0;
    GFPL_HD explicit LdsCarver(unsigned char* b) : base(b) {}
    template <typename T>
    GFPL_HD T* take(int n, int align = 0) {
        if (align) off = (off + align - 1) & ~(align - 1);
#ifdef __HIP_DEVICE_COMPILE__
        T* p = reinterpret_cast<T*>(base + off);   // (a kernel's base is never null)
#else
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
#endif
        off += n * (int)sizeof(T);
        return p;
    }
};

// ---- constants the layouts share with their kernels
constexpr int SP_CHUNK = 32;      // sorted right-keypoint entries per staged descriptor chunk (k_stereo_points, SEG)
constexpr int SP_MINR_PAD = 32;   // minr bins span [-PAD, H + PAD) (k_stereo_points, SEG): every band is shorter
constexpr int CH_STRIDE = 66;     // doubles per GN chunk row (k_pose)
constexpr int LSD_RING = 256;     // region list entries mirrored in LDS (k_lsd_grow_*)
constexpr int KNN_CHUNK = 1024;   // train rows per staged chunk (k_knn2m)
// Expansion table for the train (A) side of the knn MFMA (gfpl_knn.hpp), one entry of FP4 nibbles
// per byte value: CELL 2: 2 dwords (4 one-hot cells, 16 nibbles); CELL 1: 1 dword (8 bits, 8 nibbles)
GFPL_HD constexpr int knn_lut_entry_dwords(int cell) { return cell == 2 ? 2 : 1; }
GFPL_HD constexpr int knn_lut_dwords(int cell) { return 256 * knn_lut_entry_dwords(cell); }

// Every layout below is a struct whose members are the takes, in order (members initialise in
// declaration order): pad_* are named slack the launch has always reserved, "= x" marks an alias.

// ---- k_stereo_points<BLOCK, SEG>, BLOCK / 64 waves: right keypoints sorted by row band start with
// their x / band height / octave beside the keys, left keypoints in row order, and a per-row
// (SEG: per octave segment and minr bin) first-candidate table
struct StereoPointsLds {
    LdsCarver c;
    int KP2, nbin, nrl;   // nbin: (SEG) minr bins per octave segment; nrl: rowlo entries
    uint32_t* rkey = c.take<uint32_t>(KP2);    // sorted right keys
    uint32_t* order = c.take<uint32_t>(KP2);   // left keypoints in processing order, then the sub-pixel jobs
    uint32_t* pairs = c.take<uint32_t>(KP2);   // per left keypoint (bestDist, bestIdxR, window)
    float* recx = c.take<float>(KP2);          // right x in sorted order
    uint16_t* recm = c.take<uint16_t>(KP2);    // band height << 8 | octave
    uint16_t* rowlo = c.take<uint16_t>((nrl + 1) & ~1);
    int* misc = c.take<int>(32);   // counters, the scan's wave sums at +4, (SEG) band heights at 22 + segment
    int stg_end;                   // (SEG) the launch reserves 16 B for the staging's alignment ...
    uint32_t* stg;                 // (SEG) [waves][SP_CHUNK][8] per-wave staging of right descriptors, 16-B aligned
    uint8_t* pad;                  // SEG: ... what the alignment left of them; else the launch's 64-int misc
    int bytes = c.off;
    float* depth = recx;           // = recx: mvDepth of the sub-pixel pass (the right x are dead after the band scan)
    uint32_t* hr = reinterpret_cast<uint32_t*>(rowlo);   // = rowlo: (SEG) u16 bin counts, two per word; then
    uint16_t* offr = rowlo;                              // = rowlo: (SEG) the bin offsets
    uint32_t* hl = stg;                                  // = stg: (SEG) left row counts (u16) before the staging is live
    uint16_t* offl = reinterpret_cast<uint16_t*>(stg);   // = stg: (SEG) the left row offsets
    GFPL_HD StereoPointsLds(unsigned char* smem, int KP2, int height, int n_levels, bool seg, int waves)
        : c(smem), KP2(KP2), nbin(height + 2 * SP_MINR_PAD), nrl(seg ? (n_levels + 1) * nbin + 1 : height),
          stg_end(c.off + 16 + waves * SP_CHUNK * 32), stg(seg ? c.take<uint32_t>(waves * SP_CHUNK * 8, 16) : nullptr),
          pad(c.take<uint8_t>(seg ? stg_end - c.off : 32 * 4)) {}
};

// ---- k_stereo_lines<CELL, INITIAL, BLOCK>, one layout for both cells.
// THE KNN TABLE COMES FIRST: knn_tile (gfpl_knn.hpp) reads it at LDS address 0, so `lut` is the first
// take and a kernel using this layout (or CrossLinesLds, Knn2Lds) declares no static __shared__.
// Only the train rows sit in LDS (the query rows stream from HBM into registers).
// (k_stereo_lines, k_cross_lines and k_pose still walk their pointers by hand, for the compiler's
// sake: their launchers size the launch from these structs and tests/test_layouts.py pins the
// structs to the kernels' walks)
struct StereoLinesLds {
    LdsCarver c;
    int cap, cell;
    uint32_t* lut = c.take<uint32_t>(knn_lut_dwords(cell));   // at LDS address 0
    uint32_t* tb = c.take<uint32_t>(cap * 8);                 // train rows R (knn_stage_views)
    int* lr_i = c.take<int>(cap);    // L->R best key, then index
    int* lr_d0 = c.take<int>(cap);
    int* lr_d1 = c.take<int>(cap);   // L->R second key, then distance
    int* rl_i = c.take<int>(cap);    // R->L best key (atomicMin), then index
    int* hist = c.take<int>(260);    // lineDescriptorMAD deviations
    int* pad_a = c.take<int>(8);     // (the launch's 64-int misc block: pad_a .. scan)
    double* th = c.take<double>(1);  // nn12_dist_th
    int* pad_b = c.take<int>(6);
    int* scan = c.take<int>(48);     // block_exclusive_scan's wave sums
    uint32_t* pad_lut = c.take<uint32_t>(knn_lut_dwords(2) - knn_lut_dwords(cell));   // the launch sizes CELL 2's table for both
    int bytes = c.off;
    GFPL_HD StereoLinesLds(unsigned char* smem, int cap, int cell) : c(smem), cap(cap), cell(cell) {}
};

// ---- k_cross_lines<BLOCK>; the knn table first (see StereoLinesLds)
struct CrossLinesLds {
    LdsCarver c;
    int cap;
    uint32_t* lut = c.take<uint32_t>(knn_lut_dwords(1));   // at LDS address 0
    uint32_t* tb = c.take<uint32_t>(cap * 8);              // train rows: curr (knn_stage_views)
    int* i12 = c.take<int>(cap);
    int* d012 = c.take<int>(cap);
    int* d112 = c.take<int>(cap);
    int* i21 = c.take<int>(cap);
    int* h12 = c.take<int>(260);   // (d1 - d0) histogram; cleared together with h0
    int* h0 = c.take<int>(260);    // d0 histogram
    // block_exclusive_scan's wave sums; with 16 waves its total is a 17th int, the low word of
    // th[0]: every thread has read th before the first scan's barrier
    int* scan = c.take<int>(16);
    double* th = c.take<double>(2);   // nn12 threshold, match budget distance
    int* pad = c.take<int>(44);       // (the rest of the launch's 64-int misc block)
    int bytes = c.off;
    GFPL_HD CrossLinesLds(unsigned char* smem, int cap) : c(smem), cap(cap) {}
};

// ---- k_knn2m<CELL>; the knn table first (see StereoLinesLds), then one chunk of train rows
struct Knn2Lds {
    LdsCarver c;
    int cell;
    uint32_t* lut = c.take<uint32_t>(knn_lut_dwords(cell));   // at LDS address 0
    uint32_t* tb = c.take<uint32_t>(KNN_CHUNK * 8);           // train chunk (knn_stage_views, stride KNN_CHUNK)
    int bytes = c.off;
    GFPL_HD Knn2Lds(unsigned char* smem, int cell) : c(smem), cell(cell) {}
};

// ---- k_cross_points<XL>.  XL: the exact projections of the bucketed points in LDS too (bucket
// order, beside their float copies), so a candidate that passes the float pre-filter reads them
// from LDS instead of an L2 round trip ahead of its descriptor load; for capacities whose LDS
// then leaves two workgroups per CU (kp_cap <= 2048)
struct CrossPointsLds {
    LdsCarver c;
    int cap, ncell;
    bool xl;
    double* prevT = c.take<double>(16);
    double* Tinv = c.take<double>(16);
    double* spxy = xl ? c.take<double>(2 * cap, 16) : nullptr;   // (XL) [cap][2], 16-B aligned pairs
    int* cnt = c.take<int>(ncell + 2);     // bucket counts (incl. the wild bucket)
    int* start = c.take<int>(ncell + 2);
    int* sq = c.take<int>(cap);
    float* spx = c.take<float>(cap);
    float* spy = c.take<float>(cap);
    int* lastT = c.take<int>(cap);
    int* misc = c.take<int>(64);
    int bytes = c.off;
    GFPL_HD CrossPointsLds(unsigned char* smem, int cap, int ncell, bool xl) : c(smem), cap(cap), ncell(ncell), xl(xl) {}
};

// ---- k_pose<W>: the GN chunk rows and the outlier residuals are never live together
struct PoseLds {
    // doubles shared by the chunk rows and the sort buffer
    GFPL_HD static int region(int W, int NP2) { return W * 16 * CH_STRIDE > NP2 ? W * 16 * CH_STRIDE : NP2; }
    LdsCarver c;
    int rest, nact;
    double* cp = c.take<double>(8 * CH_STRIDE);   // [W][16 * CH_STRIDE] from here: per wave 8 point rows, then 8 line rows
    double* cl = c.take<double>(8 * CH_STRIDE);   // wave 0's line rows
    double* more = c.take<double>(rest);          // the other waves' rows / the sort buffer's tail
    double* buf = cp;                             // = cp: [NP2] MAD sort buffer
    uint8_t* act = c.take<uint8_t>(nact);         // [mpt_cap + mls_cap, 16-B padded] active flags
    uint8_t* pad = c.take<uint8_t>(16);
    int bytes = c.off;
    GFPL_HD PoseLds(unsigned char* smem, int W, int NP2, int mpt_cap, int mls_cap)
        : c(smem), rest(region(W, NP2) - 16 * CH_STRIDE), nact((mpt_cap + mls_cap + 15) & ~15) {}
};

// ---- k_orb_cellfast: one cell per wave, byte cells
struct OrbCellLds {
    LdsCarver c;
    int patch_cap, waves, wave;
    uint8_t* below = c.take<uint8_t>(wave * 4 * patch_cap);   // the lower waves' cells
    uint8_t* P = c.take<uint8_t>(patch_cap);                  // the cell's ROI
    uint8_t* Sc = c.take<uint8_t>(patch_cap);                 // FAST scores
    uint16_t* cand = c.take<uint16_t>(patch_cap);             // candidate list
    uint8_t* above = c.take<uint8_t>((waves - 1 - wave) * 4 * patch_cap);
    int bytes = c.off;
    GFPL_HD OrbCellLds(unsigned char* smem, int patch_cap, int waves, int wave)
        : c(smem), patch_cap(patch_cap), waves(waves), wave(wave) {}
};

// ---- k_lsd_grow_lds: one wave per image
struct LsdGrowLds {
    LdsCarver c;
    int cid_cap;
    uint32_t* ring = c.take<uint32_t>(LSD_RING);       // the region list's newest entries
    uint32_t* used = c.take<uint32_t>(cid_cap / 32);   // compact used bitmap
    int bytes = c.off;
    GFPL_HD LsdGrowLds(unsigned char* smem, int cid_cap) : c(smem), cid_cap(cid_cap) {}
};

// ---- the device copy of a DBoW2 vocabulary (gfpl_vocab, k_bow.hip).  Nodes are renumbered breadth
// first from the root (device node 0), so a node's children are consecutive device nodes in
// Node::children order and a child's 32-byte descriptor row and its record sit at child0 + position.
// Leaves are ranked by ascending word id: the kernels sort ranks (the same order as word ids) and
// look the word id and the weight up by rank.
constexpr int BOW_MAX_CHILDREN = 32;        // two child positions per lane of a 16-lane row (k_bow_descend)
constexpr int BOW_STOP = 0x7fffffff;        // key of a feature whose leaf weight is not > 0 (sorts last)
struct BowNode {
    int32_t child0;    // device node of the first child
    int32_t n_child;   // 0: a leaf
    int32_t key;       // leaf: its rank, or BOW_STOP when !(weight > 0); inner node: unused
    int32_t pad;
};
struct BowVocabMem {
    Carver c;
    int n_nodes, n_leaves;
    uint8_t* desc = c.take<uint8_t>((size_t)n_nodes * 32);      // [n_nodes][32], rows 32-B aligned
    BowNode* node = c.take<BowNode>((size_t)n_nodes);
    int32_t* rank_word = c.take<int32_t>((size_t)n_leaves);     // word id of rank r, ascending
    double* rank_weight = c.take<double>((size_t)n_leaves);
    size_t bytes = c.off;
    BowVocabMem(char* base, int n_nodes, int n_leaves) : c{0, base}, n_nodes(n_nodes), n_leaves(n_leaves) {}
};

// ---- k_bow_finish: one set's keys (padded to a power of two p2 for the bitonic sort), the
// unnormalised values of its words, the block scan's wave sums and the norm
struct BowFinishLds {
    LdsCarver c;
    int p2, max_count;
    int32_t* keys = c.take<int32_t>(p2);
    double* vals = c.take<double>(max_count, 8);
    double* norm = c.take<double>(1);
    int* scan = c.take<int>(8);
    int bytes = c.off;
    GFPL_HD BowFinishLds(unsigned char* smem, int p2, int max_count) : c(smem), p2(p2), max_count(max_count) {}
};

// ---- local bundle adjustment (k_lba.hip, gfpl_lba.cpp): one problem's device workspace.
// Landmarks are numbered points first, then lines; a point block has 3 rows, a line block 6.
// A coupling block W (and Y = V^-1 W) is [landmark rows][6 pose columns], one per landmark and
// local keyframe; only the keyframes of the landmark's mask are ever read.
constexpr int LBA_BLOCK = 256;    // threads of k_lba = observation rows per LDS chunk
constexpr int LBA_ROW = 14;       // doubles per observation row: J_pose[6], J_landmark[6], |err|, w
constexpr int LBA_MAX_KFS = 16;   // = GFPL_LBA_MAX_KFS (gfpl_lba.cpp asserts it)
// slots of a Levenberg-Marquardt loop's state that the LBA (LbaLds::sd, ::si) and the GBA (GbaPtrs::sd, ::si)
// share (gfpl_ba.hpp works on these); each solver's own words follow them
enum { BA_SD_LAMBDA = 0, BA_SD_ERR, BA_SD_ERRPREV, BA_SD_ERRSUM, BA_SD_N2 };
enum { BA_SI_ITERS = 0, BA_SI_STOP, BA_SI_STATUS, BA_SI_HMAX, BA_SI_DONE };
struct LbaPtrs {
    double *X, *DX;               // [6 n_kf + 3 n_pt + 6 n_ls]
    double* rows;                 // [n_obs][LBA_ROW], points first
    double *U, *gk;               // [n_kf][36], [n_kf][6]: undamped pose blocks and their gradient
    double *V, *Vi;               // [9 n_pt + 36 n_ls]: undamped landmark blocks, inverses of the damped ones
    double *glm, *z;              // [3 n_pt + 6 n_ls]: landmark gradient, V^-1 g
    double *W, *Y;                // [n_kf (18 n_pt + 36 n_ls)]
    double* q;                    // [n_lm] squared step of each landmark
    int32_t* mask;                // [n_lm] bit s: local keyframe s observes the landmark
    int32_t* state;               // [8]: 0 the last iteration evaluated
};
struct LbaMem {
    Carver c;
    int nkf, npt, nls, nobs;
    size_t N = 6 * (size_t)nkf + 3 * (size_t)npt + 6 * (size_t)nls;
    size_t nv = 9 * (size_t)npt + 36 * (size_t)nls, ng = 3 * (size_t)npt + 6 * (size_t)nls;
    size_t nw = (size_t)nkf * (18 * (size_t)npt + 36 * (size_t)nls);
    LbaPtrs p{c.take<double>(N), c.take<double>(N), c.take<double>((size_t)nobs * LBA_ROW),
              c.take<double>((size_t)nkf * 36), c.take<double>((size_t)nkf * 6),
              c.take<double>(nv), c.take<double>(nv), c.take<double>(ng), c.take<double>(ng),
              c.take<double>(nw), c.take<double>(nw), c.take<double>((size_t)npt + nls),
              c.take<int32_t>((size_t)npt + nls), c.take<int32_t>(8)};
    // the uploaded index arrays: first observation of each landmark, then per observation its landmark and slot
    int32_t* lm_start = c.take<int32_t>((size_t)npt + nls + 1);
    int32_t* obs_lm = c.take<int32_t>((size_t)nobs);
    int32_t* obs_kf = c.take<int32_t>((size_t)nobs);
    size_t bytes = (c.off + 255) & ~(size_t)255;
    LbaMem(char* base, int nkf, int npt, int nls, int nobs) : c{0, base}, nkf(nkf), npt(npt), nls(nls), nobs(nobs) {}
};

// ---- k_lba: the reduced pose system S (6 n_kf square, lower triangle used) with its right-hand
// side, pivots and solution, the inverse poses of the iteration, one chunk of observation rows
// with their slots, a reduction buffer and the loop's state.  kfs is the launch's largest n_kf.
struct LbaLds {
    LdsCarver c;
    int kfs;
    double* S = c.take<double>(36 * kfs * kfs);
    double* gr = c.take<double>(6 * kfs);
    double* D = c.take<double>(6 * kfs);
    double* dx = c.take<double>(6 * kfs);
    double* Tinv = c.take<double>(16 * kfs);
    double* rows = c.take<double>(LBA_BLOCK * LBA_ROW);
    double* red = c.take<double>(LBA_BLOCK);
    double* sd = c.take<double>(8);      // BA_SD_*
    int* slot = c.take<int>(LBA_BLOCK);
    int* si = c.take<int>(16);           // BA_SI_*, then singular, accept
    int bytes = c.off;
    GFPL_HD LbaLds(unsigned char* smem, int kfs) : c(smem), kfs(kfs) {}
};
static_assert(8 * (36 * LBA_MAX_KFS * LBA_MAX_KFS + 34 * LBA_MAX_KFS + LBA_BLOCK * (LBA_ROW + 1) + 8) + 4 * (LBA_BLOCK + 16) <=
                  160 * 1024 - 1024,
              "LbaLds at LBA_MAX_KFS must fit a workgroup's dynamic LDS");

// ---- the landmark descriptor store (gfpl_lmstore, k_lm.hip, gfpl_lm.cpp): desc_list of every
// landmark at a fixed stride of obs_cap rows, its length, and the row updateAverageDescDir picks
// (index and a copy, so a gather reads one 32-byte row and never the list).  Rows at and past a
// landmark's count keep whatever was last written there.
constexpr int LM_MAX_OBS = 64;    // = GFPL_LM_MAX_OBS: one observation per lane of a wave
constexpr int LM_BUCKETS = 6;     // lane groups of 2, 4, 8, 16, 32, 64 (k_lm_apply<G>)
constexpr int LM_BLOCK = 256;     // threads of k_lm_apply and k_lm_gather
struct LmStoreMem {
    Carver c;
    int lm_cap, obs_cap;
    uint8_t* rows = c.take<uint8_t>((size_t)lm_cap * obs_cap * 32);   // [lm_cap][obs_cap][32], rows 32-B aligned
    int32_t* count = c.take<int32_t>((size_t)lm_cap);
    int32_t* med_idx = c.take<int32_t>((size_t)lm_cap);               // -1: no observation
    uint8_t* med = c.take<uint8_t>((size_t)lm_cap * 32);              // [lm_cap][32] med_desc
    size_t bytes = (c.off + 255) & ~(size_t)255;
    LmStoreMem(char* base, int lm_cap, int obs_cap) : c{0, base}, lm_cap(lm_cap), obs_cap(obs_cap) {}
};
// one op as the kernel reads it: the planner's order, the source row resolved to its address
struct LmOpDev {
    const uint8_t* row;   // ADD: the 32-byte source row (16-B aligned)
    int32_t kind;         // GFPL_LM_ADD / _ERASE_OBS / _FREE
    int32_t pos;          // ERASE_OBS: the position
};
// one touched landmark of a call: its ops are ops[op0 .. op0 + n_ops)
struct LmWork {
    int32_t lm, op0, n_ops;
    int32_t count0;       // the list's length before the call (the host mirror's; the kernel reads it from here)
};
// the uploaded lists of one apply (work items in bucket order, then the ops grouped by landmark),
// laid out alike in the pinned staging and on the device so that one copy moves both
struct LmWorkMem {
    Carver c;
    int max_ops;
    LmWork* work = c.take<LmWork>((size_t)max_ops);    // at most one touched landmark per op
    LmOpDev* ops = c.take<LmOpDev>((size_t)max_ops);
    size_t bytes = (c.off + 255) & ~(size_t)255;
    LmWorkMem(char* base, int max_ops) : c{0, base}, max_ops(max_ops) {}
};
// lanes of bucket b, and the bucket of a list that reaches `peak` observations (at least min_g lanes):
// the host planner's and the device planner's one rule
GFPL_HD constexpr int lm_bucket_lanes(int b) { return 2 << b; }
GFPL_HD inline int lm_bucket_of(int peak, int min_g) {
    int b = 0;
    while (b < LM_BUCKETS - 1 && (lm_bucket_lanes(b) < peak || lm_bucket_lanes(b) < min_g)) ++b;
    return b;
}
// the device planner's scratch (k_lm_plan.hip), allocated at a store's first device-id call.  hdr: the
// call's error word (KFMAP_ERR_* bits), its op count and bucket_start[LM_BUCKETS + 1], zeroed when a
// call starts and copied to the host once per call.  pend: pairs a landmark receives within the running
// call (all 0 between calls); op0: a touched landmark's first op.  place: per pair its rank among its
// landmark's pairs, in pair order.  tile_w / tile_o: work items and ops of every (bucket, tile of
// LM_PLAN_TILE pairs), bucket-major, then their exclusive scans in place.
constexpr int LM_PLAN_TILE = 2048;   // pairs per workgroup of the planner's compaction; a thread takes TILE / LM_BLOCK consecutive pairs
constexpr int LM_HDR = 16;           // int32 words of the header
enum { LM_H_ERR = 0, LM_H_NOPS, LM_H_BUCKET };   // hdr[LM_H_BUCKET + b] = bucket_start[b], b = 0 .. LM_BUCKETS
static_assert(LM_H_BUCKET + LM_BUCKETS + 1 <= LM_HDR, "the header holds every bucket's start and the total");
struct LmPlanMem {
    Carver c;
    int lm_cap, max_ops;
    size_t n_tiles = ((size_t)max_ops + LM_PLAN_TILE - 1) / LM_PLAN_TILE;   // a call has at most max_ops pairs
    int32_t* hdr = c.take<int32_t>(LM_HDR);
    int32_t* pend = c.take<int32_t>((size_t)lm_cap);
    int32_t* op0 = c.take<int32_t>((size_t)lm_cap);
    int32_t* place = c.take<int32_t>((size_t)max_ops);
    int32_t* tile_w = c.take<int32_t>(LM_BUCKETS * n_tiles + 1);
    int32_t* tile_o = c.take<int32_t>(LM_BUCKETS * n_tiles + 1);
    size_t bytes = (c.off + 255) & ~(size_t)255;
    LmPlanMem(char* base, int lm_cap, int max_ops) : c{0, base}, lm_cap(lm_cap), max_ops(max_ops) {}
};
// (k_lm_apply keeps a group's rows and distances in registers: it has no LDS layout)

// ---- the loop-closure pose graph (k_pgo.hip, gfpl_pgo.cpp, gfpl_pgo_plan.cpp).  Vertices are the
// keyframes of kf_list in order, free vertices (not fixed) are numbered in that order too, and the
// free system's row r (a 6 x 6 block row) is stored from its first block column f(r) to r.
constexpr int PGO_BLOCK = 256;    // threads of k_pgo = edges per pass = entries of the chi2 staging
constexpr int PGO_ROW = 78;       // doubles per edge row: e[6], J_i[6][6], J_j[6][6]
constexpr int PGO_RED = 78;       // reduction lanes per free vertex: 36 diagonal, 6 gradient, 36 off-diagonal
constexpr int PGO_PANEL = 16;     // block columns of the pivot row staged in LDS at a time
constexpr int PGO_VERT_LC_J = 2, PGO_VERT_FIXED = 1, PGO_VERT_LC_I = 4;
// the index arrays of one problem, laid out alike in the pinned staging and on the device so that
// one copy moves them (every count is the problem's own; the arrays are the planner's, PgoPlan)
struct PgoIdx {
    Carver c;
    int nkf, nlc, nvert, nfree, nedge, njobs;
    int32_t* vert = c.take<int32_t>((size_t)nvert * 4);       // keyframe, flags, lc_id, free index
    int32_t* free_vert = c.take<int32_t>((size_t)nfree);      // vertex of free index r
    int32_t* edge = c.take<int32_t>((size_t)nedge * 4);       // vertex i, vertex j, loop entry or -1, 0
    int32_t* inc_start = c.take<int32_t>((size_t)nfree + 1);  // incident edges of free vertex r, edge-list order
    int32_t* inc = c.take<int32_t>((size_t)nedge * 2);
    int32_t* env_first = c.take<int32_t>((size_t)nfree);      // f(r)
    int32_t* env_off = c.take<int32_t>((size_t)nfree + 1);    // first block of row r in the envelope arrays
    int32_t* reach = c.take<int32_t>((size_t)nfree);          // the last row whose envelope holds column c
    int32_t* lc = c.take<int32_t>((size_t)nlc * 3);
    int32_t* alive = c.take<int32_t>((size_t)nkf);
    int32_t* jobs = c.take<int32_t>((size_t)njobs * 4);       // landmark, keyframe, first dir row, dir rows; points first
    double* lc_pose = c.take<double>((size_t)nlc * 6);
    size_t bytes = (c.off + 255) & ~(size_t)255;
    PgoIdx(char* base, int nkf, int nlc, int nvert, int nfree, int nedge, int njobs)
        : c{0, base}, nkf(nkf), nlc(nlc), nvert(nvert), nfree(nfree), nedge(nedge), njobs(njobs) {}
};
struct PgoPtrs {
    double *X, *Xt, *X0;          // [n_vert][16] poses, trial poses, start poses
    double* Z;                    // [n_edge][16] measurements
    double* rows;                 // [n_edge][PGO_ROW]
    double* esq;                  // [n_edge] e . e of the last evaluation
    double *diag, *b;             // [n_free][36], [6 n_free]: undamped diagonal blocks, J^T e
    double *H, *L;                // [env_blocks][36]: undamped envelope (diagonal places zero), the factor of H + lambda I
    double *D, *y;                // [6 n_free] pivots, right-hand side / step
    double* corr;                 // [n_kf][16] Tkfw_corr of every keyframe the write-back moved
    int32_t* moved;               // [n_kf] 1: corr is set
    int32_t* state;               // [8]: 0 linearisations so far
};
struct PgoMem {
    Carver c;
    int nkf, nvert, nfree, nedge, nenv;
    PgoPtrs p{c.take<double>((size_t)nvert * 16), c.take<double>((size_t)nvert * 16), c.take<double>((size_t)nvert * 16),
              c.take<double>((size_t)nedge * 16), c.take<double>((size_t)nedge * PGO_ROW), c.take<double>((size_t)nedge),
              c.take<double>((size_t)nfree * 36), c.take<double>((size_t)nfree * 6),
              c.take<double>((size_t)nenv * 36), c.take<double>((size_t)nenv * 36),
              c.take<double>((size_t)nfree * 6), c.take<double>((size_t)nfree * 6),
              c.take<double>((size_t)nkf * 16), c.take<int32_t>((size_t)nkf), c.take<int32_t>(8)};
    size_t bytes = (c.off + 255) & ~(size_t)255;
    PgoMem(char* base, int nkf, int nvert, int nfree, int nedge, int nenv)
        : c{0, base}, nkf(nkf), nvert(nvert), nfree(nfree), nedge(nedge), nenv(nenv) {}
};
// ---- k_pgo: the staged piece of the pivot row (L[k][m] and D[m] of PGO_PANEL block columns), the
// chi2 staging and the loop's state; the same for every problem size
struct PgoLds {
    LdsCarver c;
    double* pk = c.take<double>(6 * PGO_PANEL);
    double* pd = c.take<double>(6 * PGO_PANEL);
    double* red = c.take<double>(PGO_BLOCK);
    double* sd = c.take<double>(16);     // lambda, nu, chi2, chi2 of the trial, |delta|_inf, scale, chi2_0, chi2 before the step
    int* si = c.take<int>(16);           // iters, stop, status, rejects, done, singular, accept, rejects of the iteration
    int bytes = c.off;
    GFPL_HD explicit PgoLds(unsigned char* smem) : c(smem) {}
};

// ---- global bundle adjustment (k_gba.hip, gfpl_gba.cpp, gfpl_gba_plan.cpp): one problem spread over
// the device.  Landmarks and observations are numbered as in the LBA (points first).  A coupling
// block W (and Y = V^-1 W) exists once per PAIR (landmark, distinct local keyframe that observes
// it), pairs ordered by landmark and then by keyframe: point pairs first at 18 doubles each, line
// pairs after them at 36.  S is the dense reduced pose system, row-major 6 n_kf square in HBM; its
// lower triangle becomes L in place outside the 6 x 6 diagonal blocks, whose L is kept transposed above
// the diagonal (the block under it stays what every workgroup of its column's launch reads); the pivots go to D.
constexpr int GBA_BLOCK = 256;     // threads of the wide phases, terms per pass of the ordered sums, rows per pass of the substitutions
constexpr int GBA_ROW = LBA_ROW;   // an observation row is the LBA's
constexpr int GBA_LDLT_KFS = 6;    // block rows of the panel one workgroup of k_gba_ldlt factorises (below its copy of the diagonal block)
constexpr int GBA_MAX_KFS = 256;   // = GFPL_GBA_MAX_KFS (gfpl_gba.cpp asserts it)
constexpr int GBA_MAX_LDLT_ROWS = 24;   // the test override of GBA_LDLT_KFS: 36 (1 + rows) threads stay within 1024
// slots of the loop state (GbaPtrs::sd, ::si): the BA_* prefix, then the GBA's own words
enum { GBA_SD_N2POSE = BA_SD_N2 + 1 };
enum { GBA_SI_DONE_NEXT = BA_SI_DONE + 1, GBA_SI_SING, GBA_SI_UPDATE_IT, GBA_SI_LAST_IT, GBA_SI_LDLT_BAD0, GBA_SI_LDLT_BAD1 };
// the planner's index arrays of one problem, laid out alike in the pinned staging and on the device
struct GbaIdx {
    Carver c;
    int nkf, nlm, nobs, npairs, nterms;
    int32_t* lm_start = c.take<int32_t>((size_t)nlm + 1);      // first observation of each landmark
    int32_t* obs_lm = c.take<int32_t>((size_t)nobs);
    int32_t* obs_kf = c.take<int32_t>((size_t)nobs);           // slot: >= 0 local, < 0 fixed
    int32_t* obs_pair = c.take<int32_t>((size_t)nobs);         // the observation's pair, -1 for a fixed pose
    int32_t* pair_start = c.take<int32_t>((size_t)nlm + 1);    // pairs of each landmark
    int32_t* pair_kf = c.take<int32_t>((size_t)npairs);        // ascending within a landmark
    int32_t* kf_start = c.take<int32_t>((size_t)nkf + 1);      // observations of each local keyframe, list order
    int32_t* kf_obs = c.take<int32_t>((size_t)nobs);
    int32_t* blk_start = c.take<int32_t>((size_t)nkf * (nkf + 1) / 2 + 1);   // terms of lower block (a, b): index a (a + 1) / 2 + b
    int32_t* terms = c.take<int32_t>((size_t)nterms * 3);      // landmark (ascending within a block), pair of a, pair of b
    size_t bytes = (c.off + 255) & ~(size_t)255;
    GbaIdx(char* base, int nkf, int nlm, int nobs, int npairs, int nterms)
        : c{0, base}, nkf(nkf), nlm(nlm), nobs(nobs), npairs(npairs), nterms(nterms) {}
};
struct GbaPtrs {
    double *X, *DX;               // [6 n_kf + 3 n_pt + 6 n_ls]
    double* rows;                 // [n_obs][GBA_ROW]
    double* Tinv;                 // [n_kf][16] inverse poses of X, once per iteration
    double *U, *gk;               // [n_kf][36], [n_kf][6]
    double *V, *Vi;               // [9 n_pt + 36 n_ls]: undamped blocks; LDL^T of the damped ones (L under, pivots on the diagonal)
    double *glm, *z;              // [3 n_pt + 6 n_ls]
    double *W, *Y;                // [18 n_pt_pairs + 36 n_ls_pairs]
    double *q, *dmax;             // [n_lm] squared step, largest |diagonal| of each landmark
    double *S, *D, *gr;           // [6 n_kf][6 n_kf], [6 n_kf], [6 n_kf]: g_r, then the pose step
    double* sd;                   // [8]  BA_SD_*, GBA_SD_*
    int32_t* si;                  // [16] BA_SI_*, GBA_SI_*
};
struct GbaMem {
    Carver c;
    int nkf, npt, nls, nobs, npp, nlp;
    size_t N = 6 * (size_t)nkf + 3 * (size_t)npt + 6 * (size_t)nls;
    size_t nv = 9 * (size_t)npt + 36 * (size_t)nls, ng = 3 * (size_t)npt + 6 * (size_t)nls;
    size_t nw = 18 * (size_t)npp + 36 * (size_t)nlp, n6 = 6 * (size_t)nkf;
    GbaPtrs p{c.take<double>(N), c.take<double>(N), c.take<double>((size_t)nobs * GBA_ROW), c.take<double>((size_t)nkf * 16),
              c.take<double>((size_t)nkf * 36), c.take<double>(n6),
              c.take<double>(nv), c.take<double>(nv), c.take<double>(ng), c.take<double>(ng),
              c.take<double>(nw), c.take<double>(nw), c.take<double>((size_t)npt + nls), c.take<double>((size_t)npt + nls),
              c.take<double>(n6 * n6), c.take<double>(n6), c.take<double>(n6),
              c.take<double>(8), c.take<int32_t>(16)};
    size_t bytes = (c.off + 255) & ~(size_t)255;
    GbaMem(char* base, int nkf, int npt, int nls, int nobs, int npp, int nlp)
        : c{0, base}, nkf(nkf), npt(npt), nls(nls), nobs(nobs), npp(npp), nlp(nlp) {}
};
// ---- k_gba_ldlt: the partial sums of the diagonal block's and the panel's entries, then the factor
// of the diagonal block and its pivots; rows: 6 + 6 * (block rows per workgroup)
struct GbaLdltLds {
    LdsCarver c;
    int rows;
    double* part = c.take<double>(rows * 6);
    double* Ld = c.take<double>(36);
    double* Dd = c.take<double>(6);
    int* flag = c.take<int>(2);
    int bytes = c.off;
    GFPL_HD GbaLdltLds(unsigned char* smem, int rows) : c(smem), rows(rows) {}
};
// ---- k_gba_subst: the right-hand side / solution of the reduced system
struct GbaSubstLds {
    LdsCarver c;
    int n6;
    double* y = c.take<double>(n6);
    int bytes = c.off;
    GFPL_HD GbaSubstLds(unsigned char* smem, int n6) : c(smem), n6(n6) {}
};
static_assert(8 * 6 * GBA_MAX_KFS <= 64 * 1024, "GbaSubstLds at GBA_MAX_KFS fits the default dynamic LDS");

// ---- the map's index half (gfpl_kfmap, k_kfmap.hip, gfpl_kfmap.cpp): per keyframe its flags, row
// counts and the features' idx at a fixed stride; per landmark and kind its flags, kf_obs_list at a
// fixed stride of obs_cap with its length, and the keyframe that owns it; full_graph at a stride of
// kf_cap; then the calls' header and workspace.  Landmark arrays are [2] by kind (0 points, 1 lines).
constexpr int KFMAP_TILE = 2048;     // = GFPL_KFMAP_TILE: items per workgroup of a compaction
constexpr int KFMAP_BLOCK = 256;     // threads of every k_kfmap kernel; a thread takes TILE / BLOCK consecutive items
constexpr int KFMAP_HDR = 16;        // int32 words of the header (KFMAP_H_*), copied to the host once per call
// the first KFMAP_H_CALL words are a call's own (zeroed when it starts), the others the map's
enum { KFMAP_H_ERR = 0, KFMAP_H_COUNT0, KFMAP_H_COUNT1, KFMAP_H_FIRST_NEW, KFMAP_H_CALL, KFMAP_H_NKF = KFMAP_H_CALL, KFMAP_H_NEXT_PT, KFMAP_H_NEXT_LS };
constexpr int KFMAP_ERR_INVALID = 1, KFMAP_ERR_CAPACITY = 2;
struct KfMapMem {
    Carver c;
    int kf_cap, rows[2], lm_cap[2], obs_cap;
    size_t max_rows = (size_t)(rows[0] > rows[1] ? rows[0] : rows[1]);
    size_t max_lm = (size_t)(lm_cap[0] > lm_cap[1] ? lm_cap[0] : lm_cap[1]);
    size_t max_items = max_rows > max_lm ? max_rows : max_lm;
    size_t n_tiles = (max_items + KFMAP_BLOCK - 1) / KFMAP_BLOCK;   // an observe call scans per workgroup of pairs
    int32_t* hdr = c.take<int32_t>(KFMAP_HDR);
    uint8_t* kf_alive = c.take<uint8_t>((size_t)kf_cap);
    uint8_t* kf_local = c.take<uint8_t>((size_t)kf_cap);
    int32_t* kf_n[2] = {c.take<int32_t>((size_t)kf_cap), c.take<int32_t>((size_t)kf_cap)};
    int32_t* kf_idx[2] = {c.take<int32_t>((size_t)kf_cap * rows[0]), c.take<int32_t>((size_t)kf_cap * rows[1])};
    int32_t* graph = c.take<int32_t>((size_t)kf_cap * kf_cap);
    uint8_t* lm_alive[2] = {c.take<uint8_t>((size_t)lm_cap[0]), c.take<uint8_t>((size_t)lm_cap[1])};
    uint8_t* lm_local[2] = {c.take<uint8_t>((size_t)lm_cap[0]), c.take<uint8_t>((size_t)lm_cap[1])};
    uint8_t* lm_inlier[2] = {c.take<uint8_t>((size_t)lm_cap[0]), c.take<uint8_t>((size_t)lm_cap[1])};
    int32_t* lm_nobs[2] = {c.take<int32_t>((size_t)lm_cap[0]), c.take<int32_t>((size_t)lm_cap[1])};
    int32_t* lm_owner[2] = {c.take<int32_t>((size_t)lm_cap[0]), c.take<int32_t>((size_t)lm_cap[1])};
    int32_t* lm_obs[2] = {c.take<int32_t>((size_t)lm_cap[0] * obs_cap), c.take<int32_t>((size_t)lm_cap[1] * obs_cap)};
    // workspace.  tile: the compactions' tile sums, then their exclusive scan in place.  seen0 / seen1: the
    // call number that last named a value in column 0 / 1 of a pairs array (0: never).  pend: appends a
    // landmark receives within the running call (all 0 between calls).  first_row: remove_bad's lowest
    // carrying row (all INT32_MAX between calls).  pair_n0 / pair_slot: per pair of an observe call, its
    // landmark's list length before the call and the place of its own entry.
    int32_t* tile = c.take<int32_t>(n_tiles + 1);
    int32_t* seen0 = c.take<int32_t>(max_items);
    int32_t* seen1 = c.take<int32_t>(max_rows);
    int32_t* pend = c.take<int32_t>(max_lm);
    int32_t* first_row = c.take<int32_t>(max_lm);
    int32_t* pair_n0 = c.take<int32_t>(max_rows);
    int32_t* pair_slot = c.take<int32_t>(max_rows);
    size_t bytes = (c.off + 255) & ~(size_t)255;
    KfMapMem(char* base, int kf_cap, int pt_rows, int ls_rows, int pt_lm_cap, int ls_lm_cap, int obs_cap)
        : c{0, base}, kf_cap(kf_cap), rows{pt_rows, ls_rows}, lm_cap{pt_lm_cap, ls_lm_cap}, obs_cap(obs_cap) {}
};

// ---- the map's geometry half (gfpl_mapgeo, k_mapgeo.hip, gfpl_mapgeo.cpp), ids and caps gfpl_kfmap's:
// per keyframe T_kf_w and x_kf_w; per landmark and kind its 3D geometry, obs_list and sigma_list at a
// fixed stride of obs_cap with their length; then the calls' header, the observe calls' workspace and
// the buffers gfpl_mapgeo_assemble fills (a gfpl_lba_problem's arrays at the caps, a_*).  Landmark
// arrays are [2] by kind; a kind's 3D geometry is MAPGEO_LM_W doubles, an observation MAPGEO_OBS_W.
constexpr int MAPGEO_HDR = 16;       // int32 words of the header (MAPGEO_H_*), zeroed when a call starts, copied to the host once per call
enum { MAPGEO_H_ERR = 0, MAPGEO_H_NKF, MAPGEO_H_NFIX, MAPGEO_H_NPT, MAPGEO_H_NLS, MAPGEO_H_NPTOBS, MAPGEO_H_NLSOBS };
constexpr int MAPGEO_LM_W[2] = {3, 6}, MAPGEO_OBS_W[2] = {2, 3};
constexpr int MAPGEO_SLOT_NONE = INT32_MIN;   // kf_slot of a keyframe that is neither listed nor fixed
struct MapGeoMem {
    Carver c;
    int kf_cap, rows[2], lm_cap[2], obs_cap;
    size_t max_rows = (size_t)(rows[0] > rows[1] ? rows[0] : rows[1]);
    size_t max_lm = (size_t)(lm_cap[0] > lm_cap[1] ? lm_cap[0] : lm_cap[1]);
    size_t n_tiles = (max_lm + KFMAP_TILE - 1) / KFMAP_TILE;
    size_t lm_obs[2] = {(size_t)lm_cap[0] * obs_cap, (size_t)lm_cap[1] * obs_cap};
    int32_t* hdr = c.take<int32_t>(MAPGEO_HDR);
    double* T_kf = c.take<double>((size_t)kf_cap * 16);
    double* x_kf = c.take<double>((size_t)kf_cap * 6);
    double* lm3d[2] = {c.take<double>((size_t)lm_cap[0] * MAPGEO_LM_W[0]), c.take<double>((size_t)lm_cap[1] * MAPGEO_LM_W[1])};
    int32_t* nobs[2] = {c.take<int32_t>((size_t)lm_cap[0]), c.take<int32_t>((size_t)lm_cap[1])};
    double* obs[2] = {c.take<double>(lm_obs[0] * MAPGEO_OBS_W[0]), c.take<double>(lm_obs[1] * MAPGEO_OBS_W[1])};
    double* sigma[2] = {c.take<double>(lm_obs[0]), c.take<double>(lm_obs[1])};
    // the observe calls.  pend: pairs a landmark receives within the running call (all 0 between calls);
    // pair_n0: per pair its landmark's list length before the call.
    int32_t* pend = c.take<int32_t>(max_lm);
    int32_t* pair_n0 = c.take<int32_t>(max_rows);
    // assemble.  kf_slot: a keyframe's slot (>= 0 listed, < 0 fixed, MAPGEO_SLOT_NONE); kf_mark: named by a
    // selected landmark; lm_cnt: a landmark's observations that go into the problem (0: not selected);
    // tile_lm / tile_obs: per kind the tile sums of the selected landmarks and of their observations,
    // then their exclusive scans in place; lm_off: first observation of each selected landmark.
    int32_t* kf_slot = c.take<int32_t>((size_t)kf_cap);
    int32_t* kf_mark = c.take<int32_t>((size_t)kf_cap);
    int32_t* kf_list = c.take<int32_t>((size_t)kf_cap);
    int32_t* fix_list = c.take<int32_t>((size_t)kf_cap);
    int32_t* lm_cnt[2] = {c.take<int32_t>((size_t)lm_cap[0]), c.take<int32_t>((size_t)lm_cap[1])};
    int32_t* tile_lm[2] = {c.take<int32_t>(n_tiles + 1), c.take<int32_t>(n_tiles + 1)};
    int32_t* tile_obs[2] = {c.take<int32_t>(n_tiles + 1), c.take<int32_t>(n_tiles + 1)};
    int32_t* lm_list[2] = {c.take<int32_t>((size_t)lm_cap[0]), c.take<int32_t>((size_t)lm_cap[1])};
    int32_t* lm_off[2] = {c.take<int32_t>((size_t)lm_cap[0] + 1), c.take<int32_t>((size_t)lm_cap[1] + 1)};
    double* a_x_kf = c.take<double>((size_t)kf_cap * 6);
    double* a_x_out = c.take<double>((size_t)kf_cap * 6);
    double* a_T_kf = c.take<double>((size_t)kf_cap * 16);
    double* a_T_fix = c.take<double>((size_t)kf_cap * 16);
    double* a_lm3d[2] = {c.take<double>((size_t)lm_cap[0] * MAPGEO_LM_W[0]), c.take<double>((size_t)lm_cap[1] * MAPGEO_LM_W[1])};
    double* a_obs[2] = {c.take<double>(lm_obs[0] * MAPGEO_OBS_W[0]), c.take<double>(lm_obs[1] * MAPGEO_OBS_W[1])};
    double* a_sigma[2] = {c.take<double>(lm_obs[0]), c.take<double>(lm_obs[1])};
    int32_t* a_obs_lm[2] = {c.take<int32_t>(lm_obs[0]), c.take<int32_t>(lm_obs[1])};
    int32_t* a_obs_kf[2] = {c.take<int32_t>(lm_obs[0]), c.take<int32_t>(lm_obs[1])};
    size_t bytes = (c.off + 255) & ~(size_t)255;
    MapGeoMem(char* base, int kf_cap, int pt_rows, int ls_rows, int pt_lm_cap, int ls_lm_cap, int obs_cap)
        : c{0, base}, kf_cap(kf_cap), rows{pt_rows, ls_rows}, lm_cap{pt_lm_cap, ls_lm_cap}, obs_cap(obs_cap) {}
};

}  // namespace gfpl
