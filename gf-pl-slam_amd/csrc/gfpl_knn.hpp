// gfpl_knn.hpp — knn-2 Hamming matching on the matrix cores (gfx950 FP4 scaled MFMA).
//
// BFMatcher::knnMatch(k = 2) with NORM_HAMMING / NORM_HAMMING2 (OpenCV 3.4.1
// batchDistance; ledger T1) restated as an exact GEMM over operands that hold only 0 and +-1:
//   HAMMING  : dist(t, q) = popc(t) + popc(q) - 2 <t_bits, q_bits>
//              = <t_bits, 1 - 2 q_bits> + popc(q)            (K = 256, one element per bit)
//   HAMMING2 : dist(t, q) = 128 - <onehot(t), onehot(q)>     (K = 512, each 2-bit
//              cell one-hot over its 4 values: equal cells contribute 1; the query
//              side is negated and 128 is added with the keys)
// v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 (E2M1) operands takes a 32x32 tile of (train row t) x
// (query column q) per wave, K = 64 per instruction.  E2M1 represents 0 and +-1 exactly (1.0 is
// nibble 0x2, -1.0 nibble 0xA), the block scales are powers of two (2^0 in k_knn2m, 2^13 in
// knn2_mfma) and the f32 accumulator holds integer counts (|count| <= 256) times that power
// exactly, so the distances are exact integers.  The C layout puts one
// query column on each lane (col = lane & 31) and 16 train rows in its registers
// (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), so the per-query top-2 is lane-local.  The top-2 is
// the lexicographic minimum of the packed key (dist, t) — the OpenCV insertion rule (strict
// '<', ties keep the lower train index) is exactly that, independent of visiting order.
// The k-index each (lane half, element) holds is the same for A and B, so the
// dot products are exact whatever the hardware's k permutation inside a step.
// Accumulator start: every accumulator register starts at 1.5 * 2^23 + an integer (the first
// MFMA's C operand): a float in [2^23, 2^24) has ulp 1, so its bit pattern is 0x4B400000 + that
// integer + count * scale, with no conversion to integer.  k_knn2m (scale 2^0, train indices up to
// 65535) shifts the count up into dist << 16 | t; knn2_mfma (scale 2^13, at most 2048 rows) starts
// the accumulator with the row in the low bits and uses the register as its key unchanged
// ("knn2_mfma's keys" below).
// (The i8 form on v_mfma_i32_32x32x32_i8 that this replaced, bit-identical in its keys, is in the
// git history: the parent of "knn2_mfma: FP4 one-hot operands on the scaled MFMA".)
#pragma once
#include "gfpl_device.hpp"
#include "gfpl_layout.hpp"
#include <type_traits>

namespace gfpl {

typedef int mfma_v4i __attribute__((ext_vector_type(4)));
typedef int mfma_v8i __attribute__((ext_vector_type(8)));
typedef float mfma_v16f __attribute__((ext_vector_type(16)));

// k-steps (MFMAs) per tile: K = 512 (CELL 2) / 256 (CELL 1) in steps of 64
template <int CELL>
constexpr int knn_ksteps() { return (CELL == 2 ? 512 : 256) / 64; }

typedef mfma_v16f knn_acc_t;
constexpr float KNN_ACC_BIAS = 12582912.0f;   // 1.5 * 2^23
// 0x4B400000 + the integer the accumulator holds above 1.5 * 2^23
__device__ __forceinline__ uint32_t knn_acc_bits(float a) {
    return __float_as_uint(a);
}
// the scaled MFMA takes 8-dword operands; FP4 uses the first 4 (cbsz = blgp = 4).  Every product is
// multiplied by 2^S: the block scales are E8M0 bytes, 127 + S on the A side and 127 (2^0) on the B
// side, the same in every lane and byte, so whichever byte the hardware picks holds it
template <int S>
__device__ __forceinline__ knn_acc_t knn_mma(mfma_v4i a, mfma_v4i b, knn_acc_t c) {
    static_assert(S >= 0 && S < 32, "block scale 2^S");
    const mfma_v8i a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, -1, -1, -1, -1);
    const mfma_v8i b8 = __builtin_shufflevector(b, b, 0, 1, 2, 3, -1, -1, -1, -1);
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0x7F7F7F7F + S * 0x01010101, 0, 0x7F7F7F7F);
}

// FP4 expansions (the table entries, and the query side before its sign):
// two 2-bit cells (the low 4 bits of v) -> 8 nibbles, each cell one-hot (1.0) over its 4 values
__device__ __forceinline__ uint32_t fp4_cells2(uint32_t v) {
    return (2u << (4u * (v & 3u))) | (2u << (16u + 4u * ((v >> 2) & 3u)));
}
// 8 bits -> 8 nibbles of 0.0 / 1.0 (bit i at nibble i)
__device__ __forceinline__ uint32_t fp4_bits8(uint32_t b) {
    uint32_t x = b & 0xFFu;
    x = (x | (x << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return x << 1;
}

// operand fragment of k-step ks (K = 64) for a 32-byte descriptor held as 8 dwords.  Lane half h takes
//   CELL 2 (one-hot): bytes 4 ks + h, 4 ks + 2 + h (8 cells -> 32 nibbles)
//   CELL 1 (bits)   : bytes 8 ks + 2 h, +1, 8 ks + 4 + 2 h, +1 (32 bits -> 32 nibbles).
// Only the agreement of the A and the B side matters: element j of lane half h is multiplied with
// element j of lane half h whatever k the hardware calls it, and a dot product does not change
// under a common permutation of k.  Both sides expand the same descriptor bytes on the same lane
// half through the same function (fp4_cells2 / fp4_bits8, the table being that function tabulated).
// SIGNED (query side): CELL 1 maps bit b to 1 - 2 b, CELL 2 makes the one-hot -1.
template <int CELL, bool SIGNED>
__device__ __forceinline__ mfma_v4i knn_frag(const uint32_t* d, int ks, int h) {
    mfma_v4i f;
    if (CELL == 2) {   // bytes 4 ks + h and 4 ks + 2 + h live in dword ks
        const uint32_t w = d[ks] >> (8u * (uint32_t)h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // nibbles 0, 1 of byte 0, then of byte 2
            const uint32_t x = fp4_cells2((w >> (16 * (i >> 1) + 4 * (i & 1))) & 0xFu);
            f[i] = (int)(SIGNED ? x * 5u : x);   // 0x2 -> 0xA
        }
    } else {           // bytes 2 h, +1 of dwords 2 ks and 2 ks + 1
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = fp4_bits8(d[2 * ks + (i >> 1)] >> (16u * (uint32_t)h + 8u * (i & 1)));
            f[i] = (int)(SIGNED ? (x << 2) | 0x22222222u : x);   // bit 1 -> 0xA, bit 0 -> 0x2
        }
    }
    return f;
}

__device__ __forceinline__ int popc8(const uint32_t* d) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += __popc(d[i]);
    return s;
}

// Expansion table for the train (A) side, filled once per workgroup in LDS (knn_lut_dwords, gfpl_layout.hpp)
template <int CELL>
__device__ void knn_lut_fill(uint32_t* lut) {
    for (int b = threadIdx.x; b < 256; b += blockDim.x) {
        if (CELL == 2) {
            lut[2 * b] = fp4_cells2(b & 0xFu);
            lut[2 * b + 1] = fp4_cells2((uint32_t)b >> 4);
        } else {
            lut[b] = fp4_bits8(b);
        }
    }
}

// Train rows, staged per workgroup as per-lane-half views: the A fragment of k-step ks on lane half
// h takes the descriptor bytes knn_frag names, so view h of row t holds, in its dwords j = 0..3,
// exactly the bytes half h reads for k-steps 2j, 2j+1 (CELL 2) / j (CELL 1), in k-step order:
// V[(4 h + j) * stride + t].  A lane then reads its row's 16 bytes (4 dwords) per tile, and every
// fragment byte sits at a compile-time position of a view dword (no lane-dependent shifts).
template <int CELL>
__device__ __forceinline__ void knn_stage_views(uint32_t* T, int stride, const uint8_t* src, int nt) {
    constexpr uint32_t S0 = CELL == 2 ? 0x06040200u : 0x05040100u;   // v_perm selectors: bytes of (d[2j+1]:d[2j])
    constexpr uint32_t S1 = CELL == 2 ? 0x07050301u : 0x07060302u;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    for (int k = threadIdx.x; k < nt * 2; k += blockDim.x) {   // coalesced 16-B reads: dwords 4p .. 4p+3 of row t
        const uint4 v = s4[k];
        const int t = k >> 1, j = (k & 1) * 2;
        T[(0 + j) * stride + t] = __builtin_amdgcn_perm(v.y, v.x, S0);
        T[(1 + j) * stride + t] = __builtin_amdgcn_perm(v.w, v.z, S0);
        T[(4 + j) * stride + t] = __builtin_amdgcn_perm(v.y, v.x, S1);
        T[(5 + j) * stride + t] = __builtin_amdgcn_perm(v.w, v.z, S1);
    }
}

// ---- the pieces of a tile pass, shared by knn2_mfma (below) and k_knn2m (k_match.hip).  The
// accumulator counts from 0 and the distance offset (128 for HAMMING2 with the query one-hot
// negated, popc(q) for HAMMING) is added with the keys: acc + off is the distance.  k_knn2m's key
// bits are (acc << 16) + (off << 16) (mod 2^32); knn2_mfma's are further down.

// accumulator block holding the integer `off` (k_knn2m).  A pass builds the count-0 block once and
// holds it in 16 registers as every tile's first C operand (an empty asm per register makes it opaque
// to the compiler, which otherwise rebuilds the block with 16 moves per tile)
__device__ __forceinline__ knn_acc_t knn_acc_init(int off) {
    knn_acc_t c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = KNN_ACC_BIAS + (float)off;
    return c;
}

// distance offset of a query column's descriptor dwords qd, in key position
template <int CELL>
__device__ __forceinline__ uint32_t knn_query_offk(const uint32_t (&qd)[8]) {
    return (uint32_t)(CELL == 2 ? 128 : popc8(qd)) << 16;
}

// One 32x32 tile: a lane's four view dwords of train row rt * 32 + c from its half's view Th (zeros
// past nt), the train fragments from the knn_lut_fill<CELL> table and the k-steps' MFMAs onto acc.
// The table MUST be at LDS address 0 (first in the dynamic LDS of a kernel with no static
// __shared__): its reads are LDS instructions at the integer address (byte << log2 entry size), one
// SDWA shift of the view byte (the compiler resolves a dynamic-LDS address too late to fold it:
// table-relative reads cost one more VALU operation each, 16 per tile).
// knn2_mfma carries the same loads, table reads and MFMAs written out in its tile loop (k-step by
// k-step: its many waves hide the table reads' latency): with this function called from there the
// compiler orders the line kernels' instructions differently (the same instructions; k_cross_lines:
// four moves swapped), and those kernels are held to their assembly.  Change both together.
template <int CELL>
__device__ __forceinline__ knn_acc_t knn_tile(const uint32_t* Th, int tstride, int rt, int c, int nt, const mfma_v4i* bq,
                                              knn_acc_t acc) {
    typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const u32x2v lds_cu2;
    typedef __attribute__((address_space(3))) const uint32_t lds_cu1;
    const int t = rt * 32 + c;
    uint32_t tv[4];
    if (rt * 32 + 32 <= nt) {   // (wave-uniform: a full tile loads without bound tests)
#pragma unroll
        for (int j = 0; j < 4; ++j) tv[j] = Th[j * tstride + t];
    } else if (t < nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) tv[j] = Th[j * tstride + t];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) tv[j] = 0;
    }
    // view byte i of this lane half (knn_stage_views: k-step order) as a table byte offset
    auto ent = [&](int i, int sh) { return (uintptr_t)(((tv[i >> 2] >> (8 * (i & 3))) & 0xFFu) << sh); };
    mfma_v4i f[knn_ksteps<CELL>()];   // every k-step's table reads are issued before the first MFMA waits for one
#pragma unroll
    for (int ks = 0; ks < knn_ksteps<CELL>(); ++ks) {
        if (CELL == 2) {   // view bytes 2 ks, 2 ks + 1: 8-byte entries
            const u32x2v e0 = *reinterpret_cast<lds_cu2*>(ent(2 * ks, 3));
            const u32x2v e1 = *reinterpret_cast<lds_cu2*>(ent(2 * ks + 1, 3));
            f[ks][0] = (int)e0.x; f[ks][1] = (int)e0.y; f[ks][2] = (int)e1.x; f[ks][3] = (int)e1.y;
        } else {           // view dword ks: 4-byte entries
#pragma unroll
            for (int i = 0; i < 4; ++i) f[ks][i] = (int)*reinterpret_cast<lds_cu1*>(ent(4 * ks + i, 2));
        }
    }
#pragma unroll
    for (int ks = 0; ks < knn_ksteps<CELL>(); ++ks) acc = knn_mma<0>(f[ks], bq[ks], acc);
    return acc;
}

// train row (within the tile, less 4 * lane half) of accumulator register r
__device__ __forceinline__ uint32_t knn_acc_row(int r) { return (uint32_t)((r & 3) + 8 * (r >> 2)); }

// top-2 insertion of a key; k0 <= k1: the new second key is med3(k0, k1, key)
__device__ __forceinline__ void knn_top2(uint32_t& k0, uint32_t& k1, uint32_t key) {
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(k1) : "v"(k0), "v"(k1), "v"(key));
    k0 = min(k0, key);
}

// the two lane halves hold disjoint train rows of the same query column: both end with the column's top-2
__device__ __forceinline__ void knn_merge_halves(uint32_t& k0, uint32_t& k1) {
    const uint32_t o0 = __shfl_xor(k0, 32, 64);
    const uint32_t o1 = __shfl_xor(k1, 32, 64);
    const uint32_t lo = min(k0, o0), hi0 = max(k0, o0);
    k1 = min(hi0, min(k1, o1));
    k0 = lo;
}

// ---- knn2_mfma's keys: the accumulator's bits as the matrix core leaves them.
// Every product is scaled by 2^S (knn_mma<S>) and accumulator register r of lane half h starts at
// 1.5 * 2^23 + R0 + row(r) + 4 h, so a finished register holds the integer
//   1.5 * 2^23 + count * 2^S + (R0 + row + 4 h),
// a float in [2^23, 2^24), where ulp = 1 and the bit pattern is 0x4B000000 + that integer: read as
// uint32 it orders like (count, row in tile), lexicographically.  No shift and no add.
//   forward (per query, over the train rows): the distance offset (128 / popc(q)) is constant per
//     lane and enters only when the result is written.  The running top-2 is kept relative to the
//     current tile: both keys drop by 32 at every tile step, so a key of tile rt' seen from tile rt
//     has the row field R0 + row + 4 h - 32 (rt - rt'), >= 0 because R0 >= 32 (tiles - 1);
//   reverse (per train row, over the queries): only keys of one accumulator register and one lane
//     half are ever compared, so their row field is a common constant; adding off * 2^S + q gives
//     0x4B400000 + dist * 2^S + (R0 + row + 4 h) + q, and the lane that ends with the row's
//     minimum subtracts R0 + row + 4 h once: rl_key holds 0x4B400000 + dist * 2^S + q.
// Ranges: |count| <= 256, so count * 2^S stays within +-2^21 of the 2^22 that 1.5 * 2^23 has in
// its mantissa; the row field (plus the query index, in the reverse direction) stays below 2^S.
constexpr int KNN_KEY_S = 13;                   // log2 of the count's unit in a key
constexpr int KNN_KEY_R0 = 2016;                // row field of row 0 of the tile a key is relative to
constexpr int KNN_KEY_CAP = 2048;               // most train rows / queries of a pass: the largest kl_cap (gfpl_abi.hip)
constexpr int KNN_KEY_COUNT = 256;              // |count| <= 256 (HAMMING; HAMMING2: 128)
constexpr uint32_t KNN_KEY_BASE = 0x4B400000u;  // bits of 1.5 * 2^23
constexpr uint32_t KNN_KEY_PAD = 0x40000000u;   // added to a padded query column's reverse keys
constexpr uint32_t KNN_IDX_MASK = (1u << KNN_KEY_S) - 1u;   // the query index of a reverse key (rl_key)
static_assert(KNN_KEY_R0 >= 32 * ((KNN_KEY_CAP + 31) / 32 - 1), "a tile-relative row field would borrow from the count");
static_assert(KNN_KEY_R0 + 31 + (KNN_KEY_CAP - 1) < (1 << KNN_KEY_S), "row field + query index would carry into the count");
static_assert((KNN_KEY_COUNT << KNN_KEY_S) <= (1 << 22), "1.5 * 2^23 - 256 * 2^S must stay >= 2^23");
static_assert((KNN_KEY_COUNT << KNN_KEY_S) + (1 << KNN_KEY_S) <= (1 << 22), "1.5 * 2^23 + 256 * 2^S + row field must stay < 2^24");
static_assert(KNN_KEY_BASE + (1u << 22) + KNN_KEY_PAD < 0xFFFFFFFFu - 32u * 64u, "pad keys and aged sentinels stay apart");

// distance offset of a query column: acc + off is the distance
template <int CELL>
__device__ __forceinline__ uint32_t knn_query_off(const uint32_t (&qd)[8]) {
    return (uint32_t)(CELL == 2 ? 128 : popc8(qd));
}

// a forward key of knn2_mfma (relative to tile nrt - 1, lane's offset off) as dist << 16 | t
__device__ __forceinline__ uint32_t knn_key_decode(uint32_t k, uint32_t off, int nrt) {
    const uint32_t u = k - KNN_KEY_BASE + (off << KNN_KEY_S);
    const uint32_t t = (u & KNN_IDX_MASK) + (uint32_t)(32 * (nrt - 1) - KNN_KEY_R0);
    return k >= 0x80000000u ? 0xFFFFFFFFu : ((u >> KNN_KEY_S) << 16) | t;   // (no such train row: the start value, aged)
}

// Two levels of the reverse direction's reduce-scatter select on a lane bit that is a whole DPP
// bank (row_mirror: bit 3 = banks 2, 3; row_half_mirror: bit 2 = banks 1, 3).  A lane of the lower
// banks keeps a and takes its partner's a, a lane of the upper banks keeps b and takes its
// partner's b: a = min(a, dpp(a)) written to the lower banks only, then a = min(b, dpp(b)) to the
// upper ones — two instructions per exchange and no selects; four exchanges per statement.  A DPP
// read needs two wait states after a VALU write of its register, and the compiler does not look
// inside a statement: each statement puts them before its first DPP read itself.
#define GFPL_KNN_XCHG4(CTRL, LO, HI)                                              \
    "v_min_u32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:" LO "\n\t"         \
    "v_min_u32_dpp %0, %4, %4 " CTRL " row_mask:0xf bank_mask:" HI "\n\t"         \
    "v_min_u32_dpp %1, %1, %1 " CTRL " row_mask:0xf bank_mask:" LO "\n\t"         \
    "v_min_u32_dpp %1, %5, %5 " CTRL " row_mask:0xf bank_mask:" HI "\n\t"         \
    "v_min_u32_dpp %2, %2, %2 " CTRL " row_mask:0xf bank_mask:" LO "\n\t"         \
    "v_min_u32_dpp %2, %6, %6 " CTRL " row_mask:0xf bank_mask:" HI "\n\t"         \
    "v_min_u32_dpp %3, %3, %3 " CTRL " row_mask:0xf bank_mask:" LO "\n\t"         \
    "v_min_u32_dpp %3, %7, %7 " CTRL " row_mask:0xf bank_mask:" HI
// partner p ^ 15, on the accumulator's bits: first the eight reverse keys, a += qo, b += qo, in place
// (the eight adds also put the wait states between each key's write and its DPP read).  k0 and k1
// are not used: naming the finished top-2 as operands keeps the statement behind the last reader of
// the accumulator's registers, which it overwrites — placed earlier, the compiler copies them first
__device__ __forceinline__ void knn_xchg4_mirror(uint32_t* a, uint32_t* b, uint32_t qo, uint32_t k0, uint32_t k1) {
    asm("v_add_u32 %0, %0, %8\n\tv_add_u32 %4, %4, %8\n\tv_add_u32 %1, %1, %8\n\tv_add_u32 %5, %5, %8\n\t"
        "v_add_u32 %2, %2, %8\n\tv_add_u32 %6, %6, %8\n\tv_add_u32 %3, %3, %8\n\tv_add_u32 %7, %7, %8\n\t"
        GFPL_KNN_XCHG4("row_mirror", "0x3", "0xc")
        : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])
        : "v"(qo), "v"(k0), "v"(k1));
}
__device__ __forceinline__ void knn_xchg4_half_mirror(uint32_t* a, const uint32_t* b) {   // partner p ^ 7, on keys
    asm("s_nop 1\n\t" GFPL_KNN_XCHG4("row_half_mirror", "0x5", "0xa")
        : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]) : "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));
}
#undef GFPL_KNN_XCHG4

// One knn pass of a workgroup: every query q < nq against the train rows of T (LDS,
// knn_stage_views; the table of knn_tile at LDS address 0).  Queries are read from Q (global,
// 32-byte rows).  Writes out_k0[q] = lexicographic minimum key (dist << 16 | t) and out_k1[q] = the
// second one.  Waves split the query column tiles.
// Inlined into its callers: as a called function its register save area sat in
// scratch and capped k_stereo_lines at 128 VGPRs (inlined: 121, no scratch; 4.95 -> 4.27 ms)
// The reverse direction in the same pass: Hamming distance is symmetric, so tile
// (t, q) also holds the train-side query's distances — for every train row t the
// lexicographic minimum of (dist, q) over the queries is taken over the 16 lanes of each
// DPP row by a reduce-scatter (in the epilogue), then one LDS atomicMin per lane into
// rl_key[t] (initialised to 0xFFFFFFFF by the caller): the knn-1 of the train rows
// against the queries, the OpenCV tie rule included, without a second MFMA pass.  rl_key[t] ends
// as 0x4B400000 + dist * 2^S + q: its readers take the query index, rl_key[t] & KNN_IDX_MASK.  A
// padded query column (q >= nq) carries keys above every real one (KNN_KEY_PAD instead of q).
// The tile epilogue has no per-row branches and takes its keys from the accumulator as they are
// (above): 85 VALU per full tile — 2 to age the top-2, 32 for the top-2 (v_med3, v_min), 16 adds for
// the reverse keys, 34 for their reduce-scatter, 1 for the row field; full tiles skip the row-bound tests.
template <int CELL>
__device__ __forceinline__ void knn2_mfma(const uint32_t* T, int tstride, int nt, const uint8_t* Q, int nq, uint32_t* out_k0,
                                          uint32_t* out_k1, uint32_t* rl_key) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int nct = (nq + 31) >> 5, nrt = (nt + 31) >> 5;
    typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const u32x2v lds_cu2;
    typedef __attribute__((address_space(3))) const uint32_t lds_cu1;
    const uint32_t* Th = T + 4 * h * tstride;   // this lane half's view
    const int pr = lane & 15;   // position in the 16-lane DPP row: the train row (of the lane half) it reduces
    const bool rb1 = (pr & 2) != 0, rb0 = (pr & 1) != 0;
    const uint32_t lro = (uint32_t)(4 * h + (pr & 3) + 8 * (pr >> 2));
    const uint32_t rsub = (uint32_t)KNN_KEY_R0 + lro;   // the row field of the row this lane reduces
    // every tile's first C operand: the count-0 block with the row fields, built once and held in 16
    // registers (an empty asm per register makes it opaque to the compiler, which otherwise rebuilds
    // the block per tile)
    knn_acc_t acc0;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = KNN_ACC_BIAS + (float)(KNN_KEY_R0 + (int)knn_acc_row(r) + 4 * h);
#pragma unroll
    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(acc0[r]));   // (held)
    for (int ct = wave; ct < nct; ct += nwave) {
        const int q = ct * 32 + c;
        uint32_t qd[8];
        if (q < nq) load_desc(Q + (size_t)q * 32, qd);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) qd[i] = 0;
        }
        mfma_v4i bq[knn_ksteps<CELL>()];
#pragma unroll
        for (int ks = 0; ks < knn_ksteps<CELL>(); ++ks) {
            bq[ks] = knn_frag<CELL, true>(qd, ks, h);
        }
        const uint32_t off = knn_query_off<CELL>(qd);
        const uint32_t qo = (off << KNN_KEY_S) + (q < nq ? (uint32_t)q : KNN_KEY_PAD);   // what a reverse key adds to the accumulator's bits
        uint32_t k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu;
        for (int rt = 0; rt < nrt; ++rt) {
            // acc = knn_tile<CELL>(Th, tstride, rt, c, nt, bq, acc0), written out (see knn_tile)
            const int t = rt * 32 + c;
            uint32_t tv[4];
            if (rt * 32 + 32 <= nt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) tv[j] = Th[j * tstride + t];
            } else if (t < nt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) tv[j] = Th[j * tstride + t];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) tv[j] = 0;
            }
            knn_acc_t acc = acc0;
#pragma unroll
            for (int ks = 0; ks < knn_ksteps<CELL>(); ++ks) {
                auto ent = [&](int i, int sh) { return (uintptr_t)(((tv[i >> 2] >> (8 * (i & 3))) & 0xFFu) << sh); };
                mfma_v4i f;
                if (CELL == 2) {
                    const u32x2v e0 = *reinterpret_cast<lds_cu2*>(ent(2 * ks, 3));
                    const u32x2v e1 = *reinterpret_cast<lds_cu2*>(ent(2 * ks + 1, 3));
                    f[0] = (int)e0.x; f[1] = (int)e0.y; f[2] = (int)e1.x; f[3] = (int)e1.y;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) f[i] = (int)*reinterpret_cast<lds_cu1*>(ent(4 * ks + i, 2));
                }
                acc = knn_mma<KNN_KEY_S>(f, bq[ks], acc);
            }
            const uint32_t tb = (uint32_t)(rt * 32 + 4 * h);
            k0 -= 32u;   // the running top-2 relative to this tile (the start value stays above every key)
            k1 -= 32u;
            // the reverse direction by a reduce-scatter over each 16-lane DPP row: four exchange steps
            // (row_mirror, row_half_mirror, quad_perm 3210, quad_perm 1032: partners p ^ 15, p ^ 7,
            // p ^ 3, p ^ 1) each halve the rows a lane carries — it keeps the half its lane bit selects
            // and takes the partner's minimum of that half — so lane p ends with the 16-lane minimum of
            // row p, and every lane does one atomic.  The first two steps select on whole DPP banks
            // (knn_xchg4_*: 2 operations per exchange), the last two by v_cndmask (3 per exchange)
            auto epilogue = [&](auto chk_t) {
                constexpr bool chk = decltype(chk_t)::value;
                auto top2 = [&](int r) {
                    uint32_t key = knn_acc_bits(acc[r]);
                    if (chk && (int)(tb + knn_acc_row(r)) >= nt) key = 0xFFFFFFFFu;
                    knn_top2(k0, k1, key);
                };
                auto xchg = [](uint32_t a, uint32_t b, bool upper, auto ctrl_t) {   // keep one, take the partner's other
                    const uint32_t send = upper ? a : b, keep = upper ? b : a;
                    return min(keep, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)send, decltype(ctrl_t)::value, 0xF, 0xF, false));
                };
                uint32_t y[8], yb[8];   // reverse keys of rows r, r + 8 (+ the lane's row field, until the end)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    top2(j);
                    top2(j + 8);
                    y[j] = knn_acc_bits(acc[j]);
                    yb[j] = knn_acc_bits(acc[j + 8]);
                }
                knn_xchg4_mirror(y, yb, qo, k0, k1);   // (the accumulator's registers become the keys, in place)
                knn_xchg4_mirror(y + 4, yb + 4, qo, k0, k1);
                knn_xchg4_half_mirror(y, y + 4);
                const uint32_t w0 = xchg(y[0], y[2], rb1, std::integral_constant<int, 0x1B>{});   // quad_perm 3210
                const uint32_t w1 = xchg(y[1], y[3], rb1, std::integral_constant<int, 0x1B>{});
                const uint32_t f = xchg(w0, w1, rb0, std::integral_constant<int, 0xB1>{});       // quad_perm 1032
                const uint32_t tr = (uint32_t)(rt * 32) + lro;
                if (!chk || (int)tr < nt) atomicMin(&rl_key[tr], f - rsub);
            };
            if (rt * 32 + 32 <= nt) epilogue(std::false_type{});   // (wave-uniform)
            else epilogue(std::true_type{});
        }
        knn_merge_halves(k0, k1);
        if (h == 0 && q < nq) {
            out_k0[q] = knn_key_decode(k0, off, nrt);
            out_k1[q] = knn_key_decode(k1, off, nrt);
        }
    }
}

}  // namespace gfpl
