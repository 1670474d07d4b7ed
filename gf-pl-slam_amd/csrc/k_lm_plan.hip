// k_lm_plan.hip — the landmark descriptor store's planner on the device (include/gfpl.h):
// what gfpl_lm_plan.cpp does on the host, for the call shapes whose arrays are already on the device
// (the pairs / lm_out of gfpl_kfmap's observe calls, the id lists of remove_bad and select).
//
//  k_lm_obs_check   : one thread per pair: every refusal, the landmark's list length read from the
//                     store's count[], the pairs each landmark receives counted (pend) — the scheme of
//                     k_mapgeo_obs_check.
//  k_lm_obs_reduce  : a pair's place is its rank among its landmark's pairs, in pair order; only a
//                     landmark with more than one pair (pend > 1) looks at earlier pairs.  The pair at
//                     place 0 is its landmark's leader and stands for one work item; per tile of
//                     LM_PLAN_TILE pairs and per bucket the leaders and their ops are counted.
//  k_lm_obs_scan    : the two exclusive scans over (bucket, tile), bucket-major (one workgroup):
//                     bucket_start[] and the op total into the header, GFPL_E_CAPACITY past max_ops.
//  k_lm_obs_scatter : the leaders' LmWork in bucket order, pair order within a bucket, and every touched
//                     landmark's first op.
//  k_lm_obs_ops     : every pair's one or two LmOpDev at op0 + place of its landmark, the source row's
//                     address resolved here; pend back to zero, refused or not.
//  k_lm_ids_check, k_lm_free_apply : an id list's refusals; GFPL_LM_FREE of every listed id.
// k_lm_apply_dev<G> (k_lm.hip) then runs the six buckets from the header.  Every kernel after the check
// reads the call's error word first and neither indexes with the call's data nor changes the store when
// it is set.  Everything is integer and no result depends on the order workgroups run in.
#include <algorithm>

#include "gfpl_kernels.hpp"
#include "gfpl_wave.hpp"

namespace gfpl {

namespace {

constexpr int PER_THREAD = LM_PLAN_TILE / LM_BLOCK;
static_assert(LM_PLAN_TILE % LM_BLOCK == 0, "a thread takes whole pairs");
// a leader's ops are all the pairs its landmark receives in the call, wherever they lie: up to LM_MAX_OBS of them,
// so a tile's op sum of one bucket reaches LM_PLAN_TILE * LM_MAX_OBS and is scanned as an int of its own
static_assert((long long)LM_PLAN_TILE * LM_MAX_OBS < (1ll << 31), "a tile's op sum fits an int");

GFPL_DEV void raise(int32_t* hdr, int bits) {
    // one atomic per wave that has anything to report
    int all = bits;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) all |= __shfl_xor(all, o, 64);
    if (all && (threadIdx.x & 63) == 0) atomicOr(&hdr[LM_H_ERR], all);
}

// the desc1 row of pair (p0, p1): p1 itself, or unm_rows[p1] in the local-map stage; -1 when p1 names none
GFPL_DEV int desc1_row(const LmObserve& a, int p1) {
    if (!a.unm_rows) return p1;
    return (unsigned)p1 < (unsigned)a.n_unm ? a.unm_rows[p1] : -1;
}

// a leader's work item: the ops its landmark receives (a created one its two rows) and the bucket of the
// list's final length, which with ADDs only is also its peak
GFPL_DEV void lead_item(const LmStoreDev& st, const LmPlanDev& p, const LmObserve& a, int id, int* count0, int* n_ops, int* bucket) {
    *count0 = st.count[id];
    *n_ops = p.pend[id] + (id >= a.first_new ? 1 : 0);
    *bucket = lm_bucket_of(*count0 + *n_ops, p.min_g);
}

}  // namespace

__global__ void __launch_bounds__(LM_BLOCK) k_lm_obs_check(LmStoreDev st, LmPlanDev p, LmObserve a) {
    const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
    int err = 0;
    if (i < a.n) {
        const int p0 = a.pairs[2 * (size_t)i], p1 = a.pairs[2 * (size_t)i + 1];
        if (!a.unm_rows && (unsigned)p0 >= (unsigned)a.n0) err |= KFMAP_ERR_INVALID;
        if ((unsigned)desc1_row(a, p1) >= (unsigned)a.n1) err |= KFMAP_ERR_INVALID;
        const int id = a.lm_out[i];
        if (id < -1 || id >= p.lm_cap) {
            err |= KFMAP_ERR_INVALID;
        } else if (id >= 0) {
            const int n0 = st.count[id];
            const int before = atomicAdd(&p.pend[id], 1);
            if (id >= a.first_new) {
                if (n0 != 0 || before != 0) err |= KFMAP_ERR_INVALID;   // a created id holds nothing and has one pair
                else if (st.obs_cap < 2) err |= KFMAP_ERR_CAPACITY;
            } else if (n0 <= 0) {
                err |= KFMAP_ERR_INVALID;
            } else if (n0 + before + 1 > st.obs_cap) {
                err |= KFMAP_ERR_CAPACITY;   // the pair that counted last sees the list's final length
            }
        }
    }
    raise(p.hdr, err);
}

__global__ void __launch_bounds__(LM_BLOCK) k_lm_obs_reduce(LmStoreDev st, LmPlanDev p, LmObserve a, int nt) {
    __shared__ int cnt[2 * LM_BUCKETS];
    if (p.hdr[LM_H_ERR] != 0) return;
    if (threadIdx.x < 2 * LM_BUCKETS) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int j0 = blockIdx.x * LM_PLAN_TILE + threadIdx.x * PER_THREAD;
    int n_w[LM_BUCKETS] = {0, 0, 0, 0, 0, 0}, n_o[LM_BUCKETS] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < PER_THREAD && j0 + k < a.n; ++k) {
        const int i = j0 + k, id = a.lm_out[i];
        if (id < 0) continue;   // :308
        int place = 0;
        if (p.pend[id] > 1)
            for (int j = 0; j < i; ++j) place += a.lm_out[j] == id;
        p.place[i] = place;
        if (place != 0) continue;
        int count0, n_ops, bucket;
        lead_item(st, p, a, id, &count0, &n_ops, &bucket);
#pragma unroll
        for (int b = 0; b < LM_BUCKETS; ++b) {
            n_w[b] += bucket == b;
            n_o[b] += bucket == b ? n_ops : 0;
        }
    }
    // a thread's sums, then the wave's, then one LDS add per wave and bucket
#pragma unroll
    for (int b = 0; b < LM_BUCKETS; ++b) {
        int w = n_w[b], o = n_o[b];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            w += __shfl_xor(w, d, 64);
            o += __shfl_xor(o, d, 64);
        }
        if ((threadIdx.x & 63) == 0 && w) {
            atomicAdd(&cnt[b], w);
            atomicAdd(&cnt[LM_BUCKETS + b], o);
        }
    }
    __syncthreads();
    if (threadIdx.x < LM_BUCKETS) {
        p.tile_w[(size_t)threadIdx.x * nt + blockIdx.x] = cnt[threadIdx.x];
        p.tile_o[(size_t)threadIdx.x * nt + blockIdx.x] = cnt[LM_BUCKETS + threadIdx.x];
    }
}

__global__ void __launch_bounds__(LM_BLOCK) k_lm_obs_scan(LmPlanDev p, int nt) {
    __shared__ int scan[LM_BLOCK / 64 + 1];
    if (p.hdr[LM_H_ERR] != 0) return;
    const int n_work = scan_tiles<LM_BLOCK>(p.tile_w, LM_BUCKETS * nt, scan);
    const int n_ops = scan_tiles<LM_BLOCK>(p.tile_o, LM_BUCKETS * nt, scan);
    if (n_work > p.max_ops || n_ops > p.max_ops) {
        if (threadIdx.x == 0) atomicOr(&p.hdr[LM_H_ERR], KFMAP_ERR_CAPACITY);   // bucket_start stays all zero
        return;
    }
    __syncthreads();   // the scans' stores, by other threads of this workgroup
    if (threadIdx.x <= LM_BUCKETS) p.hdr[LM_H_BUCKET + threadIdx.x] = p.tile_w[(size_t)threadIdx.x * nt];
    if (threadIdx.x == 0) p.hdr[LM_H_NOPS] = n_ops;
}

__global__ void __launch_bounds__(LM_BLOCK) k_lm_obs_scatter(LmStoreDev st, LmPlanDev p, LmObserve a, LmWork* work, int nt) {
    __shared__ int scan[LM_BLOCK / 64 + 1];
    if (p.hdr[LM_H_ERR] != 0) return;
    const int j0 = blockIdx.x * LM_PLAN_TILE + threadIdx.x * PER_THREAD;
    int id[PER_THREAD], count0[PER_THREAD], n_ops[PER_THREAD], bucket[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        bucket[k] = -1;
        count0[k] = n_ops[k] = 0;
        id[k] = j0 + k < a.n ? a.lm_out[j0 + k] : -1;
        if (id[k] >= 0 && p.place[j0 + k] == 0) lead_item(st, p, a, id[k], &count0[k], &n_ops[k], &bucket[k]);
    }
    for (int b = 0; b < LM_BUCKETS; ++b) {
        const size_t f = (size_t)b * nt + blockIdx.x;
        const int w0 = p.tile_w[f];
        if (p.tile_w[f + 1] == w0) continue;   // (the workgroup's own count: the same in every thread)
        // two scans: a tile's leaders, and their ops (a leader has up to LM_MAX_OBS: the sums do not share a word)
        int mine_w = 0, mine_o = 0;
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k)
            if (bucket[k] == b) {
                ++mine_w;
                mine_o += n_ops[k];
            }
        int total;
        int w = w0 + block_exclusive_scan<LM_BLOCK>(mine_w, scan, &total);
        int o = p.tile_o[f] + block_exclusive_scan<LM_BLOCK>(mine_o, scan, &total);
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            if (bucket[k] != b) continue;
            work[w++] = LmWork{id[k], o, n_ops[k], count0[k]};
            p.op0[id[k]] = o;
            o += n_ops[k];
        }
    }
}

__global__ void __launch_bounds__(LM_BLOCK) k_lm_obs_ops(LmPlanDev p, LmObserve a, LmOpDev* ops) {
    const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int id = a.lm_out[i];
    if ((unsigned)id >= (unsigned)p.lm_cap) return;
    p.pend[id] = 0;   // the scratch as it was, refused or not (no kernel from here on reads it)
    if (p.hdr[LM_H_ERR] != 0) return;
    const uint8_t* row1 = a.desc1 + 32 * (size_t)desc1_row(a, a.pairs[2 * (size_t)i + 1]);
    LmOpDev* o = ops + p.op0[id];
    if (id >= a.first_new) {
        o[0] = LmOpDev{a.desc0 + 32 * (size_t)a.pairs[2 * (size_t)i], GFPL_LM_ADD, 0};
        o[1] = LmOpDev{row1, GFPL_LM_ADD, 0};
    } else {
        o[p.place[i]] = LmOpDev{row1, GFPL_LM_ADD, 0};
    }
}

// need_obs: an id whose list is empty is refused too (gather)
__global__ void __launch_bounds__(LM_BLOCK) k_lm_ids_check(LmStoreDev st, LmPlanDev p, const int32_t* ids, int n, int need_obs) {
    const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
    int err = 0;
    if (i < n) {
        const int id = ids[i];
        if ((unsigned)id >= (unsigned)p.lm_cap) err = KFMAP_ERR_INVALID;
        else if (need_obs && st.count[id] <= 0) err = KFMAP_ERR_INVALID;
    }
    raise(p.hdr, err);
}

// what GFPL_LM_FREE leaves through k_lm_apply: count 0, med_idx -1, a zeroed median row, the rows as they are
__global__ void __launch_bounds__(LM_BLOCK) k_lm_free_apply(LmStoreDev st, LmPlanDev p, const int32_t* ids, int n) {
    const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
    if (i >= n || p.hdr[LM_H_ERR] != 0) return;
    const int id = ids[i];
    st.count[id] = 0;
    st.med_idx[id] = -1;
    uint4* m = reinterpret_cast<uint4*>(st.med + (size_t)id * 32);
    m[0] = make_uint4(0, 0, 0, 0);
    m[1] = make_uint4(0, 0, 0, 0);
}

static unsigned blocks_of(int n) { return (unsigned)(((size_t)n + LM_BLOCK - 1) / LM_BLOCK); }
static unsigned tiles_of(int n) { return (unsigned)(((size_t)n + LM_PLAN_TILE - 1) / LM_PLAN_TILE); }

hipError_t enqueue_lm_observe(const LmStoreDev& st, const LmPlanDev& p, const LmObserve& a, LmWork* work, LmOpDev* ops,
                              hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const unsigned nb = blocks_of(a.n), nt = tiles_of(a.n);
    hipLaunchKernelGGL(k_lm_obs_check, dim3(nb), dim3(LM_BLOCK), 0, s, st, p, a);
    hipLaunchKernelGGL(k_lm_obs_reduce, dim3(nt), dim3(LM_BLOCK), 0, s, st, p, a, (int)nt);
    hipLaunchKernelGGL(k_lm_obs_scan, dim3(1), dim3(LM_BLOCK), 0, s, p, (int)nt);
    hipLaunchKernelGGL(k_lm_obs_scatter, dim3(nt), dim3(LM_BLOCK), 0, s, st, p, a, work, (int)nt);
    hipLaunchKernelGGL(k_lm_obs_ops, dim3(nb), dim3(LM_BLOCK), 0, s, p, a, ops);
    hipError_t e = hipGetLastError();
    // the buckets a list of 1 .. obs_cap rows can fall into, each sized for all the landmarks the call can touch
    unsigned used = 0;
    for (int peak = 1; peak <= st.obs_cap; ++peak) used |= 1u << lm_bucket_of(peak, p.min_g);
    for (int b = 0; b < LM_BUCKETS && e == hipSuccess; ++b)
        if (used >> b & 1) e = launch_lm_apply_dev(st, work, ops, p.hdr, std::min(a.n, p.lm_cap), b, s);
    return e;
}

hipError_t enqueue_lm_free_ids(const LmStoreDev& st, const LmPlanDev& p, const int32_t* ids, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_lm_ids_check, dim3(blocks_of(n)), dim3(LM_BLOCK), 0, s, st, p, ids, n, 0);
    hipLaunchKernelGGL(k_lm_free_apply, dim3(blocks_of(n)), dim3(LM_BLOCK), 0, s, st, p, ids, n);
    return hipGetLastError();
}

hipError_t enqueue_lm_gather_ids(const LmStoreDev& st, const LmPlanDev& p, const int32_t* ids, int n, uint8_t* desc_out,
                                 int32_t* med_idx_out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_lm_ids_check, dim3(blocks_of(n)), dim3(LM_BLOCK), 0, s, st, p, ids, n, 1);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_lm_gather_dev(st, p.hdr, ids, n, desc_out, med_idx_out, s);
}

}  // namespace gfpl
