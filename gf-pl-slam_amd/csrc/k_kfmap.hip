// k_kfmap.hip — the map's index half (include/gfpl.h): MapHandler's integer bookkeeping.
//
//  k_kfmap_add_kf      : initialize / addKeyFrame's keyframe record and index reset.
//  k_kfmap_obs_check   : one thread per pair of an observe call: every refusal, the pair's landmark,
//                        its list length before the call and the place of its own entry; the creating
//                        pairs of each workgroup counted.
//  k_kfmap_obs_scan    : one workgroup: the ordered exclusive scan of those counts, the id capacity,
//                        the next id and the creating pairs' graph word.
//  k_kfmap_obs_apply   : the loop body of lookForCommonMatches' two stages (src/mapHandler.cpp:266-336,
//                        404-485, 609-624, 745-764).
//  k_kfmap_flm_*       : formLocalMap (:789-857): reset, one workgroup marking keyframes from the newest
//                        row of the graph, a grid over (keyframe, row) setting landmark flags.
//  k_kfmap_cmp_*       : an ordered compaction as reduce, scan, scatter: tile sums in the workspace, no
//                        workgroup waits for another.
//  k_kfmap_bad_*       : removeBadMapLandmarks (:2550-2630) after the compaction of its landmarks: the
//                        lowest carrying row by atomicMin, then the removal.
// Everything is integer and every result independent of the order workgroups run in: ids come from
// an ordered scan, graph words from integer atomics, concurrent stores to one address write one value.
// A mutating kernel reads the call's error word first and leaves the state alone when it is set.
#include <algorithm>

#include "gfpl_kernels.hpp"
#include "gfpl_wave.hpp"

namespace gfpl {

namespace {

constexpr int PER_THREAD = KFMAP_TILE / KFMAP_BLOCK;
static_assert(PER_THREAD == 8, "a thread's items are one 8-byte word of flags");
constexpr int ROW_NONE = 0x7fffffff;

GFPL_DEV void raise(const KfMapCore& c, int bits) {
    // one atomic per wave that has anything to report
    int all = bits;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) all |= __shfl_xor(all, o, 64);
    if (all && (threadIdx.x & 63) == 0) atomicOr(&c.hdr[KFMAP_H_ERR], all);
}

// full_graph[kf1][o]++ and its mirror for the lanes with `active`, lanes of one o combined into one add
GFPL_DEV void graph_add(const KfMapCore& c, int kf1, int o, bool active) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int key = __shfl(o, lead, 64);
        const unsigned long long same = __ballot(active && o == key);
        if (lane == lead) {
            const int cnt = __popcll(same);
            atomicAdd(&c.graph[(size_t)kf1 * c.kf_cap + key], cnt);
            atomicAdd(&c.graph[(size_t)key * c.kf_cap + kf1], cnt);
        }
        todo &= ~same;
    }
}

// bit b: byte b of v is not zero
GFPL_DEV unsigned bytes_to_bits(uint64_t v) {
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) m |= (unsigned)(((v >> (8 * b)) & 0xff) != 0) << b;
    return m;
}
// cnt <= 8 flags from j0 on (j0 a multiple of 8, the array 8-B aligned and cnt == 8 wherever the word is read whole)
GFPL_DEV unsigned load_flags(const uint8_t* p, int j0, int cnt) {
    if (cnt == 8) return bytes_to_bits(*reinterpret_cast<const uint64_t*>(p + j0));
    unsigned m = 0;
    for (int b = 0; b < cnt; ++b) m |= (unsigned)(p[j0 + b] != 0) << b;
    return m;
}

// removeBadMapLandmarks' condition on an alive landmark (:2558-2560; KM2, KM4, KM7)
GFPL_DEV bool lm_is_bad(const KfMapCore& c, const KfMapLm& L, const KfMapSelect& a, int j) {
    if (L.local[j]) return false;
    const int n = L.nobs[j];
    const int k0 = L.obs[(size_t)j * c.obs_cap];
    if ((unsigned)k0 >= (unsigned)c.n_kf) return false;
    if (c.n_kf - 1 - k0 <= a.cull_age) return false;
    if (L.inlier[j] && n >= a.min_lm_obs) return false;
    return c.kf_alive[k0] != 0;
}

// the items [j0, j0 + 8) of a compaction that its condition selects, as bits
GFPL_DEV unsigned select_bits(const KfMapCore& c, const KfMapLm& L, const KfMapSelect& a, int j0) {
    if (j0 >= a.n) return 0;
    const int cnt = min(8, a.n - j0);
    unsigned m = 0;
    if (a.mode == KFMAP_SEL_UNMATCHED) {
        const int32_t* row = L.idx + (size_t)a.kf * L.rows;
        for (int b = 0; b < cnt; ++b) m |= (unsigned)(row[j0 + b] == -1) << b;
        return m;
    }
    m = load_flags(L.alive, j0, cnt);
    if (a.mode == KFMAP_SEL_ALIVE || m == 0) return m;
    if (a.mode == KFMAP_SEL_LOCAL) return m & load_flags(L.local, j0, cnt);
    if (a.mode == KFMAP_SEL_LOCAL_UNSEEN) {
        m &= load_flags(L.local, j0, cnt);
        for (int b = 0; b < cnt; ++b) {
            if (!(m >> b & 1)) continue;
            const int j = j0 + b;
            const int n = min(max(L.nobs[j], 1), c.obs_cap);
            if (L.obs[(size_t)j * c.obs_cap + n - 1] == a.kf) m &= ~(1u << b);   // kf_obs_list.back() == kf1
        }
        return m;
    }
    for (int b = 0; b < cnt; ++b)
        if ((m >> b & 1) && !lm_is_bad(c, L, a, j0 + b)) m &= ~(1u << b);
    return m;
}

}  // namespace

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_add_kf(KfMapCore c, KfMapLm pt, KfMapLm ls, int n_pt, int n_ls) {
    const int t = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    const int kf = c.n_kf;
    if (t < pt.rows) pt.idx[(size_t)kf * pt.rows + t] = -1;
    if (t < ls.rows) ls.idx[(size_t)kf * ls.rows + t] = -1;
    // expandGraphs: the new row and column are zero
    if (t <= kf) {
        c.graph[(size_t)kf * c.kf_cap + t] = 0;
        c.graph[(size_t)t * c.kf_cap + kf] = 0;
    }
    if (t == 0) {
        c.kf_alive[kf] = 1;
        c.kf_local[kf] = 1;
        pt.kf_n[kf] = n_pt;
        ls.kf_n[kf] = n_ls;
        c.hdr[KFMAP_H_NKF] = kf + 1;
    }
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_obs_check(KfMapCore c, KfMapLm L, KfMapObserve a) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    int err = 0, id = -1, creating = 0;
    if (i < a.n) {
        const int p0 = a.pairs[2 * (size_t)i], p1 = a.pairs[2 * (size_t)i + 1];
        int r1 = -1;
        if (a.kf0 >= 0) {
            if ((unsigned)p0 < (unsigned)L.kf_n[a.kf0]) {
                id = L.idx[(size_t)a.kf0 * L.rows + p0];
                if (id == -1) creating = 1;
                else if ((unsigned)id >= (unsigned)L.next) { err |= KFMAP_ERR_INVALID; id = -1; }
                else if (!L.alive[id]) id = -1;   // a freed landmark: the pair does nothing (:308)
            } else {
                err |= KFMAP_ERR_INVALID;
            }
            r1 = p1;
        } else {
            if ((unsigned)p0 < (unsigned)a.n_sel) {
                id = a.sel_ids[p0];
                if ((unsigned)id >= (unsigned)L.next || !L.alive[id]) { err |= KFMAP_ERR_INVALID; id = -1; }
            } else {
                err |= KFMAP_ERR_INVALID;
            }
            if ((unsigned)p1 < (unsigned)a.n_unm) r1 = a.unm_rows[p1];
        }
        // a value twice in a column: the call's number is already there
        if ((unsigned)p0 < (unsigned)(a.kf0 >= 0 ? L.rows : a.n_sel)) {
            if (atomicExch(&c.seen0[p0], a.epoch) == a.epoch) err |= KFMAP_ERR_INVALID;
        }
        if ((unsigned)r1 < (unsigned)L.kf_n[a.kf1]) {
            if (atomicExch(&c.seen1[r1], a.epoch) == a.epoch) err |= KFMAP_ERR_INVALID;
        } else {
            err |= KFMAP_ERR_INVALID;
        }
        if (id >= 0) {
            // the place of this pair's entry: the list before the call, then the call's appends in any order
            const int n0 = L.nobs[id];
            const int slot = n0 + atomicAdd(&c.pend[id], 1);
            if (slot >= c.obs_cap) err |= KFMAP_ERR_CAPACITY;
            c.pair_n0[i] = n0;
            c.pair_slot[i] = slot;
        }
        a.lm_out[i] = creating ? -2 : id;
    }
    raise(c, err);
    int total;
    (void)block_exclusive_scan<KFMAP_BLOCK>(creating, scan, &total);
    if (threadIdx.x == 0) c.tile[blockIdx.x] = total;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_obs_scan(KfMapCore c, KfMapLm L, KfMapObserve a, int nt) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    const int n_new = scan_tiles<KFMAP_BLOCK>(c.tile, nt, scan);
    if (threadIdx.x != 0) return;
    int err = c.hdr[KFMAP_H_ERR];
    if (n_new > L.cap - L.next) {
        err |= KFMAP_ERR_CAPACITY;
        c.hdr[KFMAP_H_ERR] = err;
    }
    c.hdr[KFMAP_H_FIRST_NEW] = L.next;
    c.hdr[KFMAP_H_COUNT0] = n_new;
    if (err || n_new == 0) return;
    c.hdr[a.kind ? KFMAP_H_NEXT_LS : KFMAP_H_NEXT_PT] = L.next + n_new;
    // every new landmark's full_graph[kf1][kf0]++ / [kf0][kf1]++ (:292-293) at once
    c.graph[(size_t)a.kf1 * c.kf_cap + a.kf0] += n_new;
    c.graph[(size_t)a.kf0 * c.kf_cap + a.kf1] += n_new;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_obs_apply(KfMapCore c, KfMapLm L, KfMapObserve a) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    const bool refused = c.hdr[KFMAP_H_ERR] != 0;
    const int id = i < a.n ? a.lm_out[i] : -1;
    const int creating = id == -2;
    int total;
    const int rank = block_exclusive_scan<KFMAP_BLOCK>(creating, scan, &total);
    if (id >= 0) c.pend[id] = 0;   // the workspace as it was, refused or not
    if (refused) return;
    int n0 = 0;
    if (i < a.n) {
        const int p0 = a.pairs[2 * (size_t)i], p1 = a.pairs[2 * (size_t)i + 1];
        const int r1 = a.kf0 >= 0 ? p1 : a.unm_rows[p1];
        if (creating) {
            const int nid = L.next + c.tile[blockIdx.x] + rank;
            L.idx[(size_t)a.kf0 * L.rows + p0] = nid;
            L.idx[(size_t)a.kf1 * L.rows + r1] = nid;
            L.alive[nid] = 1;
            L.local[nid] = 0;
            L.inlier[nid] = 1;
            L.nobs[nid] = 2;
            L.owner[nid] = a.kf0;
            L.obs[(size_t)nid * c.obs_cap] = a.kf0;
            L.obs[(size_t)nid * c.obs_cap + 1] = a.kf1;
            a.lm_out[i] = nid;
        } else if (id >= 0) {
            L.idx[(size_t)a.kf1 * L.rows + r1] = id;
            L.obs[(size_t)id * c.obs_cap + c.pair_slot[i]] = a.kf1;
            atomicAdd(&L.nobs[id], 1);
            n0 = c.pair_n0[i];
        }
    }
    // full_graph over the entries the list held before the call (:317-324): uniform trip count per wave
    int wave_n = n0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wave_n = max(wave_n, __shfl_xor(wave_n, o, 64));
    for (int e = 0; e < wave_n; ++e) {
        int o = a.kf1;
        if (e < n0) o = L.obs[(size_t)id * c.obs_cap + e];
        graph_add(c, a.kf1, o, e < n0 && o != a.kf1 && (unsigned)o < (unsigned)c.n_kf);
    }
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_flm_reset(KfMapLm pt, KfMapLm ls) {
    const int j = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (j < pt.next) pt.local[j] = 0;
    if (j < ls.next) ls.local[j] = 0;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_flm_mark(KfMapCore c, int min_cov, int min_kf) {
    const int newest = c.n_kf - 1;
    for (int i = threadIdx.x; i < c.n_kf; i += KFMAP_BLOCK) {
        bool local = i == newest;
        // KM1: an erased keyframe is passed over where the reference dereferences it
        if (i < newest && c.kf_alive[i])
            local = c.graph[(size_t)newest * c.kf_cap + i] >= min_cov || newest - i <= min_kf;
        c.kf_local[i] = local;
    }
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_flm_flags(KfMapCore c, KfMapLm pt, KfMapLm ls) {
    const int kf = blockIdx.y;
    if (!c.kf_local[kf]) return;
    const KfMapLm& L = blockIdx.z ? ls : pt;
    const int row = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (row >= L.kf_n[kf] || row >= L.rows) return;
    const int id = L.idx[(size_t)kf * L.rows + row];
    if ((unsigned)id < (unsigned)L.next && L.alive[id]) L.local[id] = 1;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_cmp_reduce(KfMapCore c, KfMapLm L, KfMapSelect a) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    const int j0 = blockIdx.x * KFMAP_TILE + threadIdx.x * PER_THREAD;
    int total;
    (void)block_exclusive_scan<KFMAP_BLOCK>(__popc(select_bits(c, L, a, j0)), scan, &total);
    if (threadIdx.x == 0) c.tile[blockIdx.x] = total;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_cmp_scan(KfMapCore c, int nt, int slot) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    const int total = scan_tiles<KFMAP_BLOCK>(c.tile, nt, scan);
    if (threadIdx.x == 0) c.hdr[slot] = total;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_cmp_scatter(KfMapCore c, KfMapLm L, KfMapSelect a) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    const int j0 = blockIdx.x * KFMAP_TILE + threadIdx.x * PER_THREAD;
    unsigned m = select_bits(c, L, a, j0);
    int total;
    int pos = c.tile[blockIdx.x] + block_exclusive_scan<KFMAP_BLOCK>(__popc(m), scan, &total);
    while (m) {
        const int b = __ffs((int)m) - 1;
        a.out[pos++] = j0 + b;
        m &= m - 1;
    }
}

// the lowest row of keyframe kf_obs[0] that carries a landmark to remove (:2565-2573 stops at the first)
__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_bad_rows(KfMapCore c, KfMapLm L, KfMapSelect a) {
    const int kf = blockIdx.y;
    if (c.n_kf - 1 - kf <= a.cull_age || !c.kf_alive[kf]) return;
    const int row = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (row >= L.kf_n[kf] || row >= L.rows) return;
    const int id = L.idx[(size_t)kf * L.rows + row];
    if ((unsigned)id >= (unsigned)L.next || !L.alive[id]) return;
    if (L.obs[(size_t)id * c.obs_cap] != kf || !lm_is_bad(c, L, a, id)) return;
    atomicMin(&c.first_row[id], row);
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_bad_finish(KfMapCore c, KfMapLm L, KfMapSelect a) {
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (i >= c.hdr[a.slot]) return;
    const int id = a.out[i];
    const int k0 = L.obs[(size_t)id * c.obs_cap];
    const int row = c.first_row[id];
    if (row != ROW_NONE) {
        L.idx[(size_t)k0 * L.rows + row] = -1;
        c.first_row[id] = ROW_NONE;
    }
    if (L.owner[id] == k0) L.owner[id] = -1;   // the erase from map_*_kf_idx.at(kf_obs) (:2576-2583)
    L.alive[id] = 0;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_inl_check(KfMapCore c, KfMapLm L, const int32_t* ids, int n) {
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    raise(c, i < n && (unsigned)ids[i] >= (unsigned)L.next ? KFMAP_ERR_INVALID : 0);
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_inl_apply(KfMapCore c, KfMapLm L, const int32_t* ids, int n, int value) {
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (i >= n || c.hdr[KFMAP_H_ERR] != 0) return;
    const int id = ids[i];
    if (L.alive[id]) L.inlier[id] = (uint8_t)value;
}

// the graph part of removeRedundantKFs (:2777-2781, k < full_graph.size() - 1 as written: KM10) and :2784
__global__ void __launch_bounds__(KFMAP_BLOCK) k_kfmap_erase_kf(KfMapCore c, int kf) {
    for (int k = threadIdx.x; k < c.n_kf - 1; k += KFMAP_BLOCK) {
        c.graph[(size_t)kf * c.kf_cap + k] = 0;
        c.graph[(size_t)k * c.kf_cap + kf] = 0;
    }
    if (threadIdx.x == 0) c.kf_alive[kf] = 0;
}

static unsigned blocks_of(int n) { return (unsigned)((n + KFMAP_BLOCK - 1) / KFMAP_BLOCK); }
static unsigned tiles_of(int n) { return (unsigned)((n + KFMAP_TILE - 1) / KFMAP_TILE); }

hipError_t enqueue_kfmap_add_keyframe(const KfMapCore& c, const KfMapLm& pt, const KfMapLm& ls, int n_pt, int n_ls, hipStream_t s) {
    const int n = std::max(std::max(pt.rows, ls.rows), c.n_kf + 1);
    hipLaunchKernelGGL(k_kfmap_add_kf, dim3(blocks_of(n)), dim3(KFMAP_BLOCK), 0, s, c, pt, ls, n_pt, n_ls);
    return hipGetLastError();
}

hipError_t enqueue_kfmap_observe(const KfMapCore& c, const KfMapLm& L, const KfMapObserve& a, hipStream_t s) {
    // (n = 0 still runs the scan: the call's first_new and count come from it)
    const unsigned nb = blocks_of(a.n);
    if (nb) hipLaunchKernelGGL(k_kfmap_obs_check, dim3(nb), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    hipLaunchKernelGGL(k_kfmap_obs_scan, dim3(1), dim3(KFMAP_BLOCK), 0, s, c, L, a, (int)nb);
    if (nb) hipLaunchKernelGGL(k_kfmap_obs_apply, dim3(nb), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    return hipGetLastError();
}

hipError_t enqueue_kfmap_form_local_map(const KfMapCore& c, const KfMapLm& pt, const KfMapLm& ls, int min_lm_cov_graph,
                                        int min_kf_local_map, hipStream_t s) {
    const int n_lm = std::max(pt.next, ls.next);
    if (n_lm > 0) hipLaunchKernelGGL(k_kfmap_flm_reset, dim3(blocks_of(n_lm)), dim3(KFMAP_BLOCK), 0, s, pt, ls);
    hipLaunchKernelGGL(k_kfmap_flm_mark, dim3(1), dim3(KFMAP_BLOCK), 0, s, c, min_lm_cov_graph, min_kf_local_map);
    hipLaunchKernelGGL(k_kfmap_flm_flags, dim3(blocks_of(std::max(pt.rows, ls.rows)), (unsigned)c.n_kf, 2), dim3(KFMAP_BLOCK), 0, s,
                       c, pt, ls);
    return hipGetLastError();
}

hipError_t enqueue_kfmap_select(const KfMapCore& c, const KfMapLm& L, const KfMapSelect& a, hipStream_t s) {
    const unsigned nt = tiles_of(a.n);
    if (nt) hipLaunchKernelGGL(k_kfmap_cmp_reduce, dim3(nt), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    hipLaunchKernelGGL(k_kfmap_cmp_scan, dim3(1), dim3(KFMAP_BLOCK), 0, s, c, (int)nt, a.slot);
    if (nt) hipLaunchKernelGGL(k_kfmap_cmp_scatter, dim3(nt), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    return hipGetLastError();
}

hipError_t enqueue_kfmap_remove_bad(const KfMapCore& c, const KfMapLm& L, const KfMapSelect& a, hipStream_t s) {
    hipError_t e = enqueue_kfmap_select(c, L, a, s);
    if (e != hipSuccess || a.n == 0) return e;
    hipLaunchKernelGGL(k_kfmap_bad_rows, dim3(blocks_of(L.rows), (unsigned)c.n_kf), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    hipLaunchKernelGGL(k_kfmap_bad_finish, dim3(blocks_of(a.n)), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    return hipGetLastError();
}

hipError_t enqueue_kfmap_set_inlier(const KfMapCore& c, const KfMapLm& L, const int32_t* ids, int n, int value, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_kfmap_inl_check, dim3(blocks_of(n)), dim3(KFMAP_BLOCK), 0, s, c, L, ids, n);
    hipLaunchKernelGGL(k_kfmap_inl_apply, dim3(blocks_of(n)), dim3(KFMAP_BLOCK), 0, s, c, L, ids, n, value);
    return hipGetLastError();
}

hipError_t enqueue_kfmap_erase_keyframe(const KfMapCore& c, int kf, hipStream_t s) {
    hipLaunchKernelGGL(k_kfmap_erase_kf, dim3(1), dim3(KFMAP_BLOCK), 0, s, c, kf);
    return hipGetLastError();
}

}  // namespace gfpl
