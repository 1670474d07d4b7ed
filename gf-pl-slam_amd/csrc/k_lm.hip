// k_lm.hip — the landmark descriptor store (include/gfpl.h).
//
//  k_lm_apply<G> : MapPoint / MapLine::desc_list under a call's ops and updateAverageDescDir's
//                  descriptor half (src/mapFeatures.cpp:50-84, 120-154) over the final list.  G
//                  lanes work on one landmark, lane r holding observation r in 8 VGPRs, so a wave
//                  carries 64 / G landmarks.  The planner (gfpl_lm_plan.cpp) put every touched
//                  landmark into the launch whose G covers the longest list it reaches.
//  k_lm_gather   : the median rows of an id list, compacted, 16 bytes per lane.
//  k_lm_apply<G, LmRangeHdr>, k_lm_gather_dev : the same bodies for a call planned on the device
//                  (k_lm_plan.hip): the range and the refusal are read from the planner's header.
// The groups of a wave run different op counts and list lengths: every loop runs to the wave's
// largest bound (a scalar), so the cross-lane reads stay under uniform control flow, and a group
// that is done is predicated off.  Rows and distances live in registers with static indices only:
// no LDS, no scratch.
#include "gfpl_kernels.hpp"
#include "gfpl_wave.hpp"

namespace gfpl {

// the wave's largest v, as a scalar
GFPL_DEV int wave_max_scalar(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return __builtin_amdgcn_readfirstlane(v);
}

GFPL_DEV void lm_load_row(const uint8_t* p, uint32_t (&d)[8]) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
    d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}
GFPL_DEV void lm_store_row(uint8_t* p, const uint32_t (&d)[8]) {
    reinterpret_cast<uint4*>(p)[0] = make_uint4(d[0], d[1], d[2], d[3]);
    reinterpret_cast<uint4*>(p)[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// where a launch's range of work items comes from: the arguments (apply and fuse, planned on the host), or
// the header a device-planned call's scan left, whose error word also calls the launch off.  That grid is
// sized on the host from the call's pairs: a workgroup past the bucket's end leaves at once.
struct LmRangeArgs {
    int work0, n_work;
    GFPL_DEV bool get(int, int* w0, int* n) const {
        *w0 = work0;
        *n = n_work;
        return true;
    }
};
struct LmRangeHdr {
    const int32_t* hdr;
    int bucket;
    GFPL_DEV bool get(int per_block, int* w0, int* n) const {
        *w0 = hdr[LM_H_BUCKET + bucket];
        *n = hdr[LM_H_BUCKET + bucket + 1] - *w0;
        return hdr[LM_H_ERR] == 0 && (size_t)blockIdx.x * per_block < (size_t)*n;
    }
};

template <int G, typename Range>
__global__ void __launch_bounds__(LM_BLOCK) k_lm_apply(LmStoreDev st, const LmWork* work, const LmOpDev* ops, Range range) {
    int work0, n_work;
    if (!range.get(LM_BLOCK / G, &work0, &n_work)) return;
    const int r = threadIdx.x & (G - 1);
    const size_t wi = ((size_t)blockIdx.x * LM_BLOCK + threadIdx.x) / G;
    const bool live = wi < (size_t)n_work;
    LmWork w{0, 0, 0, 0};
    if (live) w = work[(size_t)work0 + wi];
    // r < count <= obs_cap wherever `mine` is dereferenced
    uint8_t* mine = st.rows + ((size_t)w.lm * st.obs_cap + r) * 32;
    int count = w.count0;
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < count) lm_load_row(mine, d);

    // the ops, in the landmark's order.  `lo` is the first list position whose row changed.
    int lo = 0x7fffffff;
    const int wave_ops = wave_max_scalar(w.n_ops);
    for (int i = 0; i < wave_ops; ++i) {
        int kind = -1, pos = 0;
        const uint8_t* row = nullptr;
        if (i < w.n_ops) {
            const LmOpDev o = ops[(size_t)w.op0 + i];
            kind = o.kind; pos = o.pos; row = o.row;
        }
        if (kind == GFPL_LM_ADD) {
            if (r == count) lm_load_row(row, d);
            lo = min(lo, count);
            ++count;
        }
        if (__any(kind == GFPL_LM_ERASE_OBS)) {
            // LM5: the observations above the position move down by one, order kept
            uint32_t up[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) up[k] = __shfl_down(d[k], 1, G);
            if (kind == GFPL_LM_ERASE_OBS) {
                if (r >= pos) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) d[k] = up[k];
                }
                lo = min(lo, pos);
                --count;
            }
        }
        if (kind == GFPL_LM_FREE) count = 0;
    }
    const int n = count;
    if (r >= lo && r < n) lm_store_row(mine, d);

    // LM1: row r of the distance matrix, the landmark's own 0 included (LM2); observation j is
    // broadcast within the group.  Entries at and past n hold a value no threshold reaches.
    const int wave_n = wave_max_scalar(n);
    int dist[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        dist[j] = 1 << 20;
        if (j < wave_n) {
            int s = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t o = G == 64 ? (uint32_t)readlane_i32((int)d[k], j) : (uint32_t)__shfl((int)d[k], j, G);
                s += __popc(d[k] ^ o);
            }
            if (j < n) dist[j] = s;
        }
    }
    // LM2: the element 1 + (n - 1) / 2 of the sorted row is the smallest v with #{j : d <= v} >= that + 1;
    // d <= 256, so nine halvings of [0, 256] find it
    const int need = 2 + (n - 1) / 2;
    int vlo = 0, vhi = 256;
#pragma unroll 1
    for (int it = 0; it < 9; ++it) {
        const int mid = (vlo + vhi) >> 1;
        int c = 0;
#pragma unroll
        for (int j = 0; j < G; ++j) c += dist[j] <= mid;
        if (c >= need) vhi = mid;
        else vlo = mid + 1;
    }
    // LM3: the least median, the smaller index among equals.  LM4: with n = 1 only lane 0 has a key,
    // whatever its median field holds, so the index is 0 and no distance is read.
    int key = r < n ? vlo * 64 + r : 0x7fffffff;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o, G));
    const int med = key & 63;
    if (live) {
        uint8_t* mrow = st.med + (size_t)w.lm * 32;
        if (n > 0 && r == med) lm_store_row(mrow, d);
        if (r == 0) {
            st.count[w.lm] = n;
            st.med_idx[w.lm] = n > 0 ? med : -1;
            if (n == 0) {
                const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                lm_store_row(mrow, z);
            }
        }
    }
}

GFPL_DEV void lm_gather_rows(const LmStoreDev& st, const int32_t* ids, int n, uint4* out, int32_t* med_idx_out) {
    const size_t t = (size_t)blockIdx.x * LM_BLOCK + threadIdx.x;
    const size_t i = t >> 1;
    if (i >= (size_t)n) return;
    const int id = ids[i];
    out[t] = reinterpret_cast<const uint4*>(st.med)[(size_t)id * 2 + (t & 1)];
    if (med_idx_out && !(t & 1)) med_idx_out[i] = st.med_idx[id];
}

__global__ void __launch_bounds__(LM_BLOCK) k_lm_gather(LmStoreDev st, const int32_t* ids, int n, uint4* out,
                                                        int32_t* med_idx_out) {
    lm_gather_rows(st, ids, n, out, med_idx_out);
}

// the ids were checked on the device (k_lm_ids_check): nothing is written when one was refused
__global__ void __launch_bounds__(LM_BLOCK) k_lm_gather_dev(LmStoreDev st, const int32_t* hdr, const int32_t* ids, int n, uint4* out,
                                                            int32_t* med_idx_out) {
    if (hdr[LM_H_ERR] != 0) return;
    lm_gather_rows(st, ids, n, out, med_idx_out);
}

template <int G>
static hipError_t launch_lm_apply_g(const LmStoreDev& st, const LmWork* work, const LmOpDev* ops, int work0, int n_work,
                                    hipStream_t s) {
    const int per_block = LM_BLOCK / G;
    const unsigned blocks = (unsigned)(((size_t)n_work + per_block - 1) / per_block);
    hipLaunchKernelGGL((k_lm_apply<G, LmRangeArgs>), dim3(blocks), dim3(LM_BLOCK), 0, s, st, work, ops, LmRangeArgs{work0, n_work});
    return hipGetLastError();
}

hipError_t launch_lm_apply(const LmStoreDev& st, const LmWork* work, const LmOpDev* ops, int work0, int n_work,
                           int bucket, hipStream_t s) {
    if (n_work <= 0) return hipSuccess;
    switch (bucket) {
    case 0: return launch_lm_apply_g<2>(st, work, ops, work0, n_work, s);
    case 1: return launch_lm_apply_g<4>(st, work, ops, work0, n_work, s);
    case 2: return launch_lm_apply_g<8>(st, work, ops, work0, n_work, s);
    case 3: return launch_lm_apply_g<16>(st, work, ops, work0, n_work, s);
    case 4: return launch_lm_apply_g<32>(st, work, ops, work0, n_work, s);
    case 5: return launch_lm_apply_g<64>(st, work, ops, work0, n_work, s);
    }
    return hipErrorInvalidValue;
}

template <int G>
static hipError_t launch_lm_apply_dev_g(const LmStoreDev& st, const LmWork* work, const LmOpDev* ops, const int32_t* hdr, int n_max,
                                        int bucket, hipStream_t s) {
    const int per_block = LM_BLOCK / G;
    const unsigned blocks = (unsigned)(((size_t)n_max + per_block - 1) / per_block);
    hipLaunchKernelGGL((k_lm_apply<G, LmRangeHdr>), dim3(blocks), dim3(LM_BLOCK), 0, s, st, work, ops, LmRangeHdr{hdr, bucket});
    return hipGetLastError();
}

hipError_t launch_lm_apply_dev(const LmStoreDev& st, const LmWork* work, const LmOpDev* ops, const int32_t* hdr, int n_max,
                               int bucket, hipStream_t s) {
    if (n_max <= 0) return hipSuccess;
    switch (bucket) {
    case 0: return launch_lm_apply_dev_g<2>(st, work, ops, hdr, n_max, bucket, s);
    case 1: return launch_lm_apply_dev_g<4>(st, work, ops, hdr, n_max, bucket, s);
    case 2: return launch_lm_apply_dev_g<8>(st, work, ops, hdr, n_max, bucket, s);
    case 3: return launch_lm_apply_dev_g<16>(st, work, ops, hdr, n_max, bucket, s);
    case 4: return launch_lm_apply_dev_g<32>(st, work, ops, hdr, n_max, bucket, s);
    case 5: return launch_lm_apply_dev_g<64>(st, work, ops, hdr, n_max, bucket, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_lm_gather_dev(const LmStoreDev& st, const int32_t* hdr, const int32_t* ids, int n, uint8_t* desc_out,
                                int32_t* med_idx_out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((2 * (size_t)n + LM_BLOCK - 1) / LM_BLOCK);
    hipLaunchKernelGGL(k_lm_gather_dev, dim3(blocks), dim3(LM_BLOCK), 0, s, st, hdr, ids, n, reinterpret_cast<uint4*>(desc_out),
                       med_idx_out);
    return hipGetLastError();
}

hipError_t launch_lm_gather(const LmStoreDev& st, const int32_t* ids, int n, uint8_t* desc_out, int32_t* med_idx_out,
                            hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((2 * (size_t)n + LM_BLOCK - 1) / LM_BLOCK);
    hipLaunchKernelGGL(k_lm_gather, dim3(blocks), dim3(LM_BLOCK), 0, s, st, ids, n, reinterpret_cast<uint4*>(desc_out),
                       med_idx_out);
    return hipGetLastError();
}

}  // namespace gfpl
