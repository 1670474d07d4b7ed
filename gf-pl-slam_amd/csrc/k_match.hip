// k_match.hip — the descriptor matchers over global descriptor sets and the match-list statistics
// StereoFrame exposes to its callers (MapHandler / KeyFrame):
//
//  k_knn2m / k_knn2 : cv::BFMatcher::knnMatch(k = 2) with NORM_HAMMING / NORM_HAMMING2 (ledger T1), one
//      set against another (gfpl_knn2_hamming, the keyframe matchers) or batched over the sequences
//      (the initial frame, src/stereoFrame.cpp:183-197).  k_knn2m runs the tiles of gfpl_knn.hpp on
//      the matrix cores; its packed key holds a 16-bit train index, so above 65536 train rows the
//      scalar k_knn2 (one thread per query) takes over.
//  k_radius_count / k_radius_rows : cv::BFMatcher::radiusMatch(NORM_HAMMING[2], maxDistance) as
//      StereoFrame::matchPointFeatures_radius / matchLineFeatures_radius call it
//      (src/stereoFrame.cpp:1243-1257): per query row, every train row with distance <= maxDistance
//      (ledger T1), sorted by distance — OpenCV's std::sort on DMatch::operator< leaves equal
//      distances in an unspecified order; here they stay in train order (pinned, ledger T2).
//      One wave per query; the rows are ragged: a count pass sizes them (host scan), the row pass
//      places each match by a counting sort over the <= 257 distances (LDS histogram, then the
//      distinct distances of each 64-row chunk resolved by ballots, in train order).
//  k_match_stats : pointDescriptorMAD / lineDescriptorMAD / *DescriptorBudgetThres
//      (src/stereoFrame.cpp:1259-1341): order statistics of a knn-2 list's distances by an MSB-first
//      radix select over order-preserving float keys (NaN above +inf: ledger U12), one workgroup.
// Keyframe-rate calls (latency, not throughput).
#include "gfpl_kernels.hpp"
#include "gfpl_knn.hpp"

namespace gfpl {

// ------------------------------------------------------------------ knn2 --
// One knn-2 launch.  cap == 0: one set of nq rows against one of nt, results to idx / dist [nq][2].
// cap > 0 (batched, blockIdx.y = sequence b): rows at q / t + b * cap * 32, counts
// min(nq_arr[b], cap) / min(nt_arr[b], cap), results (idx0, d0, d1) at packed + b * cap * 6.
struct Knn2Args {
    const uint8_t *q, *t;
    const int *nq_arr, *nt_arr;
    int nq, nt, cap;
    int32_t* idx;
    float* dist;
    int32_t* packed;
    __device__ int count_q(int b) const { return nq_arr ? min(nq_arr[b], cap) : nq; }
    __device__ int count_t(int b) const { return nt_arr ? min(nt_arr[b], cap) : nt; }
    // query i's neighbours (index -1 and distance INT_MAX where there is none)
    __device__ void write(int b, int i, int i0, int i1, int d0, int d1) const {
        if (idx) {
            idx[2 * i] = i0; idx[2 * i + 1] = i1;
            dist[2 * i] = (float)d0; dist[2 * i + 1] = (float)d1;
        }
        if (packed) {
            int32_t* o = packed + (size_t)b * cap * 6;
            o[3 * i] = i0; o[3 * i + 1] = d0; o[3 * i + 2] = d1;
        }
    }
};

// grid (query tiles of 128, sequences); each wave keeps one 32-query column tile in registers
// while the train rows stream through LDS in chunks of KNN_CHUNK (knn_stage_views) and
// through the tiles of gfpl_knn.hpp, the chunk's first row c0 added to the keys' train index.
// dynamic LDS: Knn2Lds (gfpl_layout.hpp), the table at LDS address 0: no static __shared__ here
template <int CELL>
__global__ void __launch_bounds__(256) k_knn2m(Knn2Args a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Knn2Lds L(smem, CELL);
    const int b = blockIdx.y;
    const int nq = a.count_q(b), nt = a.count_t(b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int qi = (blockIdx.x * 4 + wave) * 32 + c;
    if (blockIdx.x * 128 >= nq) return;   // uniform per workgroup
    const uint8_t* Tg = a.t + (size_t)b * a.cap * 32;
    knn_lut_fill<CELL>(L.lut);
    uint32_t qd[8];
    if (qi < nq) load_desc(a.q + ((size_t)b * a.cap + qi) * 32, qd);
    else {
#pragma unroll
        for (int i = 0; i < 8; ++i) qd[i] = 0;
    }
    mfma_v4i bq[knn_ksteps<CELL>()];
#pragma unroll
    for (int ks = 0; ks < knn_ksteps<CELL>(); ++ks) bq[ks] = knn_frag<CELL, true>(qd, ks, h);
    const uint32_t offk = knn_query_offk<CELL>(qd);
    knn_acc_t acc0 = knn_acc_init(0);
#pragma unroll
    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(acc0[r]));   // (held)
    const uint32_t* Th = L.tb + 4 * h * KNN_CHUNK;   // this lane half's view
    uint32_t k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu;
    for (int c0 = 0; c0 < nt; c0 += KNN_CHUNK) {
        const int nc = min(KNN_CHUNK, nt - c0);
        __syncthreads();
        knn_stage_views<CELL>(L.tb, KNN_CHUNK, Tg + (size_t)c0 * 32, nc);
        __syncthreads();
        const int nrt = (nc + 31) >> 5;
        for (int rt = 0; rt < nrt; ++rt) {
            const knn_acc_t acc = knn_tile<CELL>(Th, KNN_CHUNK, rt, c, nc, bq, acc0);
            const uint32_t tb = (uint32_t)(rt * 32 + 4 * h);
            const uint32_t tko = offk + (uint32_t)c0 + tb;
            const bool full = rt * 32 + 32 <= nc;   // (wave-uniform)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t ro = knn_acc_row(r);
                uint32_t key = (knn_acc_bits(acc[r]) << 16) + tko + ro;
                if (!full && (int)(tb + ro) >= nc) key = 0xFFFFFFFFu;
                knn_top2(k0, k1, key);
            }
        }
    }
    knn_merge_halves(k0, k1);
    if (h == 0 && qi < nq) {
        const bool v0 = k0 != 0xFFFFFFFFu, v1 = k1 != 0xFFFFFFFFu;
        a.write(b, qi, v0 ? (int)(k0 & 0xFFFFu) : -1, v1 ? (int)(k1 & 0xFFFFu) : -1, v0 ? (int)(k0 >> 16) : 2147483647,
                v1 ? (int)(k1 >> 16) : 2147483647);
    }
}

// one thread per query over the train rows in global memory, the insertion rule of cv::batchDistance
template <int CELL>
__global__ void __launch_bounds__(256) k_knn2(Knn2Args a) {
    const int b = blockIdx.y;
    const int nq = a.count_q(b), nt = a.count_t(b);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint8_t* Q = a.q + (size_t)b * a.cap * 32;
    const uint8_t* T = a.t + (size_t)b * a.cap * 32;
    uint32_t qd[8];
    load_desc(Q + (size_t)i * 32, qd);
    int dist0 = 2147483647, dist1 = 2147483647, idx0 = -1, idx1 = -1;
    for (int j = 0; j < nt; ++j) {
        uint32_t td[8];
        load_desc(T + (size_t)j * 32, td);
        const int d = hamming8<CELL>(qd, td);
        if (d < dist1) {
            if (dist0 > d) { dist1 = dist0; idx1 = idx0; dist0 = d; idx0 = j; }
            else { dist1 = d; idx1 = j; }
        }
    }
    a.write(b, i, idx0, idx1, dist0, dist1);
}

// nq_max / nt_max: the largest count of any sequence
template <int CELL>
static hipError_t launch_knn2_as(const Knn2Args& a, int nq_max, int nt_max, int B, hipStream_t s) {
    if (nt_max <= 65536)   // MFMA path: the packed key holds a 16-bit train index
        hipLaunchKernelGGL(k_knn2m<CELL>, dim3((nq_max + 127) / 128, B), dim3(256), Knn2Lds(nullptr, CELL).bytes, s, a);
    else
        hipLaunchKernelGGL(k_knn2<CELL>, dim3((nq_max + 255) / 256, B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_knn2(const uint8_t* q, int nq, const uint8_t* t, int nt, int cell, int32_t* idx, float* dist,
                       hipStream_t s) {
    const Knn2Args a{q, t, nullptr, nullptr, nq, nt, 0, idx, dist, nullptr};
    return cell == 2 ? launch_knn2_as<2>(a, nq, nt, 1, s) : launch_knn2_as<1>(a, nq, nt, 1, s);
}

hipError_t launch_knn2_batched(const uint8_t* q, const int* nq, const uint8_t* t, const int* nt, int cap, int B,
                               int cell, int32_t* packed, hipStream_t s) {
    const Knn2Args a{q, t, nq, nt, 0, 0, cap, nullptr, nullptr, packed};
    return cell == 2 ? launch_knn2_as<2>(a, cap, cap, B, s) : launch_knn2_as<1>(a, cap, cap, B, s);
}

hipError_t launch_knn2_counts(const uint8_t* q, const int* nq, const uint8_t* t, const int* nt, int cap, int cell,
                              int32_t* idx, float* dist, hipStream_t s) {
    const Knn2Args a{q, t, nq, nt, 0, 0, cap, idx, dist, nullptr};
    return cell == 2 ? launch_knn2_as<2>(a, cap, cap, 1, s) : launch_knn2_as<1>(a, cap, cap, 1, s);
}

// ---------------------------------------------------------------- radius --
template <int CELL>
__global__ void __launch_bounds__(256) k_radius_count(const uint8_t* q, int nq, const uint8_t* t, int nt,
                                                      float radius, int32_t* cnt) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;   // (wave-uniform)
    uint32_t a[8], b[8];
    load_desc(q + 32 * (size_t)qi, a);
    int c = 0;
    for (int j = lane; j < nt; j += 64) {
        load_desc(t + 32 * (size_t)j, b);
        c += ((float)hamming8<CELL>(a, b) <= radius) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) cnt[qi] = c;
}

template <int CELL>
__global__ void __launch_bounds__(256) k_radius_rows(const uint8_t* q, int nq, const uint8_t* t, int nt, float radius,
                                                     const int32_t* row_off, int32_t* out_idx, float* out_dist) {
    __shared__ int hist[4][257 + 3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qi = blockIdx.x * 4 + w;
    if (qi >= nq) return;   // (wave-uniform; the waves of a block share no LDS row)
    int* h = hist[w];
    for (int i = lane; i < 257; i += 64) h[i] = 0;
    __builtin_amdgcn_wave_barrier();
    uint32_t a[8], b[8];
    load_desc(q + 32 * (size_t)qi, a);
    for (int j = lane; j < nt; j += 64) {
        load_desc(t + 32 * (size_t)j, b);
        const int d = hamming8<CELL>(a, b);
        if ((float)d <= radius) atomicAdd(&h[d], 1);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // exclusive scan of the 257 bins: lane l owns bins [5l, 5l + 5) (lanes 0-51), a wave scan of the partials
    int own[5], tot = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int i = 5 * lane + k;
        own[k] = i < 257 ? h[i] : 0;
        tot += own[k];
    }
    int inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    int run = inc - tot;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int i = 5 * lane + k;
        if (i < 257) h[i] = run;
        run += own[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const int base = row_off[qi];
    // placement in train order: per 64-row chunk, one ballot per distinct distance present
    for (int j0 = 0; j0 < nt; j0 += 64) {   // (wave-uniform)
        const int j = j0 + lane;
        int d = -1;
        if (j < nt) {
            load_desc(t + 32 * (size_t)j, b);
            const int x = hamming8<CELL>(a, b);
            if ((float)x <= radius) d = x;
        }
        unsigned long long todo = __ballot(d >= 0);
        while (todo) {   // (wave-uniform)
            const int src = __ffsll((long long)todo) - 1;
            const int dv = __shfl(d, src);
            const unsigned long long grp = __ballot(d == dv);
            const int off = h[dv];
            if (d == dv) {
                const int pos = off + __popcll(grp & ((1ull << lane) - 1ull));
                out_idx[base + pos] = j;
                out_dist[base + pos] = (float)dv;
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == src) h[dv] = off + __popcll(grp);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
            todo &= ~grp;
        }
    }
}

hipError_t launch_radius_count(const uint8_t* q, int nq, const uint8_t* t, int nt, int cell, float radius,
                               int32_t* cnt, hipStream_t s) {
    const dim3 g((nq + 3) / 4);
    if (cell == 2)
        hipLaunchKernelGGL(k_radius_count<2>, g, dim3(256), 0, s, q, nq, t, nt, radius, cnt);
    else
        hipLaunchKernelGGL(k_radius_count<1>, g, dim3(256), 0, s, q, nq, t, nt, radius, cnt);
    return hipGetLastError();
}

hipError_t launch_radius_rows(const uint8_t* q, int nq, const uint8_t* t, int nt, int cell, float radius,
                              const int32_t* row_off, int32_t* idx, float* dist, hipStream_t s) {
    const dim3 g((nq + 3) / 4);
    if (cell == 2)
        hipLaunchKernelGGL(k_radius_rows<2>, g, dim3(256), 0, s, q, nq, t, nt, radius, row_off, idx, dist);
    else
        hipLaunchKernelGGL(k_radius_rows<1>, g, dim3(256), 0, s, q, nq, t, nt, radius, row_off, idx, dist);
    return hipGetLastError();
}

// ----------------------------------------------------------------- stats --
// order-preserving key of a float (NaN above +inf, ledger U12), and back
__device__ __forceinline__ uint32_t fkey(float f) {
    if (f != f) return 0xFFFFFFFFu;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fval(uint32_t k) {
    if (k == 0xFFFFFFFFu) return __builtin_nanf("");
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// the value of the kind-th statistic's element i (see k_match_stats)
__device__ __forceinline__ float stat_elem(int which, const float* d0, const float* d1, int i, double med) {
    if (which == 0) return d0[i];                                                   // NN distance
    if (which == 1) return fabsf((float)((double)d0[i] - 0.0));                     // |d0 - nn_dist_median| (U1)
    if (which == 2) return fabsf((float)((double)(d1[i] - d0[i]) - 0.0));           // line: |d1 - d0 - 0| (U1)
    if (which == 3) return d0[i] / d1[i];                                           // point: d0 / d1
    return fabsf((float)((double)(d0[i] / d1[i]) - med));                           // point: |d0/d1 - median|
}

// k-th smallest (0-based) of n values of statistic `which`: 4 passes of 8 bits, MSB first
__device__ float select_kth(int which, const float* d0, const float* d1, int n, int k, double med, int* hist,
                            uint32_t* sh) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            const uint32_t key = fkey(stat_elem(which, d0, d1, i, med));
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int acc = 0, bin = 0;
            for (; bin < 256; ++bin) {
                if (acc + hist[bin] > k) break;
                acc += hist[bin];
            }
            sh[0] = (uint32_t)bin;
            sh[1] = (uint32_t)acc;
        }
        __syncthreads();
        prefix |= sh[0] << shift;
        mask |= 255u << shift;
        k -= (int)sh[1];
        __syncthreads();
    }
    return fval(prefix);
}

// out[0] nn_mad, out[1] nn12_mad, out[2] the budget threshold (kind 0 point, 1 line); n >= 1
__global__ void __launch_bounds__(256) k_match_stats(int kind, const float* d0, const float* d1, int n, int max_num,
                                                     double* out) {
    __shared__ int hist[256];
    __shared__ uint32_t sh[2];
    const int mid = n / 2;
    // nn_mad: sort by NN distance, the element at n / 2 of |d0 - 0| (the median first taken is overwritten)
    const float nn = select_kth(1, d0, d1, n, mid, 0.0, hist, sh);
    double nn12;
    if (kind == 1) {
        // lineDescriptorMAD: |d1 - d0 - nn_dist_median| (U1), element n / 2 ascending
        nn12 = 1.4826 * (double)select_kth(2, d0, d1, n, mid, 0.0, hist, sh);
    } else {
        // pointDescriptorMAD: the ratio at n / 2 of the DESCENDING ratio order (compare_descriptor_by_NN12_ratio)
        const double med = (double)select_kth(3, d0, d1, n, n - 1 - mid, 0.0, hist, sh);
        nn12 = 1.4826 * (double)select_kth(4, d0, d1, n, mid, med, hist, sh);
    }
    // *DescriptorBudgetThres: the element at min(max_num, n) - 1 of the NN distances, ascending
    const int bi = (max_num < n ? max_num : n) - 1;
    const float thr = select_kth(0, d0, d1, n, bi < 0 ? 0 : bi, 0.0, hist, sh);
    if (threadIdx.x == 0) {
        out[0] = 1.4826 * (double)nn;
        out[1] = nn12;
        out[2] = (double)thr;
    }
}

hipError_t launch_match_stats(int kind, const float* d0, const float* d1, int n, int max_num, double* out,
                              hipStream_t s) {
    hipLaunchKernelGGL(k_match_stats, dim3(1), dim3(256), 0, s, kind, d0, d1, n, max_num, out);
    return hipGetLastError();
}

}  // namespace gfpl
