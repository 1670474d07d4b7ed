// k_mapgeo.hip — the map's geometry half (include/gfpl.h): obs_list, sigma_list and
// point3D / line3D of MapPoint / MapLine, T_kf_w / x_kf_w of KeyFrame, beside gfpl_kfmap's indices.
//
//  k_mapgeo_obs_check  : one thread per pair of an observe call: every refusal, the landmark's list
//                        length before the call, the pairs each landmark receives counted (pend).
//  k_mapgeo_obs_apply  : the geometry of lookForCommonMatches' loop bodies (src/mapHandler.cpp:270-335,
//                        :407-480, :609-615, :745-764).  A pair's place is the list length before the
//                        call plus the earlier pairs of its landmark; only a landmark with more than
//                        one pair (pend > 1) looks at earlier pairs.
//  k_mapgeo_obs_reset  : pend back to zero, refused or not.
//  k_mapgeo_free_*     : n_obs = 0 of the landmarks removeBadMapLandmarks freed.
//  k_mapgeo_asm_*      : the gathering loops of localBundleAdjustment (:1113-1209) and
//                        globalBundleAdjustment (:1851-1939): the keyframe list (one workgroup), per
//                        landmark its kept observations with the fixed keyframes marked and the tile
//                        sums (reduce), the scans and the fixed keyframes' compaction (one workgroup),
//                        the selected landmarks' lists (scatter), then one thread per (selected
//                        landmark, list entry) copying the doubles.  No workgroup waits for another.
//  k_mapgeo_lba_index  : an assembled problem's index arrays in k_lba's unified numbering.
//  k_mapgeo_write_back : :1688-1712.
// Every double is copied; the one arithmetic is se3_apply (gfpl_device.hpp) per created landmark.
// A mutating kernel reads the call's error word first and leaves the state alone when it is set.
#include <algorithm>

#include "gfpl_kernels.hpp"
#include "gfpl_wave.hpp"

namespace gfpl {

namespace {

constexpr int PER_THREAD = KFMAP_TILE / KFMAP_BLOCK;

GFPL_DEV void raise(int32_t* hdr, int bits) {
    // one atomic per wave that has anything to report
    int all = bits;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) all |= __shfl_xor(all, o, 64);
    if (all && (threadIdx.x & 63) == 0) atomicOr(&hdr[MAPGEO_H_ERR], all);
}

GFPL_DEV void copy_doubles(double* dst, const double* src, int n) {
    for (int k = 0; k < n; ++k) dst[k] = src[k];
}

// the kf1 row of pair (p0, p1): p1 itself, or unm_rows[p1] in the local-map stage; -1 when p1 names none
GFPL_DEV int kf1_row(const MapGeoObserve& a, int p1) {
    if (a.kf0 >= 0) return p1;
    return (unsigned)p1 < (unsigned)a.n_unm ? a.unm_rows[p1] : -1;
}

GFPL_DEV bool asm_selected(const MapGeoAsm& a, int kind, int j) {
    return a.lm_alive[kind][j] && (a.which == GFPL_KFMAP_ALIVE || a.lm_local[kind][j]);
}

// an observation goes into the problem when its keyframe is alive (:1981; for the LBA ledger MG5)
GFPL_DEV bool asm_kf_kept(const MapGeoAsm& a, int kf) { return (unsigned)kf < (unsigned)a.n_kf && a.kf_alive[kf]; }

GFPL_DEV int tiles_of_dev(int n) { return (n + KFMAP_TILE - 1) / KFMAP_TILE; }

}  // namespace

__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_obs_check(MapGeoCore c, MapGeoLm L, MapGeoObserve a) {
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    int err = 0;
    if (i < a.n) {
        const int p0 = a.pairs[2 * (size_t)i], p1 = a.pairs[2 * (size_t)i + 1];
        if (a.kf0 >= 0 && (unsigned)p0 >= (unsigned)a.n0) err |= KFMAP_ERR_INVALID;
        if ((unsigned)kf1_row(a, p1) >= (unsigned)a.n1) err |= KFMAP_ERR_INVALID;
        const int id = a.lm_out[i];
        if (id < -1 || id >= L.cap) {
            err |= KFMAP_ERR_INVALID;
        } else if (id >= 0) {
            const int n0 = L.nobs[id];
            const int before = atomicAdd(&c.pend[id], 1);
            c.pair_n0[i] = n0;
            if (a.kf0 >= 0 && id >= a.first_new) {
                if (n0 != 0 || before != 0) err |= KFMAP_ERR_INVALID;   // a created id holds nothing and has one pair
            } else if (n0 <= 0) {
                err |= KFMAP_ERR_INVALID;
            } else if (n0 + before + 1 > c.obs_cap) {
                err |= KFMAP_ERR_CAPACITY;   // the pair that counted last sees the list's final length
            }
        }
    }
    raise(c.hdr, err);
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_obs_apply(MapGeoCore c, MapGeoLm L, MapGeoObserve a) {
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (i >= a.n || c.hdr[MAPGEO_H_ERR] != 0) return;
    const int id = a.lm_out[i];
    if (id < 0) return;   // :308
    const int p0 = a.pairs[2 * (size_t)i];
    const int r1 = kf1_row(a, a.pairs[2 * (size_t)i + 1]);
    double* obs = L.obs + (size_t)id * c.obs_cap * L.ow;
    double* sigma = L.sigma + (size_t)id * c.obs_cap;
    if (a.kf0 >= 0 && id >= a.first_new) {
        // :276-289, :413-431: the 3D geometry in the world frame by the store's pose of kf0, both observations
        const double* T = c.T_kf + (size_t)a.kf0 * 16;
        double* X = L.lm3d + (size_t)id * L.lw;
        se3_apply(T, a.P0 + 3 * (size_t)p0, X);
        if (L.lw == 6) se3_apply(T, a.Q0 + 3 * (size_t)p0, X + 3);
        copy_doubles(obs, a.o0 + (size_t)p0 * L.ow, L.ow);
        copy_doubles(obs + L.ow, a.o1 + (size_t)r1 * L.ow, L.ow);
        sigma[0] = 1.0;
        sigma[1] = 1.0;
        L.nobs[id] = 2;
        return;
    }
    // :312, :440, :613, :760: the place is the pair's rank among its landmark's pairs, in pair order
    const int total = c.pend[id];
    int rank = 0;
    if (total > 1)
        for (int j = 0; j < i; ++j) rank += a.lm_out[j] == id;
    const int place = c.pair_n0[i] + rank;
    copy_doubles(obs + (size_t)place * L.ow, a.o1 + (size_t)r1 * L.ow, L.ow);
    sigma[place] = 1.0;
    if (rank == total - 1) L.nobs[id] = c.pair_n0[i] + total;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_obs_reset(MapGeoCore c, MapGeoLm L, MapGeoObserve a) {
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int id = a.lm_out[i];
    if ((unsigned)id < (unsigned)L.cap) c.pend[id] = 0;
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_free_check(MapGeoCore c, MapGeoLm L, const int32_t* ids, int n) {
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    raise(c.hdr, i < n && (unsigned)ids[i] >= (unsigned)L.cap ? KFMAP_ERR_INVALID : 0);
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_free_apply(MapGeoCore c, MapGeoLm L, const int32_t* ids, int n) {
    const int i = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (i >= n || c.hdr[MAPGEO_H_ERR] != 0) return;
    L.nobs[ids[i]] = 0;
}

// the keyframe list (:1115-1127, :1853-1863): alive, not keyframe 0, and local unless every alive one is taken
__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_asm_kf(MapGeoCore c, MapGeoAsm a) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    int carry = 0;
    for (int k0 = 0; k0 < a.n_kf; k0 += KFMAP_BLOCK) {
        const int k = k0 + threadIdx.x;
        const int sel = k < a.n_kf && k != 0 && a.kf_alive[k] && (a.which == GFPL_KFMAP_ALIVE || a.kf_local[k]);
        int total;
        const int pos = carry + block_exclusive_scan<KFMAP_BLOCK>(sel, scan, &total);
        if (k < a.n_kf) {
            a.kf_mark[k] = 0;
            a.kf_slot[k] = sel ? pos : MAPGEO_SLOT_NONE;
        }
        if (sel) {
            a.kf_list[pos] = k;
            copy_doubles(a.a_x_kf + (size_t)pos * 6, c.x_kf + (size_t)k * 6, 6);
            copy_doubles(a.a_T_kf + (size_t)pos * 16, c.T_kf + (size_t)k * 16, 16);
        }
        carry += total;
    }
    if (threadIdx.x == 0) c.hdr[MAPGEO_H_NKF] = carry;
}

// per landmark the observations that go into the problem; grid (tiles, kind)
__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_asm_count(MapGeoCore c, MapGeoLm pt, MapGeoLm ls, MapGeoAsm a) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    const int kind = blockIdx.y;
    const int next = a.next[kind];
    if ((int)blockIdx.x >= tiles_of_dev(next)) return;
    const MapGeoLm& L = kind ? ls : pt;
    const int j0 = blockIdx.x * KFMAP_TILE + threadIdx.x * PER_THREAD;
    int n_lm = 0, n_obs = 0, err = 0;
    for (int b = 0; b < PER_THREAD && j0 + b < next; ++b) {
        const int j = j0 + b;
        int cnt = 0;
        if (asm_selected(a, kind, j)) {
            const int n = a.k_nobs[kind][j];
            if (n != L.nobs[j] || n < 0 || n > c.obs_cap) {
                err |= KFMAP_ERR_INVALID;   // the two objects' lists do not pair up
            } else {
                for (int e = 0; e < n; ++e) {
                    const int kf = a.k_obs[kind][(size_t)j * c.obs_cap + e];
                    if (!asm_kf_kept(a, kf)) continue;
                    ++cnt;
                    if (a.kf_slot[kf] == MAPGEO_SLOT_NONE) a.kf_mark[kf] = 1;   // every writer stores 1
                }
            }
        }
        a.lm_cnt[kind][j] = cnt;
        n_lm += cnt > 0;
        n_obs += cnt;
    }
    raise(c.hdr, err);
    int total_lm, total_obs;
    (void)block_exclusive_scan<KFMAP_BLOCK>(n_lm, scan, &total_lm);
    (void)block_exclusive_scan<KFMAP_BLOCK>(n_obs, scan, &total_obs);
    if (threadIdx.x == 0) {
        a.tile_lm[kind][blockIdx.x] = total_lm;
        a.tile_obs[kind][blockIdx.x] = total_obs;
    }
}

// the four scans, the fixed keyframes in ascending index (MG4) and the counts; one workgroup
__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_asm_scan(MapGeoCore c, MapGeoAsm a) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    int n_lm[2], n_obs[2];
    for (int kind = 0; kind < 2; ++kind) {
        const int nt = tiles_of_dev(a.next[kind]);
        n_lm[kind] = scan_tiles<KFMAP_BLOCK>(a.tile_lm[kind], nt, scan);
        n_obs[kind] = scan_tiles<KFMAP_BLOCK>(a.tile_obs[kind], nt, scan);
    }
    int carry = 0;
    for (int k0 = 0; k0 < a.n_kf; k0 += KFMAP_BLOCK) {
        const int k = k0 + threadIdx.x;
        const int fixed = k < a.n_kf && a.kf_mark[k] != 0;
        int total;
        const int pos = carry + block_exclusive_scan<KFMAP_BLOCK>(fixed, scan, &total);
        if (fixed) {
            a.kf_slot[k] = -1 - pos;
            a.fix_list[pos] = k;
            copy_doubles(a.a_T_fix + (size_t)pos * 16, c.T_kf + (size_t)k * 16, 16);
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        c.hdr[MAPGEO_H_NFIX] = carry;
        c.hdr[MAPGEO_H_NPT] = n_lm[0];
        c.hdr[MAPGEO_H_NLS] = n_lm[1];
        c.hdr[MAPGEO_H_NPTOBS] = n_obs[0];
        c.hdr[MAPGEO_H_NLSOBS] = n_obs[1];
    }
}

// the selected landmarks in map order with their first observation; grid (tiles, kind)
__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_asm_scatter(MapGeoAsm a) {
    __shared__ int scan[KFMAP_BLOCK / 64 + 1];
    const int kind = blockIdx.y;
    const int next = a.next[kind];
    if ((int)blockIdx.x >= tiles_of_dev(next)) return;
    const int j0 = blockIdx.x * KFMAP_TILE + threadIdx.x * PER_THREAD;
    int n_lm = 0, n_obs = 0;
    for (int b = 0; b < PER_THREAD && j0 + b < next; ++b) {
        const int cnt = a.lm_cnt[kind][j0 + b];
        n_lm += cnt > 0;
        n_obs += cnt;
    }
    int total;
    int li = a.tile_lm[kind][blockIdx.x] + block_exclusive_scan<KFMAP_BLOCK>(n_lm, scan, &total);
    int off = a.tile_obs[kind][blockIdx.x] + block_exclusive_scan<KFMAP_BLOCK>(n_obs, scan, &total);
    for (int b = 0; b < PER_THREAD && j0 + b < next; ++b) {
        const int cnt = a.lm_cnt[kind][j0 + b];
        if (cnt == 0) continue;
        a.lm_list[kind][li] = j0 + b;
        a.lm_off[kind][li] = off;
        ++li;
        off += cnt;
    }
}

// one thread per (selected landmark, list entry): the doubles and the two index lists; grid (blocks, kind)
__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_asm_gather(MapGeoCore c, MapGeoLm pt, MapGeoLm ls, MapGeoAsm a) {
    const int kind = blockIdx.y;
    const MapGeoLm& L = kind ? ls : pt;
    const long long t = (long long)blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    const int li = (int)(t / c.obs_cap), e = (int)(t % c.obs_cap);
    if (li >= a.tile_lm[kind][tiles_of_dev(a.next[kind])]) return;
    const int j = a.lm_list[kind][li];
    if (e == 0) copy_doubles(a.a_lm3d[kind] + (size_t)li * L.lw, L.lm3d + (size_t)j * L.lw, L.lw);
    const int32_t* kfs = a.k_obs[kind] + (size_t)j * c.obs_cap;
    if (e >= a.k_nobs[kind][j] || !asm_kf_kept(a, kfs[e])) return;
    int pos = 0;
    for (int q = 0; q < e; ++q) pos += asm_kf_kept(a, kfs[q]);
    const size_t o = (size_t)a.lm_off[kind][li] + pos;
    copy_doubles(a.a_obs[kind] + o * L.ow, L.obs + ((size_t)j * c.obs_cap + e) * L.ow, L.ow);
    a.a_sigma[kind][o] = L.sigma[(size_t)j * c.obs_cap + e];
    a.a_obs_lm[kind][o] = li;
    a.a_obs_kf[kind][o] = a.kf_slot[kfs[e]];
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_lba_index(MapGeoAsm a, gfpl_lba_counts n, int32_t* lm_start, int32_t* obs_lm,
                                                                  int32_t* obs_kf) {
    const int t = blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    const int n_lm = n.n_pt + n.n_ls, n_obs = n.n_pt_obs + n.n_ls_obs;
    if (t < n.n_pt) lm_start[t] = a.lm_off[0][t];
    else if (t < n_lm) lm_start[t] = n.n_pt_obs + a.lm_off[1][t - n.n_pt];
    else if (t == n_lm) lm_start[t] = n_obs;
    if (t < n.n_pt_obs) {
        obs_lm[t] = a.a_obs_lm[0][t];
        obs_kf[t] = a.a_obs_kf[0][t];
    } else if (t < n_obs) {
        obs_lm[t] = n.n_pt + a.a_obs_lm[1][t - n.n_pt_obs];
        obs_kf[t] = a.a_obs_kf[1][t - n.n_pt_obs];
    }
}

__global__ void __launch_bounds__(KFMAP_BLOCK) k_mapgeo_write_back(MapGeoCore c, MapGeoLm pt, MapGeoLm ls, MapGeoAsm a,
                                                                   gfpl_lba_counts n) {
    const long long t = (long long)blockIdx.x * KFMAP_BLOCK + threadIdx.x;
    if (t < n.n_kf * 16LL) c.T_kf[(size_t)a.kf_list[t / 16] * 16 + t % 16] = a.a_T_kf[t];   // x_kf_w is not refreshed (BA1)
    if (t < n.n_pt * 3LL) pt.lm3d[(size_t)a.lm_list[0][t / 3] * 3 + t % 3] = a.a_lm3d[0][t];
    if (t < n.n_ls * 6LL) ls.lm3d[(size_t)a.lm_list[1][t / 6] * 6 + t % 6] = a.a_lm3d[1][t];
}

static unsigned blocks_of(long long n) { return (unsigned)((n + KFMAP_BLOCK - 1) / KFMAP_BLOCK); }
static unsigned tiles_of(int n) { return (unsigned)((n + KFMAP_TILE - 1) / KFMAP_TILE); }

hipError_t enqueue_mapgeo_observe(const MapGeoCore& c, const MapGeoLm& L, const MapGeoObserve& a, hipStream_t s) {
    const unsigned nb = blocks_of(a.n);
    if (nb == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mapgeo_obs_check, dim3(nb), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    hipLaunchKernelGGL(k_mapgeo_obs_apply, dim3(nb), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    hipLaunchKernelGGL(k_mapgeo_obs_reset, dim3(nb), dim3(KFMAP_BLOCK), 0, s, c, L, a);
    return hipGetLastError();
}

hipError_t enqueue_mapgeo_free(const MapGeoCore& c, const MapGeoLm& L, const int32_t* ids, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_mapgeo_free_check, dim3(blocks_of(n)), dim3(KFMAP_BLOCK), 0, s, c, L, ids, n);
    hipLaunchKernelGGL(k_mapgeo_free_apply, dim3(blocks_of(n)), dim3(KFMAP_BLOCK), 0, s, c, L, ids, n);
    return hipGetLastError();
}

hipError_t enqueue_mapgeo_assemble(const MapGeoCore& c, const MapGeoLm& pt, const MapGeoLm& ls, const MapGeoAsm& a, hipStream_t s) {
    const unsigned nt = std::max(tiles_of(a.next[0]), tiles_of(a.next[1]));
    hipLaunchKernelGGL(k_mapgeo_asm_kf, dim3(1), dim3(KFMAP_BLOCK), 0, s, c, a);
    if (nt) hipLaunchKernelGGL(k_mapgeo_asm_count, dim3(nt, 2), dim3(KFMAP_BLOCK), 0, s, c, pt, ls, a);
    hipLaunchKernelGGL(k_mapgeo_asm_scan, dim3(1), dim3(KFMAP_BLOCK), 0, s, c, a);
    if (nt) {
        hipLaunchKernelGGL(k_mapgeo_asm_scatter, dim3(nt, 2), dim3(KFMAP_BLOCK), 0, s, a);
        const unsigned nb = blocks_of((long long)std::max(a.next[0], a.next[1]) * c.obs_cap);
        hipLaunchKernelGGL(k_mapgeo_asm_gather, dim3(nb, 2), dim3(KFMAP_BLOCK), 0, s, c, pt, ls, a);
    }
    return hipGetLastError();
}

hipError_t enqueue_mapgeo_lba_index(const MapGeoAsm& a, const gfpl_lba_counts& n, int32_t* lm_start, int32_t* obs_lm, int32_t* obs_kf,
                                    hipStream_t s) {
    const int items = std::max(n.n_pt + n.n_ls + 1, n.n_pt_obs + n.n_ls_obs);
    hipLaunchKernelGGL(k_mapgeo_lba_index, dim3(blocks_of(items)), dim3(KFMAP_BLOCK), 0, s, a, n, lm_start, obs_lm, obs_kf);
    return hipGetLastError();
}

hipError_t enqueue_mapgeo_write_back(const MapGeoCore& c, const MapGeoLm& pt, const MapGeoLm& ls, const MapGeoAsm& a,
                                     const gfpl_lba_counts& n, hipStream_t s) {
    const long long items = std::max(n.n_kf * 16LL, std::max(n.n_pt * 3LL, n.n_ls * 6LL));
    if (items <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_mapgeo_write_back, dim3(blocks_of(items)), dim3(KFMAP_BLOCK), 0, s, c, pt, ls, a, n);
    return hipGetLastError();
}

}  // namespace gfpl
