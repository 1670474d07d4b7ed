// gfpl_host.hpp — what the host files of the solver objects (gfpl_lba.cpp, gfpl_gba.cpp, gfpl_pgo.cpp,
// gfpl_lm.cpp, gfpl_bow.cpp) share: the HIP error check, the context's stream, the staging helpers,
// and for the two bundle adjustments the checks and the kernel record of a gfpl_lba_problem and the
// read-back of an evaluated system.  (gfpl_abi.hip and gfpl_detect.cpp keep their own checks: their
// messages differ.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gfpl.h"
#include "gfpl_kernels.hpp"

#define GFPL_HIPCHK(x)                                                                  \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            std::fprintf(stderr, "gfpl: %s failed: %s\n", #x, hipGetErrorString(e_));   \
            return GFPL_E_HIP;                                                          \
        }                                                                               \
    } while (0)

namespace gfpl {

inline hipStream_t stream_of(const gfpl_ctx* c) { return (hipStream_t)gfpl_ctx_stream(c); }

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// a planner's list into its place in the pinned staging
template <typename T>
void put(T* dst, const std::vector<T>& src) {
    if (!src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(T));
}

// cnt doubles from the device, when the caller asked for them
inline hipError_t get_doubles(double* dst, const double* src, size_t cnt) {
    if (!dst || cnt == 0) return hipSuccess;
    return hipMemcpy(dst, src, cnt * sizeof(double), hipMemcpyDeviceToHost);
}

// the camera of the bundle adjustments' kernels: fx, fy, cx, cy, b; everything else zero
inline DevCam dev_cam(const gfpl_camera* cam) {
    DevCam d;
    std::memset(&d, 0, sizeof d);
    d.fx = cam->fx; d.fy = cam->fy; d.cx = cam->cx; d.cy = cam->cy; d.b = cam->b;
    return d;
}

// the arrays a problem with these counts must bring (its index lists are the checkers' and planners')
inline bool ba_problem_pointers_ok(const gfpl_lba_problem& p) {
    if (!p.x_kf || !p.T_kf || (p.n.n_fix > 0 && !p.T_fix)) return false;
    if (p.n.n_pt > 0 && (!p.pt || !p.pt_obs || !p.pt_sigma)) return false;
    if (p.n.n_ls > 0 && (!p.ls || !p.ls_obs || !p.ls_sigma)) return false;
    return true;
}

// the caller's arrays into a kernel record (LbaProb / GbaProb name them alike)
template <class Prob>
void ba_fill_prob(Prob& q, const gfpl_lba_problem& p) {
    q.x_kf = p.x_kf; q.T_kf = p.T_kf; q.T_fix = p.T_fix; q.pt = p.pt; q.ls = p.ls;
    q.pt_obs = p.pt_obs; q.pt_sigma = p.pt_sigma; q.ls_obs = p.ls_obs; q.ls_sigma = p.ls_sigma;
    q.x_out = p.x_out;
}

// the part of the *_debug_system hooks that both workspaces (LbaPtrs / GbaPtrs) lay out alike: the pose
// blocks, the gradient (poses, then landmarks), the landmark blocks, and err from the problem's record,
// which the loop leaves untouched after its last evaluation
template <class Ptrs>
int ba_read_system(const Ptrs& m, const gfpl_lba_counts& n, const gfpl_lba_result* d_rec, double* U, double* g, double* V_pt,
                   double* V_ls, double* err) {
    const size_t nkf = (size_t)n.n_kf, npt = (size_t)n.n_pt, nls = (size_t)n.n_ls;
    GFPL_HIPCHK(get_doubles(U, m.U, nkf * 36));
    GFPL_HIPCHK(get_doubles(g, m.gk, nkf * 6));
    if (g) GFPL_HIPCHK(get_doubles(g + nkf * 6, m.glm, 3 * npt + 6 * nls));
    GFPL_HIPCHK(get_doubles(V_pt, m.V, 9 * npt));
    GFPL_HIPCHK(get_doubles(V_ls, m.V + 9 * npt, 36 * nls));
    if (err) {
        gfpl_lba_result r;
        GFPL_HIPCHK(hipMemcpy(&r, d_rec, sizeof r, hipMemcpyDeviceToHost));
        *err = r.err;
    }
    return GFPL_OK;
}

// what gfpl_mapgeo.cpp reads of the objects it works beside.
// gfpl_kfmap.cpp: a map's index half as the last call left it (device arrays, host counts)
struct KfMapDevice {
    gfpl_ctx* ctx;
    gfpl_kfmap_caps caps;
    KfMapCore core;
    KfMapLm lm[2];
    bool failed;
};
KfMapDevice kfmap_device(const gfpl_kfmap* m);
// gfpl_lba.cpp: gfpl_lba_solve after its staging, for one problem whose index arrays the caller writes
// on the device.  lba_stage_device checks p's counts against the object (GFPL_E_CAPACITY), makes record
// 0 from p and returns it: the caller enqueues the kernel that fills q->lm_start / obs_lm / obs_kf, then
// lba_enqueue uploads the records, launches the solve and copies n results to the host.  Nothing here
// synchronises.
gfpl_ctx* lba_ctx(const gfpl_lba* l);
int lba_stage_device(gfpl_lba* l, const gfpl_lba_problem& p, LbaProb* q);
hipError_t lba_enqueue(gfpl_lba* l, int n, int lds_kfs, const gfpl_lba_params* prm, gfpl_lba_result* results, hipStream_t s);

}  // namespace gfpl
