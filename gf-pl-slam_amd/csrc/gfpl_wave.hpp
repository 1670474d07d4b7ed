// gfpl_wave.hpp — small wave-level helpers several kernel files share (one wave = 64 lanes).
#pragma once
#include <math.h>

#include "gfpl_device.hpp"

namespace gfpl {

// LDS written by some lanes of a wave and read by others: the wave's DS operations complete
// in order; the clobber keeps the compiler from moving accesses across.  Sufficient within one
// wave; waves of a workgroup need a barrier.
GFPL_DEV void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// lane l's value (l wave-uniform)
GFPL_DEV int readlane_i32(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
GFPL_DEV float readlane_f32(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
GFPL_DEV double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
GFPL_DEV uint64_t readlane_u64(uint64_t v, int l) {
    return (uint64_t)__double_as_longlong(readlane_f64(__longlong_as_double((long long)v), l));
}

// the wave's sum, in every lane
GFPL_DEV int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Group-of-8 exchange on the DPP crossbar (no LDS): xor 1, xor 2 (quad_perm) and the half-row
// mirror (lane i <-> 7 - i) pair every lane of a group in 3 steps.  dpp_*: update_dpp with old = 0;
// dpp_mov_*: mov_dpp.
#define DPP_XOR1 0xB1
#define DPP_XOR2 0x4E
#define DPP_HALF_MIRROR 0x141
#define DPP_ROW_MIRROR 0x140   // lane i <-> 15 - i of a 16-lane row: the fourth step, for groups of 16
template <int CTRL>
GFPL_DEV int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
GFPL_DEV double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
GFPL_DEV double dpp_mov_f64(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// BORDER_REFLECT_101 index (one reflection: -n < i < 2n - 1)
GFPL_DEV int refl1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// O4: cv::fastAtan2 (degrees)
GFPL_DEV float fast_atan2(float y, float x) {
    const float p1 = 0.9997878412794807f * (float)(180 / M_PI), p3 = -0.3258083974640975f * (float)(180 / M_PI),
                p5 = 0.1555786518463281f * (float)(180 / M_PI), p7 = -0.04432655554792128f * (float)(180 / M_PI);
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, ax + (float)2.2204460492503131e-16);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = __fdiv_rn(ax, ay + (float)2.2204460492503131e-16);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

}  // namespace gfpl
