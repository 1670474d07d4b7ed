// k_rectify.hip — stereo rectification on the device (include/gfpl.h, gfpl_rectifier_* /
// gfpl_rectify*): PinholeStereoCamera::rectifyImage / rectifyImagesLR
// (src/pinholeStereoCamera.cpp:96-119), i.e. cv::remap(src, dst, map1, map2, INTER_LINEAR)
// with the CV_16SC2 + CV_16UC1 maps the constructor built (gfpl_rectify.cpp), for a batch of
// 8-bit images.  Ledger R6, integer arithmetic only.
//
// The maps are shared by the whole batch.  At upload each pixel's (map1, map2) pair becomes
// one 8-byte entry: source x, y (int16 each), the 5 + 5 fraction bits, and four bits saying
// which of the bilinear taps lie inside the image (15 = all four: the common case).  The
// kernel is linear over the output bytes of an image: a lane owns the four pixels of one
// aligned output dword, loads their four entries once, turns them into offsets and weights
// in registers, and then loops over its slice of the batch, so map traffic amortises to
// (8 B / slice length) per pixel and the per-image work is 16 byte gathers, 16 multiply-adds
// and one dword store.  Lanes whose four pixels have all taps inside (a flag formed once)
// run a loop without any test; the others select each tap by its bit.
// grid.x: dwords of one image, grid.y: (side, batch slice).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "gfpl_kernels.hpp"

namespace gfpl {

struct RectArgs {
    const uint2* ent[2];     // [H*W] entries per side
    const uint8_t* src[2];   // [n][H*W]
    uint8_t* dst[2];
    int W, WH;               // row pitch, pixels per image
    int n, per, slices;      // images, images per slice, slices per side
    int dword;               // 1: W*H % 4 == 0, every image starts at the same byte of a dword
};

namespace {

#define RECT_BLOCK 256
#define RECT_PER 8   // images per batch slice (the maps are read once per slice)

__global__ void __launch_bounds__(RECT_BLOCK) k_rectify(RectArgs a) {
    const int side = (int)blockIdx.y / a.slices;
    const int slice = (int)blockIdx.y - side * a.slices;
    const uint2* __restrict__ ent = side ? a.ent[1] : a.ent[0];
    const uint8_t* __restrict__ src = side ? a.src[1] : a.src[0];
    uint8_t* __restrict__ dst = side ? a.dst[1] : a.dst[0];
    const int W = a.W, WH = a.WH;
    // the lane's four pixels are those of one aligned dword of the output (when every image
    // of the batch has the same alignment): q0 may be -3..-1 in the first lane
    const int mis = a.dword ? (int)((uintptr_t)dst & 3) : 0;
    const int q0 = 4 * (int)(blockIdx.x * RECT_BLOCK + threadIdx.x) - mis;
    if (q0 >= WH) return;
    int off[4];
    uint32_t w00[4], w01[4], w10[4], w11[4], msk[4];
    bool all_in = true, full = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = q0 + k;
        const bool on = q >= 0 && q < WH;
        const uint2 e = on ? ent[q] : make_uint2(0u, 0u);
        const int sx = (int)(int16_t)(e.x & 0xFFFFu), sy = (int)(int16_t)(e.x >> 16);
        const uint32_t fa = e.y & 31u, fb = (e.y >> 5) & 31u;
        off[k] = sy * W + sx;
        w00[k] = (32u - fa) * (32u - fb);
        w01[k] = fa * (32u - fb);
        w10[k] = (32u - fa) * fb;
        w11[k] = fa * fb;
        msk[k] = on ? (e.y >> 16) & 15u : 16u;   // bit 4: not a pixel of this image
        all_in = all_in && msk[k] == 15u;
        full = full && on;
    }
    const int i0 = slice * a.per;
    const int i1 = min(a.n, i0 + a.per);
    const bool store_dword = full && a.dword;
    if (all_in) {
        for (int i = i0; i < i1; ++i) {
            const uint8_t* S = src + (size_t)i * WH;
            uint32_t out = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* p = S + off[k];
                const uint32_t v = (w00[k] * p[0] + w01[k] * p[1] + w10[k] * p[W] + w11[k] * p[W + 1] + 512u) >> 10;
                out |= v << (8 * k);
            }
            uint8_t* D = dst + (size_t)i * WH + q0;
            if (store_dword) {
                *reinterpret_cast<uint32_t*>(D) = out;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) D[k] = (uint8_t)(out >> (8 * k));
            }
        }
    } else {
        for (int i = i0; i < i1; ++i) {
            const uint8_t* S = src + (size_t)i * WH;
            uint32_t out = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* p = S + off[k];
                const uint32_t m = msk[k];
                const uint32_t p00 = (m & 1u) ? p[0] : 0u, p01 = (m & 2u) ? p[1] : 0u;
                const uint32_t p10 = (m & 4u) ? p[W] : 0u, p11 = (m & 8u) ? p[W + 1] : 0u;
                const uint32_t v = (w00[k] * p00 + w01[k] * p01 + w10[k] * p10 + w11[k] * p11 + 512u) >> 10;
                out |= v << (8 * k);
            }
            uint8_t* D = dst + (size_t)i * WH + q0;
            if (store_dword) {
                *reinterpret_cast<uint32_t*>(D) = out;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (!(msk[k] & 16u)) D[k] = (uint8_t)(out >> (8 * k));
            }
        }
    }
}

}  // namespace
}  // namespace gfpl

// ======================================================================= ABI ==
using namespace gfpl;

struct gfpl_rectifier {
    int device = 0;
    hipStream_t stream = nullptr;
    gfpl_ctx* ctx = nullptr;   // counted in while this object lives
    int W = 0, H = 0;
    uint2* ent[2] = {};        // device [H*W] per side (one allocation)
    void* base = nullptr;
    uint8_t* stage = nullptr;  // gfpl_rectify_host: device copies of its images (src, then dst)
    size_t stage_bytes = 0;
};

namespace {

bool overlap(const uint8_t* a, const uint8_t* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

}  // namespace

int gfpl_rectifier_width(const gfpl_rectifier* r) { return r->W; }
int gfpl_rectifier_height(const gfpl_rectifier* r) { return r->H; }

// both sides when src_r / dst_r are given, else `side` alone; on stream s
int gfpl_rectifier_enqueue(gfpl_rectifier* r, void* stream, int side, const uint8_t* src_l, const uint8_t* src_r,
                           int n, uint8_t* dst_l, uint8_t* dst_r) {
    const bool stereo = src_r || dst_r;
    if (!r || !src_l || !dst_l || n < 1 || side < 0 || side > 1) return GFPL_E_INVALID;
    if (stereo && (!src_r || !dst_r)) return GFPL_E_INVALID;
    const size_t WH = (size_t)r->W * r->H, bytes = WH * (size_t)n;
    if (overlap(src_l, dst_l, bytes)) return GFPL_E_INVALID;
    if (stereo && (overlap(src_r, dst_r, bytes) || overlap(src_l, dst_r, bytes) || overlap(src_r, dst_l, bytes) ||
                   overlap(dst_l, dst_r, bytes)))
        return GFPL_E_INVALID;
    if (hipSetDevice(r->device) != hipSuccess) return GFPL_E_HIP;
    RectArgs a{};
    a.ent[0] = r->ent[stereo ? 0 : side];
    a.ent[1] = r->ent[1];
    a.src[0] = src_l;
    a.src[1] = src_r;
    a.dst[0] = dst_l;
    a.dst[1] = dst_r;
    a.W = r->W;
    a.WH = (int)WH;
    a.n = n;
    a.dword = WH % 4 == 0;
    const int sides = stereo ? 2 : 1;
    // lanes: one per output dword, plus one for a misaligned base
    const unsigned gx = (unsigned)(((WH + 3) / 4 + 1 + RECT_BLOCK - 1) / RECT_BLOCK);
    // short batches are cut into shorter slices while the grid is small; long ones into longer
    // slices so that grid.y stays within its limit
    int per = RECT_PER;
    while (per > 1 && (size_t)gx * ((n + per - 1) / per) * sides < 2048) per >>= 1;
    while ((size_t)((n + per - 1) / per) * sides > 65535) per <<= 1;
    a.per = per;
    a.slices = (n + per - 1) / per;
    hipLaunchKernelGGL(k_rectify, dim3(gx, (unsigned)(a.slices * sides)), dim3(RECT_BLOCK), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? GFPL_OK : GFPL_E_HIP;
}

extern "C" int gfpl_rectifier_create(gfpl_ctx* ctx, const gfpl_rectify_side* left, const gfpl_rectify_side* right,
                                     int width, int height, gfpl_rectifier** out) {
    if (!ctx || !left || !right || !out || width < 8 || height < 8 || width > 8192 || height > 8192)
        return GFPL_E_INVALID;
    const size_t WH = (size_t)width * height;
    std::vector<int16_t> m1(2 * WH);
    std::vector<uint16_t> m2(WH);
    std::vector<uint2> ent(2 * WH);
    for (int side = 0; side < 2; ++side) {
        const int e = gfpl_rectify_maps_host(side ? right : left, width, height, m1.data(), m2.data());
        if (e) return e;
        uint2* E = ent.data() + side * WH;
        for (size_t q = 0; q < WH; ++q) {
            const int sx = m1[2 * q], sy = m1[2 * q + 1];
            // R6's border rule, decided here once: bit t set = tap t lies inside the image
            const bool x0 = sx >= 0 && sx < width, x1 = sx + 1 >= 0 && sx + 1 < width;
            const bool y0 = sy >= 0 && sy < height, y1 = sy + 1 >= 0 && sy + 1 < height;
            const uint32_t msk = (x0 && y0 ? 1u : 0u) | (x1 && y0 ? 2u : 0u) | (x0 && y1 ? 4u : 0u) | (x1 && y1 ? 8u : 0u);
            E[q].x = (uint32_t)(uint16_t)m1[2 * q] | ((uint32_t)(uint16_t)m1[2 * q + 1] << 16);
            E[q].y = (uint32_t)(m2[q] & 1023u) | (msk << 16);
        }
    }
    const int dev = gfpl_ctx_device(ctx);
    if (hipSetDevice(dev) != hipSuccess) return GFPL_E_HIP;
    gfpl_rectifier* r = new gfpl_rectifier();
    r->device = dev;
    r->stream = (hipStream_t)gfpl_ctx_stream(ctx);
    r->W = width;
    r->H = height;
    const size_t bytes = 2 * WH * sizeof(uint2);
    if (hipMalloc(&r->base, bytes) != hipSuccess) {
        (void)hipGetLastError();
        std::fprintf(stderr, "gfpl_rectifier_create: device allocation of %zu bytes failed\n", bytes);
        delete r;
        return GFPL_E_NOMEM;
    }
    r->ent[0] = (uint2*)r->base;
    r->ent[1] = r->ent[0] + WH;
    // (ent is pageable host memory: the copy has left it when hipMemcpy returns)
    if (hipMemcpy(r->base, ent.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(r->base);
        delete r;
        return GFPL_E_HIP;
    }
    r->ctx = ctx;
    gfpl_ctx_attach(ctx);
    *out = r;
    return GFPL_OK;
}

extern "C" int gfpl_rectifier_destroy(gfpl_rectifier* r) {
    if (!r) return GFPL_E_INVALID;
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();   // the detector's streams may still read the maps
    if (r->base) (void)hipFree(r->base);
    if (r->stage) (void)hipFree(r->stage);
    gfpl_ctx_detach(r->ctx);
    delete r;
    return GFPL_OK;
}

extern "C" int gfpl_rectifier_read_maps(gfpl_rectifier* r, int side, int16_t* map1, uint16_t* map2) {
    if (!r || side < 0 || side > 1 || !map1 || !map2) return GFPL_E_INVALID;
    if (hipSetDevice(r->device) != hipSuccess) return GFPL_E_HIP;
    const size_t WH = (size_t)r->W * r->H;
    std::vector<uint2> ent(WH);
    if (hipMemcpy(ent.data(), r->ent[side], WH * sizeof(uint2), hipMemcpyDeviceToHost) != hipSuccess) return GFPL_E_HIP;
    for (size_t q = 0; q < WH; ++q) {
        map1[2 * q] = (int16_t)(uint16_t)(ent[q].x & 0xFFFFu);
        map1[2 * q + 1] = (int16_t)(uint16_t)(ent[q].x >> 16);
        map2[q] = (uint16_t)(ent[q].y & 1023u);
    }
    return GFPL_OK;
}

extern "C" int gfpl_rectify_async(gfpl_rectifier* r, int side, const uint8_t* src, int n, uint8_t* dst) {
    if (!r) return GFPL_E_INVALID;
    return gfpl_rectifier_enqueue(r, r->stream, side, src, nullptr, n, dst, nullptr);
}

extern "C" int gfpl_rectify(gfpl_rectifier* r, int side, const uint8_t* src, int n, uint8_t* dst) {
    const int e = gfpl_rectify_async(r, side, src, n, dst);
    if (e) return e;
    return hipStreamSynchronize(r->stream) == hipSuccess ? GFPL_OK : GFPL_E_HIP;
}

extern "C" int gfpl_rectify_stereo_async(gfpl_rectifier* r, const uint8_t* src_l, const uint8_t* src_r, int n,
                                         uint8_t* dst_l, uint8_t* dst_r) {
    if (!r || !src_l || !src_r || !dst_l || !dst_r) return GFPL_E_INVALID;
    return gfpl_rectifier_enqueue(r, r->stream, 0, src_l, src_r, n, dst_l, dst_r);
}

extern "C" int gfpl_rectify_host(gfpl_rectifier* r, int side, const uint8_t* src, int n, uint8_t* dst) {
    if (!r || !src || !dst || n < 1 || side < 0 || side > 1) return GFPL_E_INVALID;
    if (hipSetDevice(r->device) != hipSuccess) return GFPL_E_HIP;
    const size_t bytes = (size_t)r->W * r->H * (size_t)n;
    if (r->stage_bytes < 2 * bytes) {
        if (hipStreamSynchronize(r->stream) != hipSuccess) return GFPL_E_HIP;
        if (r->stage) (void)hipFree(r->stage);
        r->stage = nullptr;
        r->stage_bytes = 0;
        if (hipMalloc((void**)&r->stage, 2 * bytes) != hipSuccess) {
            (void)hipGetLastError();
            r->stage = nullptr;
            std::fprintf(stderr, "gfpl_rectify_host: device allocation of %zu bytes failed\n", 2 * bytes);
            return GFPL_E_NOMEM;
        }
        r->stage_bytes = 2 * bytes;
    }
    if (hipMemcpyAsync(r->stage, src, bytes, hipMemcpyHostToDevice, r->stream) != hipSuccess) return GFPL_E_HIP;
    const int e = gfpl_rectifier_enqueue(r, r->stream, side, r->stage, nullptr, n, r->stage + bytes, nullptr);
    if (e) return e;
    if (hipMemcpyAsync(dst, r->stage + bytes, bytes, hipMemcpyDeviceToHost, r->stream) != hipSuccess) return GFPL_E_HIP;
    return hipStreamSynchronize(r->stream) == hipSuccess ? GFPL_OK : GFPL_E_HIP;
}
