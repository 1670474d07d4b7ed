// Probe behind DESIGN.md §4f "what limits k_rectify": the interior path of the remap kernel at
// 752 x 480 with a smooth barrel warp, 2048 images, in six variants — U = 1 / 2 / 4 images
// per lane and loop iteration (all loads issued before the first use), with a lane owning four
// consecutive pixels (var 0-2) or pixels lane + 64 k of a wave's 256-pixel run, transposed
// through LDS for the dword store (var 3-5) — for batch slices of 8, 16 and 32 images.  Every
// variant's output is compared with the first one's.  Not part of the product library.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/probe/rectify_variants.hip -o tools/probe/rectify_variants
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include <cstring>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Args { const uint2* ent; const uint8_t* src; uint8_t* dst; int W, WH, n, per; };

__device__ __forceinline__ uint32_t ld2(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

// U: images per loop iteration.  STRIDED: lane owns pixels lane + 64 k of a wave's 256-pixel run
// (the taps of one load instruction are 64 neighbouring pixels), transposed through LDS.
template <int U, int STRIDED>
__global__ void __launch_bounds__(256) k(Args a) {
    __shared__ uint8_t tr[STRIDED ? 1024 : 4];
    const int W = a.W, WH = a.WH;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wbase = (blockIdx.x * 4 + wave) * 256;   // first pixel of the wave's run
    int off[4]; uint32_t w00[4], w01[4], w10[4], w11[4];
    if (!STRIDED && 4 * t >= WH) return;
    if (STRIDED && wbase >= WH) return;   // (WH % 256 == 0 in this benchmark)
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) {
        const int q = STRIDED ? wbase + lane + 64 * k2 : 4 * t + k2;
        const uint2 e = a.ent[q];
        const int sx = (int)(int16_t)(e.x & 0xFFFFu), sy = (int)(int16_t)(e.x >> 16);
        const uint32_t fa = e.y & 31u, fb = (e.y >> 5) & 31u;
        off[k2] = sy * W + sx;
        w00[k2] = (32u - fa) * (32u - fb); w01[k2] = fa * (32u - fb); w10[k2] = (32u - fa) * fb; w11[k2] = fa * fb;
    }
    const int i0 = blockIdx.y * a.per, i1 = min(a.n, i0 + a.per);
    for (int i = i0; i < i1; i += U) {
        uint32_t r0[U][4], r1[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint8_t* S = a.src + (size_t)(i + u) * WH;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) { r0[u][k2] = ld2(S + off[k2]); r1[u][k2] = ld2(S + off[k2] + W); }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint32_t v[4];
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2)
                v[k2] = (w00[k2] * (r0[u][k2] & 255u) + w01[k2] * (r0[u][k2] >> 8) + w10[k2] * (r1[u][k2] & 255u) + w11[k2] * (r1[u][k2] >> 8) + 512u) >> 10;
            if (STRIDED) {
                uint8_t* T = tr + wave * 256;
#pragma unroll
                for (int k2 = 0; k2 < 4; ++k2) T[lane + 64 * k2] = (uint8_t)v[k2];
                __builtin_amdgcn_wave_barrier();
                const uint32_t out = *reinterpret_cast<const uint32_t*>(T + 4 * lane);
                __builtin_amdgcn_wave_barrier();
                *reinterpret_cast<uint32_t*>(a.dst + (size_t)(i + u) * WH + wbase + 4 * lane) = out;
            } else {
                *reinterpret_cast<uint32_t*>(a.dst + (size_t)(i + u) * WH + 4 * t) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            }
        }
    }
}

int main(int argc, char** argv) {
    const int W = 752, H = 480, WH = W * H, n = argc > 1 ? atoi(argv[1]) : 2048;
    std::vector<uint2> ent(WH);
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {   // a smooth barrel-like warp that stays inside the image
            const double x = (j - 376.0) / 435.0, y = (i - 240.0) / 435.0, r2 = x * x + y * y;
            const double kr = 1 - 0.28 * r2 + 0.07 * r2 * r2;
            double u = 458.0 * x * kr + 370.0, v = 457.0 * y * kr + 245.0;
            u = fmin(fmax(u, 0.0), W - 2.0); v = fmin(fmax(v, 0.0), H - 2.0);
            const int iu = (int)lrint(u * 32), iv = (int)lrint(v * 32);
            ent[i * W + j].x = (uint32_t)(uint16_t)(iu >> 5) | ((uint32_t)(uint16_t)(iv >> 5) << 16);
            ent[i * W + j].y = (uint32_t)((iv & 31) * 32 + (iu & 31)) | (15u << 16);
        }
    uint2* d_ent; uint8_t *d_src, *d_dst, *d_ref;
    const size_t bytes = (size_t)WH * n;
    CHECK(hipMalloc(&d_ent, WH * 8)); CHECK(hipMalloc(&d_src, bytes + 4096)); CHECK(hipMalloc(&d_dst, bytes)); CHECK(hipMalloc(&d_ref, bytes));
    CHECK(hipMemcpy(d_ent, ent.data(), WH * 8, hipMemcpyHostToDevice));
    std::vector<uint8_t> h(bytes);
    uint32_t s = 12345u;
    for (size_t i = 0; i < bytes; ++i) { s = s * 1664525u + 1013904223u; h[i] = (uint8_t)(s >> 24); }
    CHECK(hipMemcpy(d_src, h.data(), bytes, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<uint8_t> ref(bytes), got(bytes);
    for (int per : {8, 16, 32}) {
        for (int var = 0; var < 6; ++var) {
            Args a{d_ent, d_src, var == 0 && per == 8 ? d_ref : d_dst, W, WH, n, per};
            dim3 grid(var >= 3 ? (WH / 256 + 3) / 4 : (WH / 4 + 255) / 256, (n + per - 1) / per);
            auto launch = [&]() {
                switch (var) {
                    case 0: hipLaunchKernelGGL((k<1, 0>), grid, dim3(256), 0, 0, a); break;
                    case 1: hipLaunchKernelGGL((k<2, 0>), grid, dim3(256), 0, 0, a); break;
                    case 2: hipLaunchKernelGGL((k<4, 0>), grid, dim3(256), 0, 0, a); break;
                    case 3: hipLaunchKernelGGL((k<1, 1>), grid, dim3(256), 0, 0, a); break;
                    case 4: hipLaunchKernelGGL((k<2, 1>), grid, dim3(256), 0, 0, a); break;
                    default: hipLaunchKernelGGL((k<4, 1>), grid, dim3(256), 0, 0, a); break;
                }
            };
            for (int w = 0; w < 3; ++w) launch();
            CHECK(hipDeviceSynchronize());
            CHECK(hipEventRecord(e0, 0));
            for (int r = 0; r < 10; ++r) launch();
            CHECK(hipEventRecord(e1, 0));
            CHECK(hipEventSynchronize(e1));
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
            ms /= 10;
            bool same = true;
            if (var == 0 && per == 8) CHECK(hipMemcpy(ref.data(), d_ref, bytes, hipMemcpyDeviceToHost));
            else { CHECK(hipMemcpy(got.data(), d_dst, bytes, hipMemcpyDeviceToHost)); same = memcmp(got.data(), ref.data(), bytes) == 0; }
            printf("per %2d var %d (U 1/2/4, strided for var >= 3): %.4f ms  %.0f GB/s  %.2fM img/s  same %d\n", per, var, ms,
                   2.0 * bytes / ms / 1e6, n / ms / 1e3, (int)same);
            fflush(stdout);
        }
    }
    return 0;
}
