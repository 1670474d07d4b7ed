// layout_check — prints every dynamic-LDS layout of gfpl_layout.hpp (tests/test_layouts.py).
//
// Host code only: each layout is built twice, as a launcher does over a null base (its .bytes)
// and over a host buffer of exactly that many bytes (the fields' offsets), so a sanitised build
// of this program also checks that no take forms a pointer outside the bytes it announces.
// Exits 1 if a field is not aligned to its type.
//
// usage: layout_check HEIGHT:LEVELS ...      one JSON object per line
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/gfpl.h"
#include "../gf-pl-slam_amd/csrc/gfpl_layout.hpp"

using namespace gfpl;

namespace {

std::vector<unsigned char> g_buf;
const unsigned char* g_base = nullptr;

unsigned char* buffer(int bytes) {
    g_buf.assign(bytes, 0);
    g_base = g_buf.data();
    return g_buf.data();
}
long off(const void* p) { return p ? (long)((const unsigned char*)p - g_base) : -1; }

int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

int g_misaligned = 0;
template <typename T>
long checked(const char* name, T* p) {
    if (p && off(p) % (long)alignof(T)) {
        std::fprintf(stderr, "layout_check: %s at %ld is not aligned to %zu\n", name, off(p), alignof(T));
        ++g_misaligned;
    }
    return off(p);
}
#define F(name) std::printf(", \"%s\": %ld", #name, checked(#name, L.name))

void stereo_points(int kp_cap, int height, int levels, bool seg, int waves) {
    const int KP2 = next_pow2(kp_cap);
    const int bytes = StereoPointsLds(nullptr, KP2, height, levels, seg, waves).bytes;
    const StereoPointsLds L(buffer(bytes), KP2, height, levels, seg, waves);
    std::printf("{\"layout\": \"stereo_points\", \"kp_cap\": %d, \"KP2\": %d, \"height\": %d, \"levels\": %d, \"seg\": %d, "
                "\"waves\": %d, \"bytes\": %d, \"placed\": %d",
                kp_cap, KP2, height, levels, (int)seg, waves, bytes, L.bytes);
    F(rkey); F(order); F(pairs); F(recx); F(recm); F(rowlo); F(misc); F(stg);
    F(depth); F(hr); F(offr); F(hl); F(offl);
    std::printf("}\n");
}

void stereo_lines(int cap, int cell) {
    const int bytes = StereoLinesLds(nullptr, cap, cell).bytes;
    const StereoLinesLds L(buffer(bytes), cap, cell);
    std::printf("{\"layout\": \"stereo_lines\", \"kl_cap\": %d, \"cell\": %d, \"lut_dwords\": %d, \"lut2_dwords\": %d, "
                "\"bytes\": %d, \"placed\": %d",
                cap, cell, knn_lut_dwords(cell), knn_lut_dwords(2), bytes, L.bytes);
    F(lut); F(tb); F(lr_i); F(lr_d0); F(lr_d1); F(rl_i); F(hist); F(th); F(scan);
    std::printf("}\n");
}

void cross_lines(int cap) {
    const int bytes = CrossLinesLds(nullptr, cap).bytes;
    const CrossLinesLds L(buffer(bytes), cap);
    std::printf("{\"layout\": \"cross_lines\", \"kl_cap\": %d, \"lut_dwords\": %d, \"bytes\": %d, \"placed\": %d", cap,
                knn_lut_dwords(1), bytes, L.bytes);
    F(lut); F(tb); F(i12); F(d012); F(d112); F(i21); F(h12); F(h0); F(scan); F(th);
    std::printf("}\n");
}

void knn2(int cell) {
    const int bytes = Knn2Lds(nullptr, cell).bytes;
    const Knn2Lds L(buffer(bytes), cell);
    std::printf("{\"layout\": \"knn2\", \"cell\": %d, \"lut_dwords\": %d, \"chunk\": %d, \"bytes\": %d, \"placed\": %d", cell,
                knn_lut_dwords(cell), KNN_CHUNK, bytes, L.bytes);
    F(lut); F(tb);
    std::printf("}\n");
}

void cross_points(int cap, int ncell, bool xl) {
    const int bytes = CrossPointsLds(nullptr, cap, ncell, xl).bytes;
    const CrossPointsLds L(buffer(bytes), cap, ncell, xl);
    std::printf("{\"layout\": \"cross_points\", \"kp_cap\": %d, \"ncell\": %d, \"xl\": %d, \"bytes\": %d, \"placed\": %d", cap,
                ncell, (int)xl, bytes, L.bytes);
    F(prevT); F(Tinv); F(spxy); F(cnt); F(start); F(sq); F(spx); F(spy); F(lastT); F(misc);
    std::printf("}\n");
}

void pose(int W, int mpt, int mls) {
    int NP2 = 1;
    while (NP2 < mpt || NP2 < mls) NP2 <<= 1;
    const int bytes = PoseLds(nullptr, W, NP2, mpt, mls).bytes;
    const PoseLds L(buffer(bytes), W, NP2, mpt, mls);
    std::printf("{\"layout\": \"pose\", \"W\": %d, \"NP2\": %d, \"mpt_cap\": %d, \"mls_cap\": %d, \"ch_stride\": %d, "
                "\"bytes\": %d, \"placed\": %d",
                W, NP2, mpt, mls, CH_STRIDE, bytes, L.bytes);
    F(cp); F(cl); F(buf); F(act);
    std::printf("}\n");
}

void orb_cell(int patch_cap, int waves, int wave) {
    const int bytes = OrbCellLds(nullptr, patch_cap, waves, 0).bytes;
    const OrbCellLds L(buffer(bytes), patch_cap, waves, wave);
    std::printf("{\"layout\": \"orb_cell\", \"patch_cap\": %d, \"waves\": %d, \"wave\": %d, \"bytes\": %d, \"placed\": %d",
                patch_cap, waves, wave, bytes, L.bytes);
    F(P); F(Sc); F(cand);
    std::printf("}\n");
}

void lsd_grow(int cid_cap) {
    const int bytes = LsdGrowLds(nullptr, cid_cap).bytes;
    const LsdGrowLds L(buffer(bytes), cid_cap);
    std::printf("{\"layout\": \"lsd_grow\", \"cid_cap\": %d, \"ring_entries\": %d, \"bytes\": %d, \"placed\": %d", cid_cap,
                LSD_RING, bytes, L.bytes);
    F(ring); F(used);
    std::printf("}\n");
}

}  // namespace

int main(int argc, char** argv) {
    const int kp_caps[] = {2, 66, 2000, 2048, 2050, 8192};
    const int kl_caps[] = {2, 34, 200, 500, 1024, 1026, 2048};
    const int matched[][2] = {{500, 300}, {GFPL_MAX_MATCHED_PT, GFPL_MAX_MATCHED_LS}};
    for (int a = 1; a < argc; ++a) {
        int height = 0, levels = 0;
        if (std::sscanf(argv[a], "%d:%d", &height, &levels) != 2 || height < 1 || levels < 1) {
            std::fprintf(stderr, "usage: %s HEIGHT:LEVELS ...\n", argv[0]);
            return 2;
        }
        for (int kp : kp_caps)
            for (int seg = 0; seg < 2; ++seg)
                for (int waves : {8, 16}) stereo_points(kp, height, levels, seg != 0, waves);
    }
    for (int kl : kl_caps) {
        for (int cell : {1, 2}) stereo_lines(kl, cell);
        cross_lines(kl);
    }
    for (int cell : {1, 2}) knn2(cell);
    // bucket grids: the smallest, a VGA-sized one and the largest the kernel accepts
    for (int kp : kp_caps)
        for (int ncell : {1, 1200, 2048})
            for (int xl = 0; xl < 2; ++xl) cross_points(kp, ncell, xl != 0);
    for (const auto& m : matched)
        for (int W : {1, 4, 8}) pose(W, m[0], m[1]);
    for (int patch_cap : {16, 1296, 4096})
        for (int waves : {1, 4})
            for (int wave = 0; wave < waves; ++wave) orb_cell(patch_cap, waves, wave);
    for (int cid_cap : {32, 76800, 491520}) lsd_grow(cid_cap);
    return g_misaligned ? 1 : 0;
}
