// kfmap_layout_check.cpp — prints the keyframe map's layout (gfpl_layout.hpp: KfMapMem) as "layout field
// offset bytes align" lines, over a null base for the size and over a real buffer for the fields, for
// tests/test_kfmap_cpu.py.  Host code only; arguments: kf_cap pt_rows ls_rows pt_lm_cap ls_lm_cap
// obs_cap.  Every field is then written end to end, so under ASan a field that leaves the buffer is a
// report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gf-pl-slam_amd/csrc/gfpl_layout.hpp"

using namespace gfpl;

static char* g_base;

template <typename T>
static void field(const char* name, T* p, size_t n) {
    std::printf("KfMapMem %s %zu %zu %zu\n", name, (size_t)((char*)p - g_base), n * sizeof(T), alignof(T));
    if (n) std::memset(p, 0x5a, n * sizeof(T));
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    int v[6];
    for (int i = 0; i < 6; ++i) v[i] = std::atoi(argv[1 + i]);
    const KfMapMem size(nullptr, v[0], v[1], v[2], v[3], v[4], v[5]);
    char* buf = (char*)std::malloc(size.bytes);
    const KfMapMem m(buf, v[0], v[1], v[2], v[3], v[4], v[5]);
    g_base = buf;
    const size_t kf = (size_t)v[0], obs = (size_t)v[5];
    field("hdr", m.hdr, KFMAP_HDR);
    field("kf_alive", m.kf_alive, kf);
    field("kf_local", m.kf_local, kf);
    field("kf_n_pt", m.kf_n[0], kf);
    field("kf_n_ls", m.kf_n[1], kf);
    field("pt_idx", m.kf_idx[0], kf * v[1]);
    field("ls_idx", m.kf_idx[1], kf * v[2]);
    field("graph", m.graph, kf * kf);
    const char* kind[2] = {"pt", "ls"};
    char name[32];
    for (int f = 0; f < 6; ++f)
        for (int k = 0; k < 2; ++k) {
            const size_t n = (size_t)v[3 + k];
            static const char* fn[6] = {"alive", "local", "inlier", "nobs", "owner", "obs"};
            std::snprintf(name, sizeof name, "%s_%s", kind[k], fn[f]);
            switch (f) {
            case 0: field(name, m.lm_alive[k], n); break;
            case 1: field(name, m.lm_local[k], n); break;
            case 2: field(name, m.lm_inlier[k], n); break;
            case 3: field(name, m.lm_nobs[k], n); break;
            case 4: field(name, m.lm_owner[k], n); break;
            default: field(name, m.lm_obs[k], n * obs); break;
            }
        }
    field("tile", m.tile, m.n_tiles + 1);
    field("seen0", m.seen0, m.max_items);
    field("seen1", m.seen1, m.max_rows);
    field("pend", m.pend, m.max_lm);
    field("first_row", m.first_row, m.max_lm);
    field("pair_n0", m.pair_n0, m.max_rows);
    field("pair_slot", m.pair_slot, m.max_rows);
    std::printf("KfMapMem bytes %zu %zu\n", size.bytes, m.bytes);
    std::printf("KfMapMem consts %d %d\n", KFMAP_TILE, KFMAP_BLOCK);
    std::free(buf);
    return 0;
}
