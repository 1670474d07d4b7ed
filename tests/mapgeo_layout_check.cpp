// mapgeo_layout_check.cpp — prints the map geometry's layout (gfpl_layout.hpp: MapGeoMem) as "layout
// field offset bytes align" lines, over a null base for the size and over a real buffer for the fields,
// for tests/test_mapgeo_cpu.py.  Host code only; arguments: kf_cap pt_rows ls_rows pt_lm_cap ls_lm_cap
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
    std::printf("MapGeoMem %s %zu %zu %zu\n", name, (size_t)((char*)p - g_base), n * sizeof(T), alignof(T));
    if (n) std::memset(p, 0x5a, n * sizeof(T));
}

template <typename T>
static void both(const char* fn, T* const* p, size_t n0, size_t n1) {
    char name[48];
    std::snprintf(name, sizeof name, "pt_%s", fn);
    field(name, p[0], n0);
    std::snprintf(name, sizeof name, "ls_%s", fn);
    field(name, p[1], n1);
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    int v[6];
    for (int i = 0; i < 6; ++i) v[i] = std::atoi(argv[1 + i]);
    const MapGeoMem size(nullptr, v[0], v[1], v[2], v[3], v[4], v[5]);
    char* buf = (char*)std::malloc(size.bytes);
    const MapGeoMem m(buf, v[0], v[1], v[2], v[3], v[4], v[5]);
    g_base = buf;
    const size_t kf = (size_t)v[0], c0 = (size_t)v[3], c1 = (size_t)v[4], o0 = m.lm_obs[0], o1 = m.lm_obs[1];
    field("hdr", m.hdr, MAPGEO_HDR);
    field("T_kf", m.T_kf, kf * 16);
    field("x_kf", m.x_kf, kf * 6);
    both("lm3d", m.lm3d, c0 * MAPGEO_LM_W[0], c1 * MAPGEO_LM_W[1]);
    both("nobs", m.nobs, c0, c1);
    both("obs", m.obs, o0 * MAPGEO_OBS_W[0], o1 * MAPGEO_OBS_W[1]);
    both("sigma", m.sigma, o0, o1);
    field("pend", m.pend, m.max_lm);
    field("pair_n0", m.pair_n0, m.max_rows);
    field("kf_slot", m.kf_slot, kf);
    field("kf_mark", m.kf_mark, kf);
    field("kf_list", m.kf_list, kf);
    field("fix_list", m.fix_list, kf);
    both("lm_cnt", m.lm_cnt, c0, c1);
    both("tile_lm", m.tile_lm, m.n_tiles + 1, m.n_tiles + 1);
    both("tile_obs", m.tile_obs, m.n_tiles + 1, m.n_tiles + 1);
    both("lm_list", m.lm_list, c0, c1);
    both("lm_off", m.lm_off, c0 + 1, c1 + 1);
    field("a_x_kf", m.a_x_kf, kf * 6);
    field("a_x_out", m.a_x_out, kf * 6);
    field("a_T_kf", m.a_T_kf, kf * 16);
    field("a_T_fix", m.a_T_fix, kf * 16);
    both("a_lm3d", m.a_lm3d, c0 * MAPGEO_LM_W[0], c1 * MAPGEO_LM_W[1]);
    both("a_obs", m.a_obs, o0 * MAPGEO_OBS_W[0], o1 * MAPGEO_OBS_W[1]);
    both("a_sigma", m.a_sigma, o0, o1);
    both("a_obs_lm", m.a_obs_lm, o0, o1);
    both("a_obs_kf", m.a_obs_kf, o0, o1);
    std::printf("MapGeoMem bytes %zu %zu\n", size.bytes, m.bytes);
    std::printf("MapGeoMem consts %d %d\n", KFMAP_TILE, KFMAP_BLOCK);
    std::free(buf);
    return 0;
}
