// gba_layout_check.cpp — prints the global bundle adjustment's layouts (gfpl_layout.hpp: GbaMem, GbaIdx,
// GbaLdltLds, GbaSubstLds) as "layout field offset bytes align" lines, over a null base for the sizes
// and over a real buffer for the fields, for tests/test_gba_cpu.py.  Host code only; arguments: n_kf
// n_pt n_ls n_obs n_pt_pairs n_ls_pairs n_terms ldlt_rows.  Every field is then written end to end, so
// under ASan a field that leaves the buffer is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gf-pl-slam_amd/csrc/gfpl_layout.hpp"

using namespace gfpl;

static const char* g_layout;
static char* g_base;

template <typename T>
static void field(const char* name, T* p, size_t n) {
    std::printf("%s %s %zu %zu %zu\n", g_layout, name, (size_t)((char*)p - g_base), n * sizeof(T), alignof(T));
    if (n) std::memset(p, 0x5a, n * sizeof(T));
}

int main(int argc, char** argv) {
    if (argc < 9) return 2;
    const int nkf = std::atoi(argv[1]), npt = std::atoi(argv[2]), nls = std::atoi(argv[3]), nobs = std::atoi(argv[4]),
              npp = std::atoi(argv[5]), nlp = std::atoi(argv[6]), nt = std::atoi(argv[7]), rows = std::atoi(argv[8]);
    const size_t N = 6 * (size_t)nkf + 3 * (size_t)npt + 6 * (size_t)nls, n6 = 6 * (size_t)nkf, nlm = (size_t)npt + nls;
    {
        const GbaMem size(nullptr, nkf, npt, nls, nobs, npp, nlp);
        char* buf = (char*)std::malloc(size.bytes);
        const GbaMem m(buf, nkf, npt, nls, nobs, npp, nlp);
        g_layout = "GbaMem"; g_base = buf;
        const size_t nv = 9 * (size_t)npt + 36 * (size_t)nls, ng = 3 * (size_t)npt + 6 * (size_t)nls;
        const size_t nw = 18 * (size_t)npp + 36 * (size_t)nlp;
        field("X", m.p.X, N); field("DX", m.p.DX, N); field("rows", m.p.rows, (size_t)nobs * GBA_ROW);
        field("Tinv", m.p.Tinv, (size_t)nkf * 16); field("U", m.p.U, (size_t)nkf * 36); field("gk", m.p.gk, n6);
        field("V", m.p.V, nv); field("Vi", m.p.Vi, nv); field("glm", m.p.glm, ng); field("z", m.p.z, ng);
        field("W", m.p.W, nw); field("Y", m.p.Y, nw); field("q", m.p.q, nlm); field("dmax", m.p.dmax, nlm);
        field("S", m.p.S, n6 * n6); field("D", m.p.D, n6); field("gr", m.p.gr, n6);
        field("sd", m.p.sd, 8); field("si", m.p.si, 16);
        std::printf("GbaMem bytes %zu %zu\n", size.bytes, m.bytes);
        std::free(buf);
    }
    {
        const GbaIdx size(nullptr, nkf, (int)nlm, nobs, npp + nlp, nt);
        char* buf = (char*)std::malloc(size.bytes);
        const GbaIdx x(buf, nkf, (int)nlm, nobs, npp + nlp, nt);
        g_layout = "GbaIdx"; g_base = buf;
        field("lm_start", x.lm_start, nlm + 1); field("obs_lm", x.obs_lm, (size_t)nobs); field("obs_kf", x.obs_kf, (size_t)nobs);
        field("obs_pair", x.obs_pair, (size_t)nobs); field("pair_start", x.pair_start, nlm + 1);
        field("pair_kf", x.pair_kf, (size_t)npp + nlp); field("kf_start", x.kf_start, (size_t)nkf + 1);
        field("kf_obs", x.kf_obs, (size_t)nobs); field("blk_start", x.blk_start, (size_t)nkf * (nkf + 1) / 2 + 1);
        field("terms", x.terms, (size_t)nt * 3);
        std::printf("GbaIdx bytes %zu %zu\n", size.bytes, x.bytes);
        std::free(buf);
    }
    {
        const GbaLdltLds size(nullptr, 6 + 6 * rows);
        unsigned char* buf = (unsigned char*)std::malloc((size_t)size.bytes);
        const GbaLdltLds L(buf, 6 + 6 * rows);
        g_layout = "GbaLdltLds"; g_base = (char*)buf;
        field("part", L.part, (size_t)(6 + 6 * rows) * 6); field("Ld", L.Ld, 36); field("Dd", L.Dd, 6); field("flag", L.flag, 2);
        std::printf("GbaLdltLds bytes %d %d\n", size.bytes, L.bytes);
        std::free(buf);
    }
    {
        const GbaSubstLds size(nullptr, (int)n6);
        unsigned char* buf = (unsigned char*)std::malloc((size_t)size.bytes + 1);
        const GbaSubstLds L(buf, (int)n6);
        g_layout = "GbaSubstLds"; g_base = (char*)buf;
        field("y", L.y, n6);
        std::printf("GbaSubstLds bytes %d %d\n", size.bytes, L.bytes);
        std::free(buf);
    }
    return 0;
}
