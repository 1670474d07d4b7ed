// pgo_layout_check.cpp — prints the pose graph's layouts (gfpl_layout.hpp: PgoLds, PgoMem, PgoIdx) as
// "layout field offset bytes align" lines, over a null base for the sizes and over a real buffer for
// the fields, for tests/test_pgo_layout.py.  Host code only; arguments: n_kf n_lc n_vert n_free n_edge
// env_blocks n_jobs.  Every field is then written end to end, so under ASan a field that leaves the
// buffer is a report.
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
    if (argc < 8) return 2;
    const int nkf = std::atoi(argv[1]), nlc = std::atoi(argv[2]), nv = std::atoi(argv[3]), nf = std::atoi(argv[4]),
              ne = std::atoi(argv[5]), nenv = std::atoi(argv[6]), nj = std::atoi(argv[7]);
    {
        const PgoLds size(nullptr);
        unsigned char* buf = (unsigned char*)std::malloc((size_t)size.bytes);
        const PgoLds L(buf);
        g_layout = "PgoLds"; g_base = (char*)buf;
        field("pk", L.pk, 6 * PGO_PANEL); field("pd", L.pd, 6 * PGO_PANEL); field("red", L.red, PGO_BLOCK);
        field("sd", L.sd, 16); field("si", L.si, 16);
        std::printf("PgoLds bytes %d %d\n", size.bytes, L.bytes);
        std::free(buf);
    }
    {
        const PgoMem size(nullptr, nkf, nv, nf, ne, nenv);
        char* buf = (char*)std::malloc(size.bytes);
        const PgoMem m(buf, nkf, nv, nf, ne, nenv);
        g_layout = "PgoMem"; g_base = buf;
        field("X", m.p.X, (size_t)nv * 16); field("Xt", m.p.Xt, (size_t)nv * 16); field("X0", m.p.X0, (size_t)nv * 16);
        field("Z", m.p.Z, (size_t)ne * 16); field("rows", m.p.rows, (size_t)ne * PGO_ROW); field("esq", m.p.esq, (size_t)ne);
        field("diag", m.p.diag, (size_t)nf * 36); field("b", m.p.b, (size_t)nf * 6);
        field("H", m.p.H, (size_t)nenv * 36); field("L", m.p.L, (size_t)nenv * 36);
        field("D", m.p.D, (size_t)nf * 6); field("y", m.p.y, (size_t)nf * 6);
        field("corr", m.p.corr, (size_t)nkf * 16); field("moved", m.p.moved, (size_t)nkf); field("state", m.p.state, 8);
        std::printf("PgoMem bytes %zu %zu\n", size.bytes, m.bytes);
        std::free(buf);
    }
    {
        const PgoIdx size(nullptr, nkf, nlc, nv, nf, ne, nj);
        char* buf = (char*)std::malloc(size.bytes);
        const PgoIdx x(buf, nkf, nlc, nv, nf, ne, nj);
        g_layout = "PgoIdx"; g_base = buf;
        field("vert", x.vert, (size_t)nv * 4); field("free_vert", x.free_vert, (size_t)nf); field("edge", x.edge, (size_t)ne * 4);
        field("inc_start", x.inc_start, (size_t)nf + 1); field("inc", x.inc, (size_t)ne * 2);
        field("env_first", x.env_first, (size_t)nf); field("env_off", x.env_off, (size_t)nf + 1); field("reach", x.reach, (size_t)nf);
        field("lc", x.lc, (size_t)nlc * 3); field("alive", x.alive, (size_t)nkf); field("jobs", x.jobs, (size_t)nj * 4);
        field("lc_pose", x.lc_pose, (size_t)nlc * 6);
        std::printf("PgoIdx bytes %zu %zu\n", size.bytes, x.bytes);
        std::free(buf);
    }
    return 0;
}
