// A caller of the mirror's PinholeStereoCamera::rectifyImagesLR / rectifyImage
// (tests/test_rectify_mirror.py):
//   mirror_rectify RECTIFY_FILE W H LEFT.raw RIGHT.raw OUT_PREFIX
// reads the rig (the plslam_gpu --rectify format, values unchanged) and one raw stereo pair
// (W*H bytes each), and writes OUT_PREFIX_l.raw / _r.raw (rectifyImagesLR), _one.raw
// (rectifyImage of the left image), _copy_l.raw / _copy_r.raw (rectifyImagesLR of a copy of
// the camera) and _plain_l.raw / _plain_r.raw / _plain_one.raw from a camera built with the
// distortion-free constructor (copies of the input, written before any device is touched).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../gf-pl-slam_amd/host/stvo.h"

using namespace StVO;

static std::vector<uint8_t> slurp(const std::string& p, size_t n) {
    std::ifstream f(p, std::ios::binary);
    std::vector<uint8_t> v(n);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)n);
    if (!f) throw std::runtime_error(p + ": short read");
    return v;
}

static void dump(const std::string& p, const std::vector<uint8_t>& v) {
    std::ofstream f(p, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)v.size());
}

int main(int argc, char** argv) {
    try {
        if (argc != 7) { std::cerr << "usage: mirror_rectify FILE W H LEFT RIGHT OUT_PREFIX\n"; return 2; }
        const RectifyFile rf = RectifyFile::read(argv[1]);
        const int w = std::stoi(argv[2]), h = std::stoi(argv[3]);
        const std::vector<uint8_t> L = slurp(argv[4], (size_t)w * h), R = slurp(argv[5], (size_t)w * h);
        const std::string out = argv[6];
        // the distortion-free constructor first: no device is needed for its clones
        PinholeStereoCamera plain(w, h, rf.Pl[0], rf.Pl[1], rf.Pl[2], rf.Pl[3], 0.11);
        std::vector<uint8_t> a, b, c;
        plain.rectifyImagesLR(L, a, R, b);
        plain.rectifyImage(L, c);
        dump(out + "_plain_l.raw", a);
        dump(out + "_plain_r.raw", b);
        dump(out + "_plain_one.raw", c);
        if (plain.distorted()) return 3;
        PinholeStereoCamera cam(w, h, 0.11, rf.Kl.data(), rf.Kr.data(), rf.Rl.data(), rf.Rr.data(), rf.Pl.data(),
                                rf.Pr.data(), rf.Dl, rf.Dr, rf.equi);
        if (!cam.distorted() || cam.getFx() != rf.Pl[0] || cam.getCy() != rf.Pl[3]) return 3;
        cam.rectifyImagesLR(L, a, R, b);
        cam.rectifyImage(L, c);
        dump(out + "_l.raw", a);
        dump(out + "_r.raw", b);
        dump(out + "_one.raw", c);
        const PinholeStereoCamera copy(cam);   // a copy rectifies with maps of its own
        copy.rectifyImagesLR(L, a, R, b);
        dump(out + "_copy_l.raw", a);
        dump(out + "_copy_r.raw", b);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "mirror_rectify: " << e.what() << "\n";
        return 1;
    }
}
