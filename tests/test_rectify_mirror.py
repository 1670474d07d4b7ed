"""The host mirror's PinholeStereoCamera::rectifyImagesLR / rectifyImage
(gf-pl-slam_amd/host/stvo.h) through a small C++ caller (tests/mirror_rectify.cpp, built by
make): a camera of the reference's distortion constructor shape equals rectify_ref on one
752 x 480 pair, a camera built with the distortion-free constructor returns copies."""
import os
import subprocess

import numpy as np
import pytest

import rectify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gf-pl-slam_amd", "bin", "mirror_rectify")


def write_rig(path, left, right, equi=False):
    with open(path, "w") as f:
        f.write("# rig calibration (plslam_gpu --rectify format)\n")
        for key, v in (("Kl", left["K"]), ("Kr", right["K"]), ("Dl", left["D"]), ("Dr", right["D"]),
                       ("Rl", left["R"]), ("Rr", right["R"]), ("Pl", left["P"]), ("Pr", right["P"])):
            f.write(f"{key}: [" + ", ".join(repr(float(x)) for x in v) + "]\n")
        if equi:
            f.write("equi: 1\n")


def run_driver(tmp_path, left, right, w, h, imgs):
    write_rig(tmp_path / "rig.txt", left, right)
    imgs[0].tofile(tmp_path / "l.raw")
    imgs[1].tofile(tmp_path / "r.raw")
    return subprocess.run([BIN, str(tmp_path / "rig.txt"), str(w), str(h), str(tmp_path / "l.raw"),
                           str(tmp_path / "r.raw"), str(tmp_path / "out")], capture_output=True, text=True)


def load(tmp_path, name, w, h):
    return np.fromfile(tmp_path / f"out_{name}.raw", np.uint8).reshape(h, w)


@pytest.mark.gpu
def test_mirror_rectify_images_lr_matches_reference(tmp_path):
    w, h, left, right = R.euroc()
    imgs = R.random_images(2, h, w, 21)
    p = run_driver(tmp_path, left, right, w, h, imgs)
    assert p.returncode == 0, p.stderr
    want_l = R.remap(imgs[0], *R.maps(left["K"], left["D"], left["R"], left["P"], w, h))
    want_r = R.remap(imgs[1], *R.maps(right["K"], right["D"], right["R"], right["P"], w, h))
    assert (load(tmp_path, "l", w, h) == want_l).all() and (load(tmp_path, "r", w, h) == want_r).all()
    assert (load(tmp_path, "one", w, h) == want_l).all()       # rectifyImage: the left maps
    assert (load(tmp_path, "copy_l", w, h) == want_l).all() and (load(tmp_path, "copy_r", w, h) == want_r).all()
    for name, src in (("plain_l", imgs[0]), ("plain_r", imgs[1]), ("plain_one", imgs[0])):
        assert (load(tmp_path, name, w, h) == src).all(), name


def test_mirror_plain_camera_clones_without_a_device(tmp_path):
    """dist == false needs no device: the clones are written before the distortion camera's first
    use (which, without a GPU, then fails loudly)."""
    assert os.path.exists(BIN), "host mirror not built"
    w, h, left, right = R.euroc()
    imgs = R.random_images(2, h, w, 22)
    p = run_driver(tmp_path, left, right, w, h, imgs)
    for name, src in (("plain_l", imgs[0]), ("plain_r", imgs[1]), ("plain_one", imgs[0])):
        assert (load(tmp_path, name, w, h) == src).all(), name
    if p.returncode != 0:   # no GPU here
        assert p.returncode == 1 and "gfpl_create" in p.stderr, p.stderr


def test_rig_file_errors(tmp_path):
    assert os.path.exists(BIN), "host mirror not built"
    w, h, left, right = R.euroc()
    (tmp_path / "bad.txt").write_text("Kl: 1 2 3 4\nKq: 1\n")
    np.zeros(w * h, np.uint8).tofile(tmp_path / "z.raw")
    p = subprocess.run([BIN, str(tmp_path / "bad.txt"), str(w), str(h), str(tmp_path / "z.raw"), str(tmp_path / "z.raw"),
                        str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 1 and "unknown key" in p.stderr
    (tmp_path / "short.txt").write_text("Kl: 1 2 3 4\n")
    p = subprocess.run([BIN, str(tmp_path / "short.txt"), str(w), str(h), str(tmp_path / "z.raw"),
                        str(tmp_path / "z.raw"), str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 1 and "needs Kl" in p.stderr
