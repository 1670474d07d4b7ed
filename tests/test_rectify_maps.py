"""gfpl_rectify_maps_host (the host-only map builder, ledger R1-R5 of DESIGN.md §4f) against
the independent numpy restatement in rectify_ref.py, bit for bit on map1 and map2, and
against known answers that need no reference.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import gfpl
import rectify_ref as R


def product_maps(side, width, height):
    s = gfpl.RectifySide.make(side["K"], side["D"], side["R"], side["P"], side.get("equi", False))
    return gfpl.rectify_maps(s, width, height)


def assert_maps_equal(side, width, height):
    m1, m2 = product_maps(side, width, height)
    r1, r2 = R.maps(side["K"], side["D"], side["R"], side["P"], width, height, side.get("equi", False))
    assert m1.shape == (height, width, 2) and m2.shape == (height, width)
    bad1 = np.argwhere(m1 != r1)
    bad2 = np.argwhere(m2 != r2)
    assert len(bad1) == 0, f"map1 differs at {len(bad1)} entries, first {bad1[0]}"
    assert len(bad2) == 0, f"map2 differs at {len(bad2)} entries, first {bad2[0]}"
    return m1, m2


small_rotation, EQUI = R.small_rotation, R.EQUI


@pytest.mark.parametrize("which", ["left", "right"])
def test_euroc_maps_match_reference(which):
    w, h, left, right = R.euroc()
    assert (w, h) == (752, 480)
    assert_maps_equal(left if which == "left" else right, w, h)


def test_equidistant_maps_match_reference():
    assert all(v != 0 for v in EQUI["D"])
    assert_maps_equal(EQUI, 512, 512)


def test_equidistant_centre_ray_takes_scale_one():
    # R = I, P.f a power of two and P.c integer: the pixel at the principal point has r == 0 exactly (scale = 1)
    side = dict(K=[200.0, 200.0, 31.5, 17.25], D=EQUI["D"], R=R.IDENTITY, P=[128.0, 128.0, 32.0, 18.0], equi=True)
    m1, m2 = assert_maps_equal(side, 67, 35)
    assert tuple(m1[18, 32]) == (31, 17) and m2[18, 32] == 8 * 32 + 16


@pytest.mark.parametrize("n_dist", [4, 5, 8])
def test_small_odd_size_every_coefficient_count(n_dist):
    D = [-0.21, 0.06, 0.0011, -0.0007, 0.013, 0.02, -0.004, 0.0009][:n_dist]
    side = dict(K=[61.3, 60.1, 33.2, 16.9], D=D, R=small_rotation(), P=[55.0, 55.0, 32.7, 17.4])
    assert_maps_equal(side, 67, 35)


def test_more_coefficients_change_the_maps():
    # the 5th and the 6th-8th coefficients are read (not silently dropped)
    D = [-0.21, 0.06, 0.0011, -0.0007, 0.5, 0.3, -0.2, 0.1]
    base = dict(K=[61.3, 60.1, 33.2, 16.9], R=R.IDENTITY, P=[55.0, 55.0, 32.7, 17.4])
    got = [product_maps(dict(base, D=D[:n]), 67, 35) for n in (4, 5, 8)]
    assert (got[0][1] != got[1][1]).any() and (got[1][1] != got[2][1]).any()


def test_negative_coordinates_shift_mask_and_ties():
    # a principal point far to the right of the image: most u are negative, so the
    # arithmetic >> 5 and the two's-complement & 31 of negative integers are exercised
    w, h, left, _ = R.euroc()
    side = dict(left, P=[435.2, 435.2, 1200.45, 900.2])
    m1, m2 = assert_maps_equal(side, w, h)
    assert (m1[..., 0] < 0).mean() > 0.5 and (m1[..., 1] < 0).mean() > 0.5
    # exact ties of lrint(u * 32): D = 0, R = I, fx = P.fx, c shifted by k / 64: u * 32 = m + 0.5
    side = dict(K=[64.0, 64.0, 10.0, 10.0], D=[0.0, 0, 0, 0], R=R.IDENTITY, P=[64.0, 64.0, 40.0 + 1 / 64, 30.0 + 3 / 64])
    m1, m2 = assert_maps_equal(side, 67, 35)
    # u = j - 30 - 1/64: u * 32 = 32 (j - 30) - 0.5 -> ties to the even neighbour 32 (j - 30)
    assert (m1[..., 0] == np.arange(67)[None, :] - 30).all() and ((m2 & 31) == 0).all()
    # v = i - 20 - 3/64: v * 32 = 32 (i - 20) - 1.5 -> ties to the even neighbour -2
    assert (m1[..., 1] == np.arange(35)[:, None] - 21).all() and ((m2 >> 5) == 30).all()


# ---------------------------------------------------------------- known answers --
def identity_side(w, h, dcx=0.0, dcy=0.0):
    K = [80.0, 75.0, float(w // 2), float(h // 2)]
    return dict(K=K, D=[0.0, 0.0, 0.0, 0.0], R=R.IDENTITY, P=[K[0], K[1], K[2] - dcx, K[3] - dcy])


def test_identity_maps():
    w, h = 67, 35
    m1, m2 = product_maps(identity_side(w, h), w, h)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    assert (m1[..., 0] == jj).all() and (m1[..., 1] == ii).all() and (m2 == 0).all()


def test_integer_principal_point_shift():
    w, h = 67, 35
    m1, m2 = product_maps(identity_side(w, h, dcx=3.0), w, h)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    assert (m1[..., 0] == jj + 3).all() and (m1[..., 1] == ii).all() and (m2 == 0).all()


def test_half_pixel_shift_gives_sixteen():
    w, h = 67, 35
    m1, m2 = product_maps(identity_side(w, h, dcx=0.5), w, h)
    jj, _ = np.meshgrid(np.arange(w), np.arange(h))
    assert (m2 == 16).all() and (m1[..., 0] == jj).all()


# ------------------------------------------------------------------- arguments --
def raw_call(side, w, h, m1=True, m2=True):
    L = gfpl.hiplib()
    a = np.zeros((max(h, 1), max(w, 1), 2), np.int16)
    b = np.zeros((max(h, 1), max(w, 1)), np.uint16)
    return L.gfpl_rectify_maps_host(C.byref(side) if side is not None else None, w, h,
                                    a.ctypes.data if m1 else None, b.ctypes.data if m2 else None)


def test_argument_errors():
    ok = identity_side(16, 16)
    mk = lambda **o: gfpl.RectifySide.make(ok["K"], o.get("D", ok["D"]), o.get("R", ok["R"]), ok["P"], o.get("equi", False))
    assert raw_call(mk(), 16, 16) == 0
    # thin-prism (12) / tilt (14) coefficient counts are not part of this; neither are 0-3, 6, 7
    for n in (0, 1, 2, 3, 6, 7):
        assert raw_call(mk(D=[0.0] * n), 16, 16) == -7, n
    s = mk()
    s.n_dist = 12
    assert raw_call(s, 16, 16) == -7
    s.n_dist = 14
    assert raw_call(s, 16, 16) == -7
    for n in (5, 8):   # the equidistant model has exactly four
        assert raw_call(mk(D=[0.0] * n, equi=True), 16, 16) == -7
    s = mk()
    s.model = 2
    assert raw_call(s, 16, 16) == -1
    assert raw_call(None, 16, 16) == -1
    assert raw_call(mk(), 16, 16, m1=False) == -1
    assert raw_call(mk(), 16, 16, m2=False) == -1
    assert raw_call(mk(), 0, 16) == -1 and raw_call(mk(), 16, -1) == -1 and raw_call(mk(), 8193, 16) == -1
    assert raw_call(mk(R=[0.0] * 9), 16, 16) == -1   # singular P R
    with pytest.raises(gfpl.GfplError) as e:
        gfpl.rectify_maps(mk(D=[0.0] * 6), 16, 16)
    assert e.value.code == -7


def test_abi_version_unchanged_and_new_error_string():
    L = gfpl.hiplib()
    assert L.gfpl_abi_version() == 6
    assert L.gfpl_strerror(-8) == b"device memory allocation failed"
