"""k_rectify on the GPU (gfpl.StereoRectifier; ledger R6 of DESIGN.md §4f): known answers that
need no reference, and rectify_ref.remap (the numpy restatement) on random images — every
comparison bitwise on the full image."""
import functools

import numpy as np
import pytest

import gfpl
import rectify_ref as R

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    cfg = gfpl.default_config()
    c = gfpl.Context(gfpl.make_camera("vga", cfg), cfg)
    yield c
    c.close()


def side_of(d):
    return gfpl.RectifySide.make(d["K"], d["D"], d["R"], d["P"], d.get("equi", False))


def shift_side(w, h, dx=0.0, dy=0.0):
    """D = 0, R = I, P = K with the principal point moved: dst(i, j) = src(i + dy, j + dx)"""
    K = [64.0, 64.0, float(w // 2), float(h // 2)]
    return dict(K=K, D=[0.0] * 4, R=R.IDENTITY, P=[64.0, 64.0, K[2] - dx, K[3] - dy])


@functools.lru_cache(maxsize=None)
def ref_maps(key):
    w, h, left, right = R.euroc()
    d = {"euroc_l": (left, w, h), "euroc_r": (right, w, h), "equi": (R.EQUI, 752, 480),
         "far": (dict(left, P=[435.2, 435.2, 40.3, 470.6]), w, h),
         "far2": (dict(right, P=[300.0, 300.0, 700.7, 10.2]), w, h),
         "wide": (dict(left, P=[200.0, 200.0, 376.3, 240.6]), w, h),
         "small": (dict(K=[61.3, 60.1, 33.2, 16.9], D=[-0.21, 0.06, 0.0011, -0.0007, 0.013],
                        R=R.IDENTITY, P=[50.0, 50.0, 31.7, 18.4]), 67, 35)}[key]
    side, w, h = d
    m1, m2 = R.maps(side["K"], side["D"], side["R"], side["P"], w, h, side.get("equi", False))
    m1.setflags(write=False)
    m2.setflags(write=False)
    return side, w, h, m1, m2


@functools.lru_cache(maxsize=None)
def images(n, h, w, seed=7):
    img = R.random_images(n, h, w, seed)
    img.setflags(write=False)
    return img


def run(rect, side, src, offset=0, stereo_src=None):
    """rectify n host images through the device; the output sits `offset` bytes into a buffer
    filled with FILL whose bytes before and after the range must keep it.  Returns [n][H][W]
    (a pair with stereo_src: both sides in one call)."""
    import torch
    dev = torch.device("cuda", 0)
    n, h, w = src.shape
    pad = 64
    outs = []
    bufs = [torch.full((pad + offset + n * h * w + pad,), FILL, dtype=torch.uint8, device=dev)
            for _ in range(2 if stereo_src is not None else 1)]
    d_src = torch.from_numpy(np.array(src)).to(dev)   # (a writable copy: the shared inputs are read-only)
    torch.cuda.synchronize()
    if stereo_src is None:
        rect.rectify(side, d_src, n, bufs[0][pad + offset:], sync=True)
    else:
        d_src2 = torch.from_numpy(np.array(stereo_src)).to(dev)
        torch.cuda.synchronize()
        rect.rectify_stereo(d_src, d_src2, n, bufs[0][pad + offset:], bufs[1][pad + offset:])
        rect.ctx.synchronize()
    for b in bufs:
        o = b.cpu().numpy()
        assert (o[:pad + offset] == FILL).all() and (o[pad + offset + n * h * w:] == FILL).all(), "canary overwritten"
        outs.append(o[pad + offset:pad + offset + n * h * w].reshape(n, h, w))
    return outs[0] if stereo_src is None else outs


def assert_same(got, want, what=""):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ---------------------------------------------------------------- known answers --
@pytest.mark.parametrize("w,h", [(67, 35), (64, 36)])
def test_identity_maps_return_the_input(ctx, w, h):
    r = gfpl.StereoRectifier(side_of(shift_side(w, h)), side_of(shift_side(w, h)), w, h, ctx)
    src = images(3, h, w)
    assert_same(run(r, 0, src), src, "identity")
    r.close()


@pytest.mark.parametrize("w,h", [(67, 35), (64, 36)])
@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("s", [-3, -1, 1, 3])
def test_integer_shift_with_zero_fill(ctx, w, h, axis, s):
    dx, dy = (s, 0) if axis == "x" else (0, s)
    r = gfpl.StereoRectifier(side_of(shift_side(w, h, dx, dy)), side_of(shift_side(w, h)), w, h, ctx)
    src = images(2, h, w)
    want = np.zeros_like(src)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    want[:, yd, xd] = src[:, ys, xs]
    assert_same(run(r, 0, src), want, f"shift {dx} {dy}")
    r.close()


@pytest.mark.parametrize("w,h", [(67, 35), (64, 36)])
def test_half_pixel_shift_averages_neighbours(ctx, w, h):
    r = gfpl.StereoRectifier(side_of(shift_side(w, h, dx=0.5)), side_of(shift_side(w, h, dy=0.5)), w, h, ctx)
    src = images(2, h, w).astype(np.int64)
    nx = np.concatenate([src[:, :, 1:], np.zeros((2, h, 1), np.int64)], axis=2)   # beyond the edge: 0
    ny = np.concatenate([src[:, 1:, :], np.zeros((2, 1, w), np.int64)], axis=1)
    assert_same(run(r, 0, images(2, h, w)), ((src + nx + 1) >> 1).astype(np.uint8), "half x")
    assert_same(run(r, 1, images(2, h, w)), ((src + ny + 1) >> 1).astype(np.uint8), "half y")
    r.close()


# ------------------------------------------------------------ against rectify_ref --
@pytest.fixture(scope="module")
def euroc_rect(ctx):
    l, w, h, _, _ = ref_maps("euroc_l")
    rr = ref_maps("euroc_r")[0]
    r = gfpl.StereoRectifier(side_of(l), side_of(rr), w, h, ctx)
    yield r
    r.close()


def test_uploaded_maps_are_the_host_builders(euroc_rect):
    for side, key in enumerate(("euroc_l", "euroc_r")):
        d, w, h, r1, r2 = ref_maps(key)
        m1, m2 = euroc_rect.maps(side)
        h1, h2 = gfpl.rectify_maps(side_of(d), w, h)
        assert (m1 == h1).all() and (m2 == h2).all()
        assert (m1 == r1).all() and (m2 == r2).all()


@pytest.mark.parametrize("n", [1, 3])
def test_euroc_both_sides_match_reference(euroc_rect, n):
    for side, key in enumerate(("euroc_l", "euroc_r")):
        _, w, h, m1, m2 = ref_maps(key)
        src = images(n, h, w)
        assert_same(run(euroc_rect, side, src), R.remap(src, m1, m2), key)


def test_stereo_call_equals_the_two_single_calls(euroc_rect):
    _, w, h, _, _ = ref_maps("euroc_l")
    sl, sr = images(3, h, w, 11), images(3, h, w, 12)
    both = run(euroc_rect, 0, sl, stereo_src=sr)
    assert_same(both[0], run(euroc_rect, 0, sl), "stereo left")
    assert_same(both[1], run(euroc_rect, 1, sr), "stereo right")
    assert_same(both[1], R.remap(sr, *ref_maps("euroc_r")[3:]), "stereo right vs reference")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_misaligned_output_base(euroc_rect, offset):
    _, w, h, m1, m2 = ref_maps("euroc_l")
    src = images(3, h, w)
    assert_same(run(euroc_rect, 0, src, offset=offset), R.remap(src, m1, m2), f"offset {offset}")
    sr = images(3, h, w, 12)
    both = run(euroc_rect, 0, src, offset=offset, stereo_src=sr)
    assert_same(both[1], R.remap(sr, *ref_maps("euroc_r")[3:]), f"stereo offset {offset}")


def test_equidistant_and_regions_outside_on_all_four_sides(ctx):
    e, w, h, e1, e2 = ref_maps("equi")
    f, _, _, f1, f2 = ref_maps("far")
    r = gfpl.StereoRectifier(side_of(e), side_of(f), w, h, ctx)
    src = images(3, h, w)
    assert_same(run(r, 0, src), R.remap(src, e1, e2), "equidistant")
    assert_same(run(r, 1, src), R.remap(src, f1, f2), "far")
    r.close()
    g, _, _, g1, g2 = ref_maps("far2")
    r = gfpl.StereoRectifier(side_of(f), side_of(g), w, h, ctx)
    assert_same(run(r, 1, src), R.remap(src, g1, g2), "far2")
    r.close()
    # a short rectified focal length: one map whose regions beyond all four edges lie outside
    r = gfpl.StereoRectifier(side_of(ref_maps("wide")[0]), side_of(f), w, h, ctx)
    w1, w2 = ref_maps("wide")[3:]
    assert_same(run(r, 0, src), R.remap(src, w1, w2), "wide")
    r.close()
    for v, hi in ((w1[..., 0], w), (w1[..., 1], h)):
        assert (v < -1).sum() > 1000 and (v > hi).sum() > 1000
    # the two shifted cameras between them leave whole regions outside beyond every edge
    sx = np.concatenate([f1[..., 0].reshape(-1), g1[..., 0].reshape(-1)])
    sy = np.concatenate([f1[..., 1].reshape(-1), g1[..., 1].reshape(-1)])
    assert (sx < -1).sum() > 1000 and (sx > w).sum() > 1000 and (sy < -1).sum() > 1000 and (sy > h).sum() > 1000


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("offset", [0, 1])
def test_odd_size_row_tail(ctx, n, offset):
    d, w, h, m1, m2 = ref_maps("small")
    assert w % 4 != 0 and (w * h) % 4 != 0
    r = gfpl.StereoRectifier(side_of(d), side_of(d), w, h, ctx)
    src = images(n, h, w)
    assert_same(run(r, 0, src, offset=offset), R.remap(src, m1, m2), "67 x 35")
    r.close()


def tiled(base, n):
    """n images cycling through the distinct ones of base (and their indices)"""
    idx = np.arange(n) % len(base)
    return base[idx], idx


def test_batch_slices_of_two_images(euroc_rect):
    # 19 images of 752 x 480 run as slices of two images each, the last slice holding one
    _, w, h, m1, m2 = ref_maps("euroc_l")
    base = images(3, h, w)
    src, idx = tiled(base, 19)
    assert_same(run(euroc_rect, 0, src), R.remap(base, m1, m2)[idx], "n = 19")


def test_batch_slices_of_eight_images(ctx):
    # enough small images for full slices of eight, and a count that is no multiple of eight
    d, w, h, m1, m2 = ref_maps("small")
    r = gfpl.StereoRectifier(side_of(d), side_of(d), w, h, ctx)
    base = images(7, h, w)
    src, idx = tiled(base, 5461)
    assert_same(run(r, 1, src), R.remap(base, m1, m2)[idx], "n = 5461")
    r.close()


def test_batch_beyond_the_grid_limit(ctx):
    # 2 x 262147 images of 8 x 8: more slices of eight than grid.y holds, so the slices grow
    w = h = 8
    d = dict(K=[9.0, 9.0, 3.6, 3.4], D=[-0.2, 0.05, 0.001, -0.002], R=R.IDENTITY, P=[8.0, 8.0, 3.2, 4.1])
    m1, m2 = R.maps(d["K"], d["D"], d["R"], d["P"], w, h)
    r = gfpl.StereoRectifier(side_of(d), side_of(d), w, h, ctx)
    base = images(5, h, w)
    n = 262147
    assert ((n + 7) // 8) * 2 > 65535
    src, idx = tiled(base, n)
    src2, idx2 = tiled(base[::-1], n)
    want = R.remap(base, m1, m2)
    both = run(r, 0, src, stereo_src=src2)
    assert_same(both[0], want[idx], "left")
    assert_same(both[1], want[::-1][idx2], "right")
    r.close()


def test_argument_errors(euroc_rect, ctx):
    import ctypes as C
    import torch
    L = gfpl.hiplib()
    _, w, h, _, _ = ref_maps("euroc_l")
    a = torch.zeros(w * h, dtype=torch.uint8, device="cuda:0")
    b = torch.zeros(w * h, dtype=torch.uint8, device="cuda:0")
    pa, pb, hr = a.data_ptr(), b.data_ptr(), euroc_rect.h
    assert L.gfpl_rectify(hr, 0, pa, 1, pa) == -1          # in place
    assert L.gfpl_rectify(hr, 2, pa, 1, pb) == -1 and L.gfpl_rectify(hr, -1, pa, 1, pb) == -1
    assert L.gfpl_rectify(hr, 0, pa, 0, pb) == -1
    assert L.gfpl_rectify(hr, 0, None, 1, pb) == -1 and L.gfpl_rectify(hr, 0, pa, 1, None) == -1
    assert L.gfpl_rectify(None, 0, pa, 1, pb) == -1 and L.gfpl_rectify_async(None, 0, pa, 1, pb) == -1
    assert L.gfpl_rectify_stereo_async(hr, pa, None, 1, pb, pb) == -1
    assert L.gfpl_rectify_stereo_async(hr, pa, pa, 1, pb, pb) == -1   # both sides into one output
    assert L.gfpl_rectifier_read_maps(hr, 2, pa, pb) == -1 and L.gfpl_rectifier_destroy(None) == -1
    s = side_of(ref_maps("euroc_l")[0])
    out = C.c_void_p()
    assert L.gfpl_rectifier_create(ctx.h, C.byref(s), C.byref(s), 7, 480, C.byref(out)) == -1
    assert L.gfpl_rectifier_create(ctx.h, C.byref(s), C.byref(s), 752, 8193, C.byref(out)) == -1
    assert L.gfpl_rectifier_create(ctx.h, C.byref(s), None, 752, 480, C.byref(out)) == -1
    assert L.gfpl_rectifier_create(None, C.byref(s), C.byref(s), 752, 480, C.byref(out)) == -1
    s.n_dist = 12
    assert L.gfpl_rectifier_create(ctx.h, C.byref(s), C.byref(s), 752, 480, C.byref(out)) == -7
