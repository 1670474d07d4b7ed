"""Raw images in, poses out: ImagePipeline(rectifier=r) and gfpl_detector_set_rectifier on raw
images against the same pipeline / detector, without a rectifier, on images rectified on the
host by rectify_ref (the numpy restatement of ledger R1-R6) — identical detections and poses.
The smallest batch and camera tests/test_pipeline_gpu.py uses: B = 2, initialize + two steps."""
import ctypes as C

import numpy as np
import pytest

import gfpl
import rectify_ref as R
from gfpl.pipeline import ImagePipeline, synth_stereo_scene
from parity import compare_core

pytestmark = pytest.mark.gpu

B, F, KL = 2, 3, 320
NFEAT, KP = 2000, 2320


def rig(w, h):
    """a EuRoC-like rig for w x h images: mild barrel distortion, slightly rotated cameras"""
    _, _, l, r = R.euroc()
    left = dict(K=[458.654, 457.296, w / 2 + 3.2, h / 2 - 4.6], D=l["D"], R=l["R"], P=[435.2, 435.2, w / 2 + 0.45, h / 2 + 0.2])
    right = dict(K=[457.587, 456.134, w / 2 - 5.1, h / 2 + 2.3], D=r["D"], R=r["R"], P=left["P"])
    return left, right


def side_of(d):
    return gfpl.RectifySide.make(d["K"], d["D"], d["R"], d["P"])


@pytest.fixture(scope="module")
def setup():
    import torch
    cfg = gfpl.default_config()
    cam = gfpl.make_camera("vga", cfg)
    W, H = int(cam.width), int(cam.height)
    left, right = rig(W, H)
    ml = R.maps(left["K"], left["D"], left["R"], left["P"], W, H)
    mr = R.maps(right["K"], right["D"], right["R"], right["P"], W, H)
    dev = torch.device("cuda", 0)
    frames = []
    for k in range(F):
        sc = [synth_stereo_scene(b, k, W, H) for b in range(B)]
        raw_l, raw_r = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
        kl = [np.zeros((B, KL), gfpl.KEYLINE_DT) for _ in range(2)]
        n = [np.zeros(B, np.int32) for _ in range(2)]
        for b, s in enumerate(sc):
            for side in range(2):
                n[side][b] = len(s[2 + side])
                kl[side][b, :n[side][b]] = s[2 + side]
        frames.append(dict(raw=(raw_l, raw_r), rect=(R.remap(raw_l, *ml), R.remap(raw_r, *mr)), kl=kl, n=n, ts=0.05 * k))
    assert (frames[0]["raw"][0] != frames[0]["rect"][0]).mean() > 0.5   # the rectification does something
    ctx = gfpl.Context(cam, cfg)
    rect = gfpl.StereoRectifier(side_of(left), side_of(right), W, H, ctx)
    yield dict(cfg=cfg, cam=cam, W=W, H=H, frames=frames, ctx=ctx, rect=rect, dev=dev)
    rect.close()
    ctx.close()


def read_detections(ctx, fr, seq):
    out = {"kp_l": np.zeros(fr.kp_cap, gfpl.KEYPOINT_DT), "kp_r": np.zeros(fr.kp_cap, gfpl.KEYPOINT_DT),
           "pdesc_l": np.zeros((fr.kp_cap, 32), np.uint8), "pdesc_r": np.zeros((fr.kp_cap, 32), np.uint8),
           "kl_l": np.zeros(fr.kl_cap, gfpl.KEYLINE_DT), "kl_r": np.zeros(fr.kl_cap, gfpl.KEYLINE_DT),
           "ldesc_l": np.zeros((fr.kl_cap, 32), np.uint8), "ldesc_r": np.zeros((fr.kl_cap, 32), np.uint8)}
    d = gfpl.DetectionsHost()
    for k, a in out.items():
        setattr(d, k, a.ctypes.data)
    gfpl.check(ctx.L.gfpl_read_detections(ctx.h, C.byref(fr), seq, C.byref(d)), "read_detections")
    cnt = {"kp": (d.n_kp_l, d.n_kp_r), "pdesc": (d.n_kp_l, d.n_kp_r), "kl": (d.n_kl_l, d.n_kl_r), "ldesc": (d.n_kl_l, d.n_kl_r)}
    res = {k: a[:cnt[k.split("_")[0]][0 if k.endswith("_l") else 1]].copy() for k, a in out.items()}
    res["counts"] = np.array([d.n_kp_l, d.n_kp_r, d.n_kl_l, d.n_kl_r])
    return res


def assert_same_detections(ctx, fr_a, fr_b, what):
    for b in range(B):
        da, db = read_detections(ctx, fr_a, b), read_detections(ctx, fr_b, b)
        assert (da["counts"] == db["counts"]).all(), (what, b, da["counts"], db["counts"])
        assert da["counts"][0] > 50 and da["counts"][2] > 5, (what, b, da["counts"])
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), (what, b, k)


def assert_same_state(ga, gb, what):
    for b in range(B):
        fa, fb = ga.read_frame(gfpl.PREV, b), gb.read_frame(gfpl.PREV, b)
        assert not compare_core(fa, fb, f"{what} s{b} ")
        for name in ("Tfw", "DT", "DT_cov"):
            assert fa.get(name).tobytes() == fb.get(name).tobytes(), (what, b, name)
        assert fa.n_pt == fb.n_pt and fa.n_ls == fb.n_ls, (what, b)
        ta, tb = ga.read_last_track(b), gb.read_last_track(b)
        assert (np.asarray(ta["matched_pt"]) == np.asarray(tb["matched_pt"])).all(), (what, b)
        assert (np.asarray(ta["matched_ls"]) == np.asarray(tb["matched_ls"])).all(), (what, b)


@pytest.mark.parametrize("lsd", [False, True])
def test_pipeline_on_raw_images_equals_pipeline_on_rectified(setup, lsd):
    import torch
    s, dev, ctx = setup, setup["dev"], setup["ctx"]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pr = ImagePipeline(ctx, s["cam"], B, KL, lsd=lsd, rectifier=s["rect"])
    pp = ImagePipeline(ctx, s["cam"], B, KL, lsd=lsd)
    gr = gfpl.StereoFrameHandler(ctx, B, pr.kp_cap, KL)
    gp = gfpl.StereoFrameHandler(ctx, B, pp.kp_cap, KL)
    for k, f in enumerate(s["frames"]):
        ts = torch.full((B,), f["ts"], dtype=torch.float64, device=dev)
        views = []
        for pipe, (il, ir) in ((pr, f["raw"]), (pp, f["rect"])):
            if lsd:
                views.append(pipe.detect_images(to(il), to(ir), ts))
            else:
                kls = [to(a.view(np.uint8).reshape(-1)) for a in f["kl"]]
                views.append(pipe.detect(to(il), to(ir), kls[0], to(f["n"][0]), kls[1], to(f["n"][1]), ts))
            pipe.status()
            pipe.synchronize()
        assert_same_detections(ctx, views[0], views[1], f"frame {k}")
        # the right pyramid the tracker's sub-pixel refinement reads
        assert torch.equal(views[0]._keep[12], views[1]._keep[12]), k
        for g, v in ((gr, views[0]), (gp, views[1])):
            if k == 0:
                g.initialize(v)
            else:
                g.frameStep(v)
        if k:
            assert_same_state(gr, gp, f"frame {k}")
    gr.close(); gp.close()
    pr.close(); pp.close()


def test_pipeline_outstanding_view_still_raises(setup):
    import torch
    s, dev, ctx = setup, setup["dev"], setup["ctx"]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pipe = ImagePipeline(ctx, s["cam"], B, KL, lsd=True, rectifier=s["rect"], sets=1)
    f = s["frames"][0]
    ts = torch.full((B,), 0.0, dtype=torch.float64, device=dev)
    fr = pipe.detect_images(to(f["raw"][0]), to(f["raw"][1]), ts)
    with pytest.raises(RuntimeError):
        pipe.detect_images(to(f["raw"][0]), to(f["raw"][1]), ts)   # no tracker call read the set's view
    pipe.discard(fr)
    pipe.detect_images(to(f["raw"][0]), to(f["raw"][1]), ts)
    pipe.status()
    pipe.close()


def test_pipeline_rejects_a_rectifier_of_another_size(setup):
    ctx = setup["ctx"]
    l, r = rig(320, 240)
    small = gfpl.StereoRectifier(side_of(l), side_of(r), 320, 240, ctx)
    with pytest.raises(ValueError):
        ImagePipeline(ctx, setup["cam"], B, KL, rectifier=small)
    small.close()


@pytest.mark.parametrize("host", [False, True])
def test_c_detector_with_rectifier_attached(setup, host):
    import torch
    s, dev, ctx = setup, setup["dev"], setup["ctx"]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    prm = gfpl.DetectorParams.reference(s["cam"], s["cfg"], nfeatures=NFEAT)
    dr = gfpl.StereoDetector(ctx, B, KP, KL, prm)
    dp = gfpl.StereoDetector(ctx, B, KP, KL, prm)
    dr.set_rectifier(s["rect"])
    gr = gfpl.StereoFrameHandler(ctx, B, KP, KL)
    gp = gfpl.StereoFrameHandler(ctx, B, KP, KL)
    for k, f in enumerate(s["frames"]):
        tsh = np.full(B, f["ts"])
        views = []
        for det, (il, ir) in ((dr, f["raw"]), (dp, f["rect"])):
            if host:
                views.append(det.detect_host(il, ir, tsh))
            else:
                views.append(det.detect(to(il), to(ir), to(tsh)))
            det.status()
        assert_same_detections(ctx, views[0], views[1], f"frame {k}")
        for g, v in ((gr, views[0]), (gp, views[1])):
            if k == 0:
                g.initialize(v)
            else:
                g.frameStep(v)
        if k:
            assert_same_state(gr, gp, f"frame {k}")
    # detached: the same detector copies its inputs again
    dr.set_rectifier(None)
    f = s["frames"][0]
    va = dr.detect(to(f["rect"][0]), to(f["rect"][1]), to(np.zeros(B)))
    vb = dp.detect(to(f["rect"][0]), to(f["rect"][1]), to(np.zeros(B)))
    dr.status(); dp.status()
    assert_same_detections(ctx, va, vb, "detached")
    dr.discard(va); dp.discard(vb)
    gr.close(); gp.close()
    dr.close(); dp.close()


def test_c_detector_rectifier_size_and_outstanding_view(setup):
    import torch
    s, dev, ctx = setup, setup["dev"], setup["ctx"]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    l, r = rig(320, 240)
    small = gfpl.StereoRectifier(side_of(l), side_of(r), 320, 240, ctx)
    det = gfpl.StereoDetector(ctx, B, KP, KL, gfpl.DetectorParams.reference(s["cam"], s["cfg"], nfeatures=NFEAT), sets=1)
    with pytest.raises(gfpl.GfplError) as e:
        det.set_rectifier(small)
    assert e.value.code == -1
    assert ctx.L.gfpl_detector_set_rectifier(None, s["rect"].h) == -1
    small.close()
    det.set_rectifier(s["rect"])
    f = s["frames"][0]
    args = (to(f["raw"][0]), to(f["raw"][1]), to(np.zeros(B)))
    fr = det.detect(*args)
    with pytest.raises(gfpl.GfplError) as e:
        det.detect(*args)
    assert e.value.code == -6
    det.discard(fr)
    det.status()
    det.close()
