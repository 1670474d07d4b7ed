#!/usr/bin/env python3
"""Stereo rectification on one MI355X (k_rectify).  Two measurements, one JSON line:

kernel:   gfpl_rectify_stereo_async on 2 x --images raw 752 x 480 images resident in HBM (the
          EuRoC rig of tests/golden/euroc_rectify.json), HIP events on one stream around
          --reps launches after --warmup launches.  images/s, and GB/s over the algorithmic
          bytes 2 W H n (every image read and written once) plus the two 8-byte-per-pixel map
          tables once, as a fraction of the HBM peak bench.py uses for its rooflines.
pipeline: images -> poses frames/s of ImagePipeline(rectifier=r) on raw images against the
          same ImagePipeline without a rectifier on the same images rectified beforehand
          (the pipeline as it was before rectification existed), same B, camera and inputs,
          --repeats alternating runs of each, for lsd=True (the remap replaces the input
          copy) and lsd=False (the remap is extra work).  The ratio is to be read against
          the spread of the baseline's own repeats.

One image per side of the kernel leg is checked bit-exact against tests/rectify_ref.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gf-pl-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0   # as bench.py


def side_of(gfpl, d):
    return gfpl.RectifySide.make(d["K"], d["D"], d["R"], d["P"], d.get("equi", False))


def kernel_leg(a, torch, gfpl, R):
    W, H, left, right = R.euroc()
    n = a.images
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    cfg = gfpl.default_config()
    ctx = gfpl.Context(gfpl.make_camera("vga", cfg), cfg, stream=st.cuda_stream)
    rect = gfpl.StereoRectifier(side_of(gfpl, left), side_of(gfpl, right), W, H, ctx)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    src = [torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
    dst = [torch.empty((n, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        rect.rectify_stereo(src[0], src[1], n, dst[0], dst[1])
    ctx.synchronize()
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.reps):
            rect.rectify_stereo(src[0], src[1], n, dst[0], dst[1])
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.reps)
    ok = True
    for side, d in enumerate((left, right)):
        m1, m2 = R.maps(d["K"], d["D"], d["R"], d["P"], W, H)
        k = n - 1
        ok = ok and bool((dst[side][k].cpu().numpy() == R.remap(src[side][k].cpu().numpy(), m1, m2)).all())
    t = float(np.median(ms)) * 1e-3
    nbytes = 2 * W * H * (2 * n) + 2 * 8 * W * H
    rect.close()
    ctx.close()
    return {"width": W, "height": H, "images": 2 * n, "ms_per_launch": [round(x, 4) for x in ms],
            "images_per_s": 2 * n / t, "algorithmic_bytes": nbytes, "gb_per_s": nbytes / t / 1e9,
            "hbm_peak_gb_per_s": HBM_PEAK_GBS, "hbm_frac": nbytes / t / 1e9 / HBM_PEAK_GBS, "bit_exact_vs_ref": ok}


def pipeline_leg(a, torch, gfpl, R, lsd):
    from gfpl.pipeline import ImagePipeline, synth_stereo_steps
    cfg = gfpl.default_config(max_iters=10, max_iters_ref=10, min_error=0.0, min_error_change=0.0)
    cam = gfpl.make_camera("vga", cfg)
    W, H, B, KL = int(cam.width), int(cam.height), a.batch, 320
    F = a.warmup + a.steps + 1
    dev = torch.device("cuda", 0)
    _, _, l, r = R.euroc()
    left = dict(K=[458.654, 457.296, W / 2 + 3.2, H / 2 - 4.6], D=l["D"], R=l["R"], P=[435.2, 435.2, W / 2 + 0.45, H / 2 + 0.2])
    right = dict(K=[457.587, 456.134, W / 2 - 5.1, H / 2 + 2.3], D=r["D"], R=r["R"], P=left["P"])
    ctx = gfpl.Context(cam, cfg)
    rect = gfpl.StereoRectifier(side_of(gfpl, left), side_of(gfpl, right), W, H, ctx)
    distinct = min(B, 16)   # the scenes of 16 sequences, repeated over the batch
    idx = np.arange(B) % distinct
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    raw, pre = [], []
    for k in range(F):
        sc = [synth_stereo_steps(b, k, W, H) for b in range(distinct)]
        kl = [np.zeros((distinct, KL), gfpl.KEYLINE_DT) for _ in range(2)]
        n = [np.zeros(distinct, np.int32) for _ in range(2)]
        for b, s in enumerate(sc):
            for side in range(2):
                n[side][b] = len(s[2 + side])
                kl[side][b, :n[side][b]] = s[2 + side]
        il, ir = to(np.stack([s[0] for s in sc])[idx]), to(np.stack([s[1] for s in sc])[idx])
        rl, rr = torch.empty_like(il), torch.empty_like(ir)
        torch.cuda.synchronize()
        rect.rectify_stereo(il, ir, B, rl, rr)
        ctx.synchronize()
        rest = (to(kl[0][idx].view(np.uint8).reshape(-1)), to(n[0][idx]), to(kl[1][idx].view(np.uint8).reshape(-1)),
                to(n[1][idx]), torch.full((B,), 0.05 * k, dtype=torch.float64, device=dev))
        raw.append((il, ir) + rest)
        pre.append((rl, rr) + rest)
    legs = {"rectifier": (ImagePipeline(ctx, cam, B, KL, lsd=lsd, rectifier=rect), raw),
            "baseline": (ImagePipeline(ctx, cam, B, KL, lsd=lsd), pre)}
    fps = {k: [] for k in legs}
    poses = {}
    for rep in range(a.repeats):
        for name, (pipe, frames) in legs.items():   # alternating
            g = gfpl.StereoFrameHandler(ctx, B, pipe.kp_cap, KL)
            det = (lambda f: pipe.detect_images(f[0], f[1], f[6])) if lsd else (lambda f: pipe.detect(*f))
            g.initialize(det(frames[0]))
            for k in range(1, a.warmup + 1):
                g.frameStep(det(frames[k]))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.warmup + 1, F):
                g.frameStep(det(frames[k]))
            pipe.synchronize()
            ctx.synchronize()
            torch.cuda.synchronize()
            fps[name].append(B * a.steps / (time.perf_counter() - t0))
            pipe.status()
            poses[name] = g.read_frame(gfpl.PREV, 0).get("Tfw").tobytes()
            g.close()
    for pipe, _ in legs.values():
        pipe.close()
    rect.close()
    ctx.close()
    med = {k: float(np.median(v)) for k, v in fps.items()}
    base = fps["baseline"]
    return {"lsd": lsd, "batch": B, "steps": a.steps, "frames_per_s": {k: [round(x, 1) for x in v] for k, v in fps.items()},
            "median_frames_per_s": med, "ratio_rectifier_over_baseline": med["rectifier"] / med["baseline"],
            "baseline_spread": (max(base) - min(base)) / med["baseline"], "same_pose_seq0": poses["rectifier"] == poses["baseline"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024, help="stereo frames of the kernel leg (2x images)")
    ap.add_argument("--reps", type=int, default=10, help="launches per timed window (kernel leg)")
    ap.add_argument("--batch", type=int, default=256, help="sequences of the pipeline legs")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rectify: no GPU (nothing is measured without one)")
    import gfpl
    import rectify_ref as R
    res = {"bench": "rectify", "device": torch.cuda.get_device_name(0), "kernel": kernel_leg(a, torch, gfpl, R)}
    if not a.skip_pipeline:
        res["pipeline"] = [pipeline_leg(a, torch, gfpl, R, lsd) for lsd in (True, False)]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
