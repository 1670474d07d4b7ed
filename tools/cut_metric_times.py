#!/usr/bin/env python3
"""Line-cut stage times of the two cut metrics ("min-eigenvalue cut").

cfg2 (synthetic VGA, 2000 ORB + 500 LBD per side, 10 + 10 GN iterations) at batch B on one GPU, the
same frames for every configuration in one process:
  logdet_exact   cut_with_max_vol = 1, cut_certify = 0: every step of the logdet search evaluated with
                 the reference's two LLTs (k_cut_search, all steps on its exact path)
  min_eig        cut_with_max_vol = 0: k_cut_search_eig, one Jacobi per evaluation
  logdet         the default (margined search), for scale
Times are gfpl_get_kernel_times (HIP events around k_cut_prep / the search / k_cut_finish) of each
step after the first; for min_eig also the search's counters: steps, metric evaluations and Jacobi
sweeps that rotated (gfpl_debug_clocks slots 1 / 0: DbgCutEig in csrc/gfpl_records.hpp).  U unique sequences are
generated and tiled to B.

usage: python3 tools/cut_metric_times.py [--batch 16384] [--unique 1024] [--frames 4]
prints one JSON line per configuration.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gf-pl-slam_amd"))
import gfpl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--unique", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=4)
    a = ap.parse_args()
    B, U, F, KP, KL = a.batch, min(a.unique, a.batch), a.frames, 2048, 512
    assert B % U == 0
    base = dict(max_iters=10, max_iters_ref=10, min_error=0.0, min_error_change=0.0)
    cam = gfpl.make_camera("vga", gfpl.default_config(**base))
    D = gfpl.DeviceFrames.generate(cam, gfpl.synth_params(respawn=16), U, F + 1, KP, KL, threads=16)
    if B > U:   # tile the unique sequences over the batch
        D.bufs = [b.view(F + 1, U, -1).repeat(1, B // U, 1).reshape(F + 1, -1) for b in D.bufs]
        D.B = B
    for name, over in (("logdet_exact", dict(cut_certify=0.0)), ("min_eig", dict(cut_with_max_vol=0)), ("logdet", {})):
        ctx = gfpl.Context(cam, gfpl.default_config(**base, **over))
        ctx.set_timing(True)
        h = gfpl.StereoFrameHandler(ctx, B, KP, KL)
        h.initialize(D.frames(0))
        rows = []
        for k in range(1, F + 1):
            h.frameStep(D.frames(k))
            ctx.synchronize()
            kt = ctx.kernel_times()
            tc = h.last_step_track_counts()
            row = dict(frame=k, k_cut_prep_ms=float(kt[0]), search_ms=float(kt[1]), k_cut_finish_ms=float(kt[2]),
                       line_cut_ms=float(kt[0] + kt[1] + kt[2]), steps=tc["steps"], exact_steps=tc["exact_steps"],
                       matched_lines=h.last_step_counts()["M_l"])
            if name == "min_eig":
                c = h.debug_clocks()
                row.update(evaluations=int(c[:, 1].sum()), jacobi_sweeps=int(c[:, 0].sum()),
                           sweeps_per_evaluation=float(c[:, 0].sum() / max(1, c[:, 1].sum())))
            rows.append(row)
        timed = rows[1:] or rows
        print(json.dumps(dict(config=name, batch=B, unique=U,
                              search_ms_median=float(np.median([r["search_ms"] for r in timed])),
                              line_cut_ms_median=float(np.median([r["line_cut_ms"] for r in timed])), steps=rows)),
              flush=True)
        h.close()
        ctx.close()


if __name__ == "__main__":
    main()
