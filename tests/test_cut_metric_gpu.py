"""cut_with_max_vol = 0 on the device (k_cut_search_eig) against the CPU reference of that mode
(tests/cut_metric_ref.py), bit for bit.  tests/test_cut_metric_cpu.py pins the
reference and shows that these inputs separate the two metrics.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import gfpl
import cut_metric_cases as K
from parity import bitwise_equal, compare_core, compare_pose, compare_prev_matched, compare_track, diff_fields

pytestmark = pytest.mark.gpu

S = gfpl.StepSlot
CUT_SLOTS = [S.CUT_STEPS, S.CUT_EXACT, S.CUT_UNBOUNDED]


def test_min_eig_config_accepted():
    ctx = gfpl.Context(K.camera(), gfpl.default_config())
    ctx.set_config(gfpl.default_config(cut_with_max_vol=0))
    for over in (dict(best_lr_matches=0), dict(lr_in_parallel=0), dict(cut_with_max_vol=0, best_lr_matches=0)):
        with pytest.raises(gfpl.GfplError) as e:
            ctx.set_config(gfpl.default_config(**over))
        assert e.value.code == -7, over
    ctx.close()
    gfpl.Context(K.camera(), gfpl.default_config(cut_with_max_vol=0)).close()


def _canon(f: gfpl.FrameHost) -> gfpl.FrameHost:
    """NaNs to one bit pattern: the sign of a NaN an operation creates (0 * inf in the zero-covariance
    line's info) is the processor's choice, negative on x86 and positive on the GPU."""
    for a in f.arr.values():
        if a.dtype.kind == "f":
            a[np.isnan(a)] = np.nan
    return f


@functools.lru_cache(maxsize=None)
def _line_cut(name, n, rng=(0.0, 1.0), **over):
    """gfpl_line_cut on the first n states of K.states(name), written through gfpl_write_frame /
    gfpl_write_track: (PREV of every sequence, step records, track counts, proof counts)."""
    ctx = gfpl.Context(K.camera(), K.config(rng, cut_with_max_vol=0, **over))
    g = gfpl.StereoFrameHandler(ctx, n, K.KP, K.KL)
    for b, st in enumerate(K.states(name)[:n]):
        g.write_frame(gfpl.PREV, b, st.prev)
        g.write_frame(gfpl.CURR, b, st.curr)
        g.write_track(b, gfpl.track_from_dict(st.track))
    g.estimateProjUncertainty_submodular()
    out = ([_canon(g.read_frame(gfpl.PREV, b)) for b in range(n)], g.debug_step_records(), g.last_step_track_counts(),
           g.last_step_cut_proof())
    g.close()
    ctx.close()
    return out


def _check_line_cut(name, n, rng, got):
    frames, rec, counts, proof = got
    bad, steps = [], 0
    for b in range(n):
        st = K.states(name)[b]
        want, n_ref = K.reference(name, b, rng)
        want = _canon(want)
        bad += compare_prev_matched(frames[b], want, st.track, f"s{b} ")
        bad += diff_fields(frames[b], want, K.CUT_FIELDS, what=f"s{b} all rows ")
        if tuple(rec[b, CUT_SLOTS]) != (n_ref, n_ref, 0):
            bad.append(f"s{b} steps / exact steps / unbounded lines {rec[b, CUT_SLOTS]} vs {n_ref}")
        steps += n_ref
    assert not bad, "\n".join(bad[:30])
    assert counts["steps"] == steps and counts["exact_steps"] == steps and counts["lines_unbounded"] == 0, counts
    assert proof == {"redone": 0, "steps_proven": 0, "vref_evals": 0, "lines": 0}, proof


@pytest.mark.parametrize("name,n,rng", [("base", 1, (0.0, 1.0)), ("base", 8, (0.0, 1.0)), ("batch9", 9, (0.0, 1.0)),
                                        ("base", 17, (0.0, 1.0)), ("batch9", 9, K.WIDE)])
def test_line_cut_from_oracle_state(name, n, rng):
    """A lone group, a full wave, a wave plus one (with lists of 0, 1 and 2 lines, no matched points and a
    zero-covariance line in the first wave; again with the range (-0.5, 1.5)), two waves plus one."""
    _check_line_cut(name, n, rng, _line_cut(name, n, rng))


@pytest.mark.parametrize("proof,certify", [(1, 1e-9), (2, 1e-9), (0, 0.0)])
def test_proof_and_certify_modes_ignored(proof, certify):
    got = _line_cut("batch9", 9, cut_proof=proof, cut_certify=certify)
    _check_line_cut("batch9", 9, (0.0, 1.0), got)
    base = _line_cut("batch9", 9)
    for b in range(9):
        for f in K.CUT_FIELDS:
            assert bitwise_equal(got[0][b].arr[f], base[0][b].arr[f]), (b, f)
    assert (got[1][:, S.CUT_STEPS:S.CUT_UNBOUNDED + 1] == base[1][:, S.CUT_STEPS:S.CUT_UNBOUNDED + 1]).all()


def test_whole_steps():
    """frameStep over 3 frames, B = 3, against the oracle with the reference cut substituted: the new
    frame (features, pose, covariances, eigenvalues, err_norm), the track and the cut frame's line fields."""
    H = K.host_frames()
    D = gfpl.DeviceFrames(H)
    ctx = gfpl.Context(K.camera(), K.config(cut_with_max_vol=0))
    g = gfpl.StereoFrameHandler(ctx, K.STEP_B, K.KP, K.KL)
    g.initialize(D.frames_slice(0, 0, K.STEP_B))
    bad = []
    for k in range(1, 1 + K.STEP_F):
        g.frameStep(D.frames_slice(k, 0, K.STEP_B))
        rec = g.debug_step_records()
        for b in range(K.STEP_B):
            want = K.step_reference(b)["steps"][k - 1]
            tag = f"f{k} s{b} "
            new = g.read_frame(gfpl.PREV, b)
            bad += compare_core(new, want["new"], tag)
            pb, exact = compare_pose(new, want["new"], what=tag)
            bad += pb + ([] if exact else [tag + "pose not bit-exact"])
            bad += compare_track(g.read_last_track(b), want["track"], tag)
            # (the frame the step cut is in the other slot until the next insert)
            bad += compare_prev_matched(g.read_frame(gfpl.CURR, b), want["old"], want["track"], tag + "cut frame ")
            if rec[b, S.CUT_STEPS] != want["n"] or rec[b, S.CUT_EXACT] != want["n"]:
                bad.append(f"{tag}steps {rec[b, [S.CUT_STEPS, S.CUT_EXACT]]} vs {want['n']}")
            assert len(want["track"]["matched_ls"]) > 10 and want["track"]["n_inliers_ls"] > 5
    g.close()
    ctx.close()
    assert not bad, "\n".join(bad[:30])


def test_host_mirror_runs_min_eig_cut():
    """Config::cutWithMaxVol() = false through the C++ mirror (plslam_gpu --min-eig-cut): the poses of the
    Python handler with cut_with_max_vol = 0 on the same frames, and not the default config's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, seq, KP, KL = 4, 3, 2048, 512
    r = subprocess.run([os.path.join(root, "gf-pl-slam_amd", "bin", "plslam_gpu"), "--frames", str(n), "--seq", str(seq),
                        "--json", "--min-eig-cut"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == n - 1
    cam = K.camera()
    H = gfpl.HostFrames(cam, gfpl.synth_params(), 1, n, KP, KL, seq0=seq)
    D = gfpl.DeviceFrames(H)
    poses = {}
    for flag in (0, 1):
        ctx = gfpl.Context(cam, gfpl.default_config(cut_with_max_vol=flag))
        g = gfpl.StereoFrameHandler(ctx, 1, KP, KL)
        g.initialize(D.frames(0))
        poses[flag] = []
        for k in range(1, n):
            g.insertStereoPair(D.frames(k))
            g.optimizePose()
            if g.needNewKF()[0]:   # the app's keyframe step, as the driver takes it
                g.currFrameIsKF()
            c = g.read_frame(gfpl.CURR, 0)
            poses[flag].append((c.get("Tfw").reshape(-1).tolist(), c.get("DT").reshape(-1).tolist(), float(c.s.err_norm)))
            g.updateFrame()
        g.close()
        ctx.close()
    assert [(x["Tfw"], x["DT"], x["err_norm"]) for x in lines] == poses[0]
    assert poses[0] != poses[1]
