"""The step record (gfpl_debug_step_records, gfpl.StepSlot) against its readers: every
gfpl_last_step_* call is a column sum of the records at the named slots, in every line-cut mode.

B = 9: one full group of eight for the packed search (k_cut_search) and a ninth sequence alone in
its wave; sequence 8 has no keylines, so its line cut and its search slots see an empty list.
"""
import functools

import numpy as np
import pytest

import gfpl

pytestmark = pytest.mark.gpu

S = gfpl.StepSlot
B, KP, KL, F = 9, 256, 64, 3

# config overrides, GFPL_CUT_WAVE_MAX_B (None: unset)
SETTINGS = {
    "measured_packed": (dict(), "0"),       # k_cut_search<false>: 8 sequences per wave
    "measured_wave": (dict(), None),        # k_cut_search_w: one sequence per wave
    "proven": (dict(cut_proof=1), None),
    "min_eig": (dict(cut_with_max_vol=0), None),
    "no_cut": (dict(use_line_conf_cut=0), None),
}


@functools.lru_cache(maxsize=None)
def _input():
    cfg = gfpl.default_config()
    cam = gfpl.make_camera("vga", cfg)
    sp = gfpl.synth_params(n_kp=200, n_kl=50, n_world_pts=280, n_world_lines=70, seed=11)
    H = gfpl.HostFrames(cam, sp, B, F, KP, KL, threads=4)
    H.n_kl_l[:, 8] = 0
    H.n_kl_r[:, 8] = 0
    return cam, H


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_readers_are_column_sums_of_the_named_slots(monkeypatch, setting):
    over, wave_max_b = SETTINGS[setting]
    if wave_max_b is None:
        monkeypatch.delenv("GFPL_CUT_WAVE_MAX_B", raising=False)
    else:
        monkeypatch.setenv("GFPL_CUT_WAVE_MAX_B", wave_max_b)
    cam, H = _input()
    cfg = gfpl.default_config(**over)
    D = gfpl.DeviceFrames(H)
    ctx = gfpl.Context(cam, cfg)
    h = gfpl.StereoFrameHandler(ctx, B, KP, KL)
    h.initialize(D.frames(0))
    cut = bool(cfg.use_line_conf_cut)
    lines_cut = 0
    for k in range(1, F):
        h.frameStep(D.frames(k))
        rec = h.debug_step_records()
        assert rec.shape == (B, gfpl.STEP_REC)
        col = rec.sum(axis=0)
        tag = f"{setting} step {k}: "

        stage = h.last_step_stage_bytes()
        print(tag, "records", rec.tolist(), "stage bytes", stage.tolist())
        assert stage.tolist() == col[S.B_STEREO_POINTS:S.B_TOTAL + 1].tolist(), tag
        assert col[S.B_TOTAL] == col[S.B_STEREO_POINTS:S.B_POSE + 1].sum(), tag
        assert h.last_step_bytes() == col[S.B_TOTAL], tag

        counts = h.last_step_counts()
        want = {n: float(col[S.N_O + i]) / B for i, n in enumerate(h.STEP_COUNTS)}
        assert [S(S.N_O + i).name for i in range(8)] == [n.upper() for n in h.STEP_COUNTS]
        assert counts == want, tag

        track = h.last_step_track_counts()
        assert track == {"steps": col[S.CUT_STEPS], "exact_steps": col[S.CUT_EXACT],
                         "inliers_after_pose": col[S.INLIERS_POSE], "lines_unbounded": col[S.CUT_UNBOUNDED]}, tag

        proof = h.last_step_cut_proof()
        slots = [S.PROOF_REDONE, S.PROOF_STEPS, S.PROOF_VREF, S.PROOF_LINES]
        if cfg.cut_proof == 1 and cut and cfg.cut_with_max_vol:
            assert list(proof.values()) == col[slots].tolist(), tag
        else:
            assert not any(proof.values()), tag
            assert not col[slots].any(), tag

        #  k_cut_prep, k_cut_search, k_cut_finish, k_pose from this step's own counts
        M_l, M_p = int(col[S.M_L]), int(col[S.M_P])
        kb = h.last_step_kernel_bytes().tolist()
        print(tag, "kernel bytes", kb, "M_l", M_l, "M_p", M_p)
        assert kb == [212 * M_l + 44 * M_p + 552 * B if cut else 0, int(col[S.B_CUT_SEARCH]),
                      612 * M_l if cut else 0, int(col[S.B_POSE])], tag
        assert (rec[:, S.B_CUT_SEARCH] == np.where(cut & (rec[:, S.M_L] > 0), 396 * rec[:, S.M_L] + 272, 0)).all(), tag

        # sequence 8 has no lines to match, cut or search
        assert rec[8, S.N_K] == 0 and rec[8, S.S_L] == 0 and rec[8, S.M_L] == 0, tag
        assert not rec[8, [S.CUT_STEPS, S.CUT_EXACT, S.CUT_UNBOUNDED]].any(), tag
        if not cut:
            assert not col[[S.CUT_STEPS, S.CUT_EXACT, S.CUT_UNBOUNDED]].any(), tag
        elif not cfg.cut_with_max_vol:
            assert col[S.CUT_EXACT] == col[S.CUT_STEPS], tag
        lines_cut += M_l if cut else 0
    h.close()
    ctx.close()
    assert lines_cut > 0 or not cut   # the cut modes had lines to search
