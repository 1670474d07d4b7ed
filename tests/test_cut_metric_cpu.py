"""The CPU reference of the line cut with the metric as a parameter (tests/cut_metric_ref.py).

* With metric = logdet it is gfplo_line_cut bit for bit, which pins the restatement.
* Substituted into the oracle (stages up to crossFrameMatchingLines, the Python cut written into
  PREV, optimizePose, updateFrame) it reproduces the oracle's own steps bit for bit, which gives a
  whole-step reference for cut_with_max_vol = 0 without touching oracle/.
* On the inputs of tests/test_cut_metric_gpu.py the two metrics end at different ratios, so those
  tests cannot pass on a search that still maximises logdet.
* One hand-checked case where the metrics disagree by construction.
"""
import numpy as np
import pytest

import gfpl
import oracle as O
import cut_metric_cases as K
from cut_metric_ref import CutRef, logdet, min_eig, oracle_to_cross, substituted_insert
from parity import POSE, bitwise_equal, compare_track

KP, KL = 512, 128
PIN_SYNTH = dict(n_kp=300, n_kl=60, n_world_pts=390, n_world_lines=78, seed=13)


@pytest.fixture(scope="module")
def pin_frames():
    cam = K.camera()
    return cam, gfpl.HostFrames(cam, gfpl.synth_params(**PIN_SYNTH), 2, 3, KP, KL)


@pytest.mark.parametrize("case", ["default", "wide_range", "no_points"])
def test_logdet_restatement_is_the_oracle_cut(pin_frames, case):
    """Two sequences x two frames: ratios, invCovPose and the cut endpoints against gfplo_line_cut."""
    cam, H = pin_frames
    cfg = K.config(K.WIDE if case == "wide_range" else (0.0, 1.0))
    ref = CutRef(cam, cfg, logdet)
    moved = lines = 0
    for b in range(2):
        o = O.OracleHandler(cam, cfg, KP, KL)
        o.initialize(H.frames(0), b)
        for k in (1, 2):
            oracle_to_cross(o, H.frames(k), b)
            tr = o.read_track()
            if case == "no_points":
                tr["matched_pt"] = tr["matched_pt"][:0]
                tr["n_inliers_pt"] = 0
                tr["n_inliers"] = tr["n_inliers_ls"]
                o.write_track(gfpl.track_from_dict(tr))
            prev, curr = o.read_frame(gfpl.PREV), o.read_frame(gfpl.CURR)
            ref.line_cut(prev, curr, tr)
            o.estimateProjUncertainty_submodular()
            want = o.read_frame(gfpl.PREV)
            for f in K.CUT_FIELDS:
                assert bitwise_equal(prev.arr[f], want.arr[f]), (case, b, k, f)
            r = K.ratios(want, tr)
            lines += len(r)
            moved += int((r != 0).any(axis=1).sum())
            o.optimizePose()
            o.updateFrame()
    assert lines >= 4 * 40 and moved > lines // 2, (lines, moved)


def _compare_step(a: O.OracleHandler, s: O.OracleHandler, what: str):
    bad = []
    ca, cs = a.read_frame(gfpl.CURR), s.read_frame(gfpl.CURR)
    for n in POSE:
        if not bitwise_equal(ca.get(n), cs.get(n)):
            bad.append(f"{what}{n}")
    if ca.s.err_norm != cs.s.err_norm:
        bad.append(f"{what}err_norm")
    ta, ts = a.read_track(), s.read_track()
    bad += compare_track(ts, ta, what)
    pa, ps = a.read_frame(gfpl.PREV), s.read_frame(gfpl.PREV)
    for f in K.CUT_FIELDS + ["ls_inlier", "pt_inlier"]:
        if not bitwise_equal(pa.arr[f], ps.arr[f]):
            bad.append(f"{what}{f}")
    return bad


def test_substituted_oracle_reproduces_the_oracle_steps(pin_frames):
    """Three frames: the oracle with the Python logdet cut written into PREV against the oracle itself."""
    cam, _ = pin_frames
    H = gfpl.HostFrames(cam, gfpl.synth_params(**PIN_SYNTH), 1, 4, KP, KL)
    cfg = gfpl.default_config()
    ref = CutRef(cam, cfg, logdet)
    a, s = O.OracleHandler(cam, cfg, KP, KL), O.OracleHandler(cam, cfg, KP, KL)
    a.initialize(H.frames(0), 0)
    s.initialize(H.frames(0), 0)
    bad = []
    for k in (1, 2, 3):
        a.insertStereoPair(H.frames(k), 0)
        assert substituted_insert(s, H.frames(k), 0, ref) > 0
        a.optimizePose()
        s.optimizePose()
        bad += _compare_step(a, s, f"f{k} ")
        assert a.read_track()["n_inliers_ls"] > 20
        a.updateFrame()
        s.updateFrame()
    assert not bad, bad


def _differ(name, idx, rng):
    st = K.states(name)[idx]
    a = K.ratios(K.reference(name, idx, rng, "logdet")[0], st.track)
    e = K.ratios(K.reference(name, idx, rng, "min_eig")[0], st.track)
    return len(a), int((a != e).any(axis=1).sum())


@pytest.mark.parametrize("name,n,rng", [("base", K.N_SEQ, (0.0, 1.0)), ("batch9", 9, (0.0, 1.0)), ("batch9", 9, K.WIDE)])
def test_gpu_stage_inputs_separate_the_metrics(name, n, rng):
    """Every sequence with lines ends at least one line at other ratios under min-eig than under logdet.
    The zero-covariance sequence is the one exception: its invCov_sum is not finite from the first sum
    on, no metric is ever greater than another, and under both metrics every line stays at (0, 0) after
    one step."""
    for idx in range(n):
        lines, diff = _differ(name, idx, rng)
        if name == "batch9" and idx == K.ZERO_COV_SLOT:
            prev, steps = K.reference(name, idx, rng, "min_eig")
            assert lines > 0 and diff == 0 and steps == lines
            assert not K.ratios(prev, K.states(name)[idx].track).any()
            continue
        assert (diff > 0) == (lines > 0), (name, idx, rng, lines, diff)
    if name == "batch9":
        assert [len(K.states(name)[i].track["matched_ls"]) for i in (1, 2, 3)] == [0, 1, 2]
        assert len(K.states(name)[4].track["matched_pt"]) == 0
        if rng == K.WIDE:   # the wide range is used: some ratio goes negative
            assert any((K.ratios(K.reference(name, i, rng)[0], K.states(name)[i].track) < 0).any() for i in range(n))


def test_whole_step_inputs_separate_the_metrics():
    """tests/test_cut_metric_gpu.py's whole steps (B = 3, 3 frames): on every state the min-eig
    trajectory visits, the logdet cut of the same state ends some line elsewhere."""
    for b in range(K.STEP_B):
        for k, (st, prev_e) in enumerate(K.step_reference(b)["cuts"]):
            st = st.copy()
            CutRef(K.camera(), K.config(), logdet).line_cut(st.prev, st.curr, st.track)
            a, e = K.ratios(st.prev, st.track), K.ratios(prev_e, st.track)
            assert len(a) > 10 and (a != e).any(), (b, k)


def test_metrics_disagree_by_construction():
    """One line with le_obs = (1, 0): entry 1 of both endpoint Jacobians is (fgz2 * 0) * gz = 0, so row
    and column 1 of its info are exactly zero at every ratio.  With invCov_sum = diag(1e4, 1, 1e4, ...)
    + its r = 0 info, direction 1 is the weakest (eigenvalue exactly 1: the Jacobi never rotates a row
    whose off-diagonal entries are zero) and the line cannot raise it: min-eig stays at (0, 0) after
    one step.  logdet sees the other five directions grow and moves."""
    cam, cfg = K.camera(), gfpl.default_config()
    D = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    cov = [1e-4, 0.0, 0.0, 0.0, 1e-4, 0.0, 0.0, 0.0, 4e-3]
    out = {}
    for metric in (logdet, min_eig):
        ref = CutRef(cam, cfg, metric)
        L = dict(Jl=[1.0, 0.0], sP=[-0.5, -1.0, 4.0], eP=[-0.25, 1.0, 6.0], covS=list(cov), covE=list(cov),
                 cut=[0.0, 0.0])
        L["inv"] = ref.pose_info_on_line(D, L["Jl"], L["sP"], L["eP"], L["covS"], L["covE"], 0.0, 0.0)
        assert all(L["inv"][6 + k] == 0.0 and L["inv"][6 * k + 1] == 0.0 for k in range(6))
        assert L["inv"][0] > 1e3
        tot = list(L["inv"])
        for k, v in enumerate([1e4, 1.0, 1e4, 1e4, 1e4, 1e4]):
            tot[7 * k] = v + tot[7 * k]
        if metric is min_eig:
            assert min_eig(tot) == 1.0
        out[metric.__name__] = (ref.search(D, {0: L}, [0], tot), list(L["cut"]))
    assert out["min_eig"] == (1, [0.0, 0.0])
    steps, cut = out["logdet"]
    assert steps > 1 and (cut[0] > 0.0 or cut[1] > 0.0), out
