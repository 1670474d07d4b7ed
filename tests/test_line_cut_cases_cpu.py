"""The written problems of line_cut_cases.py are what their names say (CPU only).

* CutRef(logdet), instrumented (line_cut_cases.TracedCut), equals the C++ oracle bit for bit on every case, at
  every cut_step and cut_rng used: CUT_FIELDS over all rows (NaNs canonical) and the step count.  This extends
  test_logdet_restatement_is_the_oracle_cut to the new steps and ranges and makes the trace a description of what
  the oracle did.
* Per family, the describing numbers: the tie ladders' gaps inside their brackets, moves back, more than CUT_PATH
  steps per line, final ratios past the last ratio key, negative ratios of the written lines, the list lengths, the
  pivot brackets, non-finite metrics and zero moves of the written rank-deficient lists.
* What the generator's states never reach at the default step (the table of DESIGN.md §3b), re-derived.
* Deliberately wrong variants of the Python search against the families that aim at them:
    last_max      ties (an exactly equal pair of neighbour metrics: the *_hi side of the last-bit pairs)
    ge_centre     ties (the same pairs: the second of two equal neighbours is taken when none is greater than the
                  first) and degenerate (null_dir: every metric is -inf, -inf >= -inf moves until the step cap)
    unclamped     steps, by clamp_start (a written line whose start has gz^2 < homog_th at r = 0: the clamp is in
                  the line's own invCovPose) and by the flat* lines: written lines whose extension meets the
                  camera plane at a grid ratio of the wide range AND whose covariance is flat (depth variance
                  1e-12).  Without the clamp the ratio on the plane wins a step; the reference never takes it.
                  The plane* lines, with the generator's covariances, do NOT separate it: the ratio on the plane
                  is evaluated as a neighbour but never wins under either formula (nor did it for 144 further
                  written lines with covariances scaled 1 .. 1e-6).
    points_first  no family separates it: the order of the sum moves invCov_sum by an ulp, which changes a
                  decision only inside a gap of a few ulps of the metric, and the last-bit pairs (tuned in the
                  reference's order) end the same under either order.  The lists family therefore aims at the
                  kernel's chunking through bit equality on the GPU, not at this variant.
  The range test taken before the r0 + r1 > 1 test is no variant at all: all three tests skip the neighbour, so
  their order cannot change a result on any input.  The proof family aims at capacities of the proven mode, not
  at a decision, and separates none of the variants.
"""
import math

import numpy as np
import pytest

import gfpl
import line_cut_cases as M


def _first_gz(c, pos):
    st = c.state
    D = M.dt_inv(st)
    li = M.line_row(st, pos)
    return float((D[:3, :3] @ st.prev.arr["ls_sP"][li] + D[:3, 3])[2])


def test_constants():
    assert gfpl.default_config().homog_th == M.HOMOG
    assert gfpl.default_config().cut_certify == 1e-9 and gfpl.default_config().cut_step == 0.05
    assert len({c.name for c in M.all_cases()}) == len(M.all_cases())


@pytest.mark.parametrize("fam", list(M.FAMILIES))
def test_python_cut_is_the_oracle_on_every_case(fam):
    bad = []
    for c in M.family(fam):
        t = M.trace(c)
        prev, steps = M.oracle_result(c)
        if not M.same_cut(t.prev, prev):
            bad.append(f"{c}: fields differ")
        if t.steps != steps or steps != sum(r["steps"] for r in t.lines):
            bad.append(f"{c}: steps {t.steps} vs {steps}")
    assert not bad, "\n".join(bad)


def test_ties():
    rungs = {}
    for c in M.family("ties"):
        t = M.trace(c)
        lo, hi = c.tags["bracket"]
        r = t.lines[c.tags["pos"]]
        print(f"{c.name}: gap {t.gap!r} at line {c.tags['pos']} step {r['gap_step']} against the {r['gap_vs']}")
        assert t.gap == r["gap"], c                      # the tie is the tuned line's
        if c.tags["rung"] == "clear":
            assert t.gap >= 4.0 * c.tau, (c, t.gap)
        elif c.tags["rung"] == "above":
            assert c.tau < t.gap < 2.0 * c.tau, (c, t.gap)
        elif c.tags["rung"] == "below":
            assert t.gap <= c.tau / 4.0, (c, t.gap)
        else:
            assert t.gap <= 1e-12, (c, t.gap)
        assert lo <= t.gap <= hi
        ladder = c.name.split("_")[0]
        if ladder == "first":
            assert r["gap_step"] == 0, c                 # the centre is the exact logdet(invCov_sum)
        else:
            assert r["gap_step"] > 0, c
        if ladder == "mid":
            assert r["gap_vs"] == "neighbour", c
        if ladder == "centre" and c.name.endswith("_lo"):
            assert r["gap_vs"] == "centre", c
        if c.tags["rung"] == "lastbit":
            a, b = c.tags["pair"]
            assert np.nextafter(a, math.inf) == b
        rungs.setdefault(c.name.rsplit("_", 1)[0], {})[c.name.rsplit("_", 1)[1]] = (tuple(r["path"]), t.steps)
    # the two sides of every rung decide differently
    for name, sides in rungs.items():
        assert set(sides) == {"lo", "hi"} and sides["lo"][0] != sides["hi"][0], name
    for tau in M.TAUS:
        for rung in M.RUNGS:
            assert f"mid_tau{tau:g}_{rung}" in rungs
    assert {"mid_far", "mid_lastbit", "centre_lastbit", "first_lastbit"} <= set(rungs)


def test_steps_and_ranges():
    seen = set()
    for c in M.family("steps"):
        t, g = M.trace(c), c.tags
        print(f"{c.name}: steps {t.steps} max per line {t.max_steps} back {t.back} gap {t.gap:.3g} "
              f"ratios {t.ratios.min():g} .. {t.ratios.max():g}")
        if g.get("back"):
            assert t.back > 0, c
        if g.get("past_keys"):
            assert t.ratios.max() > M.last_key(c.step), c
        if g.get("over_path"):
            assert t.max_steps > M.CUT_PATH, c
        if g.get("one_step"):
            assert t.steps == c.n_ls and not t.ratios.any(), c
        if g.get("negative"):
            assert min(t.lines[g["written"]]["cut"]) < 0.0, c
        if "in_range" in g:
            lo, hi = g["in_range"]
            moved = t.ratios[t.ratios != 0.0]
            assert ((moved >= lo) & (moved <= hi)).all(), c
            if g["in_range"] in ((0.1, 0.1), (0.0, 0.0), (0.25, 0.5)):   # no neighbour of (0, 0) is in the range
                assert t.steps == c.n_ls and not t.ratios.any(), c
            if g["in_range"] == (0.0, 0.5):   # the range's end is reached (10 additions of 0.05 stay just below 0.5)
                assert t.ratios.max() == sum([0.05] * 10) <= 0.5, c
        if c.step == 0.125:   # sums of binary fractions are exact: some line ends on r0 + r1 == 1.0
            assert (t.ratios.sum(axis=1) == 1.0).any(), c
        if c.step == 1.0:     # one ratio goes to 1; the one valid diagonal from there, (-s, +s), is not taken
            assert set(np.unique(t.ratios)) <= {0.0, 1.0} and t.max_steps == 2, c
        if "pd_edge" in g:
            z = abs(_first_gz(c, g["written"]))
            assert (z > M.PD_EDGE) == (g["pd_edge"] > 1.0) and abs(z / M.PD_EDGE - 1.0) < 2e-6, (c, z)
        if g.get("clamped"):
            assert _first_gz(c, g["written"]) ** 2 < M.HOMOG, c
        seen.add((c.step, c.rng))
    assert {s for s, _ in seen} == set(M.STEPS) | {0.05} and {r for _, r in seen} == set(M.RANGES) | {(0.0, 1.0)}


def test_lists():
    st = M.long_state()
    assert len(st.track["matched_ls"]) >= 129 and len(st.track["matched_pt"]) >= 130
    cs = [c for c in M.family("lists") if c.name.startswith("long_")]
    for c in cs:
        assert (c.n_ls, c.n_pt) == (c.tags["n_ls"], c.tags["n_pt"]) and c.n_ls <= 130, c
    assert {c.n_ls for c in cs} == set(M.LIST_LS) and {c.n_pt for c in cs} == set(M.LIST_PT)
    b9 = {c.name[7:]: c for c in M.family("lists") if c.name.startswith("batch9_")}
    assert [b9[n].n_ls for n in ("empty", "one_line", "two_lines")] == [0, 1, 2] and b9["no_points"].n_pt == 0
    t = M.trace(b9["zero_cov"])
    assert t.steps == b9["zero_cov"].n_ls and not t.ratios.any() and all(r["nan"] for r in t.lines)


def test_degenerate():
    for c in M.family("degenerate"):
        t, g = M.trace(c), c.tags
        piv = [r["pivot"] for r in t.lines]
        print(f"{c.name}: steps {t.steps} pivots {['%.3g' % x for x in piv]} metric at the first line {t.lines[0]['m0']!r}")
        if "n_ls" in g:
            assert (c.n_ls, c.n_pt) == (g["n_ls"], g["n_pt"]), c
        if g.get("rank_deficient"):
            assert not piv[0] >= 1e-9, (c, piv)
        if g.get("stays") or g.get("nonfinite"):
            assert all(not math.isfinite(r["m0"]) for r in t.lines), c
            assert t.steps == c.n_ls and not t.ratios.any(), c
        if g.get("nonfinite"):
            assert all(r["nan"] for r in t.lines), c
        if g.get("pivot") == "above":
            assert M.CUT_MIN_PIVOT <= min(piv) < 2.0 * M.CUT_MIN_PIVOT, (c, piv)
        if g.get("pivot") == "below":
            assert M.CUT_MIN_PIVOT / 2.0 < min(piv) <= M.CUT_MIN_PIVOT, (c, piv)
    z = next(c for c in M.family("degenerate") if c.name == "zero_length")
    li = M.line_row(z.state, 2)
    assert (z.state.prev.arr["ls_sP"][li] == z.state.prev.arr["ls_eP"][li]).all()


def test_proof_capacities():
    by = {c.name: c for c in M.family("proof")}
    assert by["detail6_wide"].n_ls > M.CUT_DTL and by["detail6_wide"].n_ls <= M.CUT_DTL * 9
    assert by["detail6_wide"].rng == M.WIDE
    t = M.trace(by["all_back"])
    assert len(t.lines) >= 5 and all(r["back"] > 0 for r in t.lines)
    assert M.trace(by["clear"]).gap > 1000 * 1e-9
    assert sum(1 for c in by.values() if c.tags.get("over_path")) >= 2


def test_what_the_generator_never_reaches():
    """The table of DESIGN.md §3b: sequences 0-5 of cut_metric_cases.base_states() under the default, 0.02 and
    0.01 steps.  At the default step there is no comparison within 1000 x cut_certify, no move back, no line
    near the CUT_PATH-step record, no ratio past the last of the CUT_KS keys and, under the wide range, no
    negative ratio."""
    rows = {}
    for step in (0.05, 0.02, 0.01):
        ts = [M.Trace(M.small(b), step, (0.0, 1.0)) for b in range(6)]
        rows[step] = (sum(len(t.lines) for t in ts), max(t.max_steps for t in ts), sum(t.back for t in ts),
                      min(t.gap for t in ts), max(float(t.ratios.max()) for t in ts))
        print(f"step {step}: lines {rows[step][0]} max steps per line {rows[step][1]} moves back {rows[step][2]} "
              f"smallest gap {rows[step][3]:.3g} largest ratio {rows[step][4]:g} (last key {M.last_key(step):g})")
    lines, steps, back, gap, rmax = rows[0.05]
    assert lines > 140 and steps < M.CUT_PATH // 2 and back == 0 and gap > 1000 * 1e-9 and rmax <= M.last_key(0.05)
    assert rows[0.02][2] > 0 and rows[0.02][4] > M.last_key(0.02)
    assert rows[0.01][1] > M.CUT_PATH and rows[0.01][3] < rows[0.05][3]
    wide = [M.Trace(M.small(b), 0.05, M.WIDE) for b in range(6)]
    assert min(float(t.ratios.min()) for t in wide) >= 0.0


AIMED = {"last_max": ["ties"], "ge_centre": ["ties", "degenerate"], "unclamped": ["steps"], "points_first": []}


def _separated(variant, fam):
    out = []
    for c in M.family(fam):
        t = M.trace(c, variant)
        prev, steps = M.oracle_result(c)
        if not (M.same_cut(t.prev, prev) and t.steps == steps):
            out.append(c.name)
    return out


@pytest.mark.parametrize("variant", list(AIMED))
def test_families_separate_the_wrong_variants(variant):
    """See the module docstring for what each variant is and which families do not aim at it."""
    for fam in AIMED[variant]:
        sep = _separated(variant, fam)
        print(f"{variant}: {fam} separates it by {sep}")
        assert sep, (variant, fam)
    if variant == "unclamped":   # (the plane* lines do not separate it)
        assert set(_separated(variant, "steps")) == {c.name for c in M.family("steps")
                                                     if c.tags.get("clamped") or c.tags.get("clamp_decides")}
    if variant == "points_first":   # recorded, not required: tuned in the reference's order, the ties end the same
        print(f"points_first: ties separate it by {_separated(variant, 'ties')}")
