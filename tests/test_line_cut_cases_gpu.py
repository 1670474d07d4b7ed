"""gfpl_line_cut in log-det mode (k_cut.hip: k_cut_prep<1|8>, k_cut_search_w, k_cut_search<false>, <false, true>
and <true>, k_cut_vref, _vref_off, _ebound, _verify, _verify_detail, _bounds, _vtab, _finish) on the written
problems of line_cut_cases.py, against the C++ oracle.

The bar is equality with the oracle, no tolerance and no case left out: for every sequence of every batch
compare_prev_matched plus CUT_FIELDS over all rows (NaNs canonical), and StepSlot.CUT_STEPS against the oracle's
step count.  test_line_cut_cases_cpu.py shows on the reference that every case is what its name says.

Every case is written with write_frame / write_track into one sequence of a batch of B in {1, 8, 9, 17, 24}; the
cases that share a (cut_step, cut_rng) share batches, unfilled slots hold an empty list.  One context and one
handler per B serve every test, the families one after the other: what a batch leaves in cut_path, cut_flag,
cut_offl, cut_vmax, the detail list and LDS is what the next one starts from.  The search layout is forced through
GFPL_CUT_WAVE_MAX_B (unset: k_cut_search_w, "0": the 8-sequences-per-wave kernels) and the prep layout through
GFPL_CUT_PREP_W8_MAX_B (launch_line_cut reads both at every launch).

Paths actually taken are asserted where the design guarantees them, never redone == 0.
"""
import pytest

import gfpl
import line_cut_cases as M
from parity import compare_prev_matched, diff_fields

pytestmark = pytest.mark.gpu

S = gfpl.StepSlot
BS = (1, 8, 9, 17, 24)
DBG_VFY_DLINES = 7
LAYOUTS = {"wave": None, "w8": "0"}
_RIG = {}


def rig(B):
    """one context for all, one handler per batch size; every slot starts as an empty list"""
    if "ctx" not in _RIG:
        _RIG["ctx"] = gfpl.Context(M.camera(), M.config())
    if B not in _RIG:
        g = gfpl.StereoFrameHandler(_RIG["ctx"], B, M.KP, M.KL)
        e = M.empty_case()
        for b in range(B):
            g.write_frame(gfpl.PREV, b, e.state.prev)
            g.write_frame(gfpl.CURR, b, e.state.curr)
            g.write_track(b, gfpl.track_from_dict(e.state.track))
        _RIG[B] = g
    return _RIG["ctx"], _RIG[B]


def _layout(monkeypatch, layout, prep1=False):
    if LAYOUTS[layout] is None:
        monkeypatch.delenv("GFPL_CUT_WAVE_MAX_B", raising=False)
    else:
        monkeypatch.setenv("GFPL_CUT_WAVE_MAX_B", LAYOUTS[layout])
    if prep1:
        monkeypatch.setenv("GFPL_CUT_PREP_W8_MAX_B", "0")
    else:
        monkeypatch.delenv("GFPL_CUT_PREP_W8_MAX_B", raising=False)


def batch_size(n):
    return next(B for B in BS if B >= n)


def batches(cases):
    """the cases grouped by (cut_step, cut_rng), in chunks of at most 24, each with its batch size"""
    groups = {}
    for c in cases:
        groups.setdefault(c.key(), []).append(c)
    out = []
    for grp in groups.values():
        for i in range(0, len(grp), BS[-1]):
            chunk = grp[i:i + BS[-1]]
            out.append((chunk, batch_size(len(chunk))))
    return out


def run_batch(cases, B, proof, certify):
    """one gfpl_line_cut of the cases in slots 0.. of the handler of B; returns (mismatches, step records, proof
    counts, debug rows)"""
    ctx, g = rig(B)
    ctx.set_config(cases[0].cfg(cut_proof=proof, cut_certify=certify))
    slots = list(cases) + [M.empty_case()] * (B - len(cases))
    assert len(slots) == B and all(c.key() == cases[0].key() and c.n_ls <= 130 for c in cases)
    for b, c in enumerate(slots):
        g.write_frame(gfpl.PREV, b, c.state.prev)
        g.write_frame(gfpl.CURR, b, c.state.curr)
        g.write_track(b, gfpl.track_from_dict(c.state.track))
    g.estimateProjUncertainty_submodular()
    rec, pr, dbg = g.debug_step_records(), g.last_step_cut_proof(), g.debug_clocks()
    bad = []
    for b, c in enumerate(slots):
        want, n_ref = M.oracle_result(c)
        got = M.canon(g.read_frame(gfpl.PREV, b))
        w = f"{c} B {B} slot {b} proof {proof} certify {certify:g}: "
        bad += compare_prev_matched(got, want, c.state.track, w)
        bad += diff_fields(got, want, M.CUT_FIELDS, what=w + "all rows ")
        if rec[b, S.CUT_STEPS] != n_ref:
            bad.append(f"{w}steps {rec[b, S.CUT_STEPS]} vs {n_ref}")
    bad += _paths(slots, proof, certify, rec, pr, dbg, B)
    return bad, rec, pr, dbg


def _paths(slots, proof, certify, rec, pr, dbg, B):
    """the design's guarantees about the paths taken (conditions, not measurements)"""
    bad = []
    for b, c in enumerate(slots):
        w = f"{c} B {B} slot {b} proof {proof} certify {certify:g}: "
        steps, exact = int(rec[b, S.CUT_STEPS]), int(rec[b, S.CUT_EXACT])
        if certify == 0.0 and exact != steps:
            bad.append(f"{w}cut_certify 0 but exact steps {exact} of {steps}")
        if certify > 0.0 and c.family == "ties" and M.trace(c).gap <= certify / 4.0 and exact < 1:
            bad.append(f"{w}a tie of gap {M.trace(c).gap:g} and no exact step")
        if proof == 2 and c.tags.get("past_keys") and exact < 1:
            bad.append(f"{w}ratios past the last key and no exact step")
        if proof == 3 and c.n_ls > 0 and rec[b, S.PROOF_REDONE] != 1:
            bad.append(f"{w}cut_proof 3 and not redone")
        if proof in (1, 2) and (c.rng[0] < 0.0 or c.rng[1] > 1.0):
            # a range outside [0, 1] has no agreement bound.  The eager-proven search (proof 2, and the redone
            # sequences of proof 1) counts every line it opens as unbounded; a sequence proof 1 does not redo
            # keeps the recorded search's 0, and k_cut_verify must then have bounded none of its margined lines:
            # all of them go to k_cut_verify_detail, which decides their steps in the reference's arithmetic
            if proof == 2 or rec[b, S.PROOF_REDONE]:
                if rec[b, S.CUT_UNBOUNDED] != c.n_ls:
                    bad.append(f"{w}unbounded lines {rec[b, S.CUT_UNBOUNDED]} of {c.n_ls}")
            elif certify > 0.0 and (rec[b, S.CUT_UNBOUNDED] != 0 or dbg[b, DBG_VFY_DLINES] != rec[b, S.PROOF_LINES]):
                bad.append(f"{w}not redone: unbounded {rec[b, S.CUT_UNBOUNDED]}, lines with margined steps "
                           f"{rec[b, S.PROOF_LINES]}, left to the detail kernel {dbg[b, DBG_VFY_DLINES]}")
    if proof == 1:
        # (at cut_certify = 1e-9 these lines have margined steps; a line whose steps were all exact leaves nothing
        # to prove, however long its path, so a wider margin guarantees no redo)
        named = [c for c in slots if certify == 1e-9 and (c.tags.get("over_path") or (c.tags.get("detail") and B == 1))]
        if named and pr["redone"] < 1:
            bad.append(f"{named} B {B}: proof 1 and no sequence redone")
        for b, c in enumerate(slots):
            if c.tags.get("detail") and certify > 0.0 and dbg[b, DBG_VFY_DLINES] < 1:
                bad.append(f"{c} B {B} slot {b}: no line left to k_cut_verify_detail")
        if certify > 0.0 and any(c.tags.get("clear") for c in slots) and pr["steps_proven"] <= 0:
            bad.append(f"{slots} B {B}: a clear batch and no step proven")
    return bad


def run_family(fam, proof, certify):
    bad = []
    for chunk, B in batches(M.family(fam)):
        bad += run_batch(chunk, B, proof, certify)[0]
    if fam == "proof" and proof == 1:   # the detail-list sequence again at B = 9, where the list holds it
        d = [c for c in M.family("proof") if c.tags.get("detail")]
        bad += run_batch(d, 9, proof, certify)[0]
    return bad


def _report(bad):
    assert not bad, f"{len(bad)} mismatches\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("proof", [0, 1, 2, 3])
def test_line_cut_cases(monkeypatch, proof, layout):
    """Every family, in order, through the same handlers, at cut_certify = 1e-9."""
    _layout(monkeypatch, layout)
    bad = []
    for fam in M.FAMILIES:
        bad += [f"[{fam}] {m}" for m in run_family(fam, proof, 1e-9)]
    _report(bad)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("proof", [0, 1])
@pytest.mark.parametrize("certify", [0.0, 1e-10, 1e-3])
def test_ties_and_degenerate_sums_under_other_margins(monkeypatch, certify, proof, layout):
    """cut_certify 0 (every step exact), 1e-10 (the smallest cfg_supported accepts: the tau = 1e-10 ladder is
    relative to it) and 1e-3 (every tie of the ladders is below it)."""
    _layout(monkeypatch, layout)
    _report(run_family("ties", proof, certify) + run_family("degenerate", proof, certify))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("proof", [0, 1])
def test_steps_and_ranges_under_a_wide_margin(monkeypatch, proof, layout):
    """cut_certify = 1e-3 lets the rounding-error bound of d pass where 1e-9 does not (the flat* lines: v' on the
    camera plane is 1e-8 of its absolute terms), so that only the range test of line_ok keeps a margined step
    from taking the ratio on the plane."""
    _layout(monkeypatch, layout)
    _report(run_family("steps", proof, 1e-3))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("proof", [0, 1])
def test_line_cut_cases_prep_one_wave(monkeypatch, proof, layout):
    """k_cut_prep<1> (GFPL_CUT_PREP_W8_MAX_B = 0): every family."""
    _layout(monkeypatch, layout, prep1=True)
    bad = []
    for fam in M.FAMILIES:
        bad += [f"[{fam}] {m}" for m in run_family(fam, proof, 1e-9)]
    _report(bad)


def _pool():
    """the cases of the default step and range, the families interleaved"""
    fams = [[c for c in M.family(f) if c.key() == (0.05, (0.0, 1.0))] for f in M.FAMILIES]
    out, i = [], 0
    while any(fams):
        if fams[i % len(fams)]:
            out.append(fams[i % len(fams)].pop(0))
        i += 1
    return out


def _by_name(name):
    return next(c for c in M.all_cases() if c.name == name)


def mixed(B):
    """a deliberately mixed batch: in the first wave of the 8-per-wave layout a tie, an empty list, a 1-line list
    and the 129-line list (an exact round forced on groups that do not need it; a group that waits more than
    CUT_WAIT = 16 iterations at a transition), then the pool in strides"""
    first = [_by_name("mid_tau1e-09_below_lo"), M.empty_case(), _by_name("batch9_one_line"), _by_name("long_129l_130p"),
             _by_name("centre_lastbit_hi"), _by_name("null_dir_2l"), _by_name("long_64l_64p"), _by_name("first_far_lo")]
    pool = [c for c in _pool() if c not in first]
    return (first + pool[B % 5::3])[:B]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B", [8, 9, 17, 24])
def test_mixed_batches_rotated_and_reversed(monkeypatch, B, layout):
    """Each mixed batch, then its slots rotated by one, then reversed; measured and proven."""
    _layout(monkeypatch, layout)
    m = mixed(B)
    assert len(m) == B
    bad = []
    for order in (m, m[1:] + m[:1], m[::-1]):
        for proof in (0, 1):
            bad += run_batch(order, B, proof, 1e-9)[0]
    _report(bad)


def test_lone_sequences(monkeypatch):
    """B = 1: the long lists and a tie alone in the grid."""
    _layout(monkeypatch, "wave")
    bad = []
    for name in ("long_129l_130p", "long_64l_64p", "mid_lastbit_hi", "batch9_empty"):
        for proof in (0, 1, 2):
            bad += run_batch([_by_name(name)], 1, proof, 1e-9)[0]
    _report(bad)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_clear_cases_after_redone_sequences(monkeypatch, layout):
    """Stale state: a proof-1 batch in which sequences are redone (lines of more than CUT_PATH steps), then clear
    cases in the same slots of the same handler.  cut_path, cut_flag, cut_offl, cut_vmax and the detail list are
    what the first batch leaves behind."""
    _layout(monkeypatch, layout)
    long_steps = [c for c in M.family("steps") if c.step == 0.005]
    clear = [c for c in _pool() if c.family in ("lists", "proof") and 0 < c.n_ls <= 30][:8]
    assert len(long_steps) == 2 and len(clear) == 8
    bad, _, pr, _ = run_batch(long_steps, 8, 1, 1e-9)
    assert pr["redone"] >= 1, pr
    bad += run_batch(clear, 8, 1, 1e-9)[0]
    wide = [c for c in M.family("proof") if c.tags.get("detail")]
    bad += run_batch(wide, 1, 1, 1e-9)[0]
    bad += run_batch(clear[:1], 1, 1, 1e-9)[0]
    _report(bad)
