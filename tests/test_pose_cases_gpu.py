"""k_pose<1>, k_pose<4>, k_pose<8> and k_pose_finish on the written problems of pose_cases.py, against the oracle.

optimizePose is otherwise reached through frameStep on synthetic frames (no tied residuals, no list length on a
64 / 512 boundary, no degenerate solve, the layout following the batch size) and through one written problem at
B = 1.  Here every case is written with write_frame / write_track into one sequence of a batch, the cases that
share a config in one batch of at most 48, the families one after the other through the same two handlers (one
per context of pose_cases.CONTEXTS): what a family leaves in pose_in / pose_act, in the slots it does not fill
and in LDS is what the next one starts from.  The three layouts are forced through GFPL_POSE_MULTI_MAX_B /
GFPL_POSE_W8_MAX_B (launch_pose reads them at every launch).

No tolerance: the kernel evaluates the oracle's operation order.  POSE fields and err_norm are
compared bit for bit, a NaN matching a NaN at the same position (parity.bitwise_equal_nan); the track with
compare_track; pt_inlier / ls_inlier of every matched feature.  test_pose_cases_cpu.py shows on the oracle that
every case takes the path it names and that the families notice the faults they aim at.
"""
import ctypes as C

import numpy as np
import pytest

import gfpl
import pose_cases as M
from parity import POSE, bitwise_equal_nan, compare_track

pytestmark = pytest.mark.gpu

BATCH = {"small": 48, "big": 32}
LAYOUTS = {"k_pose<1>": ("0", "0"), "k_pose<4>": ("4096", "0"), "k_pose<8>": (None, None)}
_RIGS = {}


def rig(ctx_name):
    """one context and one handler per pose_cases context; every slot starts as an empty problem, so a slot a
    batch does not fill never holds anything but an earlier case"""
    if ctx_name not in _RIGS:
        k = M.CONTEXTS[ctx_name]
        ctx = gfpl.Context(M.camera(), M.config(ctx_name))
        g = gfpl.StereoFrameHandler(ctx, BATCH[ctx_name], k["KP"], k["KL"])
        empty = M.make("empty", "reset_pre", ctx_name, 0, 0)
        for b in range(g.B):
            g.write_frame(gfpl.PREV, b, empty.prev)
            g.write_frame(gfpl.CURR, b, empty.curr)
            g.write_track(b, empty.tr)
        _RIGS[ctx_name] = (ctx, g)
    return _RIGS[ctx_name]


def _set_layout(monkeypatch, layout):
    for name, v in zip(("GFPL_POSE_MULTI_MAX_B", "GFPL_POSE_W8_MAX_B"), LAYOUTS[layout]):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _compare(c, prev, curr, track):
    op, oc, ot = M.oracle_result(c)
    w = c.what() + ": "
    bad = []
    for n in POSE:
        a, b = curr.get(n), oc.get(n)
        if not bitwise_equal_nan(a, b):
            neq = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
            f = tuple(neq[0]) if len(neq) else None
            bad.append(f"{w}{n}: {len(neq)} elements differ, first at {f}: gpu {a[f] if f else '?'!r} oracle {b[f] if f else '?'!r}")
    if not bitwise_equal_nan(curr.get("err_norm"), oc.get("err_norm")):
        bad.append(f"{w}err_norm {float(curr.s.err_norm)!r} vs {float(oc.s.err_norm)!r}")
    bad += compare_track(track, ot, w)
    ip, il = c.matched()
    for name, rows in (("pt_inlier", np.unique(ip)), ("ls_inlier", np.unique(il))):
        a, b = prev.arr[name][rows], op.arr[name][rows]
        if not np.array_equal(a, b):
            bad.append(f"{w}{name}: {int(np.sum(a != b))} matched features differ, first {rows[np.flatnonzero(a != b)[0]]}")
    return bad


def _run(cases):
    bad = []
    for (ctx_name, _), grp in M.groups(cases).items():
        ctx, g = rig(ctx_name)
        ctx.set_config(grp[0].cfg())
        for i in range(0, len(grp), g.B):
            batch = grp[i:i + g.B]
            for b, c in enumerate(batch):
                g.write_frame(gfpl.PREV, b, c.prev)
                g.write_frame(gfpl.CURR, b, c.curr)
                g.write_track(b, c.tr)
            if any(c.guess is not None for c in batch):
                guesses = np.stack([np.eye(4)] * g.B)
                for b, c in enumerate(batch):
                    guesses[b] = c.dt_ini()
                g.optimizePose(guesses)
            else:
                g.optimizePose()
            for b, c in enumerate(batch):
                bad += _compare(c, g.read_frame(gfpl.PREV, b), g.read_frame(gfpl.CURR, b), g.read_track(b))
    return bad


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_pose_cases(monkeypatch, layout):
    """Every family, in order, through the same handlers, in one layout.  48 / 32 sequences are below every
    default threshold, so unset variables run k_pose<8>; GFPL_POSE_W8_MAX_B=0 leaves k_pose<4> to
    GFPL_POSE_MULTI_MAX_B=4096 and k_pose<1> to GFPL_POSE_MULTI_MAX_B=0."""
    _set_layout(monkeypatch, layout)
    bad, per_family = [], {}
    for fam in M.FAMILIES:
        b = _run(M.family(fam))
        per_family[fam] = len({m.split("]: ")[0] for m in b})
        bad += [f"[{fam}] {m}" for m in b]
    assert not bad, f"{len(bad)} mismatches, cases per family {per_family}\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_pose_cases_reversed_slots(monkeypatch, layout):
    """The gates and the loop exits again with the cases in reverse order: every case meets the scratch, the
    flags and the pose another case left in its slot."""
    _set_layout(monkeypatch, layout)
    bad = _run(M.family("gates")[::-1]) + _run(M.family("loops")[::-1])
    assert not bad, f"{len(bad)} mismatches\n" + "\n".join(bad[:40])


def test_write_track_refuses_out_of_range_indices():
    """gfpl_write_track returns GFPL_E_INVALID for a matched index outside [0, kp_cap) / [0, kl_cap) — k_pose gathers
    prev-frame records by these indices — and writes nothing of such a track.  Nothing is launched here."""
    k = M.CONTEXTS["small"]
    ctx = gfpl.Context(M.camera(), M.config("small"))
    g = gfpl.StereoFrameHandler(ctx, 2, k["KP"], k["KL"])
    c = M.make("in range", "solved", "small", 6, 4)
    g.write_frame(gfpl.PREV, 1, c.prev)
    g.write_frame(gfpl.CURR, 1, c.curr)
    L = gfpl.hiplib()
    assert L.gfpl_write_track(g.h, 1, C.byref(c.tr)) == 0
    before = g.read_track(1)
    for field, pos, cap in (("matched_pt", 0, k["KP"]), ("matched_pt", 5, k["KP"]), ("matched_ls", 0, k["KL"]),
                            ("matched_ls", 3, k["KL"])):
        for v in (cap, -1, 2 ** 31 - 1, -2 ** 31):
            tr = gfpl.TrackHost.from_buffer_copy(c.tr)
            tr.n_inliers = 77
            getattr(tr, field)[pos] = v
            assert L.gfpl_write_track(g.h, 1, C.byref(tr)) == -1, (field, pos, v)
    after = g.read_track(1)
    assert compare_track(after, before) == [] and after["n_inliers"] == c.tr.n_inliers
    # the last valid index, and an index past a list's end, are accepted
    tr = gfpl.TrackHost.from_buffer_copy(c.tr)
    tr.matched_pt[5], tr.matched_ls[3] = k["KP"] - 1, k["KL"] - 1
    tr.matched_pt[6], tr.matched_ls[4] = -5, 10 ** 6
    assert L.gfpl_write_track(g.h, 1, C.byref(tr)) == 0
    assert g.read_track(1)["matched_pt"][5] == k["KP"] - 1
    g.close()
