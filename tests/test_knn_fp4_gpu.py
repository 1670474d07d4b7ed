"""The MFMA knn-2 (gfpl_knn.hpp, FP4 operands) against a numpy brute force.

gfpl_knn2_hamming (k_knn2m) over every pair of the tile-edge sizes, for NORM_HAMMING (cell 1) and
NORM_HAMMING2 (cell 2): both indices and both distances must be equal as integers — the FP4 operands
hold only 0 and +-1 and the f32 accumulator counts exactly, so nothing is approximate; and at the
packed key's last train index, 65535, with the hand-over to the scalar k_knn2 above it.  The in-kernel
passes (knn2_mfma with its reverse direction, inside k_stereo_lines and k_cross_lines) are compared
through frameStep with the CPU oracle on the bench workload's shapes here, and on their own, on
adversarial line descriptors (ties, duplicates, zero rows, tile-edge counts) against numpy, in
test_line_match_gpu.py.
"""
import numpy as np
import pytest

import gfpl
import oracle as O
from parity import compare_core, compare_pose, compare_track

pytestmark = pytest.mark.gpu

# partial tiles (2, 31, 33, 63, 65), full tiles (32, 64), an odd tile count per wave and waves with
# no tile (k_knn2m: 4 waves of one 32-query tile per workgroup), several workgroups (300, 512)
SIZES = (2, 31, 32, 33, 63, 64, 65, 300, 512)
NMAX = max(SIZES)
KINDS = ("random", "duplicates", "all_equal", "zeros_vs_ones", "last_byte", "last_bytes")

_POP1 = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)               # NORM_HAMMING
_POP2 = np.array([bin((v | (v >> 1)) & 0x55).count("1") for v in range(256)], dtype=np.int64)  # NORM_HAMMING2


def _dist(q, t, cell):
    """Brute force: per byte, the set bits (cell 1) / the 2-bit cells that differ (cell 2) of q ^ t."""
    pop = _POP1 if cell == 1 else _POP2
    return pop[q[:, None, :] ^ t[None, :, :]].sum(axis=2)


def _top2(D):
    """BFMatcher::knnMatch(k = 2): ascending distance, ties keep the lower train index."""
    key = np.sort(D * 65536 + np.arange(D.shape[1], dtype=np.int64)[None, :], axis=1)[:, :2]
    return (key & 0xFFFF).astype(np.int32), (key >> 16).astype(np.float32)


def _descriptors(kind, nq, nt):
    """(q, t, slice_stable): slice_stable sets are prefixes of one NMAX-row set (shared reference)."""
    rng = np.random.default_rng(1234 + KINDS.index(kind))
    q = rng.integers(0, 256, (NMAX, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (NMAX, 32), dtype=np.uint8)
    if kind == "random":
        pass
    elif kind == "duplicates":
        q, t = q[:nq].copy(), t[:nt].copy()
        t[nt - 1] = t[0]                      # the same row at the lowest and at the highest index
        q[0] = t[0]                           # distance 0 to both: the tie goes to index 0
        q[nq - 1] = t[nt - 1]
        if nt > 33:
            t[32] = t[31]                     # a duplicate pair across the first tile boundary
            q[nq // 2] = t[32]
        if nt > 65:
            t[64] = t[63]                     # ... and across the second one
            q[1] = t[64]
        return q, t, False
    elif kind == "all_equal":
        q[:] = q[0]
        t[:] = q[0]
    elif kind == "zeros_vs_ones":
        q[:] = 0x00
        t[:] = 0xFF
    elif kind == "last_byte":                 # the last k-step of the upper lane half
        q[:, :31] = q[0, :31]
        t[:, :31] = q[0, :31]
    elif kind == "last_bytes":                # bytes 28 .. 31: the last k-step of both lane halves, both cells
        q[:, :28] = q[0, :28]
        t[:, :28] = q[0, :28]
    return q, t, True


_FULL = {}   # (kind, cell) -> distances of the NMAX x NMAX set, computed once


def _reference(kind, cell, nq, nt):
    q, t, stable = _descriptors(kind, nq, nt)
    if not stable:
        return q, t, _top2(_dist(q, t, cell))
    if (kind, cell) not in _FULL:
        _FULL[(kind, cell)] = _dist(q, t, cell)
    return q[:nq], t[:nt], _top2(_FULL[(kind, cell)][:nq, :nt])


@pytest.fixture(scope="module")
def ctx():
    cfg = gfpl.default_config()
    return gfpl.Context(gfpl.make_camera("vga", cfg), cfg)


@pytest.mark.parametrize("cell", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_knn2_hamming_bruteforce(ctx, kind, cell):
    import torch
    bad = []
    for nq in SIZES:
        for nt in SIZES:
            q, t, (ri, rd) = _reference(kind, cell, nq, nt)
            qd, td = torch.from_numpy(np.ascontiguousarray(q)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda()
            idx = torch.full((nq, 2), -7, dtype=torch.int32, device="cuda")
            dist = torch.full((nq, 2), -7.0, dtype=torch.float32, device="cuda")
            assert ctx.knn2(qd, nq, td, nt, cell, idx, dist) == 0
            ctx.synchronize()
            gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
            if not (np.array_equal(gi, ri) and np.array_equal(gd, rd)):
                w = np.nonzero((gi != ri).any(axis=1) | (gd != rd).any(axis=1))[0]
                bad.append(f"nq {nq} nt {nt}: {len(w)} queries differ, first q {w[0]}: "
                           f"got {gi[w[0]].tolist()} {gd[w[0]].tolist()} want {ri[w[0]].tolist()} {rd[w[0]].tolist()}")
    assert not bad, "\n".join(bad[:20])


def test_reference_extremes():
    """The brute force itself at its known answers (so a wrong reference cannot pass a wrong kernel)."""
    for cell, dmax in ((1, 256), (2, 128)):
        _, _, (ri, rd) = _reference("zeros_vs_ones", cell, 33, 65)
        assert (ri == [0, 1]).all() and (rd == dmax).all()
        _, _, (ri, rd) = _reference("all_equal", cell, 33, 65)
        assert (ri == [0, 1]).all() and (rd == 0).all()
        _, _, (ri, rd) = _reference("duplicates", cell, 65, 300)
        assert ri[0].tolist() == [0, 299] and ri[32].tolist() == [31, 32] and ri[1].tolist() == [63, 64]
        assert (rd[[0, 1, 32, 64]] == 0).all()


def _top2_blocked(q, t, cell, block=4096):
    """_top2(_dist(q, t, cell)) for a train set too large for one _dist call (and for a 16-bit index):
    the distances in row blocks of t, the key with the train index in its low 20 bits."""
    pop = (_POP1 if cell == 1 else _POP2).astype(np.uint8)
    D = np.concatenate([pop[q[:, None, :] ^ t[b0:b0 + block][None, :, :]].sum(axis=2, dtype=np.int64)
                        for b0 in range(0, len(t), block)], axis=1)
    key = np.sort((D << 20) + np.arange(len(t), dtype=np.int64)[None, :], axis=1)[:, :2]
    return (key & 0xFFFFF).astype(np.int32), (key >> 20).astype(np.float32)


@pytest.mark.parametrize("cell", [1, 2])
@pytest.mark.parametrize("nt", [65536, 65537])
def test_knn2_hamming_index_boundary(ctx, nt, cell):
    """The packed key's 16-bit train index at its last value, and the hand-over to the scalar kernel:
    nt = 65536 is the largest set the MFMA kernel takes (train row 65535 sits in the last tile of the
    last chunk), nt = 65537 the smallest that goes to k_knn2.  Random descriptors with planted rows at
    distance 0: set 0 has q[0] = t[nt - 1] and q[32] = t[65535]; set 1 also has t[nt - 1] = t[0] and
    q[1] = t[0], so the tie goes to index 0 and the second neighbour is nt - 1 at distance 0.  The
    planted answers are asserted on the brute force itself."""
    import torch
    nq = 33
    rng = np.random.default_rng(77 + cell)
    q0 = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t0 = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for dup in (0, 1):
        q, t = q0.copy(), t0.copy()
        if dup:
            t[nt - 1] = t[0]
            q[1] = t[0]
        q[0] = t[nt - 1]
        q[32] = t[65535]
        ri, rd = _top2_blocked(q, t, cell)
        assert rd[0, 0] == 0 and rd[32, 0] == 0
        if dup:
            assert ri[1].tolist() == [0, nt - 1] and rd[1].tolist() == [0, 0]
            assert ri[0].tolist() == [0, nt - 1] and rd[0].tolist() == [0, 0]
            assert ri[32, 0] == (0 if nt == 65536 else 65535)
        else:
            assert ri[0, 0] == nt - 1 and ri[32, 0] == 65535 and rd[0, 1] > 0
        qd, td = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
        idx = torch.full((nq, 2), -7, dtype=torch.int32, device="cuda")
        dist = torch.full((nq, 2), -7.0, dtype=torch.float32, device="cuda")
        assert ctx.knn2(qd, nq, td, nt, cell, idx, dist) == 0
        ctx.synchronize()
        gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
        w = np.nonzero((gi != ri).any(axis=1) | (gd != rd).any(axis=1))[0]
        assert len(w) == 0, (f"nt {nt} cell {cell} set {dup}: {len(w)} queries differ, first q {w[0]}: got "
                             f"{gi[w[0]].tolist()} {gd[w[0]].tolist()} want {ri[w[0]].tolist()} {rd[w[0]].tolist()}")


@pytest.mark.parametrize("wide", ["0", "4096"])
def test_framestep_lines_parity(monkeypatch, wide):
    """8 sequences x 3 frames of the bench workload's shapes (vga, respawn 16, caps 2048 / 512, bench
    config) through frameStep: k_stereo_lines (NORM_HAMMING2) and k_cross_lines (NORM_HAMMING) run
    knn2_mfma with the reverse direction from the same tiles; stereo features, matched lists and poses
    against the oracle.  Both workgroup layouts: 8 waves (the bench batch's) and 16."""
    monkeypatch.setenv("GFPL_SP_WIDE_MAX_B", wide)
    n_seq, n_frames, KP, KL = 8, 3, 2048, 512
    cfg = gfpl.default_config(max_iters=10, max_iters_ref=10, min_error=0.0, min_error_change=0.0)
    cam = gfpl.make_camera("vga", cfg)
    H = gfpl.HostFrames(cam, gfpl.synth_params(seed=21, respawn=16), n_seq, n_frames, KP, KL)
    D = gfpl.DeviceFrames(H)
    g = gfpl.StereoFrameHandler(gfpl.Context(cam, cfg), n_seq, KP, KL)
    orc = [O.OracleHandler(cam, cfg, KP, KL) for _ in range(n_seq)]
    g.initialize(D.frames(0))
    bad, counts = [], []
    for b, o in enumerate(orc):
        o.initialize(H.frames(0), b)
        bad += compare_core(g.read_frame(gfpl.PREV, b), o.read_frame(gfpl.PREV), f"init s{b} ")
    for k in range(1, n_frames):
        g.frameStep(D.frames(k))
        for b, o in enumerate(orc):
            o.insertStereoPair(H.frames(k), b)
            o.optimizePose()
            tr = o.read_track()
            counts.append((o.read_frame(gfpl.CURR).n_ls, len(tr["matched_ls"])))
            o.updateFrame()
            gp, op = g.read_frame(gfpl.PREV, b), o.read_frame(gfpl.PREV)
            bad += compare_core(gp, op, f"f{k} s{b} ")
            bad += compare_pose(gp, op, what=f"f{k} s{b} ")[0]
            bad += compare_track(g.read_last_track(b), tr, f"f{k} s{b} ")
    assert not bad, "\n".join(bad[:30])
    assert all(c[0] > 0 and c[1] > 0 for c in counts), counts   # lines were matched both ways
