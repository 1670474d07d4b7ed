"""The ends of the key range of knn2_mfma (gfpl_knn.hpp), in the line kernels, against plain numpy.

The line kernels take their knn keys from the bits of the scaled MFMA's accumulator (a block scale of
2^13 on the FP4 operands, the row field started into the accumulator) and reduce the reverse
direction with bank-masked DPP minima.  Two things about that rest on the hardware and show here
first: a block scale other than 2^0 leaves the integer counts exact, and a bank-masked v_min_u32
writes only the enabled banks — either one wrong changes accepted pairs in every shape below.

The test is about the contract, not the encoding: it runs the same stage entry points and the same
numpy statement as test_line_match_gpu.py (line_match_cases, imported, not edited) and passes on the
unscaled keys (dist << 16 | t) as well.  One descriptor family, "key extremes", holds what the
families there do not:
  * a query of all ones against a train of all zeros and the reverse: distance 256 (cell 1) / 128
    (cell 2) with popc(q) = 256 and 0, the accumulator at count 0 and +256;
  * mixed with exact duplicates at train index 0 (all ones: count -256, the lowest accumulator value)
    and nt - 1 (all zeros);
  * tied best pairs with one train in the first and one in the last tile (train 0 / nt - 3 for query
    0, train 1 / nt - 2 for query 2): the winner's row field, aged over the whole tile walk, is the
    smallest the layout can hold;
  * a second query of all ones: a reverse tie at distance 0 for train 0.
Each set runs with the default nn12 threshold and with a negative one (CFG_OVER of
forward_dups_open), under which a tied best match is accepted and the forward tie rule shows.

Shapes: (NL, NR) = (2, 2), (32, 33), (33, 32) at kl_cap 64; (65, 64) at kl_cap 96, the smallest
multiple of the tile that holds 65 rows (a capacity of 64 cannot); (512, 512) at 512; (2048, 2047)
and (2047, 2048) at 2048: the 1024-thread kernels and the longest tile walk.  Every assertion is
integer equality with numpy.
"""
import numpy as np
import pytest

import line_match_cases as L
import test_line_match_gpu as G

pytestmark = pytest.mark.gpu

OPEN = "forward_dups_open"          # the family name line_match_cases ties desc_th_l = -1 to
THRESHOLDS = {"planted": 0.1, OPEN: -1.0}
assert L.desc_th_l(OPEN) == -1.0 and L.desc_th_l("planted") == 0.1


class KCase(L.Case):
    """A Case whose reference runs at a stated desc_th_l (L.Case looks it up by family name)."""

    def __init__(self, q, t, ctx_family, D):
        super().__init__("key extremes" + (" open" if ctx_family == OPEN else ""), q, t)
        self.th = THRESHOLDS[ctx_family]
        self._D = D   # (shared between the two thresholds)

    def stereo(self, cell, rules=L.EXACT):
        k = ("s", cell, rules)
        if k not in self._ref:
            self._ref[k] = L.stereo_pairs(self.D(cell), self.q, self.t, cell, self.th, rules)
        return self._ref[k]

    def cross(self, rules=L.EXACT, max_num=300):
        k = ("c", rules, max_num)
        if k not in self._ref:
            self._ref[k] = L.cross_pairs(self.D(1), self.q, self.t, self.th, max_num, rules)
        return self._ref[k]


def key_extremes(nq, nt):
    rng = np.random.default_rng([2025, nq, nt])
    q, t, _ = L._planted(rng, nq, nt)
    q[0], t[0] = 0xFF, 0xFF            # duplicate at train 0: count -256, popc(q) 256
    q[nq - 1], t[nt - 1] = 0x00, 0x00  # duplicate at train nt - 1: count 0, popc(q) 0
    # (so D[0][nt - 1] = D[nq - 1][0] = 256 / 128: all ones against all zeros, both ways)
    if nq >= 6 and nt >= 6:
        t[nt - 3] = 0xFF               # query 0: tied best pair, trains 0 and nt - 3
        tied = L._flip(rng, q[2], 4)[0]
        t[1], t[nt - 2] = tied, tied   # query 2: tied best pair, trains 1 and nt - 2
        q[nq - 2] = 0xFF               # train 0: reverse tie, queries 0 and nq - 2
    return q, t


_SETS = {}


def cases(shapes, ctx_family):
    out = []
    for nq, nt in shapes:
        if (nq, nt) not in _SETS:
            _SETS[nq, nt] = key_extremes(nq, nt) + ({},)
        q, t, D = _SETS[nq, nt]
        out.append(KCase(q, t, ctx_family, D))
    return out


GROUPS = [
    ("cap64", 64, [(2, 2), (32, 33), (33, 32)], ("0", "4096")),
    ("cap96", 96, [(65, 64)], ("0", "4096")),
    ("cap512", 512, [(512, 512)], ("0", "4096")),
    ("cap2048", 2048, [(2048, 2047), (2047, 2048)], ("0",)),   # (1024 threads by the capacity alone)
]


@pytest.mark.parametrize("name,cap,shapes,wides", GROUPS, ids=[g[0] for g in GROUPS])
def test_key_extremes(monkeypatch, name, cap, shapes, wides):
    """initialize (k_stereo_lines<1, true>), stereoLines (<2, false>) and crossFrameMatchingLines
    (k_cross_lines), 512- and 1024-thread forms, both thresholds."""
    rig = G.Rig(len(shapes), cap)
    bad = []
    for fam in ("planted", OPEN):
        g = rig.handler(fam)
        cs = cases(shapes, fam)
        for wide in wides:
            monkeypatch.setenv("GFPL_SP_WIDE_MAX_B", wide)
            bad += G._stereo_initial(rig, g, cs)
            bad += G._stereo_frame(rig, g, cs)
            bad += G._cross(g, cs, cap)
    assert not bad, "\n".join(bad[:30])
