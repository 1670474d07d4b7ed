"""The key layout of knn2_mfma (gfpl_knn.hpp) as a numpy model, over its whole domain.

The line kernels take their knn keys from the bits of the scaled MFMA's f32 accumulator: register r
of lane half h starts at 1.5 * 2^23 + R0 + row(r) + 4 h, every product is scaled by 2^S, and the
finished float, read as uint32, is the key.  The model below is that sentence in float32 arithmetic:
    float32(1.5 * 2^23 + R0 + row + 4 h) + float32(count * 2^S), .view(uint32)
with the running top-2 kept relative to the current tile (-32 per tile step).  S and R0 are read from
the header, so the model is about the values the kernels are built with.  Checked over every count
in [-256, 256], every accumulator register, both lane halves and every tile 0..63:
  * uint32 order = lexicographic (count, train index) order, strictly;
  * no key reaches the start value 0xFFFFFFFF, however often that was aged by -32;
  * the decode returns (count + off, t);
  * the reverse key is 0x4B400000 + dist * 2^S + q for every query index below 2048 and every
    popc(q) in 0..256, so it orders as (dist, q), its low S bits are q, the padded columns' keys lie
    above every real one and below 0xFFFFFFFF.
The same model with S = 14 or with R0 = 0 must break one of these: the test can fail.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "gf-pl-slam_amd", "csrc", "gfpl_knn.hpp")

BASE = 0x4B400000        # bits of 1.5 * 2^23
PAD = 0x40000000         # KNN_KEY_PAD
TILES = 64               # kl_cap 2048
ROW = np.array([(r & 3) + 8 * (r >> 2) for r in range(16)])   # knn_acc_row


def header_constants():
    text = open(HDR).read()
    val = {}
    for name in ("KNN_KEY_S", "KNN_KEY_R0", "KNN_KEY_CAP"):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert m, name
        val[name] = int(m.group(1))
    assert re.search(r"KNN_KEY_BASE\s*=\s*0x4B400000u", text) and re.search(r"KNN_KEY_PAD\s*=\s*0x40000000u", text)
    return val["KNN_KEY_S"], val["KNN_KEY_R0"], val["KNN_KEY_CAP"]


def acc_bits(count, S, R0):
    """bits[count index, h, r]: the finished accumulator registers, for counts of any shape"""
    start = (np.float32(1.5 * 2 ** 23) + (R0 + ROW[None, :] + 4 * np.arange(2)[:, None]).astype(np.float32)).astype(np.float32)
    add = (np.asarray(count, np.int64) * 2 ** S).astype(np.float32)
    return (start[None] + add[:, None, None]).astype(np.float32).view(np.uint32)


def violations(S, R0, cap=2048):
    """names of the properties the layout (S, R0) breaks; [] when it holds"""
    bad = []
    counts = np.arange(-256, 257)
    bits = acc_bits(counts, S, R0).astype(np.int64)                       # [513][2][16]
    # forward keys as the last tile sees them: the key of tile rt has aged by -32 (TILES - 1 - rt)
    age = 32 * (TILES - 1 - np.arange(TILES))
    K = (bits[:, None] - age[None, :, None, None]) & 0xFFFFFFFF           # [513][64][2][16]
    t = 32 * np.arange(TILES)[:, None, None] + 4 * np.arange(2)[None, :, None] + ROW[None, None, :]   # [64][2][16]
    order = np.argsort(t.ravel())
    assert np.array_equal(t.ravel()[order], np.arange(cap))               # (every train index once)
    Kt = K.reshape(len(counts), -1)[:, order]                             # [count][t]
    if not np.all(np.diff(Kt.ravel()) > 0):
        bad.append("forward order")
    if not (Kt.max() < 0x80000000 and 0xFFFFFFFF - 32 * TILES >= 0x80000000):
        bad.append("sentinel")
    # decode (knn_key_decode): uint32 arithmetic as in the kernel
    mask = (1 << S) - 1
    for off in (0, 1, 127, 128, 255, 256):
        ok = (counts + off >= 0) & (counts + off <= 256)
        u = (Kt[ok] - BASE + (off << S)) & 0xFFFFFFFF
        dist, tt = u >> S, (u & mask) + 32 * (TILES - 1) - R0
        if not (np.array_equal(dist, np.broadcast_to((counts[ok] + off)[:, None], dist.shape))
                and np.array_equal(tt, np.broadcast_to(np.arange(cap)[None, :], tt.shape))):
            bad.append(f"decode off {off}")
    # reverse keys: acc bits + (off << S) + q, the row field taken off by the lane that holds the minimum
    field = R0 + 4 * np.arange(2)[:, None] + ROW[None, :]                 # [2][16]
    q = np.arange(cap)
    for off in range(0, 257):                                             # popc(q) (cell 1); 128 (cell 2)
        c = counts[(counts + off >= 0) & (counts + off <= 256)]
        b = bits[c + 256]                                                 # [n][2][16]
        for qq in (q[:1], q[-1:]):                                        # (linear in q: the ends suffice)
            raw = b + (off << S) + qq[0]
            if raw.max() >= 0xFFFFFFFF:
                bad.append("reverse wraps")
            key = raw - field[None]
            want = BASE + ((c + off) << S)[:, None, None] + qq[0]
            if not np.array_equal(key, np.broadcast_to(want, key.shape)):
                bad.append(f"reverse key off {off}")
                break
            if not np.all((key & mask) == qq[0]):
                bad.append("reverse index mask")
    real_max = BASE + (256 << S) + cap - 1
    # (dist, q) order of BASE + dist * 2^S + q needs q < 2^S; the padded columns: off 0 / 128, any count
    if not cap - 1 <= mask:
        bad.append("reverse order")
    pad = bits + PAD - field[None]
    for off in (0, 128):
        if not (pad.min() + (off << S) > real_max and pad.max() + (off << S) < 0xFFFFFFFF):
            bad.append("pad keys")
    return sorted(set(bad))


def test_header_layout_holds():
    S, R0, cap = header_constants()
    assert (S, R0, cap) == (13, 2016, 2048)
    assert violations(S, R0, cap) == []


def test_model_can_fail():
    """S = 14: count 256 lifts the float to 2^24, where ulp = 2 and odd row fields round away.
    R0 = 0: an aged row field goes negative and borrows from the count."""
    assert violations(14, 2016)
    assert violations(13, 0)


def test_accumulation_is_exact_step_by_step():
    """The matrix core adds +-2^S products one k-step (<= 64 of them) at a time: every partial sum of
    a worst-case order (all +1 first, then all -1, and the reverse) is an integer the f32 holds."""
    S, R0, _ = header_constants()
    start = np.float32(1.5 * 2 ** 23 + R0 + 27 + 4)
    for first in (1, -1):
        acc = start
        for sign, n in ((first, 256), (-first, 256)):
            for _ in range(4):                                            # four k-steps of 64 products
                nxt = np.float32(acc + np.float32(sign * 64 * 2 ** S))
                assert float(nxt) == float(acc) + sign * 64 * 2 ** S
                acc = nxt
            assert 2 ** 23 <= float(acc) < 2 ** 24


def test_gpu_family_holds_the_extremes():
    """The GPU test's descriptor family (test_knn_keys_gpu.key_extremes) is what its docstring says."""
    import line_match_cases as L
    import test_knn_keys_gpu as K
    key_extremes, cases, OPEN = K.key_extremes, K.cases, K.OPEN
    q, t = key_extremes(2, 2)
    assert L.distances(q, t, 1).tolist() == [[0, 256], [256, 0]] and L.distances(q, t, 2).tolist() == [[0, 128], [128, 0]]
    q, t = key_extremes(65, 64)
    for cell, far in ((1, 256), (2, 128)):
        D = L.distances(q, t, cell)
        assert D[0, 63] == far and D[64, 0] == far and D[0, 0] == 0 and D[64, 63] == 0
        lr, d0, d1, rl = L.knn(D, q, t, cell)
        assert (lr[0], d0[0], d1[0]) == (0, 0, 0) and D[0, 61] == 0          # tie 0 / nt - 3 -> 0
        assert lr[2] == 1 and d0[2] == d1[2] == 4 and D[2, 62] == 4          # tie 1 / nt - 2 -> 1
        assert rl[0] == 0 and D[63, 0] == 0                                  # reverse tie 0 / nq - 2 -> 0
    c0, c1 = cases([(65, 64)], "planted")[0], cases([(65, 64)], OPEN)[0]
    s0, s1 = {tuple(p) for p in c0.stereo(1).tolist()}, {tuple(p) for p in c1.stereo(1).tolist()}
    assert (0, 0) not in s0 and (2, 1) not in s0 and {(0, 0), (2, 1)} <= s1   # ties show under the open threshold only
