"""The landmark descriptor store's reference: the descriptor half of MapPoint / MapLine::
updateAverageDescDir (src/mapFeatures.cpp:50-84, 120-154) restated line by line in numpy, and a
list-of-lists model of the ops of include/gfpl.h (GFPL_LM_ADD / _ERASE_OBS / _FREE).
"""
import numpy as np

ADD, ERASE_OBS, FREE = 0, 1, 2
OK, E_INVALID, E_CAPACITY = 0, -1, -5
MAX_OBS = 64

_bits = int.bit_count if hasattr(int, "bit_count") else (lambda v: bin(v).count("1"))


def _as_int(row) -> int:
    return int.from_bytes(np.asarray(row, np.uint8).tobytes(), "little")


def hamming(a, b) -> int:
    """cv::norm(a, b, NORM_HAMMING) of two 32-byte rows: the set bits of their xor."""
    return _bits(_as_int(a) ^ _as_int(b))


def row_medians(desc_list):
    """Per observation i the value `idx_median` of the reference's loop (:71-77); n >= 2."""
    n = len(desc_list)
    as_int = [_as_int(d) for d in desc_list]           # (the 256 bits of a row as one Python integer)
    dist = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            d = _bits(as_int[i] ^ as_int[j])           # int d = norm(desc_list[i], desc_list[j], NORM_HAMMING)
            dist[i][j] = d
            dist[j][i] = d
    # MatrixXf conf_desc(n, n): every d is stored as a float and read back with int(conf_desc(i, j)).
    # The whole matrix goes through float32 at once here (element by element it took most of the
    # tests' time); the conversion of each element is the same.
    conf_desc = np.array(dist, np.float32)
    back = conf_desc.astype(np.int64).tolist()
    out = []
    for i in range(n):
        dist_idx = [back[i][j] for j in range(n)]
        dist_idx.sort()
        out.append(dist_idx[int(1 + 0.5 * (n - 1))])
    return out


def med_index(desc_list) -> int:
    """max_idx of updateAverageDescDir.  n = 1: the reference reads dist_idx[1] of a one-element
    vector; whatever that read gives, max_idx stays 0 (ledger LM4).  n = 0: -1 (no landmark)."""
    n = len(desc_list)
    if n == 0:
        return -1
    if n == 1:
        return 0
    max_dist, max_idx = 99999, 0
    for i, idx_median in enumerate(row_medians(desc_list)):
        if idx_median < max_dist:
            max_dist = idx_median
            max_idx = i
    return max_idx


def winner_stats(desc_list):
    """(max_idx, number of rows whose median equals the winning median); n >= 2."""
    med = row_medians(desc_list)
    return med.index(min(med)), sum(1 for m in med if m == min(med))   # LM3: the first row of least median


class Model:
    """desc_list of every landmark as a Python list of 32-byte rows."""

    def __init__(self, lm_cap: int, obs_cap: int):
        self.lm_cap, self.obs_cap = lm_cap, obs_cap
        self.lists = [[] for _ in range(lm_cap)]

    def counts(self):
        return np.array([len(l) for l in self.lists], np.int32)

    def check(self, ops, src_rows, counts=None):
        """(code, counts after) of an op list: the rules of gfpl_lm_ops_check, first failing op decides."""
        cnt = list(self.counts() if counts is None else counts)
        before = np.array(cnt, np.int32)
        for lm, kind, arg, src in np.asarray(ops, np.int64).reshape(-1, 4):
            if not 0 <= lm < self.lm_cap:
                return E_INVALID, before
            if kind == ADD:
                if not 0 <= src < len(src_rows) or not 0 <= arg < src_rows[src]:
                    return E_INVALID, before
                if cnt[lm] >= self.obs_cap:
                    return E_CAPACITY, before
                cnt[lm] += 1
            elif kind == ERASE_OBS:
                if not 0 <= arg < cnt[lm]:
                    return E_INVALID, before
                cnt[lm] -= 1
            elif kind == FREE:
                cnt[lm] = 0
            else:
                return E_INVALID, before
        return OK, np.array(cnt, np.int32)

    def apply(self, ops, srcs):
        """The ops in array order (a valid list); returns the landmarks named."""
        touched = {}
        for lm, kind, arg, src in np.asarray(ops, np.int64).reshape(-1, 4).tolist():
            touched[lm] = True
            if kind == ADD:
                self.lists[lm].append(np.array(srcs[src][arg], np.uint8))   # desc_list.push_back
            elif kind == ERASE_OBS:
                del self.lists[lm][arg]                                      # desc_list.erase(begin() + arg)
            else:
                self.lists[lm] = []
        return list(touched)   # in first-touch order

    def expect(self, lm):
        """count, med_idx, the list rows and med_desc the store must hold for a landmark."""
        l = self.lists[lm]
        mi = med_index(l)
        rows = np.array(l, np.uint8).reshape(-1, 32)
        med = rows[mi].copy() if mi >= 0 else np.zeros(32, np.uint8)
        return dict(count=len(l), med_idx=mi, rows=rows, med_desc=med)
