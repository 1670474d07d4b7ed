"""Inputs of the landmark descriptor store's tests: the generator of near-duplicate observations,
the hand-built lists with their worked answers, and the adversarial op lists of the planner.

The generator draws a random base descriptor per landmark and flips 0-5 random bits of it per
observation, as repeated ORB / LBD observations of one feature differ: the distances are small
integers, so equal medians are common and the winner is often not observation 0.  A test that
uses the generator first calls assert_adversarial(), which checks both on the reference alone.
"""
import numpy as np

import lm_store_ref as R

LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)   # the bucket edges of k_lm_apply<G> and their neighbours
TIE_MIN, MOVED_MIN = 0.20, 0.35                       # the generator's bar, per n >= 3
STAT_LANDMARKS = 200                                  # per n up to 16; 3200 / n beyond (the cost grows with n^2, and from
                                                      # n = 17 on the least measured rates are 0.84 and 0.68 against bars of 0.20 and 0.35)
MAX_LEN = 64


def near_duplicates(rng, n: int) -> np.ndarray:
    """[n][32] observations of one landmark: a random base with 0-5 random bits flipped in each."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    flips = rng.integers(0, 6, n)                                    # bits to flip per observation
    where = rng.random((n, 256)).argpartition(5, axis=1)[:, :5]      # five distinct bit positions each
    mask = np.zeros((n, 256), np.uint8)
    for j in range(5):
        rows = np.nonzero(flips > j)[0]
        mask[rows, where[rows, j]] = 1
    return base[None, :] ^ np.packbits(mask, axis=1, bitorder="little")


def generator_stats(n: int, landmarks: int = 0, seed: int = 7):
    """(fraction of landmarks with two or more rows at the winning median, fraction whose winner
    is not observation 0), from the reference alone."""
    landmarks = landmarks or min(STAT_LANDMARKS, 3200 // n)
    rng = np.random.default_rng([seed, n])
    tie = moved = 0
    for _ in range(landmarks):
        idx, at_min = R.winner_stats(list(near_duplicates(rng, n)))
        tie += at_min >= 2
        moved += idx != 0
    return tie / landmarks, moved / landmarks


_checked = {}


def assert_adversarial(lengths=range(3, MAX_LEN + 1)):
    """The generator's bar at every list length the tests reach: they grow lists one observation at
    a time up to MAX_LEN and compare at each length, so that is every n from 3 on."""
    for n in lengths:
        if n < 3:
            continue
        if n not in _checked:
            _checked[n] = generator_stats(n)
        tie, moved = _checked[n]
        assert tie >= TIE_MIN, (n, tie)
        assert moved >= MOVED_MIN, (n, moved)
    worst = [min(v[k] for n, v in _checked.items() if n in lengths) for k in (0, 1)]
    print(f"lm generator, n in {lengths}: least tie fraction {worst[0]:.3f}, least moved fraction {worst[1]:.3f}")


def prefix(p: int) -> np.ndarray:
    """The 32-byte row whose first p bits are set: hamming(prefix(p), prefix(q)) = |p - q|."""
    bits = np.zeros(256, np.uint8)
    bits[:p] = 1
    return np.packbits(bits, bitorder="little")


# (name, prefix lengths of the observations, max_idx) — worked by hand:
#  n = 3 takes element 2 of a sorted row (its largest), n = 4 element 2 (the third smallest, 0 included)
WRITTEN = [
    ("one", [7], 0),
    ("two", [0, 9], 0),                 # both rows are [0, 9]: medians 9, 9, the first wins
    ("identical", [5, 5, 5, 5, 5], 0),
    # distances 10, 5, 5: rows [0,5,10] [0,5,10] [0,5,5] -> medians 10, 10, 5
    ("n3_last", [0, 10, 5], 2),
    # rows [0,12,14,30] [0,16,18,30] [0,2,14,16] [0,2,12,18] -> medians 14, 18, 14, 12
    ("n4_last", [0, 30, 14, 12], 3),
    # rows [0,10,12,22] [0,2,10,12] [0,2,10,12] [0,10,12,22] -> medians 12, 10, 10, 12: rows 1 and 2 tie
    ("tie_smaller_index", [0, 10, 12, 22], 1),
    # n = 5 takes element 3: rows [0,1,2,3,4] [0,1,1,2,3] [0,1,1,2,2] [0,1,1,2,3] [0,1,2,3,4] -> 3, 2, 2, 2, 3
    ("n5_tie", [0, 1, 2, 3, 4], 1),
]


def written_lists():
    return [(name, [prefix(p) for p in ps], idx) for name, ps, idx in WRITTEN]


def planner_lists(lm_cap: int, obs_cap: int, src_rows):
    """Op lists for the planner, good and bad, as (name, ops [n][4]); counts start at zero."""
    A, E, F = R.ADD, R.ERASE_OBS, R.FREE
    big = 2 ** 31 - 1
    fill = [(3, A, k % src_rows[0], 0) for k in range(obs_cap)]
    rng = np.random.default_rng(11)
    mixed = []
    cnt = [0] * lm_cap
    for _ in range(4000):
        lm = int(rng.integers(0, lm_cap))
        kind = int(rng.integers(0, 8))
        if kind < 5 and cnt[lm] < obs_cap:
            src = int(rng.integers(0, len(src_rows)))
            mixed.append((lm, A, int(rng.integers(0, src_rows[src])), src))
            cnt[lm] += 1
        elif kind < 7 and cnt[lm] > 0:
            mixed.append((lm, E, int(rng.integers(0, cnt[lm])), -5))
            cnt[lm] -= 1
        else:
            mixed.append((lm, F, big, big))
            cnt[lm] = 0
    # landmark k grows to LENGTHS[k], one observation per round: every bucket, the ops interleaved
    ladder = [(k, A, step % src_rows[0], 0) for step in range(max(LENGTHS)) for k, n in enumerate(LENGTHS)
              if step < n and k < lm_cap]
    return [
        ("empty", []),
        ("ladder", ladder),
        ("fill", fill),
        ("over", fill + [(3, A, 0, 0)]),
        ("free_empty_twice", [(0, F, 0, 0), (0, F, 0, 0)]),
        ("add_erase_add", [(1, A, 0, 0), (1, A, 1, 0), (1, E, 0, 0), (1, A, 2, 0)]),
        ("erase_empty", [(2, E, 0, 0)]),
        ("erase_at_count", [(2, A, 0, 0), (2, E, 1, 0)]),
        ("erase_negative", [(2, A, 0, 0), (2, E, -1, 0)]),
        ("erase_after_free", [(2, A, 0, 0), (2, F, 0, 0), (2, E, 0, 0)]),
        ("lm_negative", [(-1, A, 0, 0)]),
        ("lm_cap", [(lm_cap, A, 0, 0)]),
        ("lm_huge", [(big, F, 0, 0), (-big - 1, F, 0, 0)]),
        ("kind_unknown", [(0, 3, 0, 0)]),
        ("kind_negative", [(0, -1, 0, 0)]),
        ("src_negative", [(0, A, 0, -1)]),
        ("src_past", [(0, A, 0, len(src_rows))]),
        ("src_huge", [(0, A, 0, big)]),
        ("row_negative", [(0, A, -1, 0)]),
        ("row_past", [(0, A, src_rows[0], 0)]),
        ("row_huge", [(0, A, big, 0)]),
        ("bad_after_good", [(5, A, 0, 0), (6, A, 1, 0), (5, E, 0, 0), (6, E, 5, 0)]),
        ("capacity_before_invalid", fill + [(3, A, 0, 0), (-1, A, 0, 0)]),
        ("invalid_before_capacity", fill + [(-1, A, 0, 0), (3, A, 0, 0)]),
        ("mixed", mixed),
    ]
