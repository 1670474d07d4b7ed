"""Op lists for gfpl_lm_fuse_check / gfpl_lmstore_fuse, good and bad.  Every list starts from empty
landmarks and builds what it needs with ADDs, so it also runs from counts that are not zero (the
tests then start from a first fill that leaves room)."""
import numpy as np

import lm_fuse_ref as FR

A, E, F, M = FR.ADD, FR.ERASE_OBS, FR.FREE, FR.APPEND_LM


def adds(lm, n, src_rows, src=0, first=0):
    return [(lm, A, (first + k) % src_rows[src], src) for k in range(n)]


def random_mixed(lm_cap, obs_cap, src_rows, n_ops, seed, start=None, max_from=4):
    """A valid list of n_ops ops over all landmarks: ADDs, appends and FREEs, no landmark named
    after its FREE."""
    rng = np.random.default_rng(seed)
    cnt = [0] * lm_cap if start is None else [int(c) for c in start]
    freed, ops = set(), []
    for _ in range(20 * n_ops):           # (full lists and short sources turn a draw into nothing)
        if len(ops) >= n_ops:
            break
        alive = [l for l in range(lm_cap) if l not in freed]
        if len(alive) < 4:
            break
        lm = int(rng.choice(alive))
        kind = int(rng.integers(0, 20))
        if kind < 12 or cnt[lm] == 0:
            if cnt[lm] < obs_cap:
                src = int(rng.integers(0, len(src_rows)))
                ops.append((lm, A, int(rng.integers(0, src_rows[src])), src))
                cnt[lm] += 1
        elif kind < 19:
            # short sources only: without re-use of a freed landmark the rows of a call are what fills the store
            short = [l for l in alive if l != lm and 0 < cnt[l] <= max_from and cnt[lm] + cnt[l] <= obs_cap]
            if short:
                arg = int(rng.choice(short))
                ops.append((lm, M, arg, -7))
                cnt[lm] += cnt[arg]
                if kind < 15 and len(alive) > 3 * lm_cap // 4:      # the reference's merge: the source is dropped
                    ops.append((arg, F, 0, 0))
                    cnt[arg] = 0
                    freed.add(arg)
        elif len(alive) > 3 * lm_cap // 4:
            ops.append((lm, F, 0, 0))
            cnt[lm] = 0
            freed.add(lm)
    return ops


def planner_lists(lm_cap: int, obs_cap: int, src_rows):
    """(name, ops [n][4]); lm_cap >= 12, obs_cap >= 6."""
    big = 2 ** 31 - 1
    half = obs_cap // 2
    two = adds(0, 2, src_rows) + adds(1, 3, src_rows, first=2)          # landmark 0 holds 2 rows, landmark 1 holds 3
    full = adds(3, obs_cap - 2, src_rows) + adds(4, 2, src_rows)        # 3 + 4 end exactly at obs_cap
    return [
        ("empty", []),
        ("append", two + [(0, M, 1, big)]),
        ("append_then_free", two + [(0, M, 1, 0), (1, F, 0, 0)]),
        ("append_to_exactly_cap", full + [(3, M, 4, 0)]),
        ("append_one_over", full + adds(4, 1, src_rows) + [(3, M, 4, 0)]),
        ("add_over", adds(3, obs_cap, src_rows) + [(3, A, 0, 0)]),
        ("arg_is_lm", two + [(0, M, 0, 0)]),
        ("arg_negative", two + [(0, M, -1, 0)]),
        ("arg_cap", two + [(0, M, lm_cap, 0)]),
        ("arg_huge", two + [(0, M, big, 0)]),
        ("append_from_empty", two + [(0, M, 2, 0)]),
        ("append_to_empty", two + [(2, M, 0, 0)]),
        ("freed_named_as_lm", two + [(1, F, 0, 0), (1, A, 0, 0)]),
        ("freed_named_as_lm_free", two + [(1, F, 0, 0), (1, F, 0, 0)]),
        ("freed_named_as_lm_append", two + [(1, F, 0, 0), (1, M, 0, 0)]),
        ("freed_named_as_arg", two + [(1, F, 0, 0), (0, M, 1, 0)]),
        ("free_empty_once", [(5, F, 0, 0)]),
        ("erase_obs", two + [(0, E, 0, 0)]),
        ("erase_obs_bad_position", two + [(0, E, 99, 0)]),
        ("kind_unknown", [(0, 4, 0, 0)]),
        ("kind_negative", [(0, -1, 0, 0)]),
        ("lm_negative", [(-1, M, 0, 0)]),
        ("lm_cap", [(lm_cap, M, 0, 0)]),
        ("src_past", [(0, A, 0, len(src_rows))]),
        ("row_past", [(0, A, src_rows[0], 0)]),
        ("capacity_before_invalid", full + adds(4, 1, src_rows) + [(3, M, 4, 0), (0, M, 0, 0)]),
        ("invalid_before_capacity", full + adds(4, 1, src_rows) + [(0, M, 0, 0), (3, M, 4, 0)]),
        ("unsupported_before_invalid", two + [(0, E, 0, 0), (0, M, 0, 0)]),
        # A -> B -> C: landmark 2 receives 1, which received 0
        ("chain", two + adds(2, 1, src_rows, first=5) + [(1, M, 0, 0), (2, M, 1, 0)]),
        ("chain_freed", two + adds(2, 1, src_rows, first=5) + [(1, M, 0, 0), (0, F, 0, 0), (2, M, 1, 0), (1, F, 0, 0)]),
        # a ring, both kept: 6 = [a b], then 7 = [b a b]
        ("ring", adds(6, 1, src_rows) + adds(7, 1, src_rows, first=1) + [(6, M, 7, 0), (7, M, 6, 0)]),
        ("append_after_adds", two + adds(1, 1, src_rows, first=7) + [(0, M, 1, 0)] + adds(1, 1, src_rows, first=8)),
        ("append_twice", adds(8, 1, src_rows) + adds(9, 1, src_rows, first=3) + [(8, M, 9, 0), (8, M, 9, 0)]),
        ("half_and_half", adds(10, half, src_rows) + adds(11, obs_cap - half, src_rows, first=1) + [(10, M, 11, 0)]),
        ("mixed", random_mixed(lm_cap, obs_cap, src_rows, 4000, 17)),
    ]


CODES = {"append_one_over": FR.E_CAPACITY, "add_over": FR.E_CAPACITY, "capacity_before_invalid": FR.E_CAPACITY,
         "erase_obs": FR.E_UNSUPPORTED, "erase_obs_bad_position": FR.E_UNSUPPORTED,
         "unsupported_before_invalid": FR.E_UNSUPPORTED}
INVALID = ("arg_is_lm", "arg_negative", "arg_cap", "arg_huge", "append_from_empty", "append_to_empty", "freed_named_as_lm",
           "freed_named_as_lm_free", "freed_named_as_lm_append", "freed_named_as_arg", "kind_unknown", "kind_negative",
           "lm_negative", "lm_cap", "src_past", "row_past", "invalid_before_capacity")


def expected_code(name):
    """The code of a list run from zero counts, worked by hand."""
    return CODES.get(name, FR.E_INVALID if name in INVALID else FR.OK)
