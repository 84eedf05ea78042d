"""tests/sa_match_model.py against the definitions of include/dark_amd.h, by brute force on small inputs (no GPU): the length of every position
against `in`, the range against the list of occurrences, the super-maximal matches against "contained in no other match of the query", and
the capped rule on a copy longer than max_len."""
import random

import pytest

from sa_match_model import common_prefix, match_model, smem_records, smems_model
from sa_query_model import occurrences, suffix_array_plain


def cases(seed, count):
    rng = random.Random(seed)
    for it in range(count):
        sigma = rng.choice([1, 2, 3, 4])
        t = bytes(rng.randrange(sigma) for _ in range(rng.randint(1, 40)))
        q = bytes(rng.randrange(sigma + (it & 1)) for _ in range(rng.randint(1, 30)))  # every second query: a byte the text lacks
        yield t, q


def test_common_prefix():
    assert [common_prefix(a, b) for a, b in ((b"", b"a"), (b"abc", b"abd"), (b"abc", b"abc"), (b"abc", b"abcd"), (b"x", b"y"))] == [0, 2, 3, 3, 0]


@pytest.mark.parametrize("max_len", [1, 3, 1000])
def test_lengths_and_ranges_are_the_definition(max_len):
    for t, q in cases(1, 400):
        sa = suffix_array_plain(t)
        rows = match_model(t, sa, [q], max_len)[0]
        assert len(rows) == len(q)
        for i, (ln, lo, hi) in enumerate(rows):
            m = min(max_len, len(q) - i)
            want = 0
            while want < m and q[i:i + want + 1] in t:
                want += 1
            assert ln == want, (t, q, i)
            assert sorted(int(v) for v in sa[lo:hi]) == occurrences(t, q[i:i + ln]) and hi > lo, (t, q, i, ln, lo, hi)


def test_several_queries_do_not_run_into_each_other():
    t = b"abcdefgh"
    sa = suffix_array_plain(t)
    rows = match_model(t, sa, [b"xabc", b"", b"defz", b"h"], 100)
    assert [[r[0] for r in q] for q in rows] == [[0, 3, 2, 1], [], [3, 2, 1, 0], [1]]  # "abc" + "def" is in the text: no match crosses the border


@pytest.mark.parametrize("min_len", [0, 1, 2, 3])
def test_smems_are_the_matches_no_other_match_contains(min_len):
    for t, q in cases(2, 400):
        sa = suffix_array_plain(t)
        lens = [r[0] for r in match_model(t, sa, [q], 1000)[0]]
        assert all(lens[i - 1] <= lens[i] + 1 for i in range(1, len(lens)))
        matches = {(i, ln) for i in range(len(q)) for ln in range(1, len(q) - i + 1) if q[i:i + ln] in t}
        # (i, l) is inside another match exactly when it can be extended by one byte to the right or to the left
        want = sorted((i, ln) for i, ln in matches if (i, ln + 1) not in matches and (i - 1, ln + 1) not in matches and ln >= max(min_len, 1))
        assert smems_model([lens], min_len, 1000) == want, (t, q)


def test_two_queries_count_positions_back_to_back():
    assert smems_model([[2, 1, 0], [], [1, 3, 2]], 0, 100) == [(0, 2), (3, 1), (4, 3)]
    assert smems_model([[2, 1, 0], [], [1, 3, 2]], 2, 100) == [(0, 2), (4, 3)]
    assert smems_model([[3, 3], [3, 3]], 0, 3) == [(0, 3), (2, 3)]  # the cap's rule looks back inside its own query only


def test_a_copy_longer_than_the_cap_is_reported_once():
    t = b"zzz" + bytes(range(40)) + b"zzz"
    sa = suffix_array_plain(t)
    q = b"\xff" + bytes(range(40)) + b"\xff"
    recs = smem_records(t, sa, [q], 0, 8)
    # positions 1 .. 33 are all at the cap: one record; from 34 on the match shrinks with the copy's end and is contained in its predecessor
    assert [(at, ln) for at, ln, _, _ in recs] == [(1, 8)]
    lo, hi = recs[0][2:]
    assert [int(v) for v in sa[lo:hi]] == [3]
    assert [(at, ln) for at, ln, _, _ in smem_records(t, sa, [q], 0, 1000)] == [(1, 40)]
    assert smem_records(t, sa, [q], 9, 8) == []
