"""Pins the plain models of tests/sa_query_model.py against the definitions, without a GPU: the check against "equals the sorted suffixes" for every
permutation of every short text, the search against brute-force occurrence lists."""
import itertools

import numpy as np

from sa_query_model import (BAD_ORDER, BAD_RANGE, NOT_PERMUTATION, OK, check_model, occurrences, search_model, suffix_array_plain)

# src/saca.rs:411-412
KNOWN = ((b"abracadabra", [10, 7, 0, 3, 5, 8, 1, 4, 6, 9, 2]), (b"banana", [5, 3, 1, 0, 4, 2]))


def test_check_model_on_every_permutation_of_every_short_text():
    """texts up to length 6 over `ab`: the model says OK for exactly one permutation, the sorted suffixes, and BAD_ORDER for every other one"""
    cases = 0
    for n in range(1, 7):
        for letters in itertools.product(b"ab", repeat=n):
            t = bytes(letters)
            want = sorted(range(n), key=lambda i: t[i:])
            for perm in itertools.permutations(range(n)):
                verdict, where = check_model(t, perm)
                if list(perm) == want:
                    assert (verdict, where) == (OK, n), (t, perm)
                else:
                    assert verdict == BAD_ORDER and 1 <= where < n, (t, perm, verdict, where)
                cases += 1
    assert cases == sum(2 ** n * len(list(itertools.permutations(range(n)))) for n in range(1, 7))


def test_check_model_kinds_and_their_order():
    t = b"abracadabra"
    sa = KNOWN[0][1]
    assert check_model(t, sa) == (OK, 11)
    assert check_model(b"banana", KNOWN[1][1]) == (OK, 6)
    for slot in (0, 5, 10):
        bad = list(sa)
        bad[slot] = 11
        assert check_model(t, bad) == (BAD_RANGE, slot)
    bad = list(sa)
    bad[3] = bad[8]  # position 3 is gone, 4 is named twice
    assert check_model(t, bad) == (NOT_PERMUTATION, 3)
    bad[9] = 99      # the range comes first
    assert check_model(t, bad) == (BAD_RANGE, 9)
    assert check_model(b"aa", [0, 1]) == (BAD_ORDER, 1)  # the end rule: "a" sorts in front of "aa"
    assert check_model(b"aa", [1, 0]) == (OK, 2)
    assert check_model(b"a", [0]) == (OK, 1)


def test_check_model_on_random_texts():
    rng = np.random.default_rng(1)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        t = rng.integers(0, int(rng.choice([1, 2, 3, 256])), size=n, dtype=np.uint8)
        sa = suffix_array_plain(t)
        assert check_model(t, sa) == (OK, n)
        perm = rng.permutation(n)
        want = OK if np.array_equal(perm, sa) else BAD_ORDER
        assert check_model(t, perm)[0] == want


def test_search_model_against_occurrence_lists():
    rng = np.random.default_rng(2)
    for _ in range(60):
        n = int(rng.integers(1, 60))
        sigma = int(rng.choice([1, 2, 3]))
        t = rng.integers(97, 97 + sigma, size=n, dtype=np.uint8)
        sa = suffix_array_plain(t)
        pats = [b""]
        for _ in range(25):
            m = int(rng.integers(1, 8))
            pats.append(bytes(rng.integers(97, 98 + sigma, size=m, dtype=np.uint8)))  # one letter above the text's too
            a = int(rng.integers(0, n))
            pats.append(bytes(t[a:a + m]))
        for p, (lo, hi) in zip(pats, search_model(t, sa, pats)):
            assert sorted(int(v) for v in sa[lo:hi]) == occurrences(t, p), (bytes(t), p)
            cut = [bytes(t[v:v + len(p)]) for v in sa]
            assert all(c < p for c in cut[:lo]) and all(c > p for c in cut[hi:]), (bytes(t), p)


def test_search_model_known_answers():
    for t, sa in KNOWN:
        assert suffix_array_plain(t).tolist() == sa
    t, sa = KNOWN[0]
    got = search_model(t, sa, [b"abra", b"a", b"", b"abracadabra", b"abracadabraa", b"b", b"zz", b"\x00", b"ac", b"ab"])
    assert got == [(1, 3), (0, 5), (0, 11), (2, 3), (3, 3), (5, 7), (11, 11), (0, 0), (3, 4), (1, 3)]
    assert search_model(b"abab", suffix_array_plain(b"abab"), [b"aba", b"ab", b"b", b"bab", b"abab", b"ababa"]) == [(1, 2), (0, 2), (2, 4), (3, 4), (1, 2), (2, 2)]
