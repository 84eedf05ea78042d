"""tests/lcp_model.py (Kasai over the inverse suffix array) is the yardstick of the GPU LCP tests: pinned here against the definition, byte by
byte, and against known answers.  Suffix arrays come from the oracle's SA-IS (a one-byte input from its direct sort: SA-IS takes none).  No GPU."""
import itertools

import numpy as np

from lcp_model import lcp_brute, lcp_kasai, lcp_kasai_packed


def _sa(orc, t):
    return orc.sa_sais(t) if len(t) > 1 else orc.sa_naive(t)


def test_known_answers(orc):
    for text, sa, lcp in ((b"banana", [5, 3, 1, 0, 4, 2], [0, 1, 3, 0, 0, 2]),
                          (b"mississippi", [10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2], [0, 1, 1, 4, 0, 0, 1, 0, 2, 1, 3])):
        assert _sa(orc, np.frombuffer(text, np.uint8)).tolist() == sa
        assert lcp_kasai(text, sa).tolist() == lcp
        assert lcp_brute(text, sa).tolist() == lcp


def test_every_short_string_over_two_letters(orc):
    for n in range(1, 8):
        for letters in itertools.product(b"ab", repeat=n):
            t = np.array(letters, np.uint8)
            sa = _sa(orc, t)
            assert np.array_equal(lcp_kasai(t, sa), lcp_brute(t, sa)), bytes(letters)


def test_seeded_random_strings(orc):
    rng = np.random.default_rng(41)
    for k in range(200):
        n = int(rng.integers(1, 65))
        t = rng.integers(0, [2, 3, 4, 256][k % 4], size=n, dtype=np.uint8)
        sa = _sa(orc, t)
        assert np.array_equal(lcp_kasai(t, sa), lcp_brute(t, sa)), (k, t.tobytes())


def test_long_repeats_take_the_chunked_extension(orc):
    """a^n, two identical halves and a planted repeat run through _extend (common prefixes of more than 32 bytes): against the definition"""
    rng = np.random.default_rng(43)
    half = rng.integers(0, 256, size=700, dtype=np.uint8)
    for t in (np.full(500, 97, np.uint8), np.concatenate([half, half]), np.concatenate([half[:300], [1], half[:300], [2]]).astype(np.uint8)):
        sa = _sa(orc, t)
        assert np.array_equal(lcp_kasai(t, sa), lcp_brute(t, sa))
    t = np.full(500, 97, np.uint8)
    assert lcp_kasai(t, _sa(orc, t)).tolist() == list(range(500))  # a^n: suffix n-1 first, LCP[i] = i


def test_packed_form_keeps_blocks_apart(orc):
    blocks = [np.frombuffer(b"banana", np.uint8), np.frombuffer(b"banana", np.uint8), np.frombuffer(b"b", np.uint8)]
    got = lcp_kasai_packed(blocks, [_sa(orc, b) for b in blocks])
    assert [g.tolist() for g in got] == [[0, 1, 3, 0, 0, 2], [0, 1, 3, 0, 0, 2], [0]]
