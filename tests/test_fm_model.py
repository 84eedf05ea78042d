"""tests/fm_model.py against the definitions: search_model and occurrences of tests/sa_query_model.py.  No GPU, no library."""
import itertools

import numpy as np

from fm_model import bwt_plain, fm_model, fm_model_packed, fm_model_plain, rank_model
from sa_query_model import occurrences, search_model, suffix_array_plain


def words(alphabet, lengths):
    return [bytes(w) for m in lengths for w in itertools.product(alphabet, repeat=m)]


PATTERNS = words(b"abc", range(0, 5))


def agree(text, patterns):
    L, origin = bwt_plain(text)
    want = search_model(text, suffix_array_plain(text), patterns)
    assert fm_model_plain(L, origin, patterns) == want, text
    assert fm_model(L, origin, patterns) == want, text
    return want


def test_every_short_text_over_two_letters():
    for t in words(b"ab", range(1, 8)):
        want = agree(t, PATTERNS)
        for p, (lo, hi) in zip(PATTERNS[:40], want[:40]):
            assert hi - lo == len(occurrences(t, p))


def test_texts_with_the_lowest_and_highest_bytes():
    rng = np.random.default_rng(5)
    alphabet = np.array([0, 1, 2, 254, 255], np.uint8)
    pats = words(bytes(alphabet), range(0, 3)) + [b"\x00" * 5, b"\xff" * 5]
    for _ in range(60):
        t = bytes(alphabet[rng.integers(0, 5, size=int(rng.integers(1, 40)))])
        agree(t, pats + [t, t[1:], t[:-1], t + b"\x00", t + b"\xff"])


def test_the_known_array():
    t = b"abracadabra"  # src/saca.rs:411
    L, origin = bwt_plain(t)
    assert bytes(L) == b"rdarcaaaabb" and origin == 2
    assert suffix_array_plain(t).tolist() == [10, 7, 0, 3, 5, 8, 1, 4, 6, 9, 2]
    pats = [b"abra", b"a", b"", t, t + b"a", b"b", b"zz", b"\x00", b"ac", b"ra", b"bra", b"cad"]
    want = agree(t, pats)
    assert want[0] == (1, 3) and want[1] == (0, 5) and want[2] == (0, 11)


def test_arbitrary_l_stays_in_range_and_both_models_agree():
    rng = np.random.default_rng(6)
    for k in (2, 3, 256):
        L = rng.integers(0, k, size=300, dtype=np.uint8)
        pats = [rng.integers(0, k, size=int(rng.integers(0, 6)), dtype=np.uint8) for _ in range(200)]
        for origin in (0, 299, int(rng.integers(0, 300))):
            got = fm_model(L, origin, pats)
            assert got == fm_model_plain(L, origin, pats)
            assert all(lo <= hi <= 300 for lo, hi in got)


def test_packed_and_rank():
    texts = [b"banana", b"a", b"abracadabra", b"banana"]
    pairs = [bwt_plain(t) for t in texts]
    pats, blocks = [b"ana", b"a", b"bra", b"nan", b""], [3, 1, 2, 0, 1]
    got = fm_model_packed([p[0] for p in pairs], [p[1] for p in pairs], pats, blocks)
    assert got == [search_model(texts[b], suffix_array_plain(texts[b]), [p])[0] for p, b in zip(pats, blocks)]
    r = rank_model(b"abca", [97, 98])
    assert r[97].tolist() == [0, 1, 1, 1, 2] and r[98].tolist() == [0, 0, 1, 1, 1]
