"""tests/fm_find_model.py against enumeration with bytes.find and against tests/fm_model.py: every text of 1 .. 6 bytes over {a, b} with every
pattern of 0 .. 3 bytes over {a, b, c}."""
import itertools

import numpy as np

from fm_find_model import HIT_DTYPE, block_structures, find_model
from fm_model import fm_model


def words(alphabet, lengths):
    return [bytes(w) for m in lengths for w in itertools.product(alphabet, repeat=m)]


def found(t, p):
    """every position of p in t, overlapping ones included, by bytes.find"""
    out, i = [], t.find(p)
    while i >= 0 and i < len(t):
        out.append(i)
        i = t.find(p, i + 1)
    return out


def test_every_short_text_and_pattern():
    texts, pats = words(b"ab", range(1, 7)), words(b"abc", range(0, 4))
    assert len(texts) == 126 and len(pats) == 40
    occ, recs, total = find_model(texts, pats)
    assert occ.shape == (40, 126) and occ.dtype == np.uint32 and recs.dtype == HIT_DTYPE and recs.dtype.itemsize == 16
    assert total == len(recs) == int(occ.sum())
    keys = list(zip(recs["pattern"].tolist(), recs["block"].tolist(), recs["slot"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    at = 0
    for q, p in enumerate(pats):
        for b, t in enumerate(texts):
            sa, L, origin = block_structures(t)
            lo, hi = fm_model(L, origin, [p])[0]
            want = found(t, p)
            assert occ[q, b] == len(want) == hi - lo, (p, t)
            mine = recs[at:at + len(want)]
            at += len(want)
            assert (mine["pattern"] == q).all() and (mine["block"] == b).all()
            assert mine["slot"].tolist() == list(range(lo, hi))
            assert mine["position"].tolist() == [sa[x] for x in range(lo, hi)] and sorted(mine["position"].tolist()) == want
    assert at == total


def test_no_patterns_and_absent_ones():
    occ, recs, total = find_model([b"abab"], [])
    assert occ.shape == (0, 1) and len(recs) == 0 and total == 0
    occ, recs, total = find_model([b"abab", b"b"], [b"c", b"abc"])
    assert not occ.any() and len(recs) == 0 and total == 0
    occ, recs, total = find_model([b"abab", b"b"], [b"", b"b"])
    assert occ.tolist() == [[4, 1], [2, 1]] and total == 8
    assert recs.tolist() == [(0, 0, 2, 0), (0, 0, 0, 1), (0, 0, 3, 2), (0, 0, 1, 3), (0, 1, 0, 0), (1, 0, 3, 2), (1, 0, 1, 3), (1, 1, 0, 0)]
