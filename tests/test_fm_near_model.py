"""tests/fm_near_model.py against an independent enumeration, against tests/fm_find_model.py, on the order of the answer and on the node limit:
every text of 1 .. 6 bytes over {a, b} with every pattern of 0 .. 3 bytes over {a, b, c}, k = 0 .. 3."""
import itertools

import numpy as np
import pytest

from fm_find_model import find_model
from fm_locate_model import sa_plain
from fm_near_model import NEAR_HIT_DTYPE, class_masks, costs, exact_classes, near_model

TEXTS = [bytes(w) for m in range(1, 7) for w in itertools.product(b"ab", repeat=m)]
PATS = [bytes(w) for m in range(0, 4) for w in itertools.product(b"abc", repeat=m)]


def hamming(t, p, at):
    return sum(1 for i in range(len(p)) if t[at + i] != p[i])


def pair_records(recs, q, b):
    return recs[(recs["pattern"] == q) & (recs["block"] == b)]


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_a_position_is_a_hit_iff_its_cost_is_at_most_k(k):
    assert len(TEXTS) == 126 and len(PATS) == 40
    occ, recs, total, cut, nodes = near_model(TEXTS, [exact_classes(p) for p in PATS], k)
    assert occ.shape == (40, 126) and recs.dtype == NEAR_HIT_DTYPE and recs.dtype.itemsize == 16 and cut == 0
    assert total == len(recs) == int(occ.sum()) and (nodes >= 1).all()
    at = 0
    for q, p in enumerate(PATS):
        for b, t in enumerate(TEXTS):
            if len(p) == 0:
                want = {(i, 0) for i in range(len(t))}  # the empty pattern stands at every position, as in find
            else:
                want = {(i, hamming(t, p, i)) for i in range(len(t) - len(p) + 1) if hamming(t, p, i) <= k}
            mine = recs[at:at + int(occ[q, b])]
            at += int(occ[q, b])
            assert (mine["pattern"] == q).all() and (mine["block"] == b).all()
            got = list(zip(mine["position"].tolist(), mine["cost"].tolist()))
            assert len(set(got)) == len(got) and set(got) == want, (p, t, k)
    assert at == total


def test_k_0_with_one_bit_classes_is_find():
    occ, recs, total, _, _ = near_model(TEXTS, [exact_classes(p) for p in PATS], 0)
    f_occ, f_recs, f_total = find_model(TEXTS, PATS)
    assert total == f_total and np.array_equal(occ, f_occ) and not recs["cost"].any()
    # (inside a pair both list the one leaf's slots in suffix order: the lists are equal, not only the sets)
    for name in ("pattern", "block", "position"):
        assert np.array_equal(recs[name], f_recs[name]), name


@pytest.mark.parametrize("k", [1, 2])
def test_order_is_the_reversed_matched_string_then_the_rank(k):
    texts = TEXTS[-40:] + [b"abracadabra", b"mississippi"]
    pats = [b"ab", b"aba", b"bab", b"issi", b"abra", b"a"]
    _, recs, _, _, _ = near_model(texts, [exact_classes(p) for p in pats], k)
    for b, t in enumerate(texts):
        sa = sa_plain(t)
        rank = {i: slot for slot, i in enumerate(sa)}
        for q, p in enumerate(pats):
            mine = pair_records(recs, q, b)["position"].tolist()
            assert mine == sorted(mine, key=lambda i: (t[i:i + len(p)][::-1], rank[i])), (t, p)


def test_costs_and_classes():
    masks = class_masks(exact_classes(b"a\x00\xff"))
    assert masks == [1 << 97, 1, 1 << 255]
    assert costs(b"a\x00\xffb\x00\xff", masks) == [0, 3, 3, 1]
    assert costs(b"ab", masks) == []
    wild = exact_classes(b"a?")
    wild[1] = 0xFF
    occ, recs, total, _, _ = near_model([b"abaa"], [wild], 0)
    assert total == 2 and sorted(recs["position"].tolist()) == [0, 2] and not recs["cost"].any()
    none = exact_classes(b"ab")
    none[0] = 0  # an empty class never matches for free
    assert near_model([b"abab"], [none], 0)[2] == 0
    occ, recs, total, _, _ = near_model([b"abab"], [none], 1)
    assert sorted(recs["position"].tolist()) == [0, 2] and (recs["cost"] == 1).all()


def test_the_limit_gives_a_prefix_and_says_when_it_cut():
    cases = [(b"abracadabra", b"abra", 2), (b"mississippi", b"issi", 1), (b"ababababab", b"aba", 3), (b"aaaa", b"", 0), (b"abcabc", b"cab", 1)]
    for t, p, k in cases:
        cls = [exact_classes(p)]
        _, whole, total, cut, nodes = near_model([t], cls, k)
        N = int(nodes[0, 0])
        assert cut == 0 and N >= 1
        lengths = []
        for limit in range(1, N + 2):
            occ, recs, part, cut, n2 = near_model([t], cls, k, limit)
            assert int(n2[0, 0]) == N and cut == (1 if limit < N else 0), (t, p, limit)
            assert part == len(recs) == int(occ[0, 0]) and np.array_equal(recs, whole[:part]), (t, p, limit)
            lengths.append(part)
        assert lengths == sorted(lengths) and lengths[-1] == lengths[-2] == total
        if len(p):
            assert lengths[0] == 0  # the root alone is no leaf
