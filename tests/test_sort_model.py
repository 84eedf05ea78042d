"""tests/sort_model.py before it judges anything (no GPU): every model against a naive loop over Python integers, on tiny seeded inputs
(n <= 200, widths 1 .. 16 and a few wide ones, bits outside the sorted range filled at random)."""
import numpy as np
import pytest

import sort_model as M


def naive_stable_order(keys, lo, hi):
    """insertion sort over Python integers: an element moves left only past strictly larger fields, so equal fields keep their order"""
    mask = (1 << max(hi - lo, 0)) - 1
    f = [(int(k) >> lo) & mask for k in keys]
    order = []
    for i in range(len(f)):
        j = len(order)
        while j > 0 and f[order[j - 1]] > f[i]:
            j -= 1
        order.insert(j, i)
    return order


def naive_sort(keys, vals, lo, hi):
    order = naive_stable_order(keys, lo, hi)
    return [int(keys[i]) for i in order], [int(vals[i]) for i in order]


def cases(seed, count=36):
    """(keys, vals, lo, hi): widths 1 .. 16 at every kind of offset, then some wide ranges; few distinct fields in a third of the cases"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(count):
        n = int(rng.integers(1, 201))
        w = c % 16 + 1 if c < 32 else (33, 40, 57, 64)[c - 32]
        lo = int(rng.integers(0, 64 - w + 1))
        keys = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
        if c % 3 == 0:  # ties: the field takes three values, the bits around it stay random
            hole = np.uint64(~(((1 << w) - 1) << lo) & 0xFFFFFFFFFFFFFFFF)
            keys = (keys & hole) | (rng.integers(0, min(3, 1 << w), size=n).astype(np.uint64) << np.uint64(lo))
        vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint32) if c % 2 else np.arange(n, dtype=np.uint32)
        out.append((keys, vals, lo, lo + w))
    return out


def test_sort_pairs_model_against_a_naive_loop():
    for keys, vals, lo, hi in cases(1):
        k, v = M.sort_pairs_model(keys, vals, lo, hi)
        wk, wv = naive_sort(keys, vals, lo, hi)
        assert k.dtype == np.uint64 and v.dtype == np.uint32
        assert k.tolist() == wk and v.tolist() == wv, (len(keys), lo, hi)


def test_bits_outside_the_range_travel_but_do_not_order():
    rng = np.random.default_rng(2)
    for keys, vals, lo, hi in cases(3, count=32):
        inside = np.uint64(((1 << (hi - lo)) - 1) << lo)
        other = (keys & inside) | (rng.integers(0, 1 << 63, size=len(keys), dtype=np.uint64) * np.uint64(2) & ~inside)
        assert np.array_equal(M.stable_order(keys, lo, hi), M.stable_order(other, lo, hi))
        k, _ = M.sort_pairs_model(keys, vals, lo, hi)
        assert sorted(k.tolist()) == sorted(keys.tolist())  # whole keys come back, not their fields


def test_empty_range_moves_nothing():
    keys = np.array([5, 3, 9, 3], np.uint64)
    vals = np.array([0, 1, 2, 3], np.uint32)
    for lo, hi in ((0, 0), (7, 7), (9, 3)):
        k, v = M.sort_pairs_model(keys, vals, lo, hi)
        assert k.tolist() == keys.tolist() and v.tolist() == vals.tolist()


def test_local_sort_model_against_a_naive_loop():
    for keys, vals, lo, hi in cases(4, count=24):
        for tile in (1, 7, 64, 200):
            k, v = M.local_sort_model(keys, vals, lo, hi, tile=tile)
            wk, wv = [], []
            for b in range(0, len(keys), tile):
                a, c = naive_sort(keys[b:b + tile], vals[b:b + tile], lo, hi)
                wk += a
                wv += c
            assert k.tolist() == wk and v.tolist() == wv, (len(keys), lo, hi, tile)
    keys = np.arange(M.TILE + 3, 0, -1, dtype=np.uint64)  # the default tile: 8192 pairs, then a short one
    k, v = M.local_sort_model(keys, np.arange(len(keys), dtype=np.uint32), 0, 64)
    assert k.tolist() == list(range(4, M.TILE + 4)) + [1, 2, 3] and v[0] == M.TILE - 1 and v[-1] == M.TILE


def test_sort_groups_model_against_a_naive_loop():
    rng = np.random.default_rng(5)
    for c, (keys, vals, lo, hi) in enumerate(cases(6, count=32)):
        n = len(keys)
        cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 12))))
        starts = [0] + cuts.tolist() + [n if c % 4 else max(n - 3, int(cuts[-1]) if len(cuts) else 0)]  # (now and then the groups stop short of the end)
        above = (0, 1, 2, 5, 40)[c % 5]
        in_place = c % 2 == 0
        kb = keys if in_place else np.full(n, 0xDEADBEEFDEADBEEF, np.uint64)
        vb = vals if in_place else np.full(n, 0xFEEDFACE, np.uint32)
        k, v = M.sort_groups_model(keys, vals, kb, vb, starts, above, lo, hi)
        wk, wv = [int(x) for x in kb], [int(x) for x in vb]
        for a, b in zip(starts[:-1], starts[1:]):
            if b - a > above and b - a <= M.TILE:
                wk[a:b], wv[a:b] = naive_sort(keys[a:b], vals[a:b], lo, hi)
        assert k.tolist() == wk and v.tolist() == wv, (n, starts, above, lo, hi)
    # the upper limit of the class: 8192 members are sorted, 8193 are left alone
    for size, sorted_ in ((M.TILE, True), (M.TILE + 1, False)):
        keys = np.arange(size, 0, -1, dtype=np.uint64)
        k, _ = M.sort_groups_model(keys, np.zeros(size, np.uint32), keys, np.zeros(size, np.uint32), [0, size], 0, 0, 64)
        assert (k[0] == 1) == sorted_


def test_inverse_permutation_model_against_a_naive_loop():
    rng = np.random.default_rng(7)
    for c in range(40):
        n = int(rng.integers(1, 201))
        sa = rng.permutation(n).astype(np.uint32)
        mode = c % 4  # plain | a third marked | all marked | values given, nothing marked
        mv = None if mode == 0 else rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        if mode == 1:
            sa[rng.random(n) < 1 / 3] |= np.uint32(M.MARK)
        if mode == 2:
            sa |= np.uint32(M.MARK)
        want = [None] * n
        for p in range(n):
            s = int(sa[p])
            want[s & 0x7FFFFFFF] = int(mv[p]) if s >> 31 else p
        assert M.inverse_permutation_model(sa, mv).tolist() == want, (n, mode)


def test_inverse_permutation_model_refuses_what_it_cannot_judge():
    with pytest.raises(ValueError):
        M.inverse_permutation_model(np.array([0, 0, 2], np.uint32))
    with pytest.raises(ValueError):
        M.inverse_permutation_model(np.array([0, 3, 1], np.uint32))
    with pytest.raises(ValueError):
        M.inverse_permutation_model(np.array([0, 1 | M.MARK], np.uint32))
