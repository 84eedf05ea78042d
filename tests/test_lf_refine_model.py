"""tests/lf_refine_model.py, the judge of the second half of tests/test_gpu_lfirst_layer.py, pinned on the CPU: with the true SA positions and the
true symbols in front (tests/sa_query_model.py: the suffix array by plain sorting) the model must reproduce the true BWT at the listed positions
and leave the rest alone; its chunked comparison must be the comparison of whole suffixes."""
import random

import numpy as np
import pytest

import lf_refine_model as M
from sa_query_model import suffix_array_plain


def texts():
    rng = np.random.default_rng(1)
    seg = rng.integers(0, 3, size=300, dtype=np.uint8)
    yield "three symbols", rng.integers(0, 3, size=1500, dtype=np.uint8)
    yield "copies longer than the comparison's chunks", np.concatenate([seg, [9], seg, [7], seg[:200], [0, 0, 0], seg[:130]]).astype(np.uint8)
    yield "a run and its end", np.concatenate([np.full(400, 97), [98], np.full(300, 97)]).astype(np.uint8)
    yield "bytes", rng.integers(0, 256, size=800, dtype=np.uint8)


@pytest.mark.parametrize("name,text", list(texts()))
def test_chunked_comparison_is_the_comparison_of_suffixes(name, text):
    t = bytes(text)
    random.seed(2)
    for _ in range(3000):
        i, j = random.randrange(len(t)), random.randrange(len(t))
        want = -1 if t[i:] < t[j:] else 1 if t[i:] > t[j:] else 0
        assert M.suffix_cmp(t, i, j) == want, (name, i, j)


@pytest.mark.parametrize("name,text", list(texts()))
@pytest.mark.parametrize("h0", [1, 2, 5])
def test_true_positions_and_symbols_give_the_true_bwt(name, text, h0):
    t = bytes(text)
    n = len(t)
    sa = suffix_array_plain(text).astype(np.int64)
    true_L = text[(sa - 1) % n]
    true_origin = int(np.flatnonzero(sa == 0)[0])
    prefix = [t[i:i + h0] for i in sa]
    gid = np.cumsum([1] + [prefix[p] != prefix[p - 1] for p in range(1, n)]).astype(np.uint32)
    rng = np.random.default_rng(h0)
    idx = sa.copy()
    for s, e in M.groups_of(gid):  # the members of a group in any order, its places in list order
        idx[s:e] = rng.permutation(idx[s:e])
    pos = np.arange(n, dtype=np.uint32)
    sym = text[(idx - 1) % n]
    L, origin = M.lf_refine_model(text, idx, pos, gid, sym, np.full(n, 0xC3, np.uint8), 0xC3C3C3C3)
    assert np.array_equal(L, true_L) and origin == true_origin, (name, h0)
    # a part of the groups only: the listed positions hold the true BWT, every other byte and (suffix 0 not listed) the origin word stay
    keep = np.isin(gid, rng.permutation(np.unique(gid))[::2]) & (gid != gid[true_origin])
    L, origin = M.lf_refine_model(text, idx[keep], pos[keep], gid[keep], sym[keep], np.full(n, 0xC3, np.uint8), 0xC3C3C3C3)
    assert np.array_equal(L[keep], true_L[keep]) and (L[~keep] == 0xC3).all() and origin == 0xC3C3C3C3, (name, h0)
    # places that are no run of positions: the k-th smallest member goes to the k-th place of the group in list order
    place = rng.permutation(3 * n)[:n].astype(np.uint32)
    L, origin = M.lf_refine_model(text, idx, place, gid, sym, np.full(3 * n, 0xC3, np.uint8), 7)
    assert np.array_equal(L[place], true_L) and origin == int(place[true_origin]) and int((L != 0xC3).sum()) <= n, (name, h0)
