"""CPU: the LF formula and the sampled walk of tests/fm_locate_model.py against sorted suffixes."""
import itertools

import numpy as np
import pytest

from fm_locate_model import lf, locate_rows, locate_slot, locate_structure, sa_plain, NO_HIT
from fm_model import bwt_plain

STEPS = [1, 2, 4, 8, 64]


def texts():
    out = [bytes(w) for m in range(1, 9) for w in itertools.product(b"ab", repeat=m)]
    assert len(out) == 510
    return out + [b"abracadabra", b"a" * 40, b"ab" * 20, bytes(np.random.default_rng(5).choice([0, 1, 2, 0xFE, 0xFF], size=60).astype(np.uint8))]


def test_lf_steps_one_position_back():
    """SA[LF(x)] = SA[x] - 1 for every slot but the origin, and LF is a bijection onto the slots other than that of suffix n - 1"""
    for t in texts():
        L, origin = bwt_plain(t)
        sa = sa_plain(t)
        assert sa[origin] == 0
        seen = set()
        for x in range(len(t)):
            if x == origin:
                continue
            y = lf(L, origin, x)
            assert 0 <= y < len(t) and sa[y] == sa[x] - 1, (t, x, y)
            seen.add(y)
        assert len(seen) == len(t) - 1 and sa.index(len(t) - 1) not in seen


@pytest.mark.parametrize("step", STEPS)
def test_sampled_walk(step):
    """every slot of every text is located, and the longest walk stays within min(step, n) - 1"""
    for t in texts():
        n = len(t)
        L, origin = bwt_plain(t)
        sa = sa_plain(t)
        marked, samples = locate_structure(L, origin, sa, step)
        assert marked[origin] and len(samples) == (n + step - 1) // step <= n // step + 1
        worst = 0
        for x in range(n):
            pos, k = locate_slot(L, origin, marked, samples, step, x)
            assert pos == sa[x], (t, step, x)
            worst = max(worst, k)
        assert worst <= min(step, n) - 1
        if set(t) == {97}:
            assert worst == min(step, n) - 1, "a^n reaches the bound"


def test_rows():
    sa = sa_plain(b"abracadabra")
    rows = locate_rows(sa, [(0, 11), (2, 4), (5, 5), (7, 3)], 3)
    assert rows.tolist() == [sa[0:3], sa[2:4] + [NO_HIT], [NO_HIT] * 3, [NO_HIT] * 3]
