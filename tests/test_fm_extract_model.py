"""CPU: the models of tests/fm_extract_model.py against slices of the text."""
import itertools

import numpy as np
import pytest

from fm_extract_model import NO_HIT, anchors, chunk, extract, extract_rows
from fm_locate_model import sa_plain
from fm_model import bwt_plain

STEPS = [1, 2, 4, 8, 64]


def texts():
    short = [bytes(w) for m in range(1, 9) for w in itertools.product(b"ab", repeat=m)]
    assert len(short) == 510
    return short + [b"abracadabra", b"a" * 40, b"ab" * 20, bytes([0, 0xFF, 1, 0xFE, 2, 0, 0xFF, 0xFF, 1, 0, 2, 0xFE])]


def structure(t, step):
    L, origin = bwt_plain(np.frombuffer(t, np.uint8))
    return L, origin, anchors(sa_plain(t), step)


@pytest.mark.parametrize("step", STEPS)
def test_every_range_of_every_text(step):
    cases = 0
    for t in texts():
        n = len(t)
        L, origin, anchor = structure(t, step)
        assert anchor[0] == origin and len(anchor) == (n + step - 1) // step
        # every chunk once: the bytes, and the bound on the steps (reached by every full chunk)
        pieces = {}
        for k in range(len(anchor)):
            piece, steps = chunk(L, origin, anchor, step, k)
            assert piece == t[k * step:(k + 1) * step] and steps == len(piece) - 1 <= min(step, n) - 1, (t, step, k)
            pieces[k] = piece
        for a in range(n + 1):
            for length in range(n + 2 - a):
                cases += 1
                assert extract(L, origin, anchor, step, a, length) == t[a:a + length], (t, step, a, length)
    assert cases == {1: 25036, 2: 25036, 4: 25036, 8: 25036, 64: 25036}[step]  # 125 180 in all


def test_the_walk_without_the_origin_step_is_wrong():
    t = b"abracadabra"
    for step in (4, 8, 64):  # (at step 2 the last chunk of the 11 bytes is one byte long and takes no step at all)
        L, origin, anchor = structure(t, step)
        last = len(anchor) - 1
        assert extract(L, origin, anchor, step, 0, len(t)) == t
        assert extract(L, origin, anchor, step, 0, len(t), special=False) != t
        assert chunk(L, origin, anchor, step, last, special=False)[0] != t[last * step:]
        assert all(chunk(L, origin, anchor, step, k, special=False)[0] == t[k * step:(k + 1) * step] for k in range(last))


def test_rows():
    t = b"abracadabra"
    rows = extract_rows(t, [(0, 11), (0, None), (3, 4), (9, 5), (10, None), (11, 3), (12, 1), (NO_HIT, 7), (5, 0), (2, 100)], 6)
    assert rows.shape == (10, 6) and rows.dtype == np.uint8
    want = [b"abraca", b"abraca", b"acad\0\0", b"ra\0\0\0\0", b"a\0\0\0\0\0", b"\0" * 6, b"\0" * 6, b"\0" * 6, b"\0" * 6, b"racada"]
    assert [bytes(r) for r in rows] == want
