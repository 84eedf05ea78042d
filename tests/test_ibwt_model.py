"""tests/ibwt_model.py before it judges anything (no GPU): the model inverts what the oracle transforms, agrees with the oracle's own inverse,
and the generator of inputs that are no BWT delivers the classes tests/test_gpu_inverse.py relies on."""
from collections import Counter

import numpy as np
import pytest

import ibwt_model as M
from conftest import seeded_inputs


def oracle_bwt(orc, t):
    return orc.bwt_forward(t, orc.sa_naive(t) if len(t) < 64 else None)


def pinned(orc, t):
    t = np.ascontiguousarray(np.frombuffer(bytes(t), np.uint8) if isinstance(t, (bytes, bytearray)) else t)
    L, origin = oracle_bwt(orc, t)
    v = M.invert(L, origin)
    assert v.text is not None and v.d == len(t) and v.longest_cycle == 0 and not v.cycle_has_splitter
    assert np.array_equal(v.text, t), "model(oracle BWT, oracle origin) is not the input (%d bytes)" % len(t)
    assert np.array_equal(v.text, orc.bwt_inverse(L, origin)), "model and oracle inverse differ (%d bytes)" % len(t)
    return L, origin


def test_model_inverts_the_oracle_on_seeded_inputs(orc):
    for t in seeded_inputs():
        pinned(orc, t)


def test_model_on_known_answers(orc, vectors, license_bytes):
    for item in vectors["reference"]["saca_rs_411_412"]:
        text = np.frombuffer(item["input"].encode(), np.uint8)
        L, origin = pinned(orc, text)
        assert L.tobytes() == item["bwt"].encode() and origin == item["origin"]
        assert M.invert(np.frombuffer(item["bwt"].encode(), np.uint8), item["origin"]).text.tobytes() == text.tobytes()
    pinned(orc, license_bytes)


def test_smallest_input_that_is_no_bwt():
    """L = a^10, origin = 8: the path is 8 -> 7 -> ... -> 0 -> END, nine entries; slot 9 is a fixed point and no multiple of 8"""
    psi, sym = M.successor_table(np.full(10, 0x61, np.uint8), 8)
    assert psi.tolist() == [M.END, 0, 1, 2, 3, 4, 5, 6, 7, 9] and (sym == 0x61).all()
    v = M.invert(np.full(10, 0x61, np.uint8), 8)
    assert v.text is None and v.d == 9 and not v.cycle_has_splitter and v.longest_cycle == 1 and v.longest_walk == 8
    v = M.invert(np.full(10, 0x61, np.uint8), 0)  # every other slot is a fixed point, slot 8 among them
    assert v.text is None and v.d == 1 and v.cycle_has_splitter
    v = M.invert(np.full(10, 0x61, np.uint8), 9)
    assert v.text is not None and v.text.tobytes() == b"a" * 10


def test_table_is_a_permutation_with_one_end(orc):
    rng = np.random.default_rng(4)
    for n in (1, 2, 9, 300, 5000):
        L = rng.integers(0, 5, size=n, dtype=np.uint8)
        for origin in {0, n // 2, n - 1}:
            psi, sym = M.successor_table(L, origin)
            assert sorted(psi.tolist()) == [M.END] + [i for i in range(n) if i != origin]
            assert np.array_equal(np.sort(sym), np.sort(L))
            v = M.invert(L, origin)
            assert (v.text is None) == (v.d < n) and 1 <= v.d <= n


@pytest.mark.parametrize("n,S", [(5000, 8), (70000, 64)])
def test_generator_delivers_every_class(orc, n, S):
    """Counts found with dark_amd.datagen.word_like(n, seed=5, vocab=2000) and max_distance = 40: class e 4 inputs at n = 5000 (S = 8,
    n - d = 9, 9, 2, 1) and 11 at n = 70000 (S = 64, n - d = 1 ... 30); class f (a leftover cycle longer than IB_REC without a splitter)
    none at n = 5000 -- at S = 8 such a cycle would have to miss 32 multiples of 8 -- and one at n = 70000 (a cycle of 273 entries).
    Classes a-d: every input is "no text" with a splitter in a leftover cycle, which is what the jump rounds have always rejected."""
    assert M.spacing(n) == S
    text, L, origin, cases = M.no_bwt_inputs(orc, n)
    assert not (text == 0xFF).any()
    assert np.array_equal(M.invert(L, origin).text, text)
    kinds = Counter(c.kind for c in cases)
    print("n = %d: %s" % (n, dict(kinds)), [(c.kind, n - c.verdict.d, c.verdict.longest_cycle) for c in cases if c.kind in "ef"])
    assert all(kinds[k] == 4 for k in "abcd")
    assert kinds["e"] >= 3, "class e needs at least three inputs at S = %d, found %d" % (S, kinds["e"])
    for c in cases:
        assert len(c.L) == n and 0 <= c.origin < n and not (c.L == 0xFF).any()
        if c.kind in "ef":
            assert c.verdict.text is None and not c.verdict.cycle_has_splitter and 0 < n - c.verdict.d
            assert (c.L != L).sum() == 2 and c.origin == origin
        if c.kind == "e":
            assert c.verdict.longest_cycle <= 40
        if c.kind == "f":
            assert c.verdict.longest_cycle > M.IB_REC
    if n == 70000:
        assert kinds["f"] >= 1
        assert M.invert(L, origin).longest_walk > M.IB_REC  # the correct input itself takes the resume branch of the copy kernel


def test_one_symbol_inputs():
    got = [(len(c.L), c.origin, c.verdict.text is None, c.verdict.d, c.verdict.cycle_has_splitter) for c in M.one_symbol()]
    assert got == [(10, 8, True, 9, False), (10, 0, True, 1, True), (70000, 69998, True, 69999, False), (70000, 0, True, 1, True)]
