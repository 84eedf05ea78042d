"""tests/period_model.py against brute-force loops written from its docstring, and what every case of tests/period_cases.py is named for -- so that
no case of tests/test_gpu_period.py is vacuous.  No GPU."""
import numpy as np
import pytest

import period_cases as K
import period_model as P
from round_model import alphabet


def texts():
    rng = np.random.default_rng(9)
    out = [np.full(300, 4, np.uint8), rng.integers(0, 2, size=333, dtype=np.uint8), np.tile(np.array([1, 2, 3], np.uint8), 200),
           np.concatenate([np.zeros(300, np.uint8), rng.integers(0, 3, size=200, dtype=np.uint8), np.zeros(530, np.uint8)])]
    out.append(np.tile(rng.integers(0, 256, size=37, dtype=np.uint8), 30))
    return out + [t[:n] for t in out[:2] for n in (1, 15, 16, 17, 71, 72, 73, 255, 256, 257)]


@pytest.mark.parametrize("p", (1, 2, 3, 7, 8, 9, 37, 74, 300))
def test_next_break_count_and_probe_against_loops(p):
    for t in texts():
        n = len(t)
        brk = [j + p >= n or t[j] != t[j + p] for j in range(n)]
        nb = [min(j for j in range(i, n) if brk[j]) for i in range(n)] if n <= 400 else None
        if nb is not None:
            assert P.next_break(t, p).tolist() == nb
        ok = lambda w: all(not brk[64 * w + k] for k in range(64))  # noqa: E731
        assert P.period_count(t, p) == sum(1 for w in range(n // 64 + 1) if 64 * w + 64 + p <= n and ok(w))
        if p <= 8:
            assert P.period_probe(t)[p - 1] == sum(1 for w in range(n // 64 + 1) if 64 * w + 72 <= n and ok(w))
            assert not P.period_probe(t, 4).any() and np.array_equal(P.period_probe(t, 8), P.period_probe(t))


def test_run_probe_against_a_loop():
    for t in texts():
        n = len(t)
        flag = pieces = 0
        for w in range(n // 256):
            win = t[256 * w:256 * w + 256].tolist()
            flag |= len(set(win)) == 1
            pieces += sum(len(set(win[16 * k:16 * k + 16])) == 1 for k in range(16))
        assert P.run_probe(t).tolist() == [flag, pieces] == P.run_probe(t, 16).tolist() and not P.run_probe(t, 8).any()


@pytest.mark.parametrize("pmax", (9, 40, 80))
def test_period_search_against_a_loop(pmax):
    for t in texts():
        n = len(t)
        want = []
        for b in range(32):
            x = (2 * b + 1) * n // 64
            hits = [p for p in range(9, pmax + 1) if x + pmax + 48 <= n and all(t[x + k] == t[x + p + k] for k in range(48))]
            want.append(hits[0] if hits else P.NONE)
        assert P.period_search(t, pmax).tolist() == want


def test_prefix_probe_against_a_loop():
    for t in texts():
        n = len(t)
        if n < 100:
            continue
        code, _, _ = alphabet(t)
        for m, span, lengths in ((20, n // 20, (1, 3)), (n // 3, 4, (2, 5, 9, 11)), (50, 1, (4,))):
            seen, dups = [set() for _ in lengths], [0, 0, 0, 0]
            for i in range(m):
                v = (i * 2654435761) & 0xFFFFFFFF
                pos = i * span + (v ^ (v >> 15)) % span
                if pos >= n:
                    continue
                for c, length in enumerate(lengths):
                    prefix = tuple(int(code[t[pos + j]]) if pos + j < n else 0 for j in range(length))
                    dups[c] += prefix in seen[c]
                    seen[c].add(prefix)
            assert P.prefix_probe(t, m, span, lengths).tolist() == dups


# ---- what the cases are named for ---------------------------------------------------------------------------------------------------------------
def test_next_break_cases():
    zeros = [n for n in K.CASES if n.startswith("nb_zeros")]
    assert len(zeros) == 3 * 7
    for name in zeros:
        c = K.CASES[name]()
        nb = K.expected(c)["next_break"][:c.n]
        first = c.n - c.parts["period"]
        assert not c.text.any() and (nb[:first] == first).all() and np.array_equal(nb[first:], np.arange(first, c.n)), "the text's end is the only break"
    names = [n for n in K.CASES if n.startswith("nb_n")]
    assert len(names) == sum(len({q for q in (1, 7, 8, 9, 300, n - 1, n) if q >= 1}) for n in (1, 15, 16, 17, 4095, 4096, 4097, 8197))
    for name in names:
        c = K.CASES[name]()
        nb = K.expected(c)["next_break"][:c.n]
        assert (nb >= np.arange(c.n)).all() and nb[-1] == c.n - 1 and (c.n < 4095 or c.parts["period"] >= c.n - 1 or len(np.unique(nb)) >= 3)
    c = K.CASES["nb_quiet_tiles"]()
    nb = K.expected(c)["next_break"]
    assert nb[0] == 2 * K.TILE + 97 and (nb[:K.TILE] > 2 * K.TILE).all(), "no break over a whole tile and more"
    c = K.CASES["nb_break_ends_a_tile"]()
    nb = K.expected(c)["next_break"]
    assert nb[0] == K.TILE - 1 == nb[K.TILE - 1] and nb[K.TILE] > K.TILE, "a break at a tile's last position"
    assert {K.CASES[n]().offset for n in K.CASES if n.startswith("nb_offset")} == {1, 8}
    for name, tiles, per in (("nb_spine_1025_tiles", 1025, 2), ("nb_spine_2049_tiles", 2049, 3)):
        c = K.CASES[name]()
        nb = K.expected(c)["next_break"][:c.n]
        assert c.n // K.TILE == tiles and 4.1e6 < c.n < 8.5e6
        tiles = -(-c.n // K.TILE)  # (the few bytes behind 1025 tiles are a tile of their own)
        assert -(-tiles // P.SPINE) == per
        first = nb[::K.TILE]  # the first break at or behind every tile's first position
        chunk_of = lambda j: int(j) // K.TILE // per  # noqa: E731
        crossing = [chunk_of(first[b]) - b // per for b in range(tiles)]
        assert max(crossing) > 100 and 0 in crossing and 1 in crossing, "stretches inside a chunk, into the next one and across hundreds of them"
        assert -(-tiles // per) < P.SPINE, "chunks without a tile at the end"


def test_probe_cases():
    want = {name: K.expected(K.CASES[name]()) for name in K.CASES if not name.startswith("nb_")}
    assert want["probe_all_equal"]["run"].tolist() == [1, 70000 // 256 * 16] and want["probe_all_equal"]["probe"].tolist() == [(70000 - 72) // 64 + 1] * 8
    assert want["probe_all_equal"]["count"] == (70000 - 5) // 64
    p3 = want["probe_period_3"]["probe"]
    assert p3[2] == p3[5] > 1000 and p3[[0, 1, 3, 4, 6, 7]].sum() == 0 and want["probe_period_3"]["count"] == want["probe_period_3_count_6"]["count"] == p3[2]
    assert not want["probe_random"]["probe"].any() and not want["probe_random"]["run"].any() and want["probe_random"]["count"] == 0
    assert want["probe_runs"]["run"].tolist() == [1, 37 + 36 + 2 + 11], "600 zeros from a window's start, 600 from 7 behind one, 40, and the last 300"
    assert [want["probe_n%d" % n]["probe"][0] for n in (71, 72, 73, 135, 136, 137)] == [0, 1, 1, 1, 2, 2]
    assert [want["probe_n%d" % n]["run"].tolist() for n in (255, 256, 257, 511, 512, 513)] == [[0, 0], [1, 16], [1, 16], [1, 16], [1, 32], [1, 32]]
    assert [want["count_n%d" % n]["count"] for n in (72, 73, 74, 1063, 1064, 1065)] == [0, 1, 1, 0, 1, 1]
    for off, run, probe in ((1, False, False), (4, False, False), (8, False, True), (16, True, True)):
        w = want["probe_runs_offset_%d" % off]
        assert bool(w["run"].any()) == run and bool(w["probe"].any()) == probe and w["count"] == want["probe_runs"]["count"] > 0
    f = want["search_table"]["found"]
    assert (f[:30] == 1000).all() and (f[30:] == P.NONE).all(), "the smallest of 1000, 2000, 3000, 4000; the last two samples are cut off"
    f = want["search_table_cut_off"]["found"]
    assert (f == 1000).sum() == 21 and (f[21:] == P.NONE).all()
    assert (want["search_none"]["found"] == P.NONE).all() and (want["search_period_above_pmax"]["found"] == P.NONE).all()
    assert (want["search_smallest_pmax"]["found"] == 9).all()
    assert want["prefix_random"]["dups"].tolist() == [0, 0, 0, 0] and (want["prefix_acgt"]["dups"] > 500).all()
    d = want["prefix_acgt_random"]["dups"].tolist()
    assert d[0] == 3000 - 256 and 0 < d[1] < 200 and d[2:] == [0, 0], "every prefix of four symbols seen; the fourth length is not asked for"
    assert want["prefix_two_lengths_past_the_end"]["dups"][0] == 300 - 64 and int(P.sample_positions(310, 10)[300:].min()) >= 3000
    w = want["all_parts_at_once"]
    assert all(v is not None for v in w.values()) and w["run"][0] == 1 and w["probe"][0] == w["count"] > 0 and (w["found"] == 9).sum() >= 1 and w["dups"][0] > 0
    assert K.POISON == "all_parts_at_once"
