"""tests/initial_sort_model.py and tests/initial_sort_cases.py on the CPU: the model against a per-position loop with sorted() on tuples, the
property of narrow keys the first rerank relies on, and what the grid, the texts and the sizes of tests/test_gpu_initial_sort.py are built for."""
import numpy as np
import pytest

import initial_sort_cases as K
import initial_sort_model as M


def test_the_grid_is_what_choose_prefix_can_choose():
    for bits in range(1, 9):
        plain, carry = K.prefixes(bits)
        assert plain and carry, bits
        assert 64 // bits in plain and max(carry) == 56 // bits
        assert all(1 <= k and bits * k <= 64 for k in plain) and all(1 <= k and bits * k <= 56 for k in carry)
    # bytes: every prefix of one to eight symbols is some period's; ACGT: the full key, the four short prefixes, periods of up to 4 and up to 8
    assert K.prefixes(8) == ([1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7])
    assert K.prefixes(2) == ([4, 8, 16, 20, 24, 28, 32], [4, 8, 16, 20, 24, 28])
    assert K.prefixes(1) == ([8, 32, 40, 48, 56, 64], [8, 32, 40, 48, 56])
    assert K.prefixes(5) == ([1, 3, 4, 6, 8, 9, 11, 12], [1, 3, 4, 6, 8, 9, 11])
    assert len(K.GRID) == len(set(K.GRID)) and {b for b, _, _ in K.GRID} == set(range(1, 9))


def test_the_cases_reach_every_path_they_are_named_for():
    reached = {}
    for name in K.GRID_CASES:
        c = K.CASES[name]()
        reached.setdefault(c.category, []).append(name)
        b = c.bits * c.spk
        assert c.want_passes == -(-b // 8) and c.want_packed == (8 < b <= 32), name  # (at a few tiles the position always fits the word)
        assert c.n == K.GRID_N and c.n % 16 and c.n > 3 * K.TILE
    assert set(K.CATEGORIES) <= set(reached), sorted(set(K.CATEGORIES) - set(reached))
    assert "unpacked at most 32 bits" not in reached  # (only DK_PACKED_SORT=0 and 2^24 positions reach it: the worker and the edge case)
    for name in K.GRID_CASES:  # narrow wherever B <= 40, and wide keys there as well
        if name.endswith("_narrow"):
            assert name[:-6] + "wide" in K.CASES
    kinds = {(c.kind, c.free) for c in (K.CASES[name]() for name in K.GRID_CASES)}
    assert kinds == {("random", False), ("random", True), ("low", False), ("low", True)}
    for point, (bits, spk, carry, narrow) in K.POINTS.items():
        assert (bits, spk, carry) in K.GRID, point
    assert {K.category(K.GRID_N, *p) for p in K.POINTS.values()} == {"B = 32 packed", "packed with middle passes", "33..40 bits, unpacked and narrow",
                                                                  "more than 40 bits"}
    for name in K.HANDOFF + K.WORKER:
        assert name in K.CASES, name
    assert [K.CASES[name]().category for name in K.HANDOFF] == ["B = 32 packed", "33..40 bits, unpacked and narrow"]
    for name, (n, bits, spk, carry, narrow, offset) in K.LARGE.items():
        assert (bits, spk, carry) in K.GRID, name


def test_the_texts():
    for name in K.GRID_CASES:
        c = K.CASES[name]()
        vals = np.unique(c.text)
        assert len(vals) <= 1 << c.bits and int(c.code.max()) < 1 << c.bits
        used = np.flatnonzero(np.bincount(c.text, minlength=256))
        if c.bits < 8:
            assert 0 in used or 255 in used or len(used) < 3
            assert len(used) < 3 or int(used[-1]) - int(used[0]) >= len(used), name  # not contiguous
        z = c.code[c.text] == 0
        assert z[-c.spk:].all(), name                    # the tail: at least spk copies of the symbol coded 0
        run = z[c.n // 3:c.n // 3 + c.spk + 5]
        assert run.all() and len(run) > c.spk, name      # an interior run longer than spk
        w = M.windows(c.text, c.code, c.bits, c.spk)
        assert w[-1] == 0 and (w == 0).sum() >= 4, name  # the zero-padded tail keys tie with real ones
        if c.kind == "low":
            assert len(np.unique(w)) < c.n // 2, name    # many full windows tie: stability shows
        if c.free and c.bits > 1:
            assert len(set(c.code[used].tolist())) < len(used) or len(used) < 3, name
        elif not c.free:
            assert sorted(c.code[used].tolist()) == sorted(set(c.code[used].tolist())), name
            assert (c.inv is None) or (c.inv[c.code[used]] == used).all()


def test_the_sizes_stand_at_the_staging_paths_edges():
    """a tile takes the 16-byte loads iff the text is aligned and goes on for 80 bytes behind the tile"""
    fast = lambda n, tile, offset=0: offset % 16 == 0 and tile * M.TILE + M.TILE + M.TEXT_AHEAD <= n  # noqa: E731
    assert fast(4176, 0) and not fast(4175, 0) and fast(8272, 1) and not fast(8271, 1) and not fast(8272, 1, offset=8)
    for n in (4175, 4176, 4177, 8271, 8272, 8273, 2, 3, 12289, 36865):
        assert n in K.SIZES
    assert K.OFFSETS == (0, 1, 8, 15)
    n = K.N_TWO_TILES
    tiles = -(-n // M.TILE)
    assert tiles == 1028 and -(-tiles // 1024) == 2  # a histogram workgroup walks two tiles
    assert fast(n, 1025) and not fast(n, 1026) and not fast(n, 1027)
    n = K.N_FAST_THEN_SLOW  # ... and here the two tiles of the last workgroup are a fast one and the slow last one
    assert -(-n // M.TILE) == 1028 and fast(n, 1026) and not fast(n, 1027)
    assert M.packed_rule(K.N_PACKED_EDGE, 8, 4, True) and not M.packed_rule(K.N_PACKED_EDGE + 1, 8, 4, True)
    assert M.packed_rule(K.N_PACKED_EDGE + 1, 8, 4, False)  # (without a carried code the position has the word to itself)
    assert not M.packed_rule(K.GRID_N, 2, 16, True, packed_sort=False)
    assert K.N_PLANE == (1 << 20) + 1


SMALL = [(bits, spk, carry) for bits, spk, carry in K.GRID if (bits + spk) % 3 == 0 or bits * spk in (8, 32, 40)]


@pytest.mark.parametrize("free", (False, True))
def test_the_model_against_the_loop(free):
    for i, (bits, spk, carry) in enumerate(SMALL):
        for n in (1, 2, spk, 257 + i):
            c = K.build("loop", n, bits, spk, carry, bits * spk <= 40 and i % 2 == 0, kind=("random", "low")[i % 2], free=free, text_seed=i)
            m = M.initial_sort_model(c.text, c.code, bits, spk, inv=c.inv, narrow=c.narrow)
            r = M.initial_sort_loop(c.text, c.code, bits, spk, inv=c.inv, narrow=c.narrow)
            what = (bits, spk, carry, n, c.narrow)
            for name in ("sa", "window", "wide_keys", "keys", "bwt", "bucket_starts"):
                a = getattr(m, name)
                assert (a is None) == (r[name] is None) and (a is None or [int(x) for x in a] == r[name]), (what, name)
            assert (m.origin, m.passes, m.sorted_elements) == (r["origin"], r["passes"], r["sorted_elements"]), what
            assert m.keys.dtype == (np.uint32 if c.narrow else np.uint64) and m.sa.dtype == np.uint32
            assert m.route == (M.ROUTE_PACKED_PAIRS if 8 < bits * spk <= 32 else 0)


def test_narrow_words_and_bucket_starts_find_the_heads_the_windows_find():
    """what the first rerank relies on: two neighbours can differ in the bits a narrow word has lost only at a bucket start"""
    narrow = [name for name in K.GRID_CASES if name.endswith("_narrow")]
    informative = 0
    for name in narrow:
        c = K.CASES[name]()
        m = K.expected(c)
        by_window = M.heads_by_window(m.window)
        assert (M.heads_by_narrow(m.keys, m.bucket_starts) == by_window).all(), name
        words_alone = M.heads_by_narrow(m.keys, [])
        assert not (words_alone & ~by_window).any(), name
        informative += int((words_alone != by_window).any())
        assert m.bucket_starts[0] == 0 and (np.diff(m.bucket_starts.astype(np.int64)) >= 0).all() and m.bucket_starts[-1] <= c.n
    assert informative > 0  # at 33 .. 40 bits the starts carry information: some head shows in no word
