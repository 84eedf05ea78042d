"""tests/round_model.py against per-suffix Python loops written from its docstring, and what every case of tests/round_cases.py is named for --
so that no case of tests/test_gpu_round.py is vacuous.  No GPU."""
import numpy as np
import pytest

import round_cases as K
import round_model as M
from period_model import next_break
from test_period_tokens import next_break as next_break_loop, token as token_loop


# ---- the keys, one suffix at a time -------------------------------------------------------------------------------------------------------------
def key_loop(form, t, n, h, x, rank=None, bits=0, code=None, tsym=0, p=0, nb=None):
    h = min(h, n)
    sym = lambda q: int(t[q]) if q < n else 0  # noqa: E731
    if form == "rank":
        return int(rank[x + h]) + h if x + h < n else n + h - 1 - (x + h)
    if form == "coded":
        key = 0
        for j in range(tsym):
            key = (key << bits) | (int(code[t[x + h + j]]) if x + h + j < n else 0)
        return key
    if form == "token" and x + h <= n and nb[x] - x + p >= h:
        ebits = M.bits_for(n + 1)
        up, e, tail = token_loop(t, nb, p, x)
        e = e if not up else ((1 << 31) - 1 - e)  # token() counts down from its own maximum: back to the length ...
        ev = e if not up else (1 << ebits) - 1 - e  # ... and down from the kernel's
        return (up << 63) | (ev << (63 - ebits)) | (int.from_bytes(bytes(tail), "big") << (31 - ebits))
    key = 0
    for j in range(8):
        key = (key << 8) | sym(x + h + j)
    return key


def round_loop(t, h, idx, gid, gstart, rank=None, tsym=0, period=0, nb=None):
    """-> (sorted keys, sorted suffixes, kb, symbols advanced) as the docstring of round_model says, one group and one member at a time"""
    n = len(t)
    code, sigma, bits = M.alphabet(np.asarray(t, np.uint8))
    sizes = [int(gstart[g + 1]) - int(gstart[g]) for g in range(len(gstart) - 1)]
    big_groups = sum(s > 1024 for s in sizes)
    bsbits = max(1, M.bits_for(big_groups))
    if period:
        form, kbits, kb, adv_small, adv_big = "token", 64, 1 + M.bits_for(n + 1) + 8, 0, 0
    elif tsym == 0:
        form, kbits, adv_small, adv_big = "rank", M.bits_for(n + min(h, n)), 0, 0
        kb = kbits
    else:
        form = "raw" if sigma >= 17 else "coded"
        tbits = 8 if form == "raw" else bits
        tsym = 8 if form == "raw" else min(tsym, 63 // tbits)
        kbits = tsym * tbits
        adv_small, adv_big = tsym, min(tsym, (63 - bsbits) // tbits, max(1, 32 // tbits))
        kb = adv_big * tbits
    keys, out = [], []
    before = 0
    for g, size in enumerate(sizes):
        members = []
        for a in range(int(gstart[g]), int(gstart[g + 1])):
            k = key_loop(form, t, n, h, int(idx[a]), rank, bits, code, tsym, period, nb)
            if size > 1024:
                k = (before << kb) | (k >> (kbits - kb))
            members.append((k, a))
        members.sort()
        keys += [k for k, _ in members]
        out += [int(idx[a]) for _, a in members]
        before += size > 1024
    return keys, out, kb, adv_big if big_groups else adv_small


def small_state(sigma, n, h, seed, end_zeros=0):
    """every group of two and more at depth h of a random text, shuffled"""
    from oracle import orc
    rng = np.random.default_rng(seed)
    t = rng.integers(0, sigma, size=n, dtype=np.uint8)
    if end_zeros:
        t[-end_zeros:] = 0
    sa = orc.sa_sais(t)
    starts, sizes = K.groups_padded(t, sa, h)
    starts, sizes = starts[sizes >= 2], sizes[sizes >= 2]
    gstart = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    gid = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    pos = (np.repeat(starts, sizes) + np.arange(gstart[-1]) - np.repeat(gstart[:-1].astype(np.int64), sizes)).astype(np.uint32)
    idx = sa[pos[np.lexsort((rng.random(len(pos)), gid))]]
    rank = np.empty(n, np.uint32)
    rank[sa] = np.arange(n, dtype=np.uint32)
    rank[sa[pos]] = np.repeat(starts, sizes)
    return t, idx, pos, gid, gstart, rank


@pytest.mark.parametrize("sigma,n,h,tsym", [(4, 700, 3, 0), (4, 700, 3, 5), (4, 700, 2, 40), (3, 5000, 1, 0), (3, 5000, 1, 6), (2, 3000, 1, 70), (40, 3000, 1, 8),
                                             (20, 5200, 0, 8), (2, 2300, 1, 0)])
def test_round_model_against_the_loop(sigma, n, h, tsym):
    h = max(h, 1)
    t, idx, pos, gid, gstart, rank = small_state(sigma, n, h, 7 * n + sigma, end_zeros=3)
    m = M.round_model(t, h, idx, pos, gid, gstart, rank=rank, tsym=tsym)
    keys, out, kb, adv = round_loop(t.tolist(), h, idx, gid, gstart, rank, tsym)
    assert m.sorted_keys.tolist() == keys and m.sorted_idx.tolist() == out and (m.plan.kb, m.advanced) == (kb, adv)
    assert bool(m.big.any()) == (sigma <= 3 and n >= 2300), "big groups where the case wants them"


@pytest.mark.parametrize("key,p,h", [("tok1", 1, 4), ("tok2", 2, 4), ("tok3", 3, 6), ("tok8", 8, 10), ("tok8", 8, 8), ("tok11", 11, 12), ("tok2_big", 2, 4)])
def test_token_rounds_against_the_loop_and_the_token_definition(key, p, h):
    c = K.build("x", key, h, 5, None, "token", 8, p)
    t = c.text.tolist()
    nb = next_break_loop(t, p)
    assert c.nb.tolist() == nb
    m = K.model_of(c, "sa")
    keys, out, kb, adv = round_loop(t, h, c.idx, c.gid, c.gstart, None, 8, p, nb)
    assert m.sorted_keys.tolist() == keys and m.sorted_idx.tolist() == out and (m.plan.kb, m.advanced) == (kb, adv)


# ---- the whole round against the suffix order ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_case_agrees_with_the_suffix_order(name):
    """what the model leaves is true: new groups in suffix order inside every old group, every final at its place of the oracle's suffix array, the
    ranks the head positions of the new groups"""
    c = K.CASES[name]()
    m, want = K.expected(name, "sa")
    borders = M.sound(m.sorted_keys, m.sorted_idx, c.gid, c.isa)
    assert borders > 0 or name.startswith("rank_h_") and m.rr.active == 0
    fin = want["sa"] != K.FILL32
    assert np.array_equal(want["sa"][fin], c.sa[fin]) and fin.sum() == c.n - m.rr.active
    if c.rank is not None:
        still = want["idx"][:m.rr.active]
        heads = want["pos"][:m.rr.active][want["gstart"][want["gid"][:m.rr.active]]]
        assert np.array_equal(want["rank"][still], heads) and np.array_equal(want["rank"][c.sa[fin]], np.flatnonzero(fin))
    ml, wl = K.expected(name, "l")
    at = int(c.isa[0])  # suffix 0: the origin word is written when it is listed and becomes final in this round, and only then
    assert np.array_equal(ml.sorted_idx, m.sorted_idx) and wl["origin"] == (at if c.sa_before[at] == K.FILL32 and fin[at] else K.FILL32)


# ---- what the cases are named for ---------------------------------------------------------------------------------------------------------------
def group_at(c, slot):
    g = int(c.gid[slot])
    return int(c.gstart[g]), int(c.gstart[g + 1])


@pytest.mark.parametrize("kind", ("rank", "text"))
def test_groups_across_slot_2048(kind):
    for label, group, front in K.EDGES:
        size = group if isinstance(group, int) else K.MARKS[group]
        for where in ("across", "ends"):
            c = K.CASES["%s_%s_%s" % (kind, where, label)]()
            assert group_at(c, M.TILE) == (M.TILE - front, M.TILE - front + size) and size <= M.LS_MAX
            assert (c.count == M.TILE - front + size) == (where == "ends")
            m, _ = K.expected(c.name, "sa")
            assert m.plan.form == ("rank" if kind == "rank" else "raw") and not m.big.any()
            assert not np.array_equal(m.order, np.arange(c.count)), "the round has something to sort"


@pytest.mark.parametrize("kind", ("rank", "text"))
def test_big_groups_and_list_lengths(kind):
    for name, big_sizes in (("big_1025", [1025]), ("big_5000", [5000]), ("two_big", [1025, 5000]), ("three_big", [1025, 5000, 1100])):
        c = K.CASES["%s_%s" % (kind, name)]()
        m, want = K.expected(c.name, "sa")
        assert c.sizes[c.sizes > M.LS_MAX].tolist() == big_sizes and (c.sizes <= 8).sum() > 50
        assert m.plan.bsbits == max(1, M.bits_for(len(big_sizes))) and "big_groups" in want["routes"]
        assert m.advanced == (0 if kind == "rank" else 4) and m.plan.kb == (M.bits_for(c.n + 2) if kind == "rank" else 32)
        # the big list's key: the dense index of the group above kb bits of the secondary key
        assert sorted(set((m.sorted_keys[m.big[m.order]] >> np.uint64(m.plan.kb)).tolist())) == list(range(len(big_sizes)))
    for k in (2047, 2048, 2049, 4097):
        assert K.CASES["%s_slots_%d" % (kind, k)]().count == k


def surviving_inside(c, m, size):
    """new groups of two and more inside the old group of `size` members: ties in the secondary key that stay a group"""
    g = int(np.flatnonzero(c.sizes == size)[0])
    inside = m.rr.out_pos[np.isin(m.rr.out_pos, c.pos[c.gstart[g]:c.gstart[g + 1]])]
    return len(inside)


def test_ties_ends_and_offsets():
    c = K.CASES["rank_ties_and_the_end"]()
    m, _ = K.expected(c.name, "sa")
    assert all(surviving_inside(c, m, k) >= 2 for k in K.MARKS.values()), "ranks that tie inside every planted group"
    x = c.idx.astype(np.int64)
    assert (x + c.h == c.n).sum() == 1 and c.text[-2] == c.text[-1] == 250
    assert m.sorted_idx[group_at(c, int(np.flatnonzero(x == c.n - 2)[0]))[0]] == c.n - 2, "the suffix that ends behind h symbols sorts first"
    for name in ("text_three_big", "text_across_g1024_half", "text_raw_past_the_end"):
        c = K.CASES[name]()
        m, _ = K.expected(name, "sa")
        assert m.plan.form == "raw" and len(np.unique(c.text)) >= 200 and m.rr.active >= 20, "keys of eight bytes that tie (the twins)"
    c = K.CASES["text_raw_past_the_end"]()
    assert (c.idx.astype(np.int64) + c.h + 8 > c.n).any()
    assert K.CASES["text_raw_with_ranks"]().rank is not None and K.CASES["text_big_1025"]().rank is None
    assert [K.CASES["text_raw_offset_%d" % o]().offset for o in (1, 3, 7)] == [1, 3, 7] == [K.CASES["text_coded_offset_%d" % o]().offset for o in (1, 3, 7)]


def test_small_alphabet_and_depths_at_the_end():
    c = K.CASES["rank_short_members"]()
    x = c.idx.astype(np.int64)
    assert sorted(x[x + c.h > c.n].tolist()) == [c.n - 3, c.n - 2, c.n - 1], "three members shorter than the depth"
    m, _ = K.expected(c.name, "sa")
    s0, _ = group_at(c, int(np.flatnonzero(x == c.n - 1)[0]))
    assert m.sorted_idx[s0:s0 + 3].tolist() == [c.n - 1, c.n - 2, c.n - 3], "shorter sorts first"
    for name, tsym, kbits, big in (("text_coded", 4, 8, False), ("text_coded_long", 31, 62, False), ("text_coded_big", 2, 4, True)):
        c = K.CASES[name]()
        m, want = K.expected(name, "sa")
        assert (m.plan.form, m.plan.tsym, m.plan.kbits, bool(m.big.all())) == ("coded", tsym, kbits, big) and len(np.unique(c.text)) == 4
        x = c.idx.astype(np.int64)
        assert (x + c.h + tsym > c.n).any() and (x + c.h + tsym + 8 <= c.n).any(), "keys past the end and keys through the word loads"
    m, _ = K.expected("text_coded_big", "sa")
    assert m.plan.bsbits == 4 and m.rr.active > 0
    for name, big in (("rank_h_above_n", False), ("rank_h_above_n_big", True), ("rank_h_equals_n", False)):
        c = K.CASES[name]()
        m, _ = K.expected(name, "sa")
        assert c.h >= c.n and bool(m.big.all()) == big and m.rr.active == 0
        assert np.array_equal(m.sorted_idx, np.sort(c.idx)[::-1]), "shorter first"


def test_token_cases():
    for p in (1, 2, 3, 8, 11):
        c = K.CASES["token_period_%d" % p]()
        m, _ = K.expected(c.name, "sa")
        tok = M.periodic(c.nb, p, c.idx, c.n, c.h)
        key = m.second[tok]
        x = c.idx[tok].astype(np.int64)
        up = key >> np.uint64(63)
        assert m.plan.form == "token" and not m.big.any() and tok.sum() > 300
        assert up.any() and not up.all(), "both break directions"
        assert (c.nb[x].astype(np.int64) + p >= c.n).any(), "a stretch that ends the text"
        ebits = M.bits_for(c.n + 1)
        top = key >> np.uint64(63 - ebits)  # direction and e
        g = c.gid[tok]
        pairs = {}
        for gg, tt, kk in zip(g.tolist(), top.tolist(), key.tolist()):
            pairs.setdefault((gg, tt), set()).add(kk)
        assert any(len(v) > 1 for v in pairs.values()), "equal e, different tails"
        counts = {}
        for gg, kk in zip(g.tolist(), key.tolist()):
            counts[(gg, kk)] = counts.get((gg, kk), 0) + 1
        assert max(counts.values()) >= 2, "equal tokens"
        plain = np.zeros(len(c.sizes), bool)
        plain[c.gid[~tok & (c.idx.astype(np.int64) + c.h <= c.n)]] = True
        assert plain.any(), "a group that is not periodic takes the text key"
        mixed = np.zeros(len(c.sizes), bool)
        mixed[c.gid[tok]] = True
        assert not (plain & mixed).any(), "the members of a group agree on being periodic"
    c = K.CASES["token_period_1"]()
    assert (c.idx.astype(np.int64) + c.h > c.n).sum() == c.h - 1, "members shorter than h"
    c = K.CASES["token_period_8_depth_8"]()
    assert c.h == c.period and M.periodic(c.nb, 8, c.idx, c.n, c.h)[c.idx.astype(np.int64) + c.h <= c.n].all(), "h == period: no test to fail"
    c = K.CASES["token_big_group"]()
    m, want = K.expected(c.name, "sa")
    assert M.periodic(c.nb, 2, c.idx, c.n, c.h)[m.big].all() and m.big.sum() > 2 * M.LS_MAX and m.plan.bsbits == 1 and "big_groups" in want["routes"]
    assert K.CASES["token_period_11_with_ranks"]().rank is not None and K.CASES["token_offset_3"]().offset == 3


def test_next_break_model_is_the_token_tests_definition():
    rng = np.random.default_rng(3)
    for p in (1, 2, 5, 9):
        t = np.tile(rng.integers(0, 3, size=p, dtype=np.uint8), 40)
        t[rng.integers(0, len(t), size=6)] ^= 1
        assert next_break(t, p).tolist() == next_break_loop(t.tolist(), p)
