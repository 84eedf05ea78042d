"""The model of the segmented suffix sort's steps (tests/packed_round_model.py) against the definition by prefixes, the cases of
tests/packed_round_cases.py against what they are named for, and the proof that the cases can fail: every plausible kernel mistake the model can
switch in (M.WRONG) gives another answer than the model on a named case.  No GPU."""
import numpy as np
import pytest

import packed_round_cases as K
import packed_round_model as M


def assert_meets_the_definition(blocks, what):
    """model and definition agree after the first step and after EVERY round to the end"""
    f, rounds = M.chain(blocks)
    assert not rounds or rounds[-1].live == 0, what
    d = f.k_used
    steps = [(f.rank, f.act[:f.live])] + [(r.rank, r.next_act[:r.live]) for r in rounds]
    settled = {}
    for i, (rank, act) in enumerate(steps):
        want_rank, want_live = M.by_prefixes(blocks, d, settled)
        assert (rank == want_rank).all(), "%s: ranks after %d rounds (d = %d)" % (what, i, d)
        assert (np.sort(act) == want_live).all(), "%s: live set after %d rounds (d = %d)" % (what, i, d)
        d *= 2
    return len(rounds)


def random_pack(seed):
    """1 .. 8 blocks of 1 .. 3000 bytes, sigma of 1, 2, 3, 26 or 256, a third of the blocks tiled repeats"""
    rng = np.random.default_rng(seed)
    sigma = int(rng.choice([1, 2, 3, 26, 256]))
    alphabet = rng.permutation(256)[:sigma].astype(np.uint8)
    blocks = []
    for _ in range(int(rng.integers(1, 9))):
        n = int(rng.integers(1, 3001))
        if rng.random() < 1 / 3:
            unit = alphabet[rng.integers(0, sigma, int(rng.integers(1, 40)))]
            blocks.append(np.tile(unit, n // len(unit) + 1)[:n])
        else:
            blocks.append(alphabet[rng.integers(0, sigma, n)])
    return blocks


@pytest.mark.parametrize("seed", range(32))
def test_random_packs_meet_the_definition(seed):
    assert_meets_the_definition(random_pack(seed), "seed %d" % seed)


def test_the_cut_mixed_pack_meets_the_definition():
    blocks = K.chain_blocks()
    assert max(len(b) for b in blocks) == 5000 and len(blocks) > 200
    assert assert_meets_the_definition(blocks, "mixed pack") >= 8


@pytest.mark.parametrize("name", sorted(K.FIRST))
def test_first_cases_are_what_they_are_named_for(name):
    make, words, prop = K.FIRST[name]
    f = M.first(make())
    for k, v in words.items():
        assert getattr(f, k) == v, (name, k, getattr(f, k), v)
    assert prop is None or prop(f), name
    assert f.end_bit <= 64 and (f.end_bit == 64 or int(f.keys.max()) >> f.end_bit == 0)
    want_rank, want_live = M.by_prefixes(make(), f.k_used)
    assert (f.rank == want_rank).all() and (np.sort(f.act[:f.live]) == want_live).all() and (f.act[f.live:] == M.FILL32).all()


def test_first_cases_cover_the_sizes():
    sizes = {len(b) for name in K.FIRST for b in K.first_blocks(name)}
    assert {1, 2, 3, 4095, 4096, 4097} <= sizes
    assert {len(K.first_blocks(name)) for name in K.FIRST} >= {1, 2, 64, 65, 65536}


def _round(name):
    c = K.ROUNDS[name]()
    K.duties(c)
    return c, M.round_(c.act, c.rank, c.off, c.h)


@pytest.mark.parametrize("name", sorted(K.ROUNDS))
def test_built_rounds_keep_the_callers_duties(name):
    c, m = _round(name)
    assert c.name == name and len(c.sizes) == (300 if name == "guard_300_blocks" else min(len(c.sizes), 3))
    listed = np.zeros(len(c.rank), bool)
    listed[c.act] = True
    assert (m.rank[~listed] == c.rank[~listed]).all()  # only the entries of listed suffixes change
    assert (m.next_act[m.live:] == M.FILL32).all() and sorted(m.vals) == sorted(c.act)


def test_built_rounds_are_what_they_are_named_for():
    T = K.TILE
    for c_want in (1, 2, 15, 16, 17, T - 1, T, T + 1):
        c, m = _round("c_%d" % c_want)
        assert len(c.act) == c_want and (c_want < 15 or 0 < m.live < c_want)
    c, m = _round("c_3_tiles_5_whole_pack")
    assert len(c.act) == len(c.rank) == 3 * T + 5 and len(c.sizes) == 3 and 0 < m.live < len(c.act)
    c, m = _round("list_already_sorted")
    assert (m.vals == c.act).all() and m.live > 0
    c, m = _round("all_keys_equal")
    assert m.live == len(c.act) > T and (m.rank == c.rank).all() and (m.next_act == c.act).all()  # (order kept: the list's own)
    c, m = _round("all_keys_distinct")
    assert m.live == 0 and len(c.act) > T and (m.rank != c.rank).any()
    for name in ("pairs_across_every_border", "pairs_across_every_border_in_order"):
        c, m = _round(name)
        eq = m.keys[1:] == m.keys[:-1]
        at = np.arange(15, len(eq), 16)
        assert eq[at].all() and not eq[at - 1].any() and len(c.act) > T and eq[T - 1]
        assert (m.vals == c.act).all() == name.endswith("in_order")
    c, m = _round("old_group_over_three_tiles")
    nh = np.r_[True, m.keys[1:] != m.keys[:-1]]
    oh = np.r_[True, (m.keys[1:] >> np.uint64(m.rbits)) != (m.keys[:-1] >> np.uint64(m.rbits))]
    assert len(c.act) == 3 * T + 5 and not nh[T:2 * T].any() and not oh[T:2 * T].any() and nh[:T].sum() > 3 and oh[2 * T:].any()
    assert np.flatnonzero(oh)[np.searchsorted(np.flatnonzero(oh), T) - 1] < np.flatnonzero(nh)[np.searchsorted(np.flatnonzero(nh), T) - 1] < T
    c, m = _round("singletons_and_pairs")
    runs = np.diff(np.flatnonzero(np.r_[True, m.keys[1:] != m.keys[:-1], True]))
    assert set(runs) == {1, 2} and 0 < m.live < len(c.act)
    assert c.rank[m.vals[0]] == 0  # an old group with the rank 0 at list index 0
    assert _round("h_1")[0].h == 1
    c, m = _round("rbits_at_a_power_of_two")
    c2, m2 = _round("rbits_past_a_power_of_two")
    assert int(c.off[-1]) + c.h == 1 << 14 and m.rbits == 14 and c2.h == c.h + 1 and m2.rbits == 15
    c, m = _round("h_at_least_the_longest_block")
    assert c.h >= max(c.sizes) and (m.keys & np.uint64((1 << m.rbits) - 1) < np.uint64(c.h)).all() and m.live > 0
    c, m = _round("short_and_long_in_one_old_group")
    e = c.off[M.block_of(c.off, c.act.astype(np.int64)) + 1]
    short = c.act + c.h >= e
    assert (c.act + c.h == e).sum() == 2 and len(set(c.rank[c.act[short]]) & set(c.rank[c.act[~short]])) > 3
    c, m = _round("collision_of_short_and_long")
    assert m.live == 0 and len(set(m.keys)) == 3 and M.round_(c.act, c.rank, c.off, c.h, wrong="r2_without_h").live == 2
    assert list(_round("guard_1_block")[1].guard) == [1]
    assert list(_round("guard_2_blocks_one_unlisted")[1].guard) == [1, 0]
    c, m = _round("guard_300_blocks")
    before = M.guard_words(c.act, c.off)
    assert len(m.guard) == 300 and before[5] == 1 and m.guard[5] == 0 and before[7] == before[8] == 0 and 100 < m.guard.sum() < before.sum()
    assert not _round("no_guard_words")[0].guard


def differs(a, b):
    return any((getattr(a, k) != getattr(b, k)).any() for k in ("keys", "vals", "rank", "out") + (("next_act", "guard") if hasattr(a, "guard") else ("act", "code")))


# every mistake, and the named small case that tells it apart (the spine's carries need the large case: test_the_large_round)
TOLD_APART = {
    "r2_without_h": "collision_of_short_and_long", "end_inclusive": "short_and_long_in_one_old_group", "rbits_from_total": "rbits_past_a_power_of_two",
    "old_on_whole_key": "singletons_and_pairs", "live_blind_16": "pairs_across_every_border", "live_blind_4096": "pairs_across_every_border_in_order",
    "nh_lost_at_tile": "old_group_over_three_tiles", "oh_lost_at_tile": "old_group_over_three_tiles", "live_scan_inclusive": "c_4097",
    "live_scan_late": "pairs_across_every_border", "guard_from_input": "guard_300_blocks",
    "pad_as_smallest": "block_shorter_than_the_key", "no_block_id": "a_block_a_prefix_of_another", "k_unclamped": "sigma_1_below_64",
}


def test_every_mistake_is_told_apart_by_a_named_case():
    assert set(TOLD_APART) | {"spine_nh", "spine_oh", "spine_live"} == set(M.WRONG)
    for wrong, name in TOLD_APART.items():
        if name in K.FIRST:
            blocks = K.first_blocks(name)
            assert differs(M.first(blocks), M.first(blocks, wrong=wrong)), (wrong, name)
        else:
            c, m = _round(name)
            assert differs(m, M.round_(c.act, c.rank, c.off, c.h, wrong=wrong)), (wrong, name)


def test_the_tile_mistakes_show_in_what_they_break():
    """not just anywhere: the blind live flag in the next list alone, a lost head in the ranks alone"""
    c, m = _round("pairs_across_every_border_in_order")
    w = M.round_(c.act, c.rank, c.off, c.h, wrong="live_blind_4096")
    assert (w.rank == m.rank).all() and w.live == m.live - 1
    w = M.round_(c.act, c.rank, c.off, c.h, wrong="live_blind_16")
    assert w.live == m.live - len(c.act) // 16
    c, m = _round("old_group_over_three_tiles")
    for wrong in ("nh_lost_at_tile", "oh_lost_at_tile"):
        w = M.round_(c.act, c.rank, c.off, c.h, wrong=wrong)
        assert (w.next_act == m.next_act).all() and (w.rank != m.rank).sum() >= K.TILE


def test_the_large_round():
    """the one case with a second spine pass: what it is built for, and that each carry lost between the passes changes the answer"""
    c = K.large()
    K.duties(c)
    m = M.round_(c.act, c.rank, c.off, c.h)
    border, T = 1024 * K.TILE, K.TILE
    assert len(c.act) == K.LARGE_C == border + T + 1
    nh = np.r_[True, m.keys[1:] != m.keys[:-1]]
    oh = np.r_[True, (m.keys[1:] >> np.uint64(m.rbits)) != (m.keys[:-1] >> np.uint64(m.rbits))]
    assert not nh[border:border + T].any() and not oh[border:border + T].any() and nh[border + T]  # tile 1024 holds no head at all
    assert border - 50 == np.flatnonzero(oh)[-1] < np.flatnonzero(nh[:border])[-1] == border - 40  # old and new group straddle the border
    live = ~(nh & np.r_[nh[1:], True])
    assert live[:border].sum() > border // 2 and live[border:].sum() == T and not live[-1]
    for wrong in ("spine_nh", "spine_oh", "spine_live"):
        w = M.round_(c.act, c.rank, c.off, c.h, wrong=wrong)
        assert differs(m, w), wrong
        small, ms = _round("old_group_over_three_tiles")
        assert not differs(ms, M.round_(small.act, small.rank, small.off, small.h, wrong=wrong)), "%s needs the large case" % wrong
