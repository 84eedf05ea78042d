"""tests/in_place_model.py and the states of tests/in_place_cases.py on the CPU: the model reaches the true suffix array from every built state,
every verdict of its chain rule agrees with the true order, a model with one rule broken is noticed, and each case has -- by the model's own
counts -- the property it is named for, so that none can quietly stop reaching its kernel path (tests/test_gpu_in_place.py runs them on the GPU)."""
import numpy as np
import pytest

import in_place_cases as K
import in_place_model as M
from sa_query_model import suffix_array_plain

MODES = ("sa", "l")


def run(name, mode="sa", **plan):
    c = K.CASES[name]()
    s = K.state_of(c, mode)
    return c, s, M.run(s, **dict(dict(chain_group=4), **c.plan, **plan))


def complete(c, s, mode):
    return np.array_equal(s["sa"], c.sa) if mode == "sa" else np.array_equal(s["bwt"], c.lab[c.sa])


def test_oracle_suffix_arrays_are_brute_force_sorted_suffixes():
    for name in ("two_halves", "cut_half", "three_copies", "four_copies", "five_copies", "parts_of_copies", "ends_two", "ends_three", "walk_free_last", "partial_four"):
        c = K.CASES[name]()
        assert np.array_equal(c.sa, suffix_array_plain(c.text)), name


@pytest.mark.parametrize("name", K.EXACT + ("own_compaction",))
def test_model_reaches_the_suffix_array(name):
    for mode in MODES:
        for plan in ("to_the_end", "always_compact"):
            s, k = K.expected(name, mode, plan)
            c = K.CASES[name]()
            assert k["live"] == 0 and complete(c, s, mode), (name, mode, plan)
            assert np.array_equal(s["rank"][c.sa], np.arange(c.n)), (name, mode, plan)
            if mode == "l":
                zero = int(np.flatnonzero(c.sa == 0)[0])
                assert s["origin"] == (zero if c.listed[zero] else K.FILL32), (name, plan)
        assert K.expected(name, "sa", "always_compact")[1]["compactions"] >= 1 or K.expected(name, "sa", "chains_only")[1]["live"] == 0


@pytest.mark.parametrize("name", ("two_halves", "cut_half", "three_copies", "four_copies", "parts_of_copies", "ends_three", "partial_four", "slots_2049"))
@pytest.mark.parametrize("chain_group", (0, 2, 3, 4))
def test_model_with_every_chain_group(name, chain_group):
    for always_compact in (False, True):
        c, s, k = run(name, chain_group=chain_group, always_compact=always_compact)
        assert k["live"] == 0 and complete(c, s, "sa")
        assert chain_group or k["records"] == 0


@pytest.mark.parametrize("name", K.EXACT + ("own_compaction",))
def test_every_chain_verdict_agrees_with_the_true_order(name):
    c = K.CASES[name]()
    k = K.expected(name, "sa", "chains_only")[1]
    isa = np.empty(c.n, np.int64)
    isa[c.sa] = np.arange(c.n)
    lo, hi, v = (np.array(a, dtype=np.int64) for a in zip(*k["pairs"])) if k["pairs"] else (np.zeros(0, np.int64),) * 3
    decided = v != 0
    assert ((isa[lo] < isa[hi])[decided] == (v == M.LT)[decided]).all()
    assert len(lo) == k["records"]


@pytest.mark.parametrize("rule,noticed_by,wrong_at_the_end", [("tie_order", ("big_group_128_in_front", "five_copies"), False),
                                                              ("moved_bit", ("parts_of_copies", "big_group_last"), True),
                                                              ("text_end", ("five_copies", "ends_two"), True)])
def test_a_broken_rule_is_noticed(rule, noticed_by, wrong_at_the_end):
    """the model with one rule broken differs from the model in what the GPU test compares after one or two rounds (or after the chains), and -- but
    for the order of ties, which only decides who stands in which slot of a group -- does not reach the suffix array"""
    for name in noticed_by:
        c = K.CASES[name]()
        differs = False
        for plan_id in ("chains_only", "one_round", "two_rounds"):
            s, k = K.expected(name, "l", plan_id)
            b = K.state_of(c, "l")
            kb = M.run(b, **dict(dict(chain_group=4), **c.plan, **K.PLANS[K.PLAN_IDS.index(plan_id)]), broken=rule)
            alive = s["idx"] < M.DEAD_BIT
            differs |= any(k[x] != kb[x] for x in ("live", "settled")) or not np.array_equal(s["idx"], b["idx"]) or not np.array_equal(s["rank"], b["rank"]) \
                or not np.array_equal(s["bwt"], b["bwt"]) or not np.array_equal(s["meta"][alive], b["meta"][alive])
        assert differs, (rule, name)
        if wrong_at_the_end:
            b = K.state_of(c, "sa")
            try:
                M.run(b, **dict(dict(chain_group=4), **c.plan), broken=rule)
                reached = complete(c, b, "sa")
            except AssertionError as e:
                assert "no convergence" in str(e)
                reached = False
            assert not reached, (rule, name)


# ---- what each case is named for ----------------------------------------------------------------------------------------------------------------------
def chains_only(name, mode="l"):
    return K.expected(name, mode, "chains_only")


def test_copies():
    for name in ("two_halves", "cut_half", "odd_front", "three_copies", "parts_of_copies"):
        s, k = chains_only(name)
        assert k["records"] > 0 and k["settled"] > 0 and k["live"] > 0 and not k["list_full"], name
    for name, sizes in (("two_halves", {2, 4}), ("three_copies", {3}), ("four_copies", {4}), ("five_copies", {5}), ("parts_of_copies", {2, 3, 4, 5})):
        assert sizes <= set(K.CASES[name]().sizes.tolist()), name
    # suffix 0 stands in a chain group and is settled there, with L carried along: the origin word is written by k_chain_apply
    c = K.CASES["two_halves"]()
    s, k = chains_only("two_halves")
    assert c.listed[np.flatnonzero(c.sa == 0)[0]] and s["origin"] != K.FILL32
    # four copies: about 1.5 records per slot, more than n; one workgroup reserves them all and nothing fits
    c = K.CASES["four_copies"]()
    assert len(M.chain_records(c.idx, M.to_inplace(c.gid, c.gstart), 4)[0]) > c.n and c.count < M.ONE_WORKGROUP
    s, k = chains_only("four_copies")
    assert k["list_full"] == 1 and k["records"] == 0 and k["settled"] == 0
    # five copies: no records but those of the groups of four at the copies' ends (the last copy's suffixes there are shorter than h); the rounds do it all
    s, k = chains_only("five_copies")
    assert k["records"] <= 6 * (K.CASES["five_copies"]().h - 1) and k["settled"] <= 4 * (K.CASES["five_copies"]().h - 1)
    assert K.expected("five_copies", "sa", "to_the_end")[1]["rounds"] >= 8


def test_the_texts_end_and_suffix_0():
    for name in ("ends_two", "ends_three"):
        c = K.CASES[name]()
        s, k = chains_only(name)
        in_chain_groups = set(c.idx[np.repeat(c.sizes, c.sizes) <= 4].tolist())
        assert 0 in in_chain_groups and c.n - 1 in in_chain_groups
        assert k["settled"] == c.count and s["origin"] != K.FILL32
        assert any(how == "verdict" and past for _, _, how, past in k["walks"]), "no pair is decided by a position past the text's end"
    # ... and in the rounds: the suffix of exactly h symbols stands in a group that the chains leave alone, its second rank is the rule's n - 1 - x
    for name in ("five_copies", "four_copies", "three_copies_chain_group_0"):
        c = K.CASES[name]()
        assert c.n - c.h in chains_only(name)[0]["idx"].tolist(), name


def test_chain_group_cases():
    rec = {(t, g): chains_only("%s_chain_group_%d" % (t, g) if g != 4 else t)[1] for t in ("three_copies", "four_copies") for g in (0, 2, 3, 4)}
    assert rec["three_copies", 0]["records"] == 0 and rec["three_copies", 2]["records"] < rec["three_copies", 3]["records"] == rec["three_copies", 4]["records"]
    assert rec["four_copies", 0]["records"] == 0 and rec["four_copies", 2]["records"] <= rec["four_copies", 3]["records"] and rec["four_copies", 3]["list_full"] == 0
    assert rec["four_copies", 4]["list_full"] == 1


def test_walk_limits():
    """each twin pair: the same walk, one comparison apart"""
    last, more = chains_only("walk_through_last")[1], chains_only("walk_through_one_more")[1]
    assert [w for w in last["walks"] if w[1] == M.WALK_THROUGH + 1] == [w for w in last["walks"] if w[1] > 100] and len([w for w in last["walks"] if w[1] > 100]) == 1
    assert [w[2] for w in last["walks"] if w[1] == M.WALK_THROUGH + 1] == ["continues"]
    assert [w[2] for w in more["walks"] if w[1] == M.WALK_THROUGH + 1] == ["undecided"] and max(w[1] for w in more["walks"]) == M.WALK_THROUGH + 1
    assert last["settled"] > more["settled"]
    last, more = chains_only("walk_free_last")[1], chains_only("walk_free_one_more")[1]
    assert [w[2] for w in last["walks"] if w[1] == M.WALK_FREE + 1] == ["verdict"]
    assert [w[2] for w in more["walks"] if w[1] == M.WALK_FREE + 1] == ["undecided"] and max(w[1] for w in more["walks"]) == M.WALK_FREE + 1
    assert last["settled"] > more["settled"]


@pytest.mark.parametrize("name,size", [("partial_three", 3), ("partial_four", 4)])
def test_partial_groups(name, size):
    """groups of three and four with some pairs decided and not all: untouched by the chains"""
    c = K.CASES[name]()
    s, k = chains_only(name, "sa")
    group_of = np.full(c.n, -1, np.int64)
    group_of[c.idx] = c.gid
    decided, pairs = np.zeros(len(c.sizes), np.int64), np.zeros(len(c.sizes), np.int64)
    for lo, hi, v in k["pairs"]:
        assert group_of[lo] == group_of[hi] >= 0
        pairs[group_of[lo]] += 1
        decided[group_of[lo]] += v != 0
    partial = np.flatnonzero((c.sizes == size) & (decided > 0) & (decided < pairs))
    assert len(partial) >= 10
    for g in partial.tolist():
        sl = slice(int(c.gstart[g]), int(c.gstart[g + 1]))
        assert np.array_equal(s["idx"][sl], c.idx[sl]) and (s["sa"][c.pos[sl]] == K.FILL32).all() and (s["rank"][c.idx[sl]] == c.starts[g]).all()


def test_tile_edges():
    for slots in (2047, 2048, 2049, 4097):
        assert K.CASES["slots_%d" % slots]().count == slots
    for in_front in (1, 128, 255):
        c = K.CASES["big_group_%d_in_front" % in_front]()
        g = int(np.flatnonzero(c.sizes == M.PL_MAX)[0])
        assert c.gstart[g] == K.TILE - in_front
        assert K.expected(c.name, "sa", "two_rounds")[0]["meta"][K.TILE - in_front:K.TILE - in_front + 256].max() >> 8 & 0xFF > 0, "the group is gone after a round"
        # two rounds leave groups with the moved bit alive: the compaction behind them has a bit to drop
        s, k = K.expected(c.name, "sa", "two_rounds")
        assert ((s["meta"][s["idx"] < M.DEAD_BIT] & M.MOVED) != 0).sum() > 1000 and K.expected(c.name, "sa", "two_rounds_compacted")[1]["compactions"] == 2
    c = K.CASES["big_group_last"]()
    assert c.sizes[-1] == M.PL_MAX and c.count == 2 * K.TILE + 100  # (the last tile edge runs through the list's last group)
    c = K.CASES["dead_slots_at_the_edge"]()
    s, k = chains_only(c.name)
    dead = s["idx"] == M.DEAD
    assert dead[K.TILE - 2:K.TILE + 1].all() and c.gstart[np.searchsorted(c.gstart, K.TILE, "right") - 1] == K.TILE - 2, "no settled group across the edge"
    assert dead[K.TILE - 100:K.TILE].sum() > 50 and dead[K.TILE:K.TILE + 100].sum() > 50 and (~dead[:K.TILE]).any() and (~dead[K.TILE:]).any()
    for records in (2047, 2048, 2049):
        s, k = chains_only("records_%d" % records)
        assert k["records"] == records and len(k["walks"]) > 20, "one chain end per tile is no test of the scan"


def test_full_lists_and_the_large_list():
    for name, workgroups in (("sound_full_two_workgroups", 2), ("sound_full_three_workgroups", 3)):
        c = K.CASES[name]()
        records = len(M.chain_records(c.idx, M.to_inplace(c.gid, c.gstart), 4)[0])
        assert (workgroups - 1) * M.ONE_WORKGROUP < c.count <= workgroups * M.ONE_WORKGROUP and records > c.plan["record_cap"]
        first = len(M.chain_records(c.idx[:M.ONE_WORKGROUP], M.to_inplace(c.gid, c.gstart)[:M.ONE_WORKGROUP], 4)[0])
        assert first <= c.plan["record_cap"], "no workgroup's records fit: the outcome would be the deterministic empty list"
    c = K.CASES["own_compaction"]()
    s, k = K.expected("own_compaction", "sa", "to_the_end")
    assert c.count >= M.COMPACT_FROM and k["settled"] * 4 >= 3 * c.count and k["settled"] < c.count and k["compactions"] >= 1
