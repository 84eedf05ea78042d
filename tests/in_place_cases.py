"""TEST HELPER: the built states of tests/test_gpu_in_place.py, shared with tests/test_in_place_model.py (which pins on the CPU what each case is
named for) and with the poison worker (tests/in_place_worker.py).

A state is built from a text and a depth h (build_state):
  * the oracle's suffix array; SA neighbours whose first h bytes exist and are equal form a group; rank[x] = the SA position of the head of x's group
  * the list holds groups of 2 .. 256 members, the members of a group in random order, a random label per suffix as its symbol in front.  The ORDER
    of the groups in the list is the case's choice (nothing in this layer needs list order to be SA order: pos[] carries the place), so a chosen
    group can stand across a chosen tile edge
  * a group the layout leaves out counts as settled before: its members get their own SA positions as ranks, which is a state the sort can be in
    (groups only ever get finer), and lets a case have exactly 2047 slots or 2049 records
Before a call sa holds the oracle's entry at unlisted places and 0xC3C3C3C3 at listed ones (bwt: the label, and 0xC3); after a run to the end the
whole array is the oracle's SA (the labels in suffix order).

The alphabets are small (4 symbols, h = 6) where groups of three to five are wanted, and 256 symbols with h = 1 or 2 where a walk's length or the
text's end is the point -- the walk limits count strides of h, so a small h keeps those texts short."""
import functools
from types import SimpleNamespace

import numpy as np

import in_place_model as M

FILL8, FILL32 = 0xC3, 0xC3C3C3C3
TILE = 2048
# (the sixth: a compaction is the call's last step, so that what it leaves in meta is looked at)
PLANS = (dict(max_rounds=0), dict(max_rounds=1), dict(max_rounds=2), dict(), dict(always_compact=True), dict(max_rounds=2, always_compact=True))
PLAN_IDS = ("chains_only", "one_round", "two_rounds", "to_the_end", "always_compact", "two_rounds_compacted")


def groups_of(text, sa, h):
    """-> (SA position of every group's head, its size) for the groups of SA neighbours whose first h bytes exist and are equal"""
    n = len(text)
    sa = sa.astype(np.int64)
    eq = (sa[:-1] + h <= n) & (sa[1:] + h <= n)
    for j in range(h):
        eq &= text[np.minimum(sa[:-1] + j, n - 1)] == text[np.minimum(sa[1:] + j, n - 1)]
    first = np.ones(n, bool)
    first[1:] = ~eq
    starts = np.flatnonzero(first)
    return starts, np.diff(np.append(starts, n))


def fit(sizes, candidates, target):
    """groups among `candidates` (in that order) whose sizes add up to exactly `target`"""
    out, left = [], int(target)
    for g in candidates:
        s = int(sizes[g])
        if s <= left and left - s != 1:
            out.append(int(g))
            left -= s
            if left == 0:
                return out
    raise AssertionError("no selection of groups adds up to %d slots" % target)


def build_state(name, text, h, seed, layout=None, **plan):
    """layout(starts, sizes, rng) -> the listed groups in list order, as indices into the groups of 2 and more members (None: all, in SA order)"""
    from oracle import orc
    rng = np.random.default_rng(seed)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    n = len(text)
    sa = orc.sa_sais(text)
    starts, sizes = groups_of(text, sa, h)
    assert sizes.max() <= M.PL_MAX, "a group of %d members: no state of the in-place rounds" % sizes.max()
    starts, sizes = starts[sizes >= 2], sizes[sizes >= 2]
    order = np.arange(len(starts)) if layout is None else np.asarray(layout(starts, sizes, rng), dtype=np.int64)
    assert len(order) and len(set(order.tolist())) == len(order)
    starts, sizes = starts[order], sizes[order]
    count = int(sizes.sum())
    gstart = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    gid = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    pos = (np.repeat(starts, sizes) + np.arange(count) - np.repeat(gstart[:-1].astype(np.int64), sizes)).astype(np.uint32)
    shuffle = np.lexsort((rng.random(count), gid))  # the members of each group in random order
    idx = sa[pos[shuffle]]
    rank = np.empty(n, np.uint32)
    rank[sa] = np.arange(n, dtype=np.uint32)  # unlisted: settled before
    rank[sa[pos]] = np.repeat(starts, sizes)
    lab = rng.integers(0, 256, size=n, dtype=np.uint8)  # the symbol in front: a free label per suffix
    listed = np.zeros(n, bool)
    listed[pos] = True
    return SimpleNamespace(name=name, text=text, n=n, h=h, sa=sa, idx=idx, pos=pos, gid=gid, gstart=gstart, rank=rank, sym=lab[idx], lab=lab, listed=listed,
                           sizes=sizes, starts=starts, count=count, sa_before=np.where(listed, FILL32, sa).astype(np.uint32),
                           bwt_before=np.where(listed, FILL8, lab[sa]).astype(np.uint8), plan=plan)


def state_of(c, mode):
    if mode == "sa":
        return M.new_state(c.n, c.h, c.idx, c.pos, c.gid, c.gstart, c.rank, sa=c.sa_before)
    return M.new_state(c.n, c.h, c.idx, c.pos, c.gid, c.gstart, c.rank, bwt=c.bwt_before, sym=c.sym, origin=FILL32)


@functools.lru_cache(maxsize=None)
def expected(name, mode, plan_id):
    """the model's state and counters for a case in a mode under one of PLANS (on top of the case's own plan), once"""
    c = CASES[name]()
    s = state_of(c, mode)
    return s, M.run(s, **dict(dict(chain_group=4), **c.plan, **PLANS[PLAN_IDS.index(plan_id)]))


def call(ctx, c, mode, pad=64, **plan):
    kw = dict(sa=c.sa_before) if mode == "sa" else dict(bwt=c.bwt_before, sym=c.sym, origin=FILL32)
    return ctx.dbg_dev_in_place(c.n, c.h, c.idx, c.pos, c.gid, c.gstart, c.rank, fill=FILL8, pad=pad, **dict(c.plan, **plan), **kw)


def first_diff(a, b):
    d = np.flatnonzero(a != b)
    return "equal" if not len(d) else "first of %d differences at %d: %s != %s" % (len(d), d[0], a[d[0]], b[d[0]])


def check_exact(c, mode, got, want, pad=64):
    """every output of a call against the model's (s, counters): whole arrays, the pad behind the lists included"""
    s, k = want
    for name in ("slots", "live", "records", "list_full", "settled", "rounds", "compactions"):
        assert got[name] == k[name], (c.name, mode, name, got[name], k[name])
    assert got["routes"] == {"inplace_rounds"} | ({"pair_chains"} if k["records"] else set()), (c.name, got["routes"])
    assert np.array_equal(got["rank"], s["rank"]), (c.name, mode, "rank", first_diff(got["rank"], s["rank"]))
    if mode == "sa":
        assert np.array_equal(got["sa"], s["sa"]), (c.name, mode, "sa", first_diff(got["sa"], s["sa"]))
        assert got["origin"] is None and got["sym"] is None
    else:
        assert np.array_equal(got["bwt"], s["bwt"]), (c.name, mode, "bwt", first_diff(got["bwt"], s["bwt"]))
        assert got["origin"] == s["origin"], (c.name, mode, "origin", got["origin"], s["origin"])
    slots = k["slots"] if k["live"] else 0  # (nothing alive: no list is copied out)
    whole = lambda a, fill, dtype: np.concatenate([a, np.full(c.count + pad - len(a), fill, dtype)])  # noqa: E731
    for name in ("idx", "pos"):
        w = whole(s[name][:slots], FILL32, np.uint32)
        assert np.array_equal(got[name], w), (c.name, mode, name, first_diff(got[name], w))
    alive = np.flatnonzero(s["idx"][:slots] < M.DEAD_BIT)
    tail = np.arange(slots, c.count + pad)
    assert np.array_equal(got["meta"][alive], s["meta"][alive]), (c.name, mode, "meta", first_diff(got["meta"][alive], s["meta"][alive]))
    assert (got["meta"][tail] == FILL32).all(), (c.name, mode, "meta behind the list")
    if mode == "l":
        assert np.array_equal(got["sym"][alive], s["sym"][alive]), (c.name, mode, "sym", first_diff(got["sym"][alive], s["sym"][alive]))
        assert (got["sym"][tail] == FILL8).all(), (c.name, mode, "sym behind the list")


def check_complete(c, mode, got):
    """a run to the end against the oracle alone"""
    assert got["live"] == 0
    if mode == "sa":
        assert np.array_equal(got["sa"], c.sa), (c.name, first_diff(got["sa"], c.sa))
    else:
        want = c.lab[c.sa]
        assert np.array_equal(got["bwt"], want), (c.name, first_diff(got["bwt"], want))
        zero = int(np.flatnonzero(c.sa == 0)[0])
        assert got["origin"] == (zero if c.listed[zero] else FILL32)
    assert np.array_equal(got["rank"][c.sa], np.arange(c.n, dtype=np.uint32)), (c.name, "rank is not the inverse of the suffix array")


def check_sound_chains(c, mode, got):
    """soundness of a chains-only call whose record list was full: which records fitted depends on the order of the workgroups' atomics, so only
    what must hold for every order -- each settled group in true order, every other listed place and every other rank untouched"""
    assert got["live"] == got["slots"] - got["settled"] and got["slots"] == c.count and got["rounds"] == 0
    assert got["list_full"] == 1 and 0 < got["records"] <= c.plan["record_cap"] and got["settled"] > 0, (got["list_full"], got["records"], got["settled"])
    dead = got["idx"][:c.count] == M.DEAD
    assert int(dead.sum()) == got["settled"] and np.array_equal(got["idx"][:c.count][~dead], c.idx[~dead])
    settled_pos = c.pos[dead]
    for g in np.flatnonzero(dead[c.gstart[:-1]]).tolist():
        assert dead[c.gstart[g]:c.gstart[g + 1]].all(), "half a group settled"
    if mode == "sa":
        want = c.sa_before.copy()
        want[settled_pos] = c.sa[settled_pos]
        assert np.array_equal(got["sa"], want), first_diff(got["sa"], want)
    else:
        want = c.bwt_before.copy()
        want[settled_pos] = c.lab[c.sa[settled_pos]]
        assert np.array_equal(got["bwt"], want), first_diff(got["bwt"], want)
    want = c.rank.copy()
    want[c.sa[settled_pos]] = settled_pos
    assert np.array_equal(got["rank"], want), first_diff(got["rank"], want)


# ---- texts ------------------------------------------------------------------------------------------------------------------------------------------
def rnd(seed, k, n):
    return np.random.default_rng(seed).integers(0, k, size=n, dtype=np.uint8)


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts])


def marker_block(seed, count=256, h=6):
    """`count` occurrences of a marker of h symbols found nowhere else, each followed by its number in eight bits, every bit three times and with
    symbols of its own: the suffixes at the markers are ONE group of `count` members at depth h that takes three rounds to come apart (4 x 64,
    then 16 x 16 ...), and no other group is larger"""
    rng = np.random.default_rng(seed)
    marker = np.arange(200, 200 + h, dtype=np.uint8)
    parts = []
    for i in rng.permutation(count).tolist():
        code = np.repeat([100 + 2 * b + ((i >> (7 - b)) & 1) for b in range(8)], 3)
        parts += [marker, code, rng.integers(0, 4, size=2)]
    return cat(*parts)


def tiles_text():
    a, b = rnd(11, 4, 1500), rnd(12, 4, 700)
    return cat(a, [4], a, [5], b, [6], b, [7], b, [8], marker_block(13), rnd(14, 4, 40))


def walk_text(q_len, through, seed=21):
    """P Q R ... P Q R with Q six times in all (through) -- the chain of P has to walk through Q's groups of six to the records in R -- or
    P Q X ... P Q Y (free): no record of P's delta behind Q, and the ranks differ where the h-gram reaches past Q.  256 symbols, h = 2"""
    rng = np.random.default_rng(seed)
    p, q, r = (rng.integers(0, 256, size=k, dtype=np.uint8) for k in (40, q_len, 40))
    sep = lambda: rng.integers(0, 256, size=3, dtype=np.uint8)  # noqa: E731
    if through:
        return cat(sep(), p, q, r, sep(), p, q, r, sep(), q, sep(), q, sep(), q, sep(), q, sep())
    return cat(sep(), p, q, sep(), p, q, sep(), q, sep(), q, sep(), q, sep(), q, sep())


def partial_text(copies, seed=31):
    """`copies` of P, two of them followed by a Q too long for the free walk (Q six times in all), the others by something else at once: in the
    groups of P's suffixes every pair but (first, second) is decided"""
    rng = np.random.default_rng(seed)
    p, q = rng.integers(0, 256, size=30, dtype=np.uint8), rng.integers(0, 256, size=60, dtype=np.uint8)
    sep = lambda: rng.integers(0, 256, size=3, dtype=np.uint8)  # noqa: E731
    parts = [sep(), p, q, sep(), p, q, sep()]
    for k in range(copies - 2):  # (at distances of their own: no two pairs of copies share a delta)
        parts += [rng.integers(0, 256, size=7 + 4 * k, dtype=np.uint8), p, sep()]
    for _ in range(4):
        parts += [q, sep()]
    return cat(*parts)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------------------
def shuffled(starts, sizes, rng):
    return rng.permutation(len(sizes))


def exact(target):
    def layout(starts, sizes, rng):
        return fit(sizes, rng.permutation(len(sizes)), target)
    return layout


def edge(in_front, big=M.PL_MAX, at=TILE):
    """small groups up to slot at - in_front, a group of `big` members, then the rest: in_front of its members lie in front of slot `at`"""
    def layout(starts, sizes, rng):
        g = int(np.flatnonzero(sizes == big)[0])
        small = [int(x) for x in rng.permutation(len(sizes)) if sizes[x] <= 4]
        front = fit(sizes, small, at - in_front)
        rest = [x for x in rng.permutation(len(sizes)).tolist() if x != g and x not in set(front)]
        return front + [g] + rest
    return layout


def big_last(starts, sizes, rng):
    """the group of 256 ends the list, 156 of its members in front of slot 4096 and 100 behind: the last tile ends inside the list's last group"""
    g = int(np.flatnonzero(sizes == M.PL_MAX)[0])
    return fit(sizes, [x for x in rng.permutation(len(sizes)).tolist() if x != g], 2 * TILE + 100 - M.PL_MAX) + [g]


def small_at_the_edge(starts, sizes, rng):
    """groups of up to four members (the chains' kind) from slot 1900 to 2200 at least, one of them across slot 2048; big groups in front and behind"""
    small = [int(x) for x in rng.permutation(len(sizes)) if sizes[x] <= 4]
    big = [int(x) for x in rng.permutation(len(sizes)) if sizes[x] > 4]
    front = []
    for x in big:
        if sum(int(sizes[y]) for y in front) + int(sizes[x]) <= 1900:
            front.append(x)
    three = next(x for x in small if sizes[x] == 3)
    mid = fit(sizes, [x for x in small if x != three], TILE - 2 - sum(int(sizes[y]) for y in front))
    more = [x for x in small if x != three and x not in set(mid)][:80]
    return front + mid + [three] + more + [x for x in big if x not in set(front)]


def pairs_only(records):
    def layout(starts, sizes, rng):
        return [int(x) for x in rng.permutation(len(sizes)) if sizes[x] == 2][:records]
    return layout


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name, text, h, seed, layout=None, **plan):
    CASES[name] = functools.lru_cache(maxsize=None)(lambda: build_state(name, text(), h, seed, layout, **plan))


A = lambda seed, k: rnd(seed, 4, k)  # noqa: E731
case("two_halves", lambda: cat(A(1, 1200), A(1, 1200)), 6, 101)
case("cut_half", lambda: cat(A(2, 1200), A(2, 1200)[:-7]), 6, 102)
case("odd_front", lambda: cat([3], A(3, 1200), A(3, 1200)), 6, 103)
case("three_copies", lambda: cat(A(4, 900), A(4, 900), A(4, 900)), 6, 104, shuffled)
case("four_copies", lambda: cat(*[A(5, 700)] * 4), 6, 105, shuffled)
case("five_copies", lambda: cat(*[A(6, 500)] * 5), 6, 106, shuffled)
case("parts_of_copies", lambda: cat(A(7, 300), A(8, 200), A(7, 300), A(9, 100), A(10, 50), cat(A(7, 300), A(8, 200), A(7, 300), A(9, 100))[100:], A(7, 300)), 6, 107, shuffled)
# 256 symbols, each at most once per copy, h = 1: every group is (i, i + |A|, ...), suffix 0 and suffix n - 1 included; the chain's end is decided
# by a position past the text's end
case("ends_two", lambda: cat(*[np.random.default_rng(41).permutation(256)[:120]] * 2), 1, 108)
case("ends_three", lambda: cat(*[np.random.default_rng(42).permutation(256)[:80]] * 3), 1, 109, shuffled)
for kmax in (0, 2, 3):  # (4 is the cases' own)
    case("three_copies_chain_group_%d" % kmax, lambda: cat(A(4, 900), A(4, 900), A(4, 900)), 6, 104, shuffled, chain_group=kmax)
    case("four_copies_chain_group_%d" % kmax, lambda: cat(*[A(5, 700)] * 4), 6, 105, shuffled, chain_group=kmax)
# walk limits: h = 2; the through walk may compare 1025 times (the gap 1 + 1025 h = 2051 is the last one it reaches), the free walk 17 times
case("walk_through_last", lambda: walk_text(2051, True), 2, 110)
case("walk_through_one_more", lambda: walk_text(2052, True), 2, 111)
case("walk_free_last", lambda: walk_text(33, False), 2, 112)
case("walk_free_one_more", lambda: walk_text(34, False), 2, 113)
case("partial_three", lambda: partial_text(3), 2, 114, shuffled)
case("partial_four", lambda: partial_text(4), 2, 115, shuffled)
# tile edges of k_plateau_sort and k_plateau_compact (2048 slots both)
for slots in (2047, 2048, 2049, 4097):
    case("slots_%d" % slots, tiles_text, 6, 120 + slots % 7, exact(slots))
for in_front in (1, 128, 255):
    case("big_group_%d_in_front" % in_front, tiles_text, 6, 130 + in_front, edge(in_front))
case("big_group_last", tiles_text, 6, 134, big_last)
case("dead_slots_at_the_edge", tiles_text, 6, 135, small_at_the_edge)
for records in (2047, 2048, 2049):
    case("records_%d" % records, lambda: cat(rnd(15, 16, 2300), rnd(15, 16, 2300)), 6, 140 + records % 7, pairs_only(records))
EXACT = tuple(CASES)
# the record list full over two and three workgroups of the extraction (4096 slots each): soundness only
case("sound_full_two_workgroups", lambda: cat(rnd(16, 16, 3000), rnd(16, 16, 3000)), 6, 150, record_cap=2500)
case("sound_full_three_workgroups", lambda: cat(rnd(17, 16, 5000), rnd(17, 16, 5000)), 6, 151, shuffled, record_cap=3000)
SOUND = ("sound_full_two_workgroups", "sound_full_three_workgroups")
# the sort's own compaction: more than 2^16 slots, the chains settle the two halves and leave the five copies alive
case("own_compaction", lambda: cat(rnd(18, 256, 40000), rnd(18, 256, 40000), *[rnd(19, 256, 3000)] * 5), 6, 152)
POISON = ("big_group_128_in_front", "walk_through_last", "sound_full_two_workgroups")
