"""TEST HELPER: the built states of tests/test_gpu_round.py, shared with tests/test_round_model.py (which pins on the CPU what each case is named
for) and with the poison worker (tests/round_worker.py).

A state is built from a text and a depth h (build), as tests/in_place_cases.py builds its own:
  * the oracle's suffix array; SA neighbours equal in their first h symbols -- the text padded with zero bytes, as the sort's keys pad it, so a suffix
    shorter than h can be a member -- form a group; rank[x] = the SA position of the head of x's group
  * the list holds groups of two and more members in the order the case's layout wants (nothing in a round needs list order to be SA order: pos[]
    carries the place), the members of a group SHUFFLED by the case's seed -- the round has to sort them -- and a random label per suffix as its
    symbol in front.  A group the layout leaves out counts as settled before: its members have their own SA positions as ranks
  * every case names its round: "rank" (tsym 0), "text" (tsym symbols, coded or raw as the text's alphabet decides) or "token" (a period, the
    next-break array from tests/period_model.py)
Before a call sa holds the oracle's entry at unlisted places and 0xC3C3C3C3 at listed ones (bwt: the label, and 0xC3)."""
import functools
from types import SimpleNamespace

import numpy as np

import period_model as P
import rerank_model as R
import round_model as M
from in_place_cases import FILL8, FILL32, first_diff, fit

FILL64 = 0xC3C3C3C3C3C3C3C3
PAD = 64
MODES = ("sa", "l")


def rnd(seed, sigma, n):
    return np.random.default_rng(seed).integers(0, sigma, size=n, dtype=np.uint8)


def groups_padded(text, sa, h):
    """-> (SA position of every group's head, its size): SA neighbours whose first h symbols are equal, zero bytes behind the text's end"""
    n = len(text)
    depth = min(h, n)
    padded = np.concatenate([text, np.zeros(depth, np.uint8)])
    s = sa.astype(np.int64)
    eq = np.ones(n - 1, bool)
    for j in range(depth):
        eq &= padded[s[:-1] + j] == padded[s[1:] + j]
    first = np.ones(n, bool)
    first[1:] = ~eq
    starts = np.flatnonzero(first)
    return starts, np.diff(np.append(starts, n))


@functools.lru_cache(maxsize=None)
def suffix_array(key):
    from oracle import orc
    text = TEXTS[key]()
    sa = orc.sa_sais(text)
    isa = np.empty(len(sa), np.int64)
    isa[sa] = np.arange(len(sa))
    return text, sa, isa


def build(name, text_key, h, seed, layout=None, kind="rank", tsym=0, period=0, offset=0, with_rank=None):
    """layout(sizes, rng) -> the listed groups in list order, as indices into the groups of two and more members in SA order (None: all of them)"""
    rng = np.random.default_rng(seed)
    text, sa, isa = suffix_array(text_key)
    n = len(text)
    starts, sizes = groups_padded(text, sa, h)
    starts, sizes = starts[sizes >= 2], sizes[sizes >= 2]
    order = np.arange(len(starts)) if layout is None else np.asarray(layout(sizes, rng), dtype=np.int64)
    assert len(order) and len(set(order.tolist())) == len(order), name
    starts, sizes = starts[order], sizes[order]
    count = int(sizes.sum())
    gstart = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    gid = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    pos = (np.repeat(starts, sizes) + np.arange(count) - np.repeat(gstart[:-1].astype(np.int64), sizes)).astype(np.uint32)
    shuffle = np.lexsort((rng.random(count), gid))  # the members of each group in random order
    idx = sa[pos[shuffle]]
    rank = np.empty(n, np.uint32)
    rank[sa] = np.arange(n, dtype=np.uint32)
    rank[sa[pos]] = np.repeat(starts, sizes)
    lab = rng.integers(0, 256, size=n, dtype=np.uint8)
    listed = np.zeros(n, bool)
    listed[pos] = True
    with_rank = kind == "rank" if with_rank is None else with_rank
    return SimpleNamespace(name=name, text=text, n=n, h=h, sa=sa, isa=isa, idx=idx, pos=pos, gid=gid, gstart=gstart, rank=rank if with_rank else None,
                           sym=lab[idx], count=count, sizes=sizes, kind=kind, tsym=tsym, period=period, offset=offset,
                           nb=P.next_break(text, period) if period else None, sa_before=np.where(listed, FILL32, sa).astype(np.uint32),
                           bwt_before=np.where(listed, FILL8, lab[sa]).astype(np.uint8))


def model_of(c, mode):
    l_mode = mode == "l"
    return M.round_model(c.text, c.h, c.idx, c.pos, c.gid, c.gstart, rank=c.rank, tsym=c.tsym, period=c.period, nb=c.nb,
                         sym=c.sym if l_mode else None, bwt=c.bwt_before if l_mode else None)


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """the model's round and every output array as the entry leaves it (whole, over the fill), once per case and mode"""
    c = CASES[name]()
    m = model_of(c, mode)
    l_mode = mode == "l"
    words = lambda: np.full(c.count + PAD, FILL32, np.uint32)  # noqa: E731
    syms = lambda: np.full(c.count + PAD, FILL8, np.uint8) if l_mode else None  # noqa: E731
    before = dict(out_idx=words(), out_pos=words(), out_gid=words(), sym_out=syms(), gstart=words(), bigidx=np.zeros(c.count, np.uint32),
                  bigoff=np.zeros(c.count, np.uint32), rank=None if c.rank is None else c.rank.copy(), sa=None if l_mode else c.sa_before.copy(),
                  bwt=c.bwt_before.copy() if l_mode else None, origin=FILL32 if l_mode else None)
    after = R.apply_model(m.rr, m.sorted_idx, before)
    over = lambda a, fill, dtype: None if a is None else np.concatenate([a, np.full(PAD, fill, dtype)])  # noqa: E731
    want = dict(sorted_keys=over(m.sorted_keys, FILL64, np.uint64), sorted_idx=over(m.sorted_idx, FILL32, np.uint32), sorted_sym=over(m.sorted_sym, FILL8, np.uint8),
                idx=after["out_idx"], pos=after["out_pos"], gid=after["out_gid"], gstart=after["gstart"], sym=after["sym_out"], rank=after["rank"],
                sa=after["sa"], bwt=after["bwt"], origin=after["origin"], active=m.rr.active, groups=m.rr.groups, big_slots=m.rr.big_slots,
                big_groups=m.rr.big_groups, above_pl_slots=m.rr.above_pl_slots, advanced=m.advanced, kb=m.plan.kb,
                routes={dict(rank="general_round", coded="text_round", raw="text_round", token="period_round")[m.plan.form]} | ({"big_groups"} if m.big.any() else set()))
    return m, want


def call(ctx, c, mode):
    kw = dict(sa=c.sa_before) if mode == "sa" else dict(bwt=c.bwt_before, sym=c.sym, origin=FILL32)
    return ctx.dbg_dev_round(c.text, c.h, c.idx, c.pos, c.gid, c.gstart, rank=c.rank, tsym=c.tsym, period=c.period, next_break=c.nb, text_offset=c.offset,
                             fill=FILL8, pad=PAD, **kw)


ARRAYS = ("sorted_keys", "sorted_idx", "sorted_sym", "idx", "pos", "gid", "gstart", "sym", "rank", "sa", "bwt")
WORDS = ("active", "groups", "big_slots", "big_groups", "above_pl_slots", "advanced", "kb", "routes", "origin")


def check(c, mode, got, want):
    """every output of a call against the model's: whole arrays, the pad behind the lists included; then the check that needs no model"""
    for name in WORDS:
        assert got[name] == want[name], (c.name, mode, name, got[name], want[name])
    for name in ARRAYS:
        if want[name] is None:
            assert got[name] is None, (c.name, mode, name)
        else:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (c.name, mode, name, first_diff(got[name], want[name]))
    M.sound(got["sorted_keys"][:c.count], got["sorted_idx"][:c.count], c.gid, c.isa)


# ---- texts ------------------------------------------------------------------------------------------------------------------------------------
MARKS = dict(A=1023, B=1024, C=1025, D=5000, E=1100)  # occurrences of the two-byte word (250 + i, 250 + i)


def planted_text():
    """70 000 random bytes of 200 values and five two-byte words of byte values above them, each planted an exact number of times; behind the
    first 40 occurrences of every word, in pairs, the same 12 bytes: ties in a key of eight bytes.  The text ends with word A"""
    rng = np.random.default_rng(11)
    n, twins = 70000, 40
    t = rng.integers(0, 200, size=n, dtype=np.uint8)
    tail = n - 3400                                                     # 200 cells of 16 bytes for the twins, and 200 bytes of nothing
    main = rng.permutation(tail // 6)[:sum(MARKS.values()) - twins * len(MARKS)] * 6   # cells of 6 bytes for the rest: nothing planted overlaps
    at = 0
    for i, (_, k) in enumerate(sorted(MARKS.items())):
        where = np.concatenate([tail + 16 * (twins * i + np.arange(twins)), main[at:at + k - twins]])
        at += k - twins
        if i == 0:
            where[-1] = n - 2  # x + h == n
        t[where] = t[where + 1] = 250 + i
        for j in range(0, twins, 2):
            t[where[j + 1] + 2:where[j + 1] + 14] = t[where[j] + 2:where[j] + 14]
    return t


def small_text():
    """20 000 bytes of the values 0 .. 3, the last three of them 0: three suffixes shorter than a depth of 4 in the group of 0000"""
    t = rnd(12, 4, 20000)
    t[-3:] = 0
    return t


def zeros_text(run):
    return lambda: np.concatenate([np.full(40, 5, np.uint8), np.zeros(run, np.uint8)])


def token_text(p, seed, stretches, longest, zero_unit=False):
    """stretches of one period string of p bytes in pairs of one length, every start at phase 0.  A pair is broken by the same byte, below or
    above the one the period asks for in turn, and shares the first byte behind it (equal e, different tails), or two, or four (equal tokens);
    between the stretches random bytes with a planted twelve-byte word, which is no stretch of any period used here.  The text ends inside a stretch"""
    rng = np.random.default_rng(seed)
    unit = np.zeros(p, np.uint8) if zero_unit else rng.integers(60, 190, size=p, dtype=np.uint8)
    if p > 1:
        unit[0] = 59  # (primitive: one byte value occurs once)
    word = rng.integers(200, 256, size=12, dtype=np.uint8)
    parts = []
    for pair in range(stretches // 2):
        length = int(rng.integers(3 * p + 8, longest))
        want = int(unit[length % p])  # the byte the period asks for behind the stretch
        step = 1 + pair % 3
        brk = want - step if pair % 2 == 0 and want >= step else want + step
        tails = rng.integers(0, 256, size=(2, 6), dtype=np.uint8)
        tails[1, :(1, 4, 2)[pair % 3]] = tails[0, :(1, 4, 2)[pair % 3]]
        for tail in tails:
            parts += [np.tile(unit, length // p + 2)[:length], np.array([brk], np.uint8), tail, rng.integers(190, 200, size=int(rng.integers(2, 9)), dtype=np.uint8),
                      word, rng.integers(0, 256, size=3, dtype=np.uint8)]
    parts.append(np.tile(unit, longest // p + 2)[:longest // 2])
    return np.concatenate(parts)


TEXTS = dict(planted=planted_text, small=small_text, zeros_small=zeros_text(1000), zeros_big=zeros_text(3000),
             tok1=lambda: token_text(1, 21, 12, 120, zero_unit=True), tok2=lambda: token_text(2, 22, 24, 120), tok3=lambda: token_text(3, 23, 24, 200),
             tok8=lambda: token_text(8, 24, 24, 400), tok11=lambda: token_text(11, 25, 24, 500), tok2_big=lambda: token_text(2, 26, 40, 400))


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------------
def mark_group(sizes, mark):
    g = np.flatnonzero(sizes == MARKS[mark])
    assert len(g) == 1, (mark, len(g))
    return int(g[0])


def fillers(sizes, rng, target, taken=()):
    """groups of at most 8 members, in a random order, whose sizes add up to exactly `target`"""
    cand = [g for g in rng.permutation(np.flatnonzero(sizes <= 8)) if g not in taken]
    return fit(sizes, cand, target) if target else []


def across(size_or_mark, front, ends):
    """the chosen group with `front` members in front of slot 2048, small groups before it and (unless it ends the list) 500 slots behind it"""
    def layout(sizes, rng):
        g = mark_group(sizes, size_or_mark) if isinstance(size_or_mark, str) else int(np.flatnonzero(sizes == size_or_mark)[0])
        head = fillers(sizes, rng, M.TILE - front, (g,))
        return head + [g] + ([] if ends else fillers(sizes, rng, 500, set(head) | {g}))
    return layout


def with_big(marks, small=300):
    """the big groups named, `small` slots of small groups in front of each and behind the last"""
    def layout(sizes, rng):
        out, taken = [], {mark_group(sizes, m) for m in marks}
        for m in marks:
            f = fillers(sizes, rng, small, taken)
            taken |= set(f)
            out += f + [mark_group(sizes, m)]
        return out + fillers(sizes, rng, small, taken)
    return layout


def slots(target):
    return lambda sizes, rng: fillers(sizes, rng, target)


CASES = {}


def case(name, *args, **kw):
    CASES[name] = functools.lru_cache(maxsize=None)(lambda: build(name, *args, **kw))


# the planted text at depth 2, each layout once as a rank round and once as a text round (200 byte values and more: raw keys)
EDGES = [("pair", 2, 1)] + [("g%d_%s" % (MARKS[m], w), m, f) for m in "AB" for w, f in (("one", 1), ("half", MARKS[m] // 2), ("all_but_one", MARKS[m] - 1))]
for kind, tsym in (("rank", 0), ("text", 8)):
    for seed, (label, group, front) in enumerate(EDGES):
        case("%s_across_%s" % (kind, label), "planted", 2, 100 + seed, across(group, front, False), kind, tsym)
        case("%s_ends_%s" % (kind, label), "planted", 2, 120 + seed, across(group, front, True), kind, tsym)
    case(kind + "_big_1025", "planted", 2, 140, with_big("C"), kind, tsym)
    case(kind + "_big_5000", "planted", 2, 141, with_big("D"), kind, tsym)
    case(kind + "_two_big", "planted", 2, 142, with_big("CD"), kind, tsym)
    case(kind + "_three_big", "planted", 2, 143, with_big("CDE"), kind, tsym)
    for k in (2047, 2048, 2049, 4097):
        case("%s_slots_%d" % (kind, k), "planted", 2, 150 + k, slots(k), kind, tsym)
case("rank_ties_and_the_end", "planted", 2, 160, None, "rank")                               # every group: ranks that tie; word A ends the text: x + h == n
case("text_raw_past_the_end", "planted", 2, 161, with_big("A", small=100), "text", 8)
case("text_raw_with_ranks", "planted", 2, 162, with_big("C"), "text", 8, with_rank=True)
for off in (1, 3, 7):
    case("text_raw_offset_%d" % off, "planted", 2, 163, with_big("C"), "text", 8, offset=off)
# four byte values: coded keys of two bits
case("rank_short_members", "small", 4, 170, None, "rank")
case("text_coded", "small", 4, 171, None, "text", 4)
case("text_coded_long", "small", 4, 172, None, "text", 31)
case("text_coded_big", "small", 2, 173, None, "text", 2)       # sixteen groups of about 1250: four bits number them
case("rank_coded_big", "small", 2, 174, None, "rank")
for off in (1, 3, 7):
    case("text_coded_offset_%d" % off, "small", 4, 175, None, "text", 4, offset=off)
# the depth at and above the text's length
case("rank_h_above_n", "zeros_small", 2048, 180, None, "rank")
case("rank_h_above_n_big", "zeros_big", 4096, 181, None, "rank")
case("rank_h_equals_n", "zeros_small", 1040, 182, None, "rank")
# token rounds
for key, p, h in (("tok1", 1, 4), ("tok2", 2, 4), ("tok3", 3, 6), ("tok8", 8, 10), ("tok11", 11, 12)):
    case("token_period_%d" % p, key, h, 190 + p, None, "token", 8, p)
case("token_period_8_depth_8", "tok8", 8, 201, None, "token", 8, 8)     # h == period: every member of full length takes the token
case("token_period_11_with_ranks", "tok11", 12, 202, None, "token", 8, 11, with_rank=True)
case("token_big_group", "tok2_big", 4, 203, None, "token", 8, 2)
case("token_offset_3", "tok3", 6, 204, None, "token", 8, 3, offset=3)

POISON = ("rank_across_g1024_half", "text_three_big", "token_period_3")
