"""The rerank layer by itself (csrc/suffix_array.hip): k_rerank_reduce<u64 | u32>, k_rerank_scan / _scan_a / _scan_c, k_rerank_apply,
k_rerank_apply_first and the classification behind them (k_big_reduce / _spine / _apply), through dk_dbg_dev_rerank and against the plain model
of tests/rerank_model.py (tests/test_rerank_model.py pins that on the CPU).  Bit-exact, and over WHOLE arrays: every output holds 0xC3 bytes
(rank: random words, L: random bytes) before the call, so what must stay untouched is compared too -- rank of kept groups, sa / bwt at
non-final positions and all of both in the first rerank, the lists from `active` on, gstart from groups + 1 on, bigidx of small groups, bigoff
from big_groups on, the origin when suffix 0 survives.

The lists are BUILT from group sizes (make_case): where a head is, and what makes it one (the key, the old group, both, a bucket start alone), is
the case's choice.  Every case runs with the sort's own launch shapes and with overrides of the tiles per workgroup of k_rerank_reduce and
k_rerank_apply_first (1, 2, 3, 64) and of the sparse limit (0 .. 2048): the multi-tile stretches, which the sort takes from 2^26 and 2^25 slots,
are reached at three tiles, and all runs of a case must give the same bytes.  The three-phase scan has no override: its cases have 4096 (the last
one-workgroup size), 4097 and 5121 tiles -- 8.4 to 10.5 Mi slots -- and are the only large ones."""
import ctypes as C

import numpy as np
import pytest
import torch

import dark_amd
import rerank_model as M
from dark_amd._lib import DK_E_ARG

pytestmark = pytest.mark.gpu
TILE = M.TILE
BIG_TILES = 4 * M.SCAN_CHUNK + M.SCAN_CHUNK + 1   # the largest list of test_three_phase_scan
CAP = (BIG_TILES + 1) * TILE
PAD = 64                                          # words of every output behind what a call may write (Context.dbg_dev_rerank: pad)
FILL8, FILL32 = 0xC3, 0xC3C3C3C3
ARRAYS = ("out_idx", "out_pos", "out_gid", "sym_out", "gstart", "bigidx", "bigoff", "rank", "sa", "bwt")
KEY, OLD, BOTH, FORCED = 0, 1, 2, 3               # what makes a group's first slot a head: the key | gid_in alone (equal keys) | both | a bucket start alone
# (reduce_tiles_per_wg, first_tiles_per_wg, sparse_max) beside the sort's own (0, 0, -1)
OVERRIDES = [(1, 1, 0), (2, 2, 2048), (3, 3, -1), (64, 64, 1), (2, 3, 5), (3, 2, 65)]
FORMS = ("first", "narrow", "later", "later_gid")


@pytest.fixture(scope="module")
def ctx():
    c = dark_amd.Context(CAP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """for the large cases: two lists of distinct words below CAP + 1000, random bytes and random words, made once and never written"""
    rng = np.random.default_rng(77)
    wide = CAP + 1000
    p = dict(wide=wide, perm_a=rng.permutation(wide).astype(np.uint32), perm_b=rng.permutation(wide).astype(np.uint32),
             bytes=rng.integers(0, 256, size=wide, dtype=np.uint8), words=rng.integers(0, 1 << 32, size=wide, dtype=np.uint32))
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return p


# ---- building a list from its groups ------------------------------------------------------------------------------------------------------------
def heavy_sizes(rng, count, a=1.5, cap=None):
    """group sizes from a heavy-tailed law (Zipf: mostly singletons and pairs, now and then thousands), summing to count"""
    out, total = [], 0
    while total < count:
        out.append(np.minimum(rng.zipf(a, size=max(count // 4, 16)), cap or count))  # (a draw can be 2^63)
        total += int(out[-1].sum())
    s = np.concatenate(out).astype(np.int64)
    s = s[:int(np.searchsorted(np.cumsum(s), count)) + 1]
    s[-1] -= int(s.sum()) - count
    return s[s > 0]


def sizes_from_heads(count, heads):
    h = np.unique(np.concatenate([[0], np.asarray(heads, dtype=np.int64)]))
    h = h[h < count]
    return np.diff(np.append(h, count))


def sizes_from_groups(count, groups):
    """groups: (start, size) of the groups of more than one member, in order and apart; every other slot is a singleton"""
    head = np.ones(count, bool)
    for start, size in groups:
        assert size >= 1 and start + size <= count
        head[start + 1:start + size] = False
    return sizes_from_heads(count, np.flatnonzero(head))


def make_case(rng, sizes, form, kinds=None, key_style="low", cmp_shift=None, zero=None, with_bwt=True, with_rank=True, with_sa=True, ls_max=1024,
              pool=None):
    """-> the arguments of rerank_model / Context.dbg_dev_rerank for a list whose groups have these sizes.  kinds: per group KEY / OLD / BOTH /
    FORCED (default: KEY; later_gid: a random mixture; narrow: up to 200 random FORCED).  key_style: the keys of neighbouring groups differ only
    below bit 32 ("low") or only from bit 32 up ("high").  zero: "final" / "survivor" puts suffix 0 into a group of one / of more.  Suffixes and
    positions are distinct words of a range somewhat wider than the list."""
    sizes = np.asarray(sizes, dtype=np.int64)
    count, ng = int(sizes.sum()), len(sizes)
    starts = np.cumsum(sizes) - sizes
    first, narrow = form in ("first", "narrow"), form == "narrow"
    if kinds is None:
        kinds = np.zeros(ng, np.int64)
        if form == "later_gid":
            kinds = rng.choice([KEY, OLD, BOTH], size=ng, p=[0.5, 0.25, 0.25])
        elif narrow and ng > 1:
            kinds[rng.integers(1, ng, size=min(200, ng))] = FORCED
    kinds = np.asarray(kinds)
    assert narrow or not (kinds == FORCED).any()
    assert form == "later_gid" or not ((kinds == OLD) | (kinds == BOTH)).any()
    field = np.repeat(np.cumsum((kinds == KEY) | (kinds == BOTH)) + 1, sizes).astype(np.uint64)
    kw = dict(pos_in=None, gid_in=None, cmp_shift=0, bucket_starts=None, sym_in=None, bwt=None, ls_max=ls_max)
    if narrow:
        kw["keys"] = field.astype(np.uint32)
        forced = starts[kinds == FORCED]
        assert len(forced) <= 250
        rest = 256 - len(forced)  # empty buckets: in front, behind, and twice the same start in the middle
        filler = np.concatenate([np.zeros(rest // 3, np.int64), np.full(rest // 3, count), np.resize(forced if len(forced) else [count], rest - 2 * (rest // 3))])
        kw["bucket_starts"] = np.sort(np.concatenate([forced, filler])).astype(np.uint32)
    else:
        keys = field << np.uint64(32) | np.uint64(0x9E3779B9) if key_style == "high" else field | np.uint64(0x5A5A << 40)
        if first:
            kw["cmp_shift"] = 8 if cmp_shift is None else cmp_shift
            if kw["cmp_shift"]:  # below the shift: noise that must not split anything
                keys = keys << np.uint64(kw["cmp_shift"]) | rng.integers(0, 1 << kw["cmp_shift"], size=count, dtype=np.uint64)
        kw["keys"] = keys
    big = pool is not None
    wide = pool["wide"] if big else count + 37
    idx = (pool["perm_a"][:count] if big else rng.permutation(wide)[:count].astype(np.uint32)).copy()
    if zero:
        cand = np.flatnonzero(sizes == 1 if zero == "final" else sizes > 1)
        if len(cand):
            g = int(cand[len(cand) // 2])
            at = int(starts[g]) + (0 if zero == "final" else int(sizes[g]) - 1)
            had = np.flatnonzero(idx == 0)
            if len(had):
                idx[had[0]] = idx[at]
            idx[at] = 0
    kw["idx"] = idx
    c = dict(form=form, count=count, kw=kw, rank=None, origin=None, sa=None)
    if first:
        if with_bwt:
            kw["bwt"] = pool["bytes"][:count] if big else rng.integers(0, 256, size=count, dtype=np.uint8)
            c["origin"] = FILL32
        if with_sa:  # handed in and never looked at: finals stand where they are
            c["sa"] = np.full(count, FILL32, np.uint32)
    else:
        kw["pos_in"] = pool["perm_b"][:count] if big else rng.permutation(wide)[:count].astype(np.uint32)
        if form == "later_gid":
            kw["gid_in"] = (np.repeat(np.cumsum((kinds == OLD) | (kinds == BOTH)), sizes) + 7).astype(np.uint32)
        if with_bwt:
            kw["bwt"] = pool["bytes"][:wide] if big else rng.integers(0, 256, size=wide, dtype=np.uint8)
            kw["sym_in"] = pool["bytes"][::-1][:count] if big else rng.integers(0, 256, size=count, dtype=np.uint8)
            c["origin"] = FILL32
        if with_rank:
            c["rank"] = pool["words"][:wide] if big else rng.integers(0, 1 << 32, size=wide, dtype=np.uint32)
        if with_sa:
            c["sa"] = np.full(wide, FILL32, np.uint32)
    return c


# ---- running and judging ------------------------------------------------------------------------------------------------------------------------
def expected(c):
    """the model's verdict on a case, once: (model, the arrays after the call)"""
    if "want" not in c:
        kw, n = c["kw"], c["count"]
        m = M.rerank_model(**kw)
        before = dict(out_idx=np.full(n + PAD, FILL32, np.uint32), out_pos=np.full(n + PAD, FILL32, np.uint32), out_gid=np.full(n + PAD, FILL32, np.uint32),
                      sym_out=None if kw["bwt"] is None else np.full(n + PAD, FILL8, np.uint8), gstart=np.full(n // 2 + 1 + PAD, FILL32, np.uint32),
                      bigidx=np.full(n // 2 + PAD, FILL32, np.uint32), bigoff=np.full(n // 2 + PAD, FILL32, np.uint32),
                      rank=c["rank"], sa=c["sa"], bwt=kw["bwt"], origin=c["origin"])
        c["want"] = (m, M.apply_model(m, kw["idx"], before))
    return c["want"]


def run(ctx, c, override=None, shift=None):
    shape = {} if override is None else dict(zip(("reduce_tiles_per_wg", "first_tiles_per_wg", "sparse_max"), override))
    return ctx.dbg_dev_rerank(rank=c["rank"], sa=c["sa"], origin=c["origin"], shift=shift, fill=FILL8, pad=PAD, **c["kw"], **shape)


def first_diff(what, got, want):
    if want is None or got is None:
        return None if want is None and got is None else "%s: %s, want %s" % (what, "null" if got is None else "an array", "null" if want is None else "an array")
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: %d entries, want %d" % (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return None
    i = int(bad[0])
    return "%s: %d of %d differ, first at %d: got %#x want %#x" % (what, len(bad), len(got), i, int(got[i]), int(want[i]))


def judge(label, got, c):
    m, want = expected(c)
    assert got["counts"] == m.counts, "%s: counts %s, model %s (%s)" % (label, got["counts"], m.counts, ", ".join(M.COUNT_NAMES))
    for name in ARRAYS:
        d = first_diff(name, got[name], want[name])
        assert d is None, "%s: %s" % (label, d)
    assert got["origin"] == want["origin"], "%s: origin %r, model %r" % (label, got["origin"], want["origin"])


def check(ctx, c, label, overrides=OVERRIDES, shift=None):
    """the sort's own shapes and every override against the model -- and so the same bytes from all of them"""
    label = "%s, %s form, %d slots" % (label, c["form"], c["count"])
    judge(label + ", the sort's own shapes", run(ctx, c, shift=shift), c)
    if c["form"].startswith("later"):  # k_rerank_apply has no shapes
        overrides = sorted({(o[0], 0, -1) for o in overrides})
    for o in overrides:
        judge(label + ", tiles per workgroup %d / %d, sparse limit %d" % o, run(ctx, c, o, shift), c)


def patterns(rng, count, form):
    """(name, case) of the patterns every size gets: all singletons, one group, all pairs, a heavy-tailed mixture, one group behind three
    singletons (its head is not slot 0, whose code in the running max is that of "no head yet")"""
    out = [("all singletons", np.ones(count, np.int64)), ("one group", [count]),
           ("all pairs", [2] * (count // 2) + [1] * (count % 2)), ("heavy tail", heavy_sizes(rng, count))]
    if count > 4:
        out.append(("one group from slot 3", [1, 1, 1, count - 3]))
    for i, (name, sizes) in enumerate(out):
        yield name, make_case(rng, sizes, form, key_style="high" if i % 2 else "low", zero=("final", "survivor", None)[i % 3],
                              with_bwt=i != 2, with_sa=i != 3 or form != "later", with_rank=i != 1 or form != "later")


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 7, 8, 9, 2047, 2048, 2049, 4095, 4097])
def test_small_counts(ctx, count):
    for form in FORMS:
        rng = np.random.default_rng(count * 10 + FORMS.index(form))
        for name, c in patterns(rng, count, form):
            check(ctx, c, name)


STRETCH_COUNTS = [t * TILE + d for t in (3, 64, 65, 129) for d in (-1, 0, 1)]


@pytest.mark.parametrize("count", STRETCH_COUNTS)
def test_stretches_of_tiles(ctx, count):
    """3, 64, 65 and 129 tiles, a slot less and a slot more, with 1, 2, 3 and 64 tiles per workgroup: full stretches, a short last stretch, a
    last stretch of one tile, a last tile of one slot"""
    for form in FORMS:
        rng = np.random.default_rng(count + FORMS.index(form))
        for name, c in patterns(rng, count, form):
            if name in ("one group", "heavy tail", "one group from slot 3") or form in ("first", "later_gid"):
                check(ctx, c, name)


# ---- borders ----------------------------------------------------------------------------------------------------------------------------------------
def border_heads(rng, count, turn=0, every=TILE):
    """heads around every multiple of `every`: on the last slot in front of it (the members follow behind it), on it (a group ends exactly there),
    on both (a singleton in front), on the slot behind it, or nowhere near (a group lies across); random heads in between"""
    heads = [np.flatnonzero(rng.random(count) < 0.01)]
    for i, b in enumerate(range(every, count, every)):
        near = np.arange(b - 3, min(b + 4, count))
        heads[0] = np.setdiff1d(heads[0], near)
        heads.append({0: [b - 1], 1: [b], 2: [b - 1, b], 3: [b + 1], 4: [], 5: [b - 2, b - 1, b, b + 1]}[(i + turn) % 6])
    return np.concatenate([np.asarray(h, dtype=np.int64) for h in heads])


@pytest.mark.parametrize("form", FORMS)
def test_heads_and_group_ends_on_tile_and_stretch_borders(ctx, form):
    """13 tiles and a few slots: with 1, 2 and 3 tiles per workgroup every kind of border of border_heads meets a tile border inside a stretch and
    a stretch border; every turn moves the kinds on by one border, so that each border sees each"""
    count = 13 * TILE + 5
    for turn in range(6):
        rng = np.random.default_rng(600 + turn)
        sizes = sizes_from_heads(count, border_heads(rng, count, turn))
        kinds = None
        if form == "narrow":  # the heads next to a border are bucket starts with equal words on both sides
            starts = np.cumsum(sizes) - sizes
            kinds = np.where(np.abs((starts + 4) % TILE - 4) <= 2, FORCED, KEY)
            kinds[0] = KEY
        check(ctx, make_case(rng, sizes, form, kinds=kinds, zero=("final", "survivor")[turn % 2]), "borders, turn %d" % turn)


# ---- the first rerank's sparse and dense tiles ---------------------------------------------------------------------------------------------------------
def tile_plan_sizes(plan):
    """plan: survivors per tile -- 0, 2 .. 2043 (one group inside the tile), 2048 (one group over the tile), or "pair" (the tile's last slot and
    the next tile's first: one survivor each, and the next tile must be 0 or 2048-free)"""
    groups = []
    for t, c in enumerate(plan):
        if c == "pair":
            groups.append((t * TILE + TILE - 1, 2))
        elif c == TILE:
            groups.append((t * TILE, TILE))
        elif c:
            assert 2 <= c <= TILE - 5
            groups.append((t * TILE + 3, c))
    count = len(plan) * TILE
    groups.sort()
    return sizes_from_groups(count, groups)


@pytest.mark.parametrize("limit", [-1, 0, 1, 5, 64, 2048])
def test_sparse_and_dense_tiles_inside_a_stretch(ctx, limit):
    """tiles of 0, 1, limit, limit + 1 and 2048 survivors mixed, surviving-free tiles at the start, in the middle and at the end of stretches of
    2, 3 and 64 tiles and whole stretches of them; the sparse limit as the sort has it (64) and passed"""
    s = 64 if limit < 0 else limit
    menu = [0, 0, 0, "pair", max(s, 2) if s <= TILE - 5 else TILE, min(max(s + 1, 2), TILE - 5), TILE, 2, 3]
    fixed = [0, "pair", 0, menu[4], menu[5], TILE, 0, 0, 0, 0, 0, 0, menu[4], 0, menu[5], 0, 0, TILE, "pair", 0]
    for turn in range(4):
        rng = np.random.default_rng(1000 + turn + 10 * s)
        plan = list(fixed)
        while len(plan) < 40:
            plan.append(0 if plan[-1] == "pair" else menu[int(rng.integers(0, len(menu)))])
        plan = plan[turn:] + [0] * turn  # the same tiles at other places of their stretches
        if plan[-1] == "pair":
            plan[-1] = 0
        for i in range(len(plan) - 1):  # a pair's second slot must be free
            if plan[i] == "pair" and plan[i + 1] == TILE:
                plan[i + 1] = 0
        for form in ("first", "narrow"):
            c = make_case(rng, tile_plan_sizes(plan), form, with_bwt=turn % 2 == 0, zero="survivor")
            over = [(r, f, limit) for r, f in ((1, 1), (2, 2), (3, 3), (64, 64), (1, 64))]
            check(ctx, c, "tile plan %d, sparse limit %d" % (turn, limit), overrides=over)


# ---- what makes a head ----------------------------------------------------------------------------------------------------------------------------
def test_key_bits(ctx):
    """keys that differ only from bit 32 up, only below bit 32 (make_case's styles, here with the shift and without), and only below cmp_shift = 8:
    the last is ONE group"""
    rng = np.random.default_rng(5)
    count = 2 * TILE + 77
    for style in ("low", "high"):
        for shift in (0, 8):
            c = make_case(rng, heavy_sizes(rng, count), "first", key_style=style, cmp_shift=shift)
            check(ctx, c, "%s bits differ, cmp_shift %d" % (style, shift))
        check(ctx, make_case(rng, heavy_sizes(rng, count), "later", key_style=style), "%s bits differ" % style)
    c = make_case(rng, [count], "first", cmp_shift=8)
    assert len(np.unique(c["kw"]["keys"])) > 200 and expected(c)[0].counts[:2] == (count, 1)
    check(ctx, c, "keys that differ below cmp_shift only")
    c = make_case(rng, [count], "first", cmp_shift=8)
    c["kw"]["cmp_shift"] = 0  # the same keys with every bit compared: the noise splits
    assert expected(c)[0].groups > 1
    check(ctx, c, "the same keys with cmp_shift 0")


def test_old_groups(ctx):
    """equal keys across an old-group border split, and that head is an old one: its members keep their ranks; an old group that splits in the
    middle gives ranks to the members behind the new head only"""
    rng = np.random.default_rng(6)
    sizes = [3, 2, 1, 4, 1, 1, 5] * 700 + [TILE + 9, 7, 1, 2]  # seven groups a turn, the kinds below; then a long one across a tile
    kinds = np.array([BOTH, KEY, OLD, OLD, KEY, BOTH, KEY] * 700 + [OLD, KEY, OLD, KEY])
    c = make_case(rng, sizes, "later_gid", kinds=kinds, zero="final")
    m, want = expected(c)
    idx, slot0 = c["kw"]["idx"], int(np.sum(sizes[:3]))
    assert m.head[slot0] and m.old_head[slot0] and c["kw"]["keys"][slot0] == c["kw"]["keys"][slot0 - 1]         # OLD: the old border alone splits
    assert np.array_equal(want["rank"][idx[slot0:slot0 + 4]], c["rank"][idx[slot0:slot0 + 4]])                  # ... and its members keep their ranks
    assert (want["rank"][idx[3:5]] == c["kw"]["pos_in"][3]).all()                                               # KEY inside an old group: ranked
    kept = int(np.isin(np.arange(len(idx)), m.ranked, invert=True).sum())
    assert 0 < kept < len(idx)
    check(ctx, c, "old groups")
    check(ctx, make_case(rng, heavy_sizes(rng, 3 * TILE + 1), "later_gid"), "a random mixture of old and new heads")
    sizes = heavy_sizes(rng, 3 * TILE + 1)  # every head an old head: no rank is written at all
    c = make_case(rng, sizes, "later_gid", kinds=np.full(len(sizes), OLD))
    assert len(expected(c)[0].ranked) == 0
    check(ctx, c, "old heads only")


def test_bucket_starts(ctx):
    """narrow keys, ONE word everywhere: only the bucket starts make heads.  On tile borders, on the borders of stretches of 2 and 3 tiles, next to
    them, twice the same (empty buckets), at 0 and at count (make_case's filler)"""
    rng = np.random.default_rng(8)
    count = 7 * TILE
    for marks in ([TILE, 2 * TILE, 3 * TILE, 4 * TILE, 6 * TILE], [TILE - 1, 2 * TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1, 6 * TILE - 1, count - 1],
                  [1, 2, 3, 4, 5, 6, 7, 8, 9, 2 * TILE - 8, 2 * TILE - 7], []):
        sizes = sizes_from_heads(count, marks)
        c = make_case(rng, sizes, "narrow", kinds=np.array([KEY] + [FORCED] * (len(sizes) - 1)), zero="survivor")
        assert len(np.unique(c["kw"]["keys"])) == 1 and expected(c)[0].head.sum() == len(sizes)
        assert {0, count} <= set(c["kw"]["bucket_starts"].tolist()) and len(set(c["kw"]["bucket_starts"].tolist())) < 200
        check(ctx, c, "bucket starts %s" % marks[:4])
    # 250 forced heads and as many made by the words, mixed
    sizes = heavy_sizes(rng, count + 3, cap=300)
    kinds = np.zeros(len(sizes), np.int64)
    kinds[rng.permutation(len(sizes) - 1)[:250] + 1] = FORCED
    check(ctx, make_case(rng, sizes, "narrow", kinds=kinds), "250 bucket starts")


def test_suffix_zero(ctx):
    """final in a later rerank: the origin is its SA position.  Surviving, or in the first rerank, or without L: the origin word stays"""
    rng = np.random.default_rng(9)
    sizes = heavy_sizes(rng, 2 * TILE + 100, cap=50)
    for form in FORMS:
        for zero in ("final", "survivor"):
            c = make_case(rng, sizes, form, zero=zero)
            m, want = expected(c)
            written = form.startswith("later") and zero == "final"
            assert (want["origin"] != FILL32) == written and (m.origin is not None) == written
            check(ctx, c, "suffix 0 %s" % zero)
    c = make_case(rng, sizes, "later", zero="final", with_bwt=False)
    assert expected(c)[1]["origin"] is None
    check(ctx, c, "suffix 0 final, no L")


@pytest.mark.parametrize("seed", range(6))
def test_random_mixtures(ctx, seed):
    """six turns of six lists: 1 .. 40 tiles and a rest, group sizes from Zipf laws of several exponents, every form, with and without each of the
    optional arrays"""
    rng = np.random.default_rng(2000 + seed)
    for turn in range(6):
        count = int(rng.integers(1, 41)) * TILE + int(rng.integers(-TILE + 1, TILE))
        form = FORMS[(seed + turn) % 4]
        sizes = heavy_sizes(rng, count, a=[1.2, 1.5, 2.0, 3.0][turn % 4], cap=[None, 3000, 40][turn % 3])
        c = make_case(rng, sizes, form, key_style=("low", "high")[turn % 2], zero=(None, "final", "survivor")[turn % 3], with_bwt=turn % 4 != 3,
                      with_rank=turn != 2, with_sa=turn != 4, ls_max=[1024, 2, 255][turn % 3])
        check(ctx, c, "mixture %d.%d" % (seed, turn), overrides=[OVERRIDES[(seed + turn) % 6], OVERRIDES[(seed + turn + 3) % 6]])


# ---- views that start behind their allocation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_unaligned_views(ctx, form):
    """keys a key behind their allocation (8 or 4 bytes off the 16-byte grid), gid_in and idx a word, sym_in and bwt 1, 3 and 7 bytes: the
    slot-by-slot branches of all three kernels over whole arrays instead of at their ends"""
    rng = np.random.default_rng(11)
    count = 5 * TILE + 3
    for turn, sizes in enumerate((heavy_sizes(rng, count), heavy_sizes(rng, count, a=3.0), sizes_from_heads(count, border_heads(rng, count)))):
        c = make_case(rng, sizes, form, zero="final")
        for shift in (dict(keys=1), dict(gid_in=1), dict(idx=1), dict(sym_in=1, bwt=1), dict(sym_in=3, bwt=3), dict(sym_in=7, bwt=7),
                      dict(keys=1, gid_in=1, idx=1, sym_in=7, bwt=3), dict(keys=3, gid_in=3, idx=2, sym_in=4, bwt=4)):
            check(ctx, c, "views shifted by %s, turn %d" % (shift, turn), overrides=OVERRIDES[1:4], shift=shift)


# ---- classification ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls_max", [1, 2, 255, 256, 1024])
def test_classification(ctx, ls_max):
    """groups of ls_max and ls_max + 1, PL_MAX and PL_MAX + 1 members among many of two and three (more than BG_TILE groups: several workgroups);
    no big group at all; every group big; big groups only in the last workgroup's stretch.  (Survivors have two members at least: with ls_max 1
    every group is big, and "no big group" is a list of singletons.)"""
    rng = np.random.default_rng(ls_max)
    special = [s for s in (ls_max, ls_max + 1, M.PL_MAX, M.PL_MAX + 1) if s >= 2]
    mixed = np.concatenate([rng.integers(1, 4, size=2 * M.BG_TILE + 100), np.repeat(special, 12)])
    rng.shuffle(mixed)
    cases = [("mixed", mixed),
             ("no big group", np.concatenate([rng.integers(1, min(ls_max, 3) + 1, size=3 * M.BG_TILE), [ls_max] * 9])),
             ("every group big", rng.integers(ls_max + 1, ls_max + 4, size=2 * M.BG_TILE + 7 if ls_max < 200 else 40))]
    if ls_max > 1:
        cases.append(("big groups in the last stretch only", np.concatenate([np.full(2 * M.BG_TILE + 5, 2), [ls_max + 1, 1, ls_max + 2, 2]])))
    for name, sizes in cases:
        for form in ("first", "later_gid"):
            c = make_case(rng, sizes, form, ls_max=ls_max, with_bwt=False)
            m = expected(c)[0]
            if name == "mixed":
                assert 0 < m.big_groups and (m.big_groups < m.groups or ls_max == 1) and m.groups > M.BG_TILE and m.above_pl_slots > 0
            elif name == "no big group":
                assert m.big_groups == 0 and (m.groups > M.BG_TILE or ls_max == 1)
            elif name == "every group big":
                assert m.big_groups == m.groups > 0
            else:
                assert m.groups > 2 * M.BG_TILE and m.big_groups == 2 and m.big.min() >= 2 * M.BG_TILE
            check(ctx, c, "%s, ls_max %d" % (name, ls_max), overrides=OVERRIDES[:2])


# ---- the three-phase scan --------------------------------------------------------------------------------------------------------------------------
def chunk_border_sizes(rng, count):
    """heavy-tailed groups, and at the chunk borders (tiles 1024, 2048 ...): a head on the last slot of tile 1023 with its members in tile 1024, a
    group that ends exactly on the second border, a singleton on each side of the third, one group across the fourth"""
    heads = np.flatnonzero(rng.random(count) < 0.3)
    edge = M.SCAN_CHUNK * TILE
    keep = np.ones(len(heads), bool)
    for b in range(edge, count, edge):
        keep &= np.abs(heads - b) > 40
    extra = [edge - 1, 2 * edge - 30, 2 * edge, 3 * edge - 1, 3 * edge, 3 * edge + 1, 4 * edge - 40, 4 * edge + 40, 5 * edge - 1]
    return sizes_from_heads(count, np.concatenate([heads[keep], [e for e in extra if e < count]]))


BIG_COUNTS = [4096 * TILE, 4096 * TILE + 1, 4097 * TILE - 3, BIG_TILES * TILE - TILE + 5]


@pytest.mark.parametrize("count", BIG_COUNTS)
def test_three_phase_scan(ctx, pool, count):
    """4096 tiles: the last size of the one-workgroup scan.  4096 tiles and a slot, 4097 tiles: two chunks.  5121 tiles: five chunks and one of a
    single tile, whose only slots are the list's last five.  One group over everything but three slots: the head is slot 3, a new head behind an
    old one, every tile behind reads its position from global memory, and the running max carries it through every tile and chunk.  Pairs and a few triples: nearly the most groups there can
    be, more than BG_GRID * BG_TILE of them from 4097 tiles on, so that a workgroup of the classification takes two tiles of groups, a big group
    in each."""
    rng = np.random.default_rng(count)
    c = make_case(rng, [1, 1, 1, count - 3], "later_gid", kinds=[KEY, OLD, KEY, KEY], pool=pool, zero="survivor")
    judge("one group from slot 3, later form, %d slots" % count, run(ctx, c), c)
    k = count * M.BG_TILE // (2 * M.BG_TILE + 1)  # groups: pairs, and every 4096th a triple -- the one big group (ls_max 2) of its tile of groups
    sizes = np.full(k, 2)
    sizes[M.BG_TILE - 1::M.BG_TILE] = 3
    c = make_case(rng, np.concatenate([sizes, np.ones(count - int(sizes.sum()), np.int64)]), "first", pool=pool, ls_max=2, with_sa=False)
    m = expected(c)[0]
    assert m.groups == k and (k > M.BG_GRID * M.BG_TILE) == (count >= 4097 * TILE - 3) and m.big_groups == k // M.BG_TILE
    judge("pairs, first form, %d slots" % count, run(ctx, c, (64, 64, 0)), c)
    if count in (BIG_COUNTS[0], BIG_COUNTS[-1]):
        sizes = chunk_border_sizes(rng, count)
        starts = np.cumsum(sizes) - sizes
        for form in ("later_gid", "narrow"):
            kinds = None
            if form == "narrow":
                kinds = np.where(starts % (M.SCAN_CHUNK * TILE) == 0, FORCED, KEY)
                kinds[0] = KEY
            c = make_case(rng, sizes, form, kinds=kinds, pool=pool, with_sa=form == "narrow", zero="final")
            got = run(ctx, c, None if form == "narrow" else (3, 0, -1))
            judge("chunk borders, %s form, %d slots" % (form, count), got, c)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_then_a_correct_call(ctx):
    lib, h = ctx._lib, ctx._h
    n = 5000
    filled = lambda words: torch.full((words,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")  # noqa: E731  (0xC3C3C3C3)
    bufs = {name: filled(2 * n) for name in ("keys", "starts", "idx", "pos", "gid", "rank", "sa", "bwt", "sym_in", "sym_out", "origin", "out_idx", "out_pos",
                                             "out_gid", "gstart", "bigidx", "bigoff")}
    counts = np.full(5, FILL32, np.uint32)
    torch.cuda.synchronize()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}

    def call(ctx_h=h, key_bytes=8, count=n, cmp_shift=0, reduce=0, first=0, sparse=-1, counts_p=C.c_void_p(counts.ctypes.data), **over):
        a = dict(p, starts=None)
        a.update(over)
        return lib.dk_dbg_dev_rerank(ctx_h, a["keys"], key_bytes, a["starts"], a["idx"], a["pos"], a["gid"], cmp_shift, count, a["rank"], a["sa"], a["bwt"],
                                     a["sym_in"], a["sym_out"], a["origin"], a["out_idx"], a["out_pos"], a["out_gid"], a["gstart"], a["bigidx"], a["bigoff"],
                                     1024, counts_p, reduce, first, sparse)

    first_form = dict(pos=None, gid=None, rank=None)
    refused = [("null context", dict(ctx_h=None)), ("no slots", dict(count=0)), ("above the capacity", dict(count=CAP + 1)),
               ("above 2^31 - 2", dict(count=(1 << 31) - 1)), ("keys of 2 bytes", dict(key_bytes=2)), ("keys of 16 bytes", dict(key_bytes=16)),
               ("narrow keys with d_pos_in", dict(key_bytes=4, starts=p["starts"], gid=None)),
               ("narrow keys with d_gid_in", dict(key_bytes=4, starts=p["starts"], pos=None, rank=None)),
               ("narrow keys without bucket starts", dict(first_form, key_bytes=4)), ("bucket starts with 8-byte keys", dict(first_form, starts=p["starts"])),
               ("d_rank in the first rerank", dict(pos=None, gid=None)), ("d_rank in the first rerank, old groups", dict(pos=None)),
               ("cmp_shift in a later rerank", dict(cmp_shift=8)), ("cmp_shift with narrow keys", dict(first_form, key_bytes=4, starts=p["starts"], cmp_shift=8)),
               ("cmp_shift 64", dict(first_form, cmp_shift=64)), ("cmp_shift -1", dict(first_form, cmp_shift=-1)),
               ("d_bwt without d_sym_out", dict(sym_out=None)), ("d_bwt without d_sym_in", dict(sym_in=None)), ("d_bwt without d_origin", dict(origin=None)),
               ("65 tiles per workgroup in the reduce kernel", dict(reduce=65)), ("65 tiles per workgroup in the first apply kernel", dict(first_form, first=65)),
               ("sparse limit 2049", dict(first_form, sparse=2049)), ("no counts", dict(counts_p=None))]
    refused += [("null " + name, {name: None}) for name in ("keys", "idx", "out_idx", "out_pos", "out_gid", "gstart", "bigidx", "bigoff")]
    for name, over in refused:
        assert call(**over) == DK_E_ARG, name
    assert b"rerank" in lib.dk_last_error(h)
    with ctx.batch_begin("dark", host_threads=1):
        assert call() == DK_E_ARG, "an open batch"
    assert b"batch" in lib.dk_last_error(h)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == -0x3C3C3C3D).all()), "a refused call wrote to " + name
    assert (counts == FILL32).all()
    rng = np.random.default_rng(12)
    for form in FORMS:
        check(ctx, make_case(rng, heavy_sizes(rng, n), form, zero="final"), "after refused calls")
