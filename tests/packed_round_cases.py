"""TEST HELPER: the cases of tests/test_gpu_packed_round.py and tests/test_packed_round_model.py, built from their seeds -- packs for the first step
of the segmented suffix sort (FIRST), built states for one round (ROUNDS, and large() for the one that reaches a second spine pass) and the pack the
chain runs on -- and the glue of the GPU test: call_*, check_*.

A built round is a state no text need stand behind.  Two builders:
  random_round   a list drawn from the pack, old groups drawn over it, the other ranks drawn from `ties` values: few values, many equal keys
  laid_round     the SORTED list is what is laid out -- the sizes of its new groups and which of them start an old group -- and realised at
                 h = 1: the listed suffixes at even positions, each with its own partner behind it, whose rank is the new group's number.  So the
                 list is half the pack at most, and every border of 16 and of 4096 entries falls where the case wants it."""
from types import SimpleNamespace

import numpy as np

import packed_round_model as M

PAD, FILL32, FILL64 = 64, M.FILL32, 0xC3C3C3C3C3C3C3C3
TILE = M.TILE
LARGE_C = 1024 * TILE + TILE + 1  # 1025 tiles and one entry: k_pk_spine's second pass


# ---- first keys -----------------------------------------------------------------------------------------------------------------------------

def _draw(rng, alphabet, n):
    return np.array(list(alphabet), dtype=np.uint8)[rng.integers(0, len(alphabet), n)]


def _with_all(rng, alphabet, n):
    """n bytes over the alphabet, every symbol present"""
    a = np.asarray(alphabet, dtype=np.uint8)
    return np.concatenate([rng.permutation(a), _draw(rng, a, n - len(a))])


def _sigma(s, seed):
    def make():
        rng = np.random.default_rng(seed)
        alphabet = rng.permutation(256)[:s] if s < 256 else np.arange(256)
        return [_with_all(rng, alphabet, max(700, 2 * s)), _draw(rng, alphabet, 300)]
    return make


def _counted(count, seed, one_byte=False):
    def make():
        rng = np.random.default_rng(seed)
        if one_byte:
            return list(rng.integers(0, 256, (count, 1), dtype=np.uint8))
        return [_draw(rng, b"abc", int(n)) for n in rng.integers(1, 61, count)]
    return make


def _sized(sizes, alphabet, seed):
    def make():
        rng = np.random.default_rng(seed)
        return [_draw(rng, alphabet, n) for n in sizes]
    return make


def _prefix_blocks():
    x = _draw(np.random.default_rng(41), b"ab", 50)
    return [x, x[:20], x[:49]]


# name -> (builder, the out words the case is named for, a property of the model's result or None)
FIRST = {
    "count_1": (_counted(1, 1), dict(blk_bits=0), None),
    "count_2": (_counted(2, 2), dict(blk_bits=1), None),
    "count_64": (_counted(64, 3), dict(blk_bits=6), None),
    "count_65": (_counted(65, 4), dict(blk_bits=7), None),
    "count_65536_of_one_byte": (_counted(65536, 5, one_byte=True), dict(blk_bits=16, sigma=256, bits=9, k_used=5, live=0), None),
    "sigma_1_below_64": (lambda: [np.full(40, 0x41, np.uint8)], dict(sigma=1, bits=1, k_used=40, end_bit=40), None),
    "sigma_1_above_64": (lambda: [np.full(200, 0x41, np.uint8)], dict(sigma=1, bits=1, k_used=64, end_bit=64), lambda f: int(f.keys.max()) == (1 << 64) - 1),
    "sigma_3": (_sigma(3, 13), dict(sigma=3, bits=2), None),
    "sigma_4": (_sigma(4, 14), dict(sigma=4, bits=3), None),
    "sigma_7": (_sigma(7, 17), dict(sigma=7, bits=3), None),
    "sigma_8": (_sigma(8, 18), dict(sigma=8, bits=4), None),
    "sigma_255": (_sigma(255, 19), dict(sigma=255, bits=8), None),
    "sigma_256": (_sigma(256, 20), dict(sigma=256, bits=9), lambda f: int(f.code.max()) == 256),
    "bytes_not_contiguous": (_sized([900, 333], [0x00, 0x07, 0x80, 0xFE, 0xFF], 21), dict(sigma=5, bits=3),
                             lambda f: [int(f.code[c]) for c in (0x00, 0x07, 0x80, 0xFE, 0xFF, 0x01)] == [1, 2, 3, 4, 5, 0]),
    # heads at 256, 4096 and 8192 (on), 8447 (off), 8448 (on), 8549 (off)
    "heads_on_and_off_256_and_4096": (_sized([256, 3840, 4096, 255, 1, 101, 77], b"abc", 22), dict(blk_bits=3),
                                      lambda f: list(f.off[1:6]) == [256, 4096, 8192, 8447, 8448]),
    "blocks_1_2_3_4095_4096_4097": (_sized([1, 2, 3, 4095, 4096, 4097], b"abc", 23), dict(blk_bits=3), None),
    # bits = 2, blk_bits = 2: a key holds 31 symbols, the first and the last block fewer -- the zero padding decides their order
    "block_shorter_than_the_key": (lambda: [np.frombuffer(b"ab" * 3, np.uint8), np.frombuffer(b"ab" * 40, np.uint8), np.full(5, 0x61, np.uint8)],
                                   dict(bits=2, blk_bits=2, k_used=31), lambda f: f.live > 0 and bool((f.rank[:6] == [2, 5, 1, 4, 0, 3]).all())),
    # the same text in three blocks: ranks stay inside each block's slots
    "a_block_a_prefix_of_another": (_prefix_blocks, dict(blk_bits=2), lambda f: all(
        bool(((f.rank[a:b] >= a) & (f.rank[a:b] < b)).all()) for a, b in zip(f.off[:-1], f.off[1:]))),
}


def first_blocks(name):
    return FIRST[name][0]()


# ---- built rounds ---------------------------------------------------------------------------------------------------------------------------

def _case(name, sizes, h, act, rank, guard=True):
    return SimpleNamespace(name=name, sizes=[int(n) for n in sizes], off=M.offsets(sizes), h=int(h), act=np.ascontiguousarray(act, dtype=np.uint32),
                           rank=np.ascontiguousarray(rank, dtype=np.uint32), guard=guard)


def random_round(name, sizes, c, h, seed, gmax=6, ties=4, force=(), exclude=(), sort_first=False, guard=True):
    """c listed suffixes (the forced ones among them) in drawn order; old groups of 1 .. gmax members over the list with ranks that leave each its
    room; every other rank one of `ties` drawn values"""
    rng = np.random.default_rng(seed)
    total = int(sum(sizes))
    rest = np.setdiff1d(np.arange(total), np.concatenate([np.asarray(force, dtype=np.int64), np.asarray(exclude, dtype=np.int64)]))
    act = rng.permutation(np.concatenate([np.asarray(force, dtype=np.int64), rng.choice(rest, c - len(force), replace=False)]))
    msizes = []
    while sum(msizes) < c:
        msizes.append(min(int(rng.integers(1, gmax + 1)), c - sum(msizes)))
    msizes = np.array(msizes)
    slack = np.sort(rng.integers(0, total - c + 1, len(msizes)))
    slack[0] = 0  # an old group with the rank 0
    g = np.cumsum(msizes) - msizes + slack
    rank = rng.integers(0, total, ties)[rng.integers(0, ties, total)]
    rank[rng.permutation(act)] = np.repeat(g, msizes)
    case = _case(name, sizes, h, act, rank, guard)
    if sort_first:  # the list in the order the round's sort leaves it: the sort has nothing to move
        case.act = M.round_(case.act, case.rank, case.off, case.h).vals.copy()
    return case


def laid_round(name, new_sizes, old_start, seed, tail=(3,), scrambled=True, rank0=True):
    """new_sizes: the sizes of the new groups along the sorted list; old_start[k]: new group k starts an old group (the first one does)"""
    rng = np.random.default_rng(seed)
    new_sizes, old_start = np.asarray(new_sizes, dtype=np.int64), np.asarray(old_start, dtype=bool).copy()
    old_start[0] = True
    c = int(new_sizes.sum())
    sizes = [2 * c] + list(tail)
    total = int(sum(sizes))
    new_id = np.repeat(np.arange(len(new_sizes)), new_sizes)            # per slot of the sorted list
    old_id = np.repeat(np.cumsum(old_start) - 1, new_sizes)
    old_first = np.flatnonzero(np.r_[True, old_id[1:] != old_id[:-1]])  # list index of every old group's head
    slack = np.sort(rng.integers(0, total - c + 1, len(old_first)))
    if rank0:
        slack[0] = 0
    g = old_first + slack
    where = 2 * rng.permutation(c)                                      # the suffix at every slot: even positions of block 0
    rank = rng.integers(0, total, total)
    rank[where] = g[old_id]
    rank[where + 1] = new_id
    act = where[rng.permutation(c)] if scrambled else where
    return _case(name, sizes, 1, act, rank)


def _pairs_across_every_border(c):
    """a singleton, then pairs: every pair starts at an odd index, so one lies across every border of 16 and of 4096; old groups of even size behind
    the first, so that none of them cuts a pair"""
    new = [1] + [2] * ((c - 1) // 2) + [1] * ((c - 1) % 2)
    old = np.zeros(len(new), bool)
    old[1::37] = True
    return new, old


def _three_tiles():
    """old group B = slots [4, 9016): its new group of 9000 starts at slot 12 and ends in tile 2 -- tile 1 holds no head of either kind"""
    rng = np.random.default_rng(77)
    head, b = [1, 2, 1], [5, 3, 9000, 2, 1, 1]
    rest = []
    while sum(rest) < 3 * TILE + 5 - 4 - 9012:
        rest.append(min(int(rng.integers(1, 4)), 3 * TILE + 5 - 4 - 9012 - sum(rest)))
    new = head + b + rest
    old = np.zeros(len(new), bool)
    old[[0, 3]] = True
    old[9:] = rng.random(len(rest)) < 0.4
    old[9] = True
    return new, old


def _singletons_and_pairs(c, seed):
    rng = np.random.default_rng(seed)
    new = []
    while sum(new) < c:
        new.append(min(int(rng.integers(1, 3)), c - sum(new)))
    return new, rng.random(len(new)) < 0.2


def _collision():
    """one block of 40 bytes at offset 0, h = 8, three suffixes of one old group (rank 20): 10 is long with rank[18] = 4 < h, 35 is short with
    e - 1 - 35 = 4, 32 ends exactly at e (p + h == e: short, rank2 = 7).  Without the + h the first two collide."""
    rank = np.arange(40, dtype=np.uint32)[::-1].copy()
    rank[[10, 35, 32]] = 20
    rank[18] = 4
    return _case("collision_of_short_and_long", [40], 8, [35, 10, 32], rank)


def _guard_300():
    """300 blocks; blocks 7 and 8 hold no listed suffix (nor do some of the others); block 5's listed suffixes are its first two, an old group of
    their own that falls apart in this round: the block is in the input list and not in the next one"""
    sizes = np.random.default_rng(300).integers(2, 41, 300)
    off = M.offsets(sizes)
    a = int(off[5])
    skip = np.concatenate([np.arange(off[i], off[i + 1]) for i in (5, 7, 8)])
    case = random_round("guard_300_blocks", sizes, 1500, 1, 301, ties=3, force=(a, a + 1), exclude=skip)
    case.rank[[a, a + 1]] = int(off[-1]) - 2
    return case


def _rounds():
    r = {}
    three = 3 * TILE + 5
    for c in (1, 2, 15, 16, 17, TILE - 1, TILE, TILE + 1):
        r["c_%d" % c] = lambda c=c: random_round("c_%d" % c, [c // 2 + 1, c - c // 2 + 6], c, 3, 100 + c)
    r["c_3_tiles_5_whole_pack"] = lambda: random_round("c_3_tiles_5_whole_pack", [5000, 7000, three - 12000], three, 5, 112, gmax=9)
    r["list_already_sorted"] = lambda: random_round("list_already_sorted", [3000, 2000], 4500, 2, 113, sort_first=True)
    r["all_keys_equal"] = lambda: laid_round("all_keys_equal", [TILE + 9], [True], 114, rank0=False)
    r["all_keys_distinct"] = lambda: laid_round("all_keys_distinct", [1] * (TILE + 9), np.arange(TILE + 9) % 5 == 0, 115)
    r["pairs_across_every_border"] = lambda: laid_round("pairs_across_every_border", *_pairs_across_every_border(2 * TILE + 5), 116)
    r["pairs_across_every_border_in_order"] = lambda: laid_round("pairs_across_every_border_in_order", *_pairs_across_every_border(TILE + 40), 117, scrambled=False)
    r["old_group_over_three_tiles"] = lambda: laid_round("old_group_over_three_tiles", *_three_tiles(), 118)
    r["singletons_and_pairs"] = lambda: laid_round("singletons_and_pairs", *_singletons_and_pairs(700, 119), 119, tail=(2, 9))
    r["h_1"] = lambda: random_round("h_1", [900, 100], 600, 1, 120)
    # total = 12293: total + h = 2^14 (rbits 14), and one more (rbits 15)
    r["rbits_at_a_power_of_two"] = lambda: random_round("rbits_at_a_power_of_two", [three], 2000, (1 << 14) - three, 121)
    r["rbits_past_a_power_of_two"] = lambda: random_round("rbits_past_a_power_of_two", [three], 2000, (1 << 14) - three + 1, 121)
    r["h_at_least_the_longest_block"] = lambda: random_round("h_at_least_the_longest_block", [700, 512, 300], 900, 700, 122, ties=2)
    r["short_and_long_in_one_old_group"] = lambda: random_round("short_and_long_in_one_old_group", [400, 300], 500, 150, 123, gmax=60, ties=3,
                                                                force=(250, 550))  # 250 + 150 = e_0 and 550 + 150 = e_1: p + h == e
    r["collision_of_short_and_long"] = _collision
    r["guard_1_block"] = lambda: random_round("guard_1_block", [800], 300, 4, 124)
    r["guard_2_blocks_one_unlisted"] = lambda: random_round("guard_2_blocks_one_unlisted", [800, 40], 300, 4, 125, force=tuple(range(0, 600, 2)))
    r["guard_300_blocks"] = _guard_300
    r["no_guard_words"] = lambda: random_round("no_guard_words", [500, 77], 200, 2, 126, guard=False)
    return r


ROUNDS = _rounds()


def duties(c):
    """what dk_dbg_dev_packed_round leaves to its caller (include/dark_amd.h)"""
    total = int(c.off[-1])
    assert 0 < len(c.act) <= total and len(c.rank) == total and 0 < c.h <= 1 << 31
    assert len(np.unique(c.act)) == len(c.act) and int(c.act.max()) < total and int(c.rank.max()) < total
    g, members = np.unique(c.rank[c.act], return_counts=True)
    assert bool((g.astype(np.int64) + members <= total).all())


def large():
    """c = 1025 tiles + 1.  Old group X starts 50 slots in front of slot 1024 * 4096; its third new group starts 40 in front and runs to the end of
    tile 1024, which therefore holds no head at all; the last slot, alone in tile 1025, is a singleton of X.  In front of X: singletons, pairs and
    triples (live entries on both sides of the border)."""
    rng = np.random.default_rng(1024)
    border = 1024 * TILE
    left = rng.choice(np.array([1, 1, 2, 3]), border)
    left = left[np.cumsum(left) <= border - 50]
    left = np.append(left, border - 50 - left.sum()) if left.sum() < border - 50 else left
    new = np.concatenate([left, [7, 3, 40 + TILE, 1]])
    old = rng.random(len(new)) < 0.3
    old[len(left)] = True
    old[len(left) + 1:] = False
    assert int(new.sum()) == LARGE_C
    return laid_round("two_spine_passes", new, old, 1025, tail=(1,))


def chain_blocks():
    """the mixed pack of tests/test_gpu_packed.py cut to blocks of at most 5000 bytes"""
    from test_gpu_packed import mixed_blocks
    return [b[i:i + 5000] for b in mixed_blocks() for i in range(0, len(b), 5000)]


# ---- the GPU test's glue --------------------------------------------------------------------------------------------------------------------

def framed(a, fill):
    a = np.asarray(a)
    g = np.full(PAD, fill, a.dtype)
    return np.concatenate([g, a, g])


def same(name, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s has %s entries, the model %s" % (name, what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), "%s: %s differs at %d of %d entries, first at %d (framed by %d guards): got %s, want %s" % (
        name, what, len(bad), len(want), bad[0], PAD, got[bad[:4]], want[bad[:4]])


def check_first(name, got, m):
    """every output WHOLE: guards, the untouched tail of act, code and out"""
    same(name, "out", got["out"], m.out)
    same(name, "code", got["code"], m.code)
    same(name, "keys", got["keys"], framed(m.keys, FILL64))
    same(name, "vals", got["vals"], framed(m.vals, FILL32))
    same(name, "rank", got["rank"], framed(m.rank, FILL32))
    same(name, "act", got["act"], framed(m.act, FILL32))


def call_round(ctx, c):
    return ctx.dbg_dev_packed_round(c.sizes, c.h, c.act, c.rank, guard=c.guard, fill=0xC3, pad=PAD)


def check_round(name, got, m, guard=True):
    same(name, "out", got["out"], m.out)
    same(name, "keys", got["keys"], framed(m.keys, FILL64))
    same(name, "vals", got["vals"], framed(m.vals, FILL32))
    same(name, "rank", got["rank"], framed(m.rank, FILL32))
    same(name, "next_act", got["next_act"], framed(m.next_act, FILL32))
    if guard:
        same(name, "guard", got["guard"], framed(m.guard, FILL32))
    else:
        assert got["guard"] is None
