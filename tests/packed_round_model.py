"""TEST HELPER: plain numpy model of the segmented suffix sort of csrc/packed.hip, one step at a time -- what dk_dbg_dev_packed_first and
dk_dbg_dev_packed_round run (include/dark_amd.h), and what packed_sort_device chains.  The model is the definition of every output; it sorts with
a stable argsort and scans with cumulative maxima, and knows nothing of tiles.

  first(blocks)               the code table, the first keys, their stable sort, the first regroup
  round_(act, rank, off, h)   one round at depth h on ANY list and ANY ranks, and the guard words of the list it leaves
  by_prefixes(blocks, d)      the definition both must meet on a real pack, independent of everything above: rank[p] = off_blk + the suffixes of
                              p's block whose d-prefix is smaller (a proper prefix is smaller), live = the suffixes whose d-prefix is shared

wrong=<name> (WRONG) switches in one plausible kernel mistake: tests/test_packed_round_model.py proves with them that the cases of
tests/packed_round_cases.py can fail.  Only those variants know the kernels' shape (16 entries a thread, 4096 a tile, 1024 tiles a spine pass).
No variant ever runs on a GPU."""
from types import SimpleNamespace

import numpy as np

TILE, IPT, SPINE = 4096, 16, 1024
FILL32 = 0xC3C3C3C3
M32 = (1 << 32) - 1

WRONG = (
    "r2_without_h",        # 1  rank2 = rank[p + h], no + h: the short range [0, h) and the long one collide
    "end_inclusive",       # 2  p + h <= e takes the long branch: reads the rank of the next block's head
    "rbits_from_total",    # 3  rbits = ceil_log2(total): rank2 spills into the rank bits
    "old_on_whole_key",    # 4  old groups compared on the whole key: every new head is an old head
    "live_blind_16",       # 5  the live flag does not look at the next entry at a thread's last entry
    "live_blind_4096",     # 6  ... at a tile's last entry
    "nh_lost_at_tile",     # 7  the last new head is not carried into a tile
    "oh_lost_at_tile",     # 8  the last old head is not carried into a tile
    "spine_nh", "spine_oh", "spine_live",  # 9  one carry lost between spine passes, at tile 1024
    "live_scan_inclusive", "live_scan_late",  # 10 a tile's live count added twice / not at all in the exclusive scan
    "pad_as_smallest",     # 11 first keys: past the end coded like the smallest symbol
    "no_block_id",         # 12 first keys without the block id
    "k_unclamped",         # 13 k_used not clamped to total
    "guard_from_input",    # 14 guard words from the round's input list
)


def ceil_log2(x):
    return 0 if x <= 1 else (int(x) - 1).bit_length()


def offsets(blocks_or_sizes):
    sizes = [int(b) if np.isscalar(b) else len(b) for b in blocks_or_sizes]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def block_of(off, p):
    return np.searchsorted(off, p, side="right") - 1


def _last_head(flags, reset_every=0, reset_from=0):
    """per entry the index of the last set flag at or in front of it; reset_every / reset_from: a WRONG carry, forgotten at every such border / at
    that one index (the kernel's run value then starts from 0)"""
    idx = np.arange(len(flags), dtype=np.int64)
    marked = np.where(flags, idx, 0)
    if reset_every:
        pad = (-len(flags)) % reset_every
        m = np.concatenate([marked, np.zeros(pad, np.int64)]).reshape(-1, reset_every)
        return np.maximum.accumulate(m, axis=1).reshape(-1)[:len(flags)]
    if reset_from and reset_from < len(flags):
        return np.concatenate([np.maximum.accumulate(marked[:reset_from]), np.maximum.accumulate(marked[reset_from:])])
    return np.maximum.accumulate(marked)


def regroup(keys, vals, rbits, rank, wrong=None):
    """one scan over a sorted list: rank (changed in place) at the listed suffixes, -> (next list, c words with FILL32 behind `live`; live)"""
    c = len(keys)
    idx = np.arange(c, dtype=np.int64)
    old = np.zeros(c, np.uint64) if rbits >= 64 else keys >> np.uint64(rbits)
    nh = np.ones(c, bool)
    nh[1:] = keys[1:] != keys[:-1]
    oh = np.ones(c, bool)
    oh[1:] = old[1:] != old[:-1]
    if wrong == "old_on_whole_key":
        oh = nh.copy()
    differs_next = np.ones(c, bool)
    differs_next[:-1] = keys[1:] != keys[:-1]
    if wrong == "live_blind_16":
        differs_next |= idx % IPT == IPT - 1
    if wrong == "live_blind_4096":
        differs_next |= idx % TILE == TILE - 1
    live = ~(nh & differs_next)
    border = SPINE * TILE
    head_new = _last_head(nh, TILE if wrong == "nh_lost_at_tile" else 0, border if wrong == "spine_nh" else 0)
    head_old = _last_head(oh, TILE if wrong == "oh_lost_at_tile" else 0, border if wrong == "spine_oh" else 0)
    rank[vals] = ((old.astype(np.int64) + head_new - head_old) & M32).astype(np.uint32)
    nxt = np.full(c, FILL32, np.uint32)
    count = int(live.sum())
    if wrong in ("spine_live", "live_scan_inclusive", "live_scan_late"):
        per_tile = np.add.reduceat(live.astype(np.int64), np.arange(0, c, TILE))
        incl = np.cumsum(per_tile)
        base = incl - per_tile
        if wrong == "live_scan_inclusive":
            base = incl
        elif wrong == "live_scan_late":
            base = np.concatenate([[0], base[:-1]])
        else:
            base[SPINE:] -= base[SPINE] if len(base) > SPINE else 0
            count = int(per_tile[SPINE:].sum()) if len(base) > SPINE else count
        local = np.cumsum(live) - live - np.repeat(incl - per_tile, TILE)[:c]
        pos = np.repeat(base, TILE)[:c] + local
        ok = live & (pos < c)  # (a kernel would store past the list: the model drops those)
        nxt[pos[ok]] = vals[ok]
    else:
        nxt[:count] = vals[live]
    return nxt, count


def first(blocks, wrong=None):
    """-> code (256 uint16), sigma, bits, blk_bits, k_used, end_bit, keys / vals (the sorted list), rank, act (total words, FILL32 behind live), live, off"""
    blocks = [np.ascontiguousarray(b, dtype=np.uint8) for b in blocks]
    off = offsets(blocks)
    count, total = len(blocks), int(off[-1])
    text = np.concatenate(blocks)
    present = np.zeros(256, bool)
    present[text] = True
    code = np.where(present, np.cumsum(present), 0).astype(np.uint16)
    sigma = int(present.sum())
    bits = max(1, ceil_log2(sigma + 1))
    blk_bits = ceil_log2(count)
    k = max(1, (64 - blk_bits) // bits)
    k_used = k if wrong == "k_unclamped" else min(k, max(1, total))
    p = np.arange(total, dtype=np.int64)
    blk = block_of(off, p)
    e = off[blk + 1]
    keys = np.zeros(total, np.uint64) if wrong == "no_block_id" else blk.astype(np.uint64)
    padded = np.concatenate([code[text].astype(np.uint64), np.zeros(k_used, np.uint64)])
    for j in range(k_used):
        sym = np.where(p + j < e, padded[p + j], np.uint64(1 if wrong == "pad_as_smallest" else 0))
        keys = (keys << np.uint64(bits)) | sym
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], order.astype(np.uint32)
    rank = np.full(total, FILL32, np.uint32)
    act, live = regroup(keys, vals, 64, rank, wrong)
    return SimpleNamespace(code=code, sigma=sigma, bits=bits, blk_bits=blk_bits, k_used=k_used, end_bit=blk_bits + bits * k_used, keys=keys, vals=vals,
                           rank=rank, act=act, live=live, off=off, out=np.array([sigma, bits, blk_bits, k_used, live, blk_bits + bits * k_used, 0, 0], np.uint32))


def guard_words(act, off):
    g = np.zeros(len(off) - 1, np.uint32)
    act = np.asarray(act, dtype=np.int64)
    g[block_of(off, act[act < off[-1]])] = 1  # (a WRONG next list may hold words that are no suffix: a kernel would read past the table)
    return g


def round_(act, rank, off, h, wrong=None):
    """one round on the list act at depth h; rank (total words) is NOT changed: -> keys / vals (the sorted list), rank (the new array), next_act
    (c words, FILL32 behind live), live, rbits, gbits, guard (count words)"""
    off = np.asarray(off, dtype=np.int64)
    total = int(off[-1])
    act = np.asarray(act, dtype=np.uint32)
    p = act.astype(np.int64)
    rank = np.array(rank, dtype=np.uint32)
    rbits = ceil_log2(total if wrong == "rbits_from_total" else total + h)
    gbits = ceil_log2(total)
    e = off[block_of(off, p) + 1]
    long_ = p + h <= e if wrong == "end_inclusive" else p + h < e
    behind = np.concatenate([rank.astype(np.int64), [0]])[np.minimum(p + h, total)]  # (a kernel that reads rank[total] reads past the array)
    r2 = np.where(long_, behind + (0 if wrong == "r2_without_h" else h), e - 1 - p)
    keys = (rank[p].astype(np.uint64) << np.uint64(rbits)) | r2.astype(np.uint64)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], act[order]
    nxt, live = regroup(keys, vals, rbits, rank, wrong)
    guard = guard_words(act if wrong == "guard_from_input" else nxt[:live], off)
    return SimpleNamespace(keys=keys, vals=vals, rank=rank, next_act=nxt, live=live, rbits=rbits, gbits=gbits, guard=guard,
                           out=np.array([rbits, gbits, live, 0, 0, 0, 0, 0], np.uint32))


def by_prefixes(blocks, d, settled=None):
    """the definition: -> (rank, sorted array of the live suffixes) at depth d, from the prefixes themselves.  settled (a dict the caller keeps
    over growing d): the ranks of the blocks whose prefixes were all distinct at a smaller depth -- distinct prefixes stay distinct and in their
    order at every greater one, so such a block is not sorted again"""
    off = offsets(blocks)
    rank = np.zeros(int(off[-1]), np.uint32)
    live = []
    for i, (b, o) in enumerate(zip(blocks, off[:-1])):
        if settled is not None and i in settled:
            rank[o:o + len(b)] = settled[i]
            continue
        t = bytes(bytearray(np.asarray(b, dtype=np.uint8)))
        pre = [t[p:p + d] for p in range(len(t))]
        srt = sorted(pre)  # (bytes compare as the sort must: a proper prefix is smaller)
        head, members = {}, {}
        for j, s in enumerate(srt):
            head.setdefault(s, j)
            members[s] = members.get(s, 0) + 1
        shared = False
        for p, s in enumerate(pre):
            rank[o + p] = o + head[s]
            if members[s] > 1:
                live.append(int(o) + p)
                shared = True
        if settled is not None and not shared:
            settled[i] = rank[o:o + len(b)].copy()
    return rank, np.array(live, dtype=np.uint32)


def chain(blocks, max_rounds=64):
    """first and then rounds to the end: -> (the first step, [every round's result])"""
    f = first(blocks)
    act, rank, h, rounds = f.act[:f.live], f.rank, f.k_used, []
    while len(act) and len(rounds) < max_rounds:
        r = round_(act, rank, f.off, h)
        rounds.append(r)
        act, rank, h = r.next_act[:r.live], r.rank, 2 * h
    return f, rounds
