"""TEST HELPER: plain model of the last stage of the suffix-array path -- what dk_dbg_dev_in_place (in_place_rounds of csrc/suffix_array.hip) must
produce from a list.  Written from the comments that head the two sections of that file ("plateau rounds", "pair chains"), in numpy over whole
arrays; nothing here works tile by tile.

The state (a dict):  n, h | idx, meta, pos, sym (per slot; sym None in the suffix-array mode) | rank (n words) | sa or bwt (n entries), origin.
  idx     the slot's suffix; suffix | bit 31: final since the last round; 0xFFFFFFFF: dead for longer (settled by the chains, or final before)
  meta    offset inside the group | (group size - 1) << 8 | MOVED
The second rank of suffix x at offset o is rank[x + o] + o, or n - 1 - x when x + o >= n (the shorter suffix is the smaller one, and all of them
stand in front of every suffix that goes on).

run() drives the pieces the way the host does: the live count of a round is read one round late, so one more round is launched than needed
(it finds nothing alive and does nothing), and `rounds` counts launches.  `broken` breaks one rule (tests/test_in_place_model.py shows that the
cases notice): "tie_order", "moved_bit", "text_end"."""
import numpy as np

PL_BITS, PL_MAX = 8, 256
OFF_MASK = 0xFF
MOVED = 1 << 16
DEAD, DEAD_BIT = 0xFFFFFFFF, 0x80000000
WALK_THROUGH, WALK_FREE = 1024, 16   # strides of h a chain end may walk with / without a later record of its delta (one comparison more each)
LT, GT = 2, 4
COMPACT_FROM = 1 << 16               # the sort compacts a list of at least this many slots once three quarters of it are dead
ONE_WORKGROUP = 4096                 # slots one workgroup of the record extraction takes: below, a full list is deterministic (nothing fits)


def second_rank(rank, x, o, n, broken=None):
    x = np.asarray(x, dtype=np.int64)
    p = x + o
    inside = p < n
    past = (x + 2 * o) if broken == "text_end" else (n - 1 - x)
    return np.where(inside, rank[np.minimum(p, n - 1)].astype(np.int64) + o, past)


def to_inplace(gid, gstart):
    gid = np.asarray(gid, dtype=np.int64)
    gstart = np.asarray(gstart, dtype=np.int64)
    a = np.arange(len(gid), dtype=np.int64)
    return ((a - gstart[gid]) | ((gstart[gid + 1] - gstart[gid] - 1) << PL_BITS)).astype(np.uint32)


def chain_records(idx, meta, kmax):
    """every pair inside a live group of 2 .. kmax members -> (slot of the first member, distance in slots, lower position, delta), ordered by
    (delta, lower position)"""
    idx = idx.astype(np.int64)
    off, last = (meta & OFF_MASK).astype(np.int64), ((meta >> PL_BITS) & OFF_MASK).astype(np.int64)
    ok = (idx < DEAD_BIT) & (last >= 1) & (last < kmax)
    slot, dist = [], []
    for d in range(1, kmax):
        a = np.flatnonzero(ok & (off + d <= last))
        slot.append(a)
        dist.append(np.full(len(a), d, np.int64))
    slot, dist = np.concatenate(slot), np.concatenate(dist)
    v, w = idx[slot], idx[slot + dist] & (DEAD_BIT - 1)
    lo, delta = np.minimum(v, w), np.abs(v - w)
    order = np.lexsort((lo, delta))
    return slot[order], dist[order], lo[order], delta[order]


def chain_verdicts(lo, delta, rank, n, h, broken=None):
    """-> (verdict per record: 0 undecided | LT: the lower position is the smaller suffix | GT, the walks: (record, comparisons, how it ended:
    "verdict" / "continues" / "undecided", did a comparison look past the text's end) per record that does not continue at once)"""
    m = len(lo)
    nxt_same = np.zeros(m, bool)
    nxt_same[:-1] = delta[1:] == delta[:-1]
    cont = np.zeros(m, bool)
    cont[:-1] = nxt_same[:-1] & (lo[1:] == lo[:-1] + 1)
    own = np.zeros(m, np.uint8)
    end = ~cont
    walks = []
    for r in np.flatnonzero(end).tolist():
        gap = int(lo[r + 1] - lo[r]) if nxt_same[r] else 0
        o, how, compared, past = 1, "undecided", 0, False
        for _ in range((WALK_THROUGH if gap else WALK_FREE) + 1):
            a, b = second_rank(rank, [lo[r], lo[r] + delta[r]], o, n, broken).tolist()
            compared += 1
            past |= bool(lo[r] + delta[r] + o >= n)
            if a != b:
                own[r], how = (LT if a < b else GT), "verdict"
                break
            o += h
            if gap and o >= gap:  # equal all the way to the next record of this delta: the chain goes on there
                end[r], how = False, "continues"
                break
        walks.append((r, compared, how, past))
    at = np.where(end, np.arange(m), m)
    nearest = np.minimum.accumulate(at[::-1])[::-1]  # the nearest chain end at or after every record (the last record always is one)
    return own[nearest], walks


def chains(s, kmax, cap=0, broken=None):
    """the pair chains on a state behind to_inplace -> dict(records, list_full, settled, pairs = (lower position, higher, verdict) per record,
    walks = those of chain_verdicts)"""
    n, h = s["n"], min(s["h"], s["n"])
    idx, meta, pos, rank = s["idx"], s["meta"], s["pos"], s["rank"]
    slots = len(idx)
    none = dict(records=0, list_full=0, settled=0, pairs=[], walks=[])
    if slots < 2:
        return none
    slot, dist, lo, delta = chain_records(idx, meta, kmax)
    m = len(slot)
    if m > (cap or n):
        assert slots <= ONE_WORKGROUP, "which records fit depends on the order of the workgroups: no model"
        return dict(none, list_full=1)
    if m == 0:
        return none
    verdict, walks = chain_verdicts(lo, delta, rank, n, h, broken)
    planes = np.zeros((kmax, slots), np.uint8)
    planes[dist, slot] = verdict
    live_head = (idx < DEAD_BIT) & ((meta & OFF_MASK) == 0)
    size = ((meta >> PL_BITS) & OFF_MASK).astype(np.int64) + 1
    settled = 0
    for g in range(2, kmax + 1):
        heads = np.flatnonzero(live_head & (size == g))
        x = np.stack([idx[heads + i].astype(np.int64) for i in range(g)])
        before = np.zeros((g, len(heads)), np.int64)
        decided = np.ones(len(heads), bool)
        for i in range(g):
            for j in range(i + 1, g):
                v = planes[j - i, heads + i]
                decided &= v != 0
                i_first = (x[i] < x[j]) == (v == LT)
                before[j] += i_first
                before[i] += ~i_first
        heads, x, before = heads[decided], x[:, decided], before[:, decided]
        for i in range(g):
            p = pos[heads + before[i]]
            if s["sym"] is None:
                s["sa"][p] = x[i]
            else:
                s["bwt"][p] = s["sym"][heads + i]
                if (x[i] == 0).any():
                    s["origin"] = int(p[x[i] == 0][0])
            moved = before[i] > 0  # the smallest keeps the group's rank
            rank[x[i][moved]] = p[moved]
        for i in range(g):
            idx[heads + i] = DEAD
        settled += g * len(heads)
    return dict(records=m, list_full=0, settled=settled, pairs=list(zip(lo.tolist(), (lo + delta).tolist(), verdict.tolist())), walks=walks)


def one_round(s, broken=None):
    """one in-place round at depth min(h, n) -> live slots afterwards; h doubles (capped at 2 n)"""
    n, h = s["n"], min(s["h"], s["n"])
    idx, meta, pos, rank = s["idx"], s["meta"], s["pos"], s["rank"]
    slots = len(idx)
    a = np.flatnonzero(idx < DEAD_BIT)
    x = idx[a].astype(np.int64)
    gs = a - (meta[a] & OFF_MASK)
    r2 = second_rank(rank, x, h, n, broken)
    order = np.lexsort((-a if broken == "tie_order" else a, r2, gs))  # stable inside every group: ties in slot order
    a, x, gs, r2 = a[order], x[order], gs[order], r2[order]
    k = np.arange(len(a))
    first_of_old = np.ones(len(a), bool)
    first_of_old[1:] = gs[1:] != gs[:-1]
    first_of_new = first_of_old.copy()
    first_of_new[1:] |= r2[1:] != r2[:-1]
    old_at = np.maximum.accumulate(np.where(first_of_old, k, 0))
    new_at = np.maximum.accumulate(np.where(first_of_new, k, 0))
    dest = gs + (k - old_at)
    head = gs + (new_at - old_at)            # slot of the new group's head
    ends = np.append(np.flatnonzero(first_of_new)[1:], len(a))
    size = (ends - np.flatnonzero(first_of_new))[np.cumsum(first_of_new) - 1]
    moved = head != gs
    if broken == "moved_bit":  # only the last new group of every old one
        moved &= np.append(first_of_old, True)[ends[np.cumsum(first_of_new) - 1]]
    single = size == 1
    new_idx = np.full(slots, DEAD, np.uint32)
    new_meta = np.zeros(slots, np.uint32)
    new_idx[dest] = np.where(single, x | DEAD_BIT, x).astype(np.uint32)
    new_meta[dest] = ((k - new_at) | ((size - 1) << PL_BITS) | np.where(moved, MOVED, 0)).astype(np.uint32)
    p = pos[dest[single]]
    if s["sym"] is None:
        s["sa"][p] = x[single]
    else:
        new_sym = np.zeros(slots, np.uint8)
        new_sym[dest] = s["sym"][a]
        s["bwt"][p] = s["sym"][a[single]]
        if (x[single] == 0).any():
            s["origin"] = int(p[x[single] == 0][0])
        s["sym"] = new_sym
    rank[x[moved]] = pos[head[moved]]
    s["idx"], s["meta"] = new_idx, new_meta
    s["h"] = min(2 * s["h"], 2 * n)
    return int((~single).sum())


def compact(s):
    keep = s["idx"] < DEAD_BIT
    s["idx"], s["meta"], s["pos"] = s["idx"][keep], s["meta"][keep] & np.uint32(MOVED - 1), s["pos"][keep]
    if s["sym"] is not None:
        s["sym"] = s["sym"][keep]


def new_state(n, h, idx, pos, gid, gstart, rank, sa=None, bwt=None, sym=None, origin=0xC3C3C3C3):
    u32 = lambda a: np.array(a, dtype=np.uint32)  # noqa: E731  (copies)
    return dict(n=int(n), h=int(h), idx=u32(idx), pos=u32(pos), meta=to_inplace(gid, gstart), rank=u32(rank), sa=None if sa is None else u32(sa),
                bwt=None if bwt is None else np.array(bwt, dtype=np.uint8), sym=None if sym is None else np.array(sym, dtype=np.uint8),
                origin=origin if sa is None else None)


def run(s, chain_group=4, record_cap=0, max_rounds=-1, always_compact=False, broken=None, round_limit=45):
    """a state from new_state() through the chains, the rounds and the compactions, in place -> the counters of dk_dbg_dev_in_place (and the
    chains' `pairs` and `walks`)"""
    count = len(s["idx"])
    c = chains(s, max(2, chain_group), record_cap, broken) if chain_group else dict(records=0, list_full=0, settled=0, pairs=[], walks=[])
    live = count - c["settled"]
    compactions = rounds = 0
    if live > 0 and (always_compact or (c["settled"] and live * 4 <= count and count >= COMPACT_FROM)):
        compact(s)
        compactions += 1
    in_flight = []      # live counts of the rounds launched and not read yet
    device_live = None  # what the last round launched since the last compaction left alive
    while live > 0 and (max_rounds < 0 or rounds < max_rounds):
        assert rounds < round_limit, "no convergence"
        device_live = 0 if device_live == 0 else one_round(s, broken)  # (nothing alive: the round does nothing)
        in_flight.append(device_live)
        rounds += 1
        if len(in_flight) < 2:
            continue
        live = in_flight.pop(0)
        if live == 0:
            break
        slots = len(s["idx"])
        if always_compact or (live * 4 <= slots and slots >= COMPACT_FROM):
            live = in_flight.pop(0)
            if live == 0:
                break
            compact(s)
            compactions += 1
            device_live = None
    if max_rounds >= 0:
        while in_flight:
            live = in_flight.pop(0)
    return dict(slots=len(s["idx"]), live=live, records=c["records"], list_full=c["list_full"], settled=c["settled"], rounds=rounds,
                compactions=compactions, pairs=c["pairs"], walks=c["walks"])
