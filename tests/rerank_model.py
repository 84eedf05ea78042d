"""TEST HELPER: plain numpy model of one regrouping of the suffix sort -- rerank() and classify_and_read() of csrc/suffix_array.hip, what
dk_dbg_dev_rerank runs -- written from the definition below and not from the kernels.  tests/test_rerank_model.py pins it against a per-slot
Python loop and lets a prefix-doubling suffix sort regroup through it before tests/test_gpu_rerank_layer.py lets it judge the device.
Integers only, no tolerance anywhere.

The input is a list of `count` SLOTS in sorted order: keys[a], the suffix idx[a], and in a LATER rerank the SA position pos_in[a] and the symbol
sym_in[a] in front of the suffix.  In the FIRST rerank (pos_in None) slot a is SA position a and L = bwt already holds every slot's symbol.

Heads and groups.  Slot a is a HEAD if a == 0, or gid_in is given and gid_in[a] != gid_in[a - 1], or keys[a] >> cmp_shift != keys[a - 1] >>
cmp_shift, or (narrow keys: 32-bit words and 256 bucket starts) a is one of the bucket starts.  A group is the run of slots from a head up
to the next one; it SURVIVES if it has more than one member, and the slot of a group of one is FINAL.

Active list.  The surviving slots in slot order: out_idx = idx[a], out_pos = pos_in[a] (first rerank: a), out_gid = the number of surviving
groups in front of a's group, sym_out = sym_in[a] (first rerank: bwt[a]; no symbols without bwt).  active = its length, groups = the surviving
groups.  gstart[g] = the place of group g's head in the list for g < groups, gstart[groups] = active.

Finals.  Later reranks only: sa[pos_in[a]] = idx[a] (if sa is given) and bwt[pos_in[a]] = sym_in[a] (if bwt is given); with bwt, origin =
pos_in[a] for the final slot that holds suffix 0, and only for it.  The first rerank writes none of the three: its finals stand where they are.

Ranks.  Later reranks with a rank array only: rank[idx[a]] = pos_in[head slot of a's group] for every slot, singletons included -- except where
that head is an OLD head (gid_in changes there, or it is slot 0 and gid_in is given): the members of such a group keep the rank they have.

Classification of the surviving groups by size = gstart[g + 1] - gstart[g]: a group of more than ls_max members is BIG.  big_groups and
big_slots count them and their members; bigidx[g] = the number of big groups in front of big group g (nothing is stored for a small one),
bigoff[j] = the members of the big groups in front of the j-th big one; above_pl_slots = the members of the groups of more than PL_MAX.

Everything else stays as it was: rank of kept groups, sa / bwt at non-final positions, the lists from `active` on, gstart from groups + 1 on,
bigidx of small groups, bigoff from big_groups on, origin when suffix 0 survives.  apply_model() lays the model's values over what the arrays
held before, so that a comparison of whole arrays says that too."""
from types import SimpleNamespace

import numpy as np

TILE = 2048        # RR_TILE: slots per tile of the rerank kernels
SCAN_CHUNK = 1024  # RSC_CHUNK: tiles per chunk of the three-phase scan, which runs above 4 * SCAN_CHUNK tiles
PL_MAX = 256
BG_TILE = 4096     # groups per tile of the classification kernels
BG_GRID = 1024     # their workgroups: each takes a stretch of ceil(ceil(groups / BG_TILE) / BG_GRID) tiles
COUNT_NAMES = ("active", "groups", "big_slots", "big_groups", "above_pl_slots")


def heads_model(keys, gid_in=None, cmp_shift=0, bucket_starts=None):
    """-> (head, old_head): boolean per slot"""
    keys = np.asarray(keys)
    n = len(keys)
    k = keys if bucket_starts is not None else keys.astype(np.uint64) >> np.uint64(cmp_shift)
    head = np.zeros(n, bool)
    head[0] = True
    head[1:] = k[1:] != k[:-1]
    old = np.zeros(n, bool)
    if gid_in is not None:
        g = np.asarray(gid_in)
        old[0] = True
        old[1:] = g[1:] != g[:-1]
        head |= old
    if bucket_starts is not None:
        s = np.asarray(bucket_starts, dtype=np.int64)
        head[s[s < n]] = True
    return head, old


def rerank_model(keys, idx, pos_in=None, gid_in=None, cmp_shift=0, bucket_starts=None, sym_in=None, bwt=None, ls_max=1024):
    """-> namespace: active, groups, out_idx / out_pos / out_gid / sym_out (active entries; sym_out None without symbols), gstart (groups + 1),
    final (slots), final_pos, head_slot (per slot), ranked (slots whose suffix gets a rank) and rank_val (its value; later reranks only),
    origin (None: not written), big_groups, big_slots, above_pl_slots, big (group numbers), bigoff (big_groups entries)"""
    idx = np.asarray(idx, dtype=np.uint32)
    n = len(idx)
    first = pos_in is None
    slots = np.arange(n, dtype=np.int64)
    head, old = heads_model(keys, gid_in, cmp_shift, bucket_starts)
    starts = np.flatnonzero(head)
    sizes = np.diff(np.append(starts, n))
    surv = np.repeat(sizes > 1, sizes)
    head_slot = np.repeat(starts, sizes)
    act = np.flatnonzero(surv)
    pos = slots.astype(np.uint32) if first else np.asarray(pos_in, dtype=np.uint32)
    sym = None if bwt is None else np.asarray(bwt if first else sym_in, dtype=np.uint8)
    m = SimpleNamespace(first=first, active=len(act), groups=int((sizes > 1).sum()), head=head, old_head=old, head_slot=head_slot)
    m.out_idx, m.out_pos = idx[act], pos[act]
    m.out_gid = (np.cumsum(head & surv)[act] - 1).astype(np.uint32)
    m.sym_out = None if sym is None else sym[act]
    m.gstart = np.append(np.searchsorted(act, starts[sizes > 1]), len(act)).astype(np.uint32)
    m.final = np.flatnonzero(~surv)
    m.final_pos = pos[m.final]
    m.final_sym = None if sym is None else sym[m.final]
    m.origin = None
    if not first and bwt is not None:
        zero = m.final[idx[m.final] == 0]
        if len(zero):
            m.origin = int(pos[zero[0]])
    m.ranked = slots[:0] if first else np.flatnonzero(~old[head_slot])
    m.rank_val = pos[head_slot[m.ranked]]
    gsz = np.diff(m.gstart.astype(np.int64))
    m.big = np.flatnonzero(gsz > ls_max)
    m.big_groups, m.big_slots = len(m.big), int(gsz[m.big].sum())
    m.above_pl_slots = int(gsz[gsz > PL_MAX].sum())
    m.bigoff = (np.cumsum(gsz[m.big]) - gsz[m.big]).astype(np.uint32)
    m.counts = (m.active, m.groups, m.big_slots, m.big_groups, m.above_pl_slots)
    return m


def apply_model(m, idx, before):
    """before: {name: array or None} of out_idx, out_pos, out_gid, sym_out, gstart, bigidx, bigoff, rank, sa, bwt and origin (an int or None) as
    they are before the call -> the same after it.  Entries of idx are distinct and so are those of pos_in (the sort's own lists are
    permutations), so no two stores of the model meet."""
    idx = np.asarray(idx, dtype=np.uint32)
    after = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    for name in ("out_idx", "out_pos", "out_gid", "sym_out"):
        if after.get(name) is not None:
            after[name][:m.active] = getattr(m, name)
    after["gstart"][:m.groups + 1] = m.gstart
    after["bigidx"][m.big] = np.arange(m.big_groups, dtype=np.uint32)
    after["bigoff"][:m.big_groups] = m.bigoff
    if not m.first:
        if after.get("rank") is not None:
            after["rank"][idx[m.ranked]] = m.rank_val
        if after.get("sa") is not None:
            after["sa"][m.final_pos] = idx[m.final]
        if after.get("bwt") is not None:
            after["bwt"][m.final_pos] = m.final_sym
            if m.origin is not None:
                after["origin"] = m.origin
    return after


# ---- the same, one slot at a time (tests/test_rerank_model.py compares the two) --------------------------------------------------------------
def rerank_loop(keys, idx, pos_in=None, gid_in=None, cmp_shift=0, bucket_starts=None, sym_in=None, bwt=None, ls_max=1024):
    """-> dict of plain lists and numbers under rerank_model's names, straight from the sentences of the module docstring"""
    n = len(idx)
    first = pos_in is None
    narrow = bucket_starts is not None
    forced = set(int(s) for s in bucket_starts) if narrow else set()
    cmp = [int(k) if narrow else int(k) >> cmp_shift for k in keys]
    head, old = [], []
    for a in range(n):
        o = gid_in is not None and (a == 0 or int(gid_in[a]) != int(gid_in[a - 1]))
        head.append(a == 0 or o or cmp[a] != cmp[a - 1] or a in forced)
        old.append(bool(o))
    r = dict(out_idx=[], out_pos=[], out_gid=[], sym_out=[], gstart=[], sa={}, bwt={}, rank={}, origin=None)
    a = 0
    while a < n:
        b = a + 1
        while b < n and not head[b]:
            b += 1
        pos_of = (lambda s: s) if first else (lambda s: int(pos_in[s]))
        if b - a > 1:
            r["gstart"].append(len(r["out_idx"]))
            for s in range(a, b):
                r["out_idx"].append(int(idx[s]))
                r["out_pos"].append(pos_of(s))
                r["out_gid"].append(len(r["gstart"]) - 1)
                if bwt is not None:
                    r["sym_out"].append(int(bwt[s]) if first else int(sym_in[s]))
        elif not first:
            r["sa"][pos_of(a)] = int(idx[a])
            if bwt is not None:
                r["bwt"][pos_of(a)] = int(sym_in[a])
                if int(idx[a]) == 0:
                    r["origin"] = pos_of(a)
        if not first and not old[a]:
            for s in range(a, b):
                r["rank"][int(idx[s])] = pos_of(a)
        a = b
    r["active"], r["groups"] = len(r["out_idx"]), len(r["gstart"])
    r["gstart"].append(r["active"])
    r["bigidx"], r["bigoff"], r["big_slots"], r["above_pl_slots"] = {}, [], 0, 0
    for g in range(r["groups"]):
        size = r["gstart"][g + 1] - r["gstart"][g]
        if size > ls_max:
            r["bigidx"][g] = len(r["bigoff"])
            r["bigoff"].append(r["big_slots"])
            r["big_slots"] += size
        if size > PL_MAX:
            r["above_pl_slots"] += size
    r["big_groups"] = len(r["bigoff"])
    return r
